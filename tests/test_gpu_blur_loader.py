"""training.DevicePatchLoader over a GaussianMotionDeblurring dataset on the GPU: only the clean files are decoded, the
blurred arena is made on the device with each file's own kernel, and every batch is tests/pair_ref.py's paired
restatement applied to the oracle-blurred (tests/blur_ref.py) and the clean pictures, bit for bit.

Four small PNGs (70 x 90, 33 x 47, 130 x 64, 40 x 25), patches of 32 x 32 with all eight turns and flips; one kernel
for all files under the wrap boundary, and a drawn kernel per file -- four kernels of unlike sides -- under reflect."""
import logging

import numpy as np
import pytest
import torch

from tests import blur_ref as ref, pair_ref, patch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((70, 90), (33, 47), (130, 64), (40, 25))
N = 14
SPECS = [["gaussian:9:1.6", "motion:15:30", "box:3", "motion:5:90"], [0.1, 0.2, 0.3, 0.4]]
CASES = {"one": ("gaussian:25:1.6", "wrap"), "drawn": (SPECS, "reflect")}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, training
    return type("G", (), dict(K=kernels, T=training))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    folder = tmp_path_factory.mktemp("blur")
    csv_path, pics = patch_ref.write_pictures(str(folder), SHAPES)
    for v in pics:
        v.setflags(write=False)
    return str(folder), csv_path, pics


def dataset_of(G, files, case, **over):
    kernel, boundary = CASES[case]
    conf = dict(kernel=kernel, boundary=boundary, use_data_aug=True, patch_size=32, max_num_patchs=N, seed=31)
    conf.update(over)
    return G.T.GaussianMotionDeblurring(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"), **conf)


def loader_of(G, files, case, batch=4, shared=None, **over):
    ds = dataset_of(G, files, case, **over)
    return G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, batch), batch, device=torch.device(DEV), shared=shared)


def batches(loader, epoch=1):
    loader.sampler.set_epoch_and_current_sample(epoch, -1)
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in loader]


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_batch_is_the_paired_restatement_on_the_oracle_blurred_pictures(G, files, case):
    loader = loader_of(G, files, case)
    ds = loader.dataset
    boundary = CASES[case][1]
    assert loader.synthetic and loader.paired
    if case == "drawn":
        want = [SPECS[0][int(k)] for k in np.random.RandomState(31).choice(4, p=SPECS[1], size=4)]
        assert [k.spec for k in ds.kernels] == want and len(set(ds.kernels)) > 1          # a mixed-kernel draw
    oracle = [ref.blur(p, np.array(k.table), boundary) for p, k in zip(files[2], ds.kernels)]
    # the arenas: the clean files as decoded, the oracle's blur of each, one image table
    degraded, clean = loader.prepare()
    assert degraded.table is clean.table and degraded.arena.data_ptr() != clean.arena.data_ptr()
    for i in range(4):
        assert np.array_equal(clean.image(i).cpu().numpy(), files[2][i])
        bad = int(np.count_nonzero(degraded.image(i).cpu().numpy() != oracle[i]))
        print(f"{case} image {i} {ds.kernels[i].spec}: {bad} mismatching bytes")
        assert bad == 0
    got = batches(loader)
    assert len(got) == len(loader) == 4 and [i.shape[0] for i, _ in got] == [4, 4, 4, 2]
    modes, sigma = loader.epoch_draws(1)
    assert not sigma.any() and len(set(modes.tolist())) > 2 and (modes & 2).any()        # odd quarter turns among them
    rows = [(img, r, c, modes[p]) for p, (r, c, _, img) in enumerate(ds.patchs_data)]
    assert {r[0] for r in rows} == {0, 1, 2, 3}
    ids = (1 << 32) | np.arange(len(ds), dtype=np.int64)
    target_ref, inp_ref, _ = pair_ref.pair_batch_ref(oracle, files[2], rows, ids, None, ds.seed, 32, 32)
    inp, target = np.concatenate([i for i, _ in got]), np.concatenate([t for _, t in got])
    assert inp.dtype == np.float32 and inp.shape == (N, 3, 32, 32)
    assert np.array_equal(target, target_ref) and np.array_equal(inp, inp_ref)
    assert all((inp[k] != target[k]).any() for k in range(N))
    # the host path's patches under the same rows and modes: the restatement on the pictures the host path cuts from
    host = dataset_of(G, files, case)
    assert host.kernels == ds.kernels
    for i in range(4):
        assert np.array_equal(host.load_pair(i)[0], oracle[i]) and np.array_equal(host.load_pair(i)[1], files[2][i])
    host_pics = [host.load_pair(i) for i in range(4)]
    host_target, host_inp, _ = pair_ref.pair_batch_ref([p[0] for p in host_pics], [p[1] for p in host_pics], rows, ids,
                                                       None, ds.seed, 32, 32)
    assert np.array_equal(inp, host_inp) and np.array_equal(target, host_target)


def test_an_additive_mode_adds_its_noise_to_the_blurred_patch_only(G, files):
    plain = batches(loader_of(G, files, "drawn"))
    noised = batches(loader_of(G, files, "drawn", dist_mode="addictive_noise", lambda_noise=10.0))
    for (i0, t0), (i1, t1) in zip(plain, noised):
        assert np.array_equal(t0, t1)
        diff = (i1.astype(np.float64) - i0).reshape(i0.shape[0], -1)
        assert (diff != 0).mean() > 0.9 and np.all(np.abs(diff.std(axis=1) - 10.0 / 255.0) < 0.1 * 10.0 / 255.0)


def test_loaders_with_different_kernels_or_boundaries_do_not_share_a_store_entry(G, files):
    shared = {}
    one, two = loader_of(G, files, "one", shared=shared), loader_of(G, files, "drawn", shared=shared)
    three = loader_of(G, files, "one", shared=shared, kernel="gaussian:25:2.0")
    four = loader_of(G, files, "one", shared=shared, boundary="replicate")
    for loader in (one, two, three, four):
        loader.prepare()
    assert len(shared) == 4
    k = G.T.parse_blur_spec("gaussian:25:1.6")
    assert any(key[-3:] == ("blur", (k,) * 4, "wrap") for key in shared)
    assert any(key[-3:] == ("blur", tuple(two.dataset.kernels), "reflect") for key in shared)
    assert any(key[-3:] == ("blur", (G.T.parse_blur_spec("gaussian:25:2.0"),) * 4, "wrap") for key in shared)
    assert any(key[-3:] == ("blur", (k,) * 4, "replicate") for key in shared)
    assert one.prepare()[0].arena.data_ptr() != three.prepare()[0].arena.data_ptr()
    assert not torch.equal(one.prepare()[0].arena, three.prepare()[0].arena)
    assert not torch.equal(one.prepare()[0].arena, four.prepare()[0].arena)
    # the same degradation again shares the entry, also when the kernel is given as its table
    assert loader_of(G, files, "one", shared=shared).prepare()[0].arena is one.prepare()[0].arena and len(shared) == 4
    assert loader_of(G, files, "one", shared=shared, kernel=np.array(k.table)).prepare()[0].arena is one.prepare()[0].arena
    assert len(shared) == 4


def test_a_device_resident_training_stage_takes_the_dataset(G, files):
    stage = dict(type="GaussianMotionDeblurring", device_resident=True,
                 dataset_args=dict(csv_path=files[1], root_folder=files[0], kernel=SPECS, boundary="wrap", patch_size=32,
                                   max_num_patchs=N),
                 dataloader_args=dict(batch_size=4))
    st = G.T.TrainStage(0, stage, {}, 0, 1, {})
    assert isinstance(st.loader, G.T.DevicePatchLoader) and st.loader.paired and st.loader.synthetic and st.steps == 4
