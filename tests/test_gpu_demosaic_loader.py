"""training.DevicePatchLoader over a BayerDemosaicking dataset on the GPU: only the clean files are decoded, the filled
arena is made on the device with each file's own pattern, and every batch is tests/pair_ref.py's paired restatement
applied to the oracle-filled (tests/demosaic_ref.py) and the clean pictures, bit for bit.

Four small PNGs (70 x 90, 33 x 47, 130 x 64, 40 x 25), patches of 32 x 32 with all eight turns and flips; one pattern
for all files with the malvar fill, and a drawn pattern per file with the bilinear fill."""
import logging

import numpy as np
import pytest
import torch

from tests import demosaic_ref as ref, pair_ref, patch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((70, 90), (33, 47), (130, 64), (40, 25))
N = 14
NAMES = [["rggb", "grbg", "gbrg", "bggr"], [0.1, 0.2, 0.3, 0.4]]
CASES = {"grbg": ("grbg", "malvar"), "drawn": (NAMES, "bilinear")}


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
    folder = tmp_path_factory.mktemp("bayer")
    csv_path, pics = patch_ref.write_pictures(str(folder), SHAPES)
    for v in pics:
        v.setflags(write=False)
    return str(folder), csv_path, pics


def dataset_of(G, files, case, **over):
    pattern, fill = CASES[case]
    conf = dict(pattern=pattern, fill=fill, use_data_aug=True, patch_size=32, max_num_patchs=N, seed=31)
    conf.update(over)
    return G.T.BayerDemosaicking(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"), **conf)


def loader_of(G, files, case, batch=4, shared=None, **over):
    ds = dataset_of(G, files, case, **over)
    return G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, batch), batch, device=torch.device(DEV), shared=shared)


def batches(loader, epoch=1):
    loader.sampler.set_epoch_and_current_sample(epoch, -1)
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in loader]


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_batch_is_the_paired_restatement_on_the_oracle_filled_pictures(G, files, case):
    loader = loader_of(G, files, case)
    ds = loader.dataset
    fill = CASES[case][1]
    assert loader.synthetic and loader.paired
    if case == "drawn":
        assert ds.patterns == [NAMES[0][int(k)] for k in np.random.RandomState(31).choice(4, p=NAMES[1], size=4)]
        assert len(set(ds.patterns)) > 1
    oracle = [ref.degrade(p, q, fill) for p, q in zip(files[2], ds.patterns)]
    # the arenas: the clean files as decoded, the oracle's filled mosaic of each, one image table
    degraded, clean = loader.prepare()
    assert degraded.table is clean.table and degraded.arena.data_ptr() != clean.arena.data_ptr()
    for i in range(4):
        assert np.array_equal(clean.image(i).cpu().numpy(), files[2][i])
        bad = int(np.count_nonzero(degraded.image(i).cpu().numpy() != oracle[i]))
        print(f"{case} image {i}: {bad} mismatching bytes")
        assert bad == 0
    got = batches(loader)
    assert len(got) == len(loader) == 4 and [i.shape[0] for i, _ in got] == [4, 4, 4, 2]
    modes, sigma = loader.epoch_draws(1)
    assert not sigma.any() and len(set(modes.tolist())) > 2 and (modes & 2).any()        # odd quarter turns among them
    rows = [(img, r, c, modes[p]) for p, (r, c, _, img) in enumerate(ds.patchs_data)]
    assert {r[0] for r in rows} == {0, 1, 2, 3}
    assert any(r % 2 for _, r, _, _ in rows) and any(c % 2 for _, _, c, _ in rows)      # odd origins: other CFA phases
    ids = (1 << 32) | np.arange(len(ds), dtype=np.int64)
    target_ref, inp_ref, _ = pair_ref.pair_batch_ref(oracle, files[2], rows, ids, None, ds.seed, 32, 32)
    inp, target = np.concatenate([i for i, _ in got]), np.concatenate([t for _, t in got])
    assert inp.dtype == np.float32 and inp.shape == (N, 3, 32, 32)
    assert np.array_equal(target, target_ref) and np.array_equal(inp, inp_ref)
    assert all((inp[k] != target[k]).any() for k in range(N))
    # the host path's patches under the same rows and modes: the restatement on the pictures the host path cuts from
    host = dataset_of(G, files, case)
    assert host.patterns == ds.patterns
    for i in range(4):
        assert np.array_equal(host.load_pair(i)[0], oracle[i]) and np.array_equal(host.load_pair(i)[1], files[2][i])
    host_pics = [host.load_pair(i) for i in range(4)]
    host_target, host_inp, _ = pair_ref.pair_batch_ref([p[0] for p in host_pics], [p[1] for p in host_pics], rows, ids,
                                                       None, ds.seed, 32, 32)
    assert np.array_equal(inp, host_inp) and np.array_equal(target, host_target)


def test_a_sample_does_not_change_with_the_batch_size(G, files):
    whole = batches(loader_of(G, files, "drawn", batch=4))
    for batch in (1, 3, 14):
        other = batches(loader_of(G, files, "drawn", batch=batch))
        for k in (0, 1):
            assert np.array_equal(np.concatenate([b[k] for b in other]), np.concatenate([b[k] for b in whole])), batch


def test_an_additive_mode_adds_its_noise_to_the_filled_patch_only(G, files):
    plain = batches(loader_of(G, files, "grbg"))
    noised = batches(loader_of(G, files, "grbg", dist_mode="addictive_noise", lambda_noise=10.0))
    for (i0, t0), (i1, t1) in zip(plain, noised):
        assert np.array_equal(t0, t1)
        diff = (i1.astype(np.float64) - i0).reshape(i0.shape[0], -1)
        assert (diff != 0).mean() > 0.9 and np.all(np.abs(diff.std(axis=1) - 10.0 / 255.0) < 0.1 * 10.0 / 255.0)


def test_loaders_with_different_patterns_or_fills_do_not_share_a_store_entry(G, files):
    shared = {}
    one, two = loader_of(G, files, "grbg", shared=shared), loader_of(G, files, "drawn", shared=shared)
    three = loader_of(G, files, "grbg", shared=shared, pattern="rggb")
    four = loader_of(G, files, "grbg", shared=shared, fill="zero")
    for loader in (one, two, three, four):
        loader.prepare()
    assert len(shared) == 4
    assert any(k[-3:] == ("bayer", ("grbg",) * 4, "malvar") for k in shared)
    assert any(k[-3:] == ("bayer", tuple(two.dataset.patterns), "bilinear") for k in shared)
    assert any(k[-3:] == ("bayer", ("rggb",) * 4, "malvar") for k in shared)
    assert any(k[-3:] == ("bayer", ("grbg",) * 4, "zero") for k in shared)
    assert one.prepare()[0].arena.data_ptr() != three.prepare()[0].arena.data_ptr()
    assert not torch.equal(one.prepare()[0].arena, three.prepare()[0].arena)
    # the same degradation again shares the entry
    assert loader_of(G, files, "grbg", shared=shared).prepare()[0].arena is one.prepare()[0].arena and len(shared) == 4
    # a plain loader over the same files is unpaired and has an entry of its own
    ds = G.T.ImageSuperResolution(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"),
                                  dist_mode="addictive_noise", lambda_noise=10.0, use_data_aug=True, patch_size=32,
                                  max_num_patchs=N, seed=31)
    plain = G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, 4), 4, device=torch.device(DEV), shared=shared)
    plain.prepare()
    assert len(shared) == 5 and not isinstance(plain.source, G.K.PatchPairSource)


def test_a_device_resident_training_stage_takes_the_dataset(G, files):
    stage = dict(type="BayerDemosaicking", device_resident=True,
                 dataset_args=dict(csv_path=files[1], root_folder=files[0], pattern=NAMES, fill="malvar", patch_size=32,
                                   max_num_patchs=N),
                 dataloader_args=dict(batch_size=4))
    st = G.T.TrainStage(0, stage, {}, 0, 1, {})
    assert isinstance(st.loader, G.T.DevicePatchLoader) and st.loader.paired and st.loader.synthetic and st.steps == 4
