"""training.DevicePatchLoader over a JpegArtifactRemoval dataset on the GPU: only the clean files are decoded, the
degraded arena is made on the device at each file's own quality, and every batch is tests/pair_ref.py's paired
restatement applied to the oracle-degraded (tests/jpeg_ref.py) and the clean pictures, bit for bit.

Four small PNGs (70 x 90, 33 x 47, 130 x 64, 40 x 25), patches of 32 x 32 with all eight turns and flips; one quality
for all files at 4:4:4, and a drawn quality per file at 4:2:0."""
import logging

import numpy as np
import pytest
import torch

from tests import jpeg_ref, pair_ref, patch_ref, resize_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((70, 90), (33, 47), (130, 64), (40, 25))
N = 14
LEVELS = [[10, 20, 30, 40], [0.1, 0.2, 0.3, 0.4]]
CASES = {"q10": (10, 0), "drawn": (LEVELS, 2)}


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
    folder = tmp_path_factory.mktemp("car")
    csv_path, pics = patch_ref.write_pictures(str(folder), SHAPES)
    for v in pics:
        v.setflags(write=False)
    return str(folder), csv_path, pics


def loader_of(G, files, case, batch=4, shared=None, **over):
    quality, sub = CASES[case]
    conf = dict(quality=quality, subsampling=sub, use_data_aug=True, patch_size=32, max_num_patchs=N, seed=31)
    conf.update(over)
    ds = G.T.JpegArtifactRemoval(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"), **conf)
    return G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, batch), batch, device=torch.device(DEV), shared=shared)


def other_loader_of(G, files, cls, batch=4, shared=None, **conf):
    ds = cls(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"), use_data_aug=True, patch_size=32,
             max_num_patchs=N, seed=31, **conf)
    return G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, batch), batch, device=torch.device(DEV), shared=shared)


def batches(loader, epoch=1):
    loader.sampler.set_epoch_and_current_sample(epoch, -1)
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in loader]


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_batch_is_the_paired_restatement_on_the_oracle_degraded_pictures(G, files, case):
    loader = loader_of(G, files, case)
    ds = loader.dataset
    sub = CASES[case][1]
    if case == "drawn":
        assert ds.qualities == [int(q) for q in np.random.RandomState(31).choice(LEVELS[0], p=LEVELS[1], size=4)]
        assert len(set(ds.qualities)) > 1
    oracle = [jpeg_ref.degrade(p, q, sub) for p, q in zip(files[2], ds.qualities)]
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
    # the arenas: the clean files as decoded, the oracle's degradation of each, one image table
    degraded, clean = loader.prepare()
    assert degraded.table is clean.table and degraded.arena.data_ptr() != clean.arena.data_ptr()
    for i in range(4):
        assert np.array_equal(clean.image(i).cpu().numpy(), files[2][i])
        assert np.array_equal(degraded.image(i).cpu().numpy(), oracle[i])
    # the host path yields the same pictures: sample 0 without the augmentation
    host = G.T.JpegArtifactRemoval(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"),
                                   quality=CASES[case][0], subsampling=sub, patch_size=32, max_num_patchs=N, seed=31)
    assert np.array_equal(host.load_pair(2)[0], oracle[2])


def test_a_sample_does_not_change_with_the_batch_size(G, files):
    whole = batches(loader_of(G, files, "drawn", batch=4))
    for batch in (1, 3, 14):
        other = batches(loader_of(G, files, "drawn", batch=batch))
        for k in (0, 1):
            assert np.array_equal(np.concatenate([b[k] for b in other]), np.concatenate([b[k] for b in whole])), batch


def test_an_additive_mode_adds_its_noise_to_the_degraded_patch_only(G, files):
    plain = batches(loader_of(G, files, "q10"))
    noised = batches(loader_of(G, files, "q10", dist_mode="addictive_noise", lambda_noise=10.0))
    for (i0, t0), (i1, t1) in zip(plain, noised):
        assert np.array_equal(t0, t1)
        diff = (i1.astype(np.float64) - i0).reshape(i0.shape[0], -1)
        assert (diff != 0).mean() > 0.9 and np.all(np.abs(diff.std(axis=1) - 10.0 / 255.0) < 0.1 * 10.0 / 255.0)


def test_the_plain_and_the_bicubic_loaders_are_unchanged_beside_it(G, files):
    """A plain ImageSuperResolution loader and a BicubicSuperResolution loader yield the same batches before and after
    the JPEG loaders ran over the same files and the same shared dict; the plain clean batch is the unpaired
    restatement's and the bicubic input the oracle's."""
    shared = {}
    plain_conf = dict(dist_mode="addictive_noise", lambda_noise=10.0)
    before = batches(other_loader_of(G, files, G.T.ImageSuperResolution, shared=shared, **plain_conf))
    sr_before = batches(other_loader_of(G, files, G.T.BicubicSuperResolution, shared=shared, scale=2))
    one, two = loader_of(G, files, "q10", shared=shared), loader_of(G, files, "drawn", shared=shared)
    batches(one)
    batches(two)
    assert len(shared) == 4                     # plain, bicubic at scale 2, and one per (qualities, subsampling)
    assert any(k[-3:] == ("jpeg", (10, 10, 10, 10), 0) for k in shared)
    assert any(k[-3:] == ("jpeg", tuple(two.dataset.qualities), 2) for k in shared)
    assert loader_of(G, files, "q10", shared=shared).prepare()[0].arena is one.prepare()[0].arena
    plain = other_loader_of(G, files, G.T.ImageSuperResolution, shared=shared, **plain_conf)
    after = batches(plain)
    sr = other_loader_of(G, files, G.T.BicubicSuperResolution, shared=shared, scale=2)
    sr_after = batches(sr)
    assert len(shared) == 4 and not isinstance(plain.source, G.K.PatchPairSource) and sr.synthetic and sr.paired
    for (n0, c0), (n1, c1) in zip(before + sr_before, after + sr_after):
        assert np.array_equal(n0.view(np.int32), n1.view(np.int32)) and np.array_equal(c0, c1)
    ds = plain.dataset
    modes, sigma = plain.epoch_draws(1)
    rows = [(img, r, c, modes[p]) for p, (r, c, _, img) in enumerate(ds.patchs_data)]
    ids = (1 << 32) | np.arange(len(ds), dtype=np.int64)
    clean_ref, _, _ = patch_ref.patch_batch_ref(files[2], rows, ids, sigma, ds.seed, 32, 32)
    assert np.array_equal(np.concatenate([c for _, c in after]), clean_ref)
    degraded = sr.prepare()[0]
    for i in range(4):
        assert np.array_equal(degraded.image(i).cpu().numpy(), resize_ref.degrade(files[2][i], 2))


def test_a_device_resident_training_stage_takes_the_dataset(G, files):
    stage = dict(type="JpegArtifactRemoval", device_resident=True,
                 dataset_args=dict(csv_path=files[1], root_folder=files[0], quality=LEVELS, subsampling=2, patch_size=32,
                                   max_num_patchs=N),
                 dataloader_args=dict(batch_size=4))
    st = G.T.TrainStage(0, stage, {}, 0, 1, {})
    assert isinstance(st.loader, G.T.DevicePatchLoader) and st.loader.paired and st.loader.synthetic and st.steps == 4
