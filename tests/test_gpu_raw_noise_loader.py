"""training.DevicePatchLoader over a NoisyBayerDemosaicking dataset on the GPU: the device holds the clean arena alone,
every batch is the oracle tests/raw_noise_ref.py under the loader's own draws, bit for bit, and batch size, resume point
and epoch behave as tests/test_gpu_patches.py shows for the plain loader.  The pictures are patch_ref.write_pictures';
tests/test_raw_noise_ref.py holds the epochs used here away from the rounding ties."""
import logging

import numpy as np
import pytest
import torch

from tests import patch_ref, raw_noise_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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
    folder = tmp_path_factory.mktemp("raw_noise")
    csv_path, pics = patch_ref.write_pictures(str(folder))
    return str(folder), csv_path, pics


def loader_of(G, files, batch=4, shared=None, **over):
    conf = dict(ref.LOADER_CONF)
    conf.update(over)
    ds = G.T.NoisyBayerDemosaicking(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"), **conf)
    return G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, batch), batch, device=torch.device(DEV), shared=shared)


def batches(loader, epoch, after=-1):
    loader.sampler.set_epoch_and_current_sample(epoch, after)
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in loader]


@pytest.mark.parametrize("epoch", (1, 2))
def test_every_batch_is_the_oracle_under_the_loaders_draws(G, files, epoch):
    loader = loader_of(G, files)
    ds = loader.dataset
    got = batches(loader, epoch)
    assert len(got) == len(loader) == 10 and not loader.paired and not loader.synthetic and loader.raw
    target_ref, inp_ref, margin = ref.loader_reference(ds, loader, epoch, files[2])
    assert margin >= ref.TIE_MARGIN
    inp, target = np.concatenate([i for i, _ in got]), np.concatenate([t for _, t in got])
    assert inp.shape == (40, 3, 16, 16) and inp.dtype == np.float32
    assert np.array_equal(target, target_ref) and np.array_equal(inp, inp_ref)
    modes, _ = loader.epoch_draws(epoch)
    noise = loader.epoch_noise(epoch)
    assert set(modes.tolist()) == set(range(8)) and len(set(map(tuple, noise.tolist()))) > 4


def test_batch_size_resume_point_and_epoch(G, files):
    loader = loader_of(G, files)
    full = batches(loader, 1)
    rest = batches(loader, 1, 3 * 4 - 1)
    assert len(full) == 10 and len(rest) == 7
    for (i0, t0), (i1, t1) in zip(full[3:], rest):
        assert np.array_equal(i0, i1) and np.array_equal(t0, t1)
    for batch in (1, 3, 40):          # a loader made afresh, other batch sizes over the same positions
        other = batches(loader_of(G, files, batch=batch), 1)
        for k in (0, 1):
            assert np.array_equal(np.concatenate([b[k] for b in other]), np.concatenate([b[k] for b in full])), batch
    nxt = batches(loader, 2)
    assert not any(np.array_equal(a[0], b[0]) for a, b in zip(full, nxt))


def test_the_device_holds_one_arena_and_a_curriculum_shares_it(G, files):
    shared = {}
    one = loader_of(G, files, shared=shared)
    two = loader_of(G, files, shared=shared, patch_size=(32, 32), max_num_patchs=8, seed=2224, shot=0.0, read=0.0)
    pack = one.prepare()
    assert two.prepare() is pack and pack.arena.dtype == torch.uint8
    assert pack.arena.numel() == sum(p.size for p in files[2])           # the clean pictures and nothing else
    assert isinstance(one.source, G.K.PatchSource) and isinstance(one.raw_source, G.K.PatchRawSource)
    assert one.raw_source.pack is pack and two.raw_source.pack is pack
    assert one.raw_source.patterns.dtype == torch.int32 and tuple(one.raw_source.patterns.shape) == (len(files[2]),)
    assert one.raw_source.host_patterns == tuple(G.K.DEMOSAIC_PATTERNS.index(p) for p in one.dataset.patterns)
    arenas = {v.pack.arena.data_ptr() for v in shared.values()}
    assert len(arenas) == 1 and len(shared) == 3            # the arena, and one pattern list per dataset seed
    # a plain denoising stage over the same csv takes the same arena
    ds = G.T.ImageSuperResolution(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"),
                                  dist_mode="addictive_noise", lambda_noise=10.0, patch_size=16, max_num_patchs=8)
    plain = G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, 4), 4, device=torch.device(DEV), shared=shared)
    assert plain.prepare() is pack and len(shared) == 3
    # the noise-free stage computes no noise: its input is the oracle's without a table
    two.sampler.set_epoch_and_current_sample(0, -1)
    inp, target = next(iter(two))
    assert inp.shape == (4, 3, 32, 32) and two.dataset.noise_free
    modes, _ = two.epoch_draws(0)
    rows = [(img, r, c, modes[p]) for p, (r, c, _, img) in enumerate(two.dataset.patchs_data)][:4]
    want = ref.batch(files[2], two.dataset.patterns, rows, np.arange(4, dtype=np.int64), None, 2224, 32, 32, "malvar", 12, True)
    assert np.array_equal(inp.cpu().numpy(), want[1]) and np.array_equal(target.cpu().numpy(), want[0])


def test_a_device_resident_training_stage_takes_the_dataset(G, files):
    stage = dict(type="NoisyBayerDemosaicking", device_resident=True,
                 dataset_args=dict(csv_path=files[1], root_folder=files[0], shot=0.01, read=5.0, patch_size=16,
                                   max_num_patchs=8),
                 dataloader_args=dict(batch_size=4))
    st = G.T.TrainStage(0, stage, {}, 0, 1, {})
    assert isinstance(st.loader, G.T.DevicePatchLoader) and st.loader.raw and st.steps == 2
    inp, target = next(iter(st.loader))
    assert inp.shape == target.shape == (4, 3, 16, 16) and torch.isfinite(inp).all() and not torch.equal(inp, target)
