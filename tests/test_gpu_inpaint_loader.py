"""training.DevicePatchLoader over a RandomMaskInpainting dataset on the GPU: only the clean arena is held, and every
batch is tests/inpaint_ref.py's restatement for the loader's own table, ids and known shares, bit for bit.

Three small PNGs (40 x 56, 33 x 47, 20 x 25: the last smaller than the patch), patches of 32 x 32 with all eight turns
and flips, a drawn known share per sample, a Gaussian 5 x 5 table."""
import logging

import numpy as np
import pytest
import torch

from tests import inpaint_ref as ref, patch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((40, 56), (33, 47), (20, 25))
N = 10
KEEP = [[0.2, 0.5, 1.0], [0.4, 0.4, 0.2]]


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
    folder = tmp_path_factory.mktemp("inpaint")
    csv_path, pics = patch_ref.write_pictures(str(folder), SHAPES)
    for v in pics:
        v.setflags(write=False)
    return str(folder), csv_path, pics


def loader_of(G, files, batch=4, shared=None, **over):
    conf = dict(keep=KEEP, fill="conv", fill_side=5, fill_sigma=1.5, hole=60, use_data_aug=True, patch_size=32,
                max_num_patchs=N, seed=31)
    conf.update(over)
    ds = G.T.RandomMaskInpainting(csv_path=files[1], root_folder=files[0], logger=logging.getLogger("test"), **conf)
    return G.T.DevicePatchLoader(ds, G.T.ResumeableSampler(ds, batch), batch, device=torch.device(DEV), shared=shared)


def batches(loader, epoch=1):
    loader.sampler.set_epoch_and_current_sample(epoch, -1)
    out = []
    for inp, target in loader:
        out.append((inp.cpu().numpy(), target.cpu().numpy(), loader.last_mask.cpu().numpy()))
    return out


@pytest.fixture(scope="module")
def epoch_one(G, files):
    loader = loader_of(G, files)
    got = batches(loader, 1)
    return loader, got


def test_every_batch_is_the_oracle_for_the_loaders_own_tables(G, files, epoch_one):
    loader, got = epoch_one
    ds = loader.dataset
    assert loader.masked and not loader.paired and not loader.raw
    pack = loader.prepare()
    for i in range(3):
        assert np.array_equal(pack.image(i).cpu().numpy(), files[2][i])
    assert len(got) == len(loader) == 3 and [b[0].shape[0] for b in got] == [4, 4, 2]
    modes, _ = loader.epoch_draws(1)
    keeps = loader.epoch_keep(1)
    rs = np.random.RandomState((31 * 1000003 + 1) % 2 ** 32)
    assert np.array_equal(modes, rs.randint(0, 8, N))
    levels = rs.choice(KEEP[0], p=KEEP[1], size=N)
    assert np.array_equal(keeps, [G.K.keep_units(float(v)) for v in levels]) and len(set(keeps.tolist())) > 1
    at = 0
    for inp, target, mask in got:
        n = inp.shape[0]
        pos = np.arange(at, at + n)
        rows = [(int(ds.plan[p, 0]), int(ds.plan[p, 1]), int(ds.plan[p, 2]), int(modes[p])) for p in pos]
        ids = [(1 << 32) | int(p) for p in pos]
        want = ref.mask_fill_patch(files[2], rows, ids, keeps[pos], 31, 32, 32, ds.weights, "conv", 60)
        assert inp.shape == target.shape == (n, 3, 32, 32) and mask.shape == (n, 1, 32, 32)
        assert np.array_equal(target, want[0]) and np.array_equal(inp, want[1]) and np.array_equal(mask, want[2])
        # last_mask against input != target: a missing pixel differs wherever the fill differs from the clean value
        differs = (inp != target).any(axis=1, keepdims=True)
        assert not (differs & (mask == 1)).any()
        assert np.array_equal(differs, (want[1] != want[0]).any(axis=1, keepdims=True)) and differs.any()
        at += n


def test_two_epochs_differ_in_mask_and_two_loaders_with_one_seed_agree(G, files, epoch_one):
    loader, got = epoch_one
    second = batches(loader, 2)
    # position 0 of both epochs with a share below 1: another id, another mask
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(got, second))
    again = batches(loader, 1)
    other = batches(loader_of(G, files), 1)
    for a, b, c in zip(got, again, other):
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    shared = {}
    one, two = loader_of(G, files, shared=shared), loader_of(G, files, shared=shared, fill="zero")
    first = batches(one, 1)
    zero = batches(two, 1)
    assert one.prepare().arena.data_ptr() == two.prepare().arena.data_ptr() and len(shared) == 1      # one arena for both
    for a, b, z in zip(got, first, zero):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], z[2]) and np.array_equal(a[1], z[1])
        assert np.array_equal(z[0], z[1] * z[2])                                                       # the zero fill
