"""grr_patch_batch, training.DevicePatchLoader and the planar training step on the GPU, against the numpy
restatement tests/patch_ref.py.

The arena: pictures of 5 x 7, 16 x 16, 40 x 56 and 70 x 33 packed back to back (images start at odd bytes), for
C = 1 and C = 3.  Patches of 16 x 16 and 48 x 48 (mirror fills of several periods, an odd turn wider than one
32-wide tile), 16 x 32 (even-k modes only) and 6 x 6 (a row of pw C elements that is no multiple of 4: the noise
blocks straddle lanes, and the scalar stores)."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

from tests import patch_ref

pytestmark = pytest.mark.gpu

SHAPES = ((5, 7), (16, 16), (40, 56), (70, 33))
SEED = 2204
PATCHES = ((16, 16), (48, 48), (16, 32), (6, 6))
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore, training
    return type("G", (), dict(K=kernels, R=restore, T=training))


def images_of(c):
    return [patch_ref.picture(k + 3, h, w, c) for k, (h, w) in enumerate(SHAPES)]


def rows_of(n, ph, pw):
    """n rows (img, row, col, mode): the images in turn, all legal modes, (row, col) at 0, at the last pixel and
    in between."""
    modes = range(8) if ph == pw else (0, 1, 4, 5)
    rows = []
    for s in range(n):
        img = s % len(SHAPES)
        h, w = SHAPES[img]
        where = (s // len(SHAPES)) % 3
        r, c = ((0, 0), (h - 1, w - 1), ((s * 7) % h, (s * 5) % w))[where]
        rows.append((img, r, c, list(modes)[(s // 2) % len(modes)]))
    return rows


_CASES = {}


def case(G, c, ph, pw, n=37):
    """The kernel's and the restatement's batch of one (C, patch) case, computed once."""
    key = (c, ph, pw, n)
    if key not in _CASES:
        images = images_of(c)
        pack = G.R.pack_images(images, "cuda")
        rows = rows_of(n, ph, pw)
        ids = np.array([(3 << 32) | (s * 11 + 1) for s in range(n)], dtype=np.int64)
        sigma = np.array([(5.0, 25.0, 50.0)[s % 3] / 255.0 for s in range(n)], dtype=np.float32)
        clean, noisy = G.K.patch_batch(pack, rows, ids, sigma, SEED, ph, pw)
        ref = patch_ref.patch_batch_ref(images, rows, ids, sigma, SEED, ph, pw)
        _CASES[key] = dict(images=images, pack=pack, rows=rows, ids=ids, sigma=sigma, clean=clean.cpu().numpy(),
                           noisy=noisy.cpu().numpy(), ref=ref)
        for v in ref:
            v.setflags(write=False)
    return _CASES[key]


def within_one_ulp(got, ref):
    return (got == ref) | (got == np.nextafter(ref, np.float32(np.inf))) | (got == np.nextafter(ref, np.float32(-np.inf)))


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("ph,pw", PATCHES)
def test_clean_is_the_restatement_bit_for_bit(G, c, ph, pw):
    k = case(G, c, ph, pw)
    assert k["clean"].shape == (37, c, ph, pw) and k["clean"].dtype == np.float32
    assert np.array_equal(k["clean"], k["ref"][0])
    if ph == pw:
        assert {r[3] for r in k["rows"]} == set(range(8))


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("ph,pw", PATCHES)
def test_noisy_on_a_real_arena(G, c, ph, pw):
    """|noisy - ref| <= 2^-23 (|noise_ref| + |noisy_ref|): one ulp of the noise plus one of the sum."""
    k = case(G, c, ph, pw)
    _, noisy_ref, noise_ref = k["ref"]
    err = np.abs(k["noisy"].astype(np.float64) - noisy_ref.astype(np.float64))
    bound = EPS * (np.abs(noise_ref).astype(np.float64) + np.abs(noisy_ref).astype(np.float64))
    print(f"C {c} {ph}x{pw}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
          f"differing {np.count_nonzero(err)} of {err.size}")
    assert np.isfinite(k["noisy"]).all() and (err <= bound).all()


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("ph,pw", PATCHES)
def test_noise_on_a_zero_arena_is_within_one_ulp(G, c, ph, pw):
    k = case(G, c, ph, pw)
    zero = G.R.pack_images([np.zeros_like(im) for im in k["images"]], "cuda")
    clean, noisy = G.K.patch_batch(zero, k["rows"], k["ids"], k["sigma"], SEED, ph, pw)
    assert not clean.any()
    got, ref = noisy.cpu().numpy(), k["ref"][2]
    ok = within_one_ulp(got, ref)
    print(f"C {c} {ph}x{pw}: {np.count_nonzero(got != ref)} of {got.size} differ, {np.count_nonzero(~ok)} by more than 1 ulp")
    assert ok.all()


def test_sigma_zero_gives_clean(G):
    k = case(G, 3, 48, 48)
    clean, noisy = G.K.patch_batch(k["pack"], k["rows"], k["ids"], np.zeros(37, np.float32), SEED, 48, 48)
    assert torch.equal(clean.view(torch.int32), noisy.view(torch.int32))
    assert np.array_equal(clean.cpu().numpy(), k["clean"])


@pytest.mark.parametrize("c,ph,pw", [(3, 48, 48), (1, 16, 32), (3, 6, 6)])
def test_a_sample_does_not_depend_on_its_batch(G, c, ph, pw):
    k = case(G, c, ph, pw)
    run = lambda idx, seed=SEED, ids=k["ids"]: [t.cpu().numpy() for t in G.K.patch_batch(
        k["pack"], [k["rows"][i] for i in idx], ids[idx], k["sigma"][idx], seed, ph, pw)]
    again = run(list(range(37)))
    assert np.array_equal(again[0], k["clean"]) and np.array_equal(again[1], k["noisy"])        # two runs
    for s in (0, 9, 36):
        alone = run([s])                                                                         # n = 1
        assert np.array_equal(alone[0][0], k["clean"][s]) and np.array_equal(alone[1][0], k["noisy"][s])
    order = list(np.random.RandomState(1).permutation(37))
    mixed = run(order)
    assert np.array_equal(mixed[0], k["clean"][order]) and np.array_equal(mixed[1], k["noisy"][order])
    other_seed = run(list(range(37)), seed=SEED + 1)
    other_ids = run(list(range(37)), ids=k["ids"] + 1)
    high_ids = run(list(range(37)), ids=k["ids"] + (1 << 32))
    for other in (other_seed, other_ids, high_ids):
        assert np.array_equal(other[0], k["clean"])
        assert all(not np.array_equal(other[1][s], k["noisy"][s]) for s in range(37))
    assert all(not np.array_equal(k["noisy"][s] - k["clean"][s], k["noisy"][s + 4] - k["clean"][s + 4])
               for s in range(33))


def test_out_of_range_tables_are_clamped(G):
    """The clamping contract: img, row, col and mode outside their ranges give some pixels of the arena, finite,
    and nothing beyond the two outputs is written."""
    from irdu_amd import _native
    k = case(G, 3, 16, 16)
    pack, n, c, ph, pw = k["pack"], 8, 3, 16, 16
    big = 2 ** 31 - 1
    table = torch.tensor([(-1, 0, 0, 0), (99, 3, 3, 1), (0, -5, -5, 2), (1, big, big, 3), (2, 10 ** 6, 2, -1), (3, 2, 10 ** 6, 8),
                          (-big, -big, -big, -big), (big, big, big, big)], dtype=torch.int32, device="cuda")
    ids = torch.arange(n, dtype=torch.int64, device="cuda")
    sigma = torch.full((n,), 0.1, dtype=torch.float32, device="cuda")
    size, guard = n * c * ph * pw, 1024
    buf = torch.full((2 * size + 3 * guard,), -7.0, dtype=torch.float32, device="cuda")
    clean, noisy = buf[guard:guard + size], buf[2 * guard + size:2 * guard + 2 * size]
    _native.call("grr_patch_batch", pack.arena.data_ptr(), pack.arena.numel(), c, pack.table.data_ptr(), len(SHAPES),
                 table.data_ptr(), ids.data_ptr(), sigma.data_ptr(), n, SEED, ph, pw, clean.data_ptr(), noisy.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    for lo in (0, guard + size, 2 * guard + 2 * size):
        assert (host[lo:lo + guard] == -7.0).all()
    got_clean, got_noisy = host[guard:guard + size], host[2 * guard + size:2 * guard + 2 * size]
    assert np.isfinite(got_noisy).all() and (got_clean >= 0).all() and (got_clean <= 1).all()
    # the wrapper takes the same device tables; rows 0 and 1 clamp to images 0 and 3
    c2, _ = G.K.patch_batch(pack, table, ids, sigma, SEED, ph, pw)
    assert np.array_equal(c2.cpu().numpy().reshape(-1), got_clean)
    want = patch_ref.patch_batch_ref(k["images"], [(0, 0, 0, 0), (3, 3, 3, 1)], [0, 1], [0.1, 0.1], SEED, ph, pw)[0]
    assert np.array_equal(c2[:2].cpu().numpy(), want)


# ---------------------------------------------------------------------------
# the loader
@pytest.fixture(scope="module")
def pictures(tmp_path_factory):
    folder = tmp_path_factory.mktemp("pictures")
    csv_path, pics = patch_ref.write_pictures(str(folder))
    return str(folder), csv_path, pics


def loader_of(G, pictures, name="aug16", batch=4, rank=0, world=1, **over):
    folder, csv_path, _ = pictures
    conf = dict(patch_ref.GOLDEN_CONFIGS[name])
    conf.update(over)
    ds = G.T.ImageSuperResolution(csv_path=csv_path, root_folder=folder, logger=logging.getLogger("test"), **conf)
    sampler = G.T.ResumeableSampler(ds, batch, rank, world)
    return G.T.DevicePatchLoader(ds, sampler, batch, device=torch.device("cuda:0"))


def batches(loader):
    return [(n.cpu().numpy(), c.cpu().numpy()) for n, c in loader]


@pytest.mark.parametrize("name", ("aug16", "vary64"))
def test_loader_clean_is_the_restatement_on_the_plan(G, pictures, name):
    loader = loader_of(G, pictures, name)
    ds = loader.dataset
    loader.sampler.set_epoch_and_current_sample(2, -1)
    got = batches(loader)
    assert len(got) == len(loader) and all(n.shape == c.shape for n, c in got)
    modes, sigma = loader.epoch_draws(2)
    rows = [(img, r, c, modes[p]) for p, (r, c, _, img) in enumerate(ds.patchs_data)]
    ids = (2 << 32) | np.arange(len(ds), dtype=np.int64)
    ph, pw = ds.out_size()
    clean_ref, noisy_ref, noise_ref = patch_ref.patch_batch_ref(pictures[2], rows, ids, sigma, ds.seed, ph, pw)
    clean, noisy = np.concatenate([c for _, c in got]), np.concatenate([n for n, _ in got])
    assert np.array_equal(clean, clean_ref)
    assert (np.abs(noisy.astype(np.float64) - noisy_ref) <= EPS * (np.abs(noise_ref).astype(np.float64) + np.abs(noisy_ref))).all()
    if name == "aug16":
        assert set(modes.tolist()) == set(range(8))
    else:
        assert any(pad for _, _, pad, _ in ds.patchs_data) and len(set(sigma.tolist())) == 3


def test_loader_resumes_bitwise_and_epochs_differ(G, pictures):
    loader = loader_of(G, pictures)
    loader.sampler.set_epoch_and_current_sample(1, -1)
    full = batches(loader)
    assert len(full) == 10
    loader.sampler.set_epoch_and_current_sample(1, 3 * 4 - 1)
    rest = batches(loader)
    assert len(rest) == 7
    for (n0, c0), (n1, c1) in zip(full[3:], rest):
        assert np.array_equal(n0, n1) and np.array_equal(c0, c1)
    # a loader made afresh (another process's resume), and another batch size over the same positions
    fresh = loader_of(G, pictures, batch=2)
    fresh.sampler.set_epoch_and_current_sample(1, 3 * 4 - 1)
    pairs = batches(fresh)
    assert np.array_equal(np.concatenate([n for n, _ in pairs]), np.concatenate([n for n, _ in rest]))
    loader.sampler.set_epoch_and_current_sample(2, -1)
    nxt = batches(loader)
    assert not any(np.array_equal(a[0], b[0]) for a, b in zip(full, nxt))


def test_two_ranks_make_the_one_rank_global_batch(G, pictures):
    one = loader_of(G, pictures, batch=8)
    ranks = [loader_of(G, pictures, batch=4, rank=r, world=2) for r in (0, 1)]
    for ld in [one] + ranks:
        ld.sampler.set_epoch_and_current_sample(0, -1)
    whole, parts = batches(one), [batches(ld) for ld in ranks]
    assert len(whole) == len(parts[0]) == len(parts[1]) == 5
    for gb, p0, p1 in zip(whole, *parts):
        assert np.array_equal(gb[0], np.concatenate([p0[0], p1[0]]))
        assert np.array_equal(gb[1], np.concatenate([p0[1], p1[1]]))


# ---------------------------------------------------------------------------
# training
def test_planar_step_is_the_hwc_step(G, pictures):
    import irdu_amd
    loader = loader_of(G, pictures)
    noisy, clean = next(iter(loader))
    losses = []
    for planar in (False, True):
        torch.manual_seed(5)
        model = irdu_amd.GLRImageFilter(n_channels_in=3, n_channels_out=3, ngraphs=4, n_cgd_iters=1)
        trainer = G.T.Trainer(model, {}, torch.device("cuda:0"))
        torch.manual_seed(6)
        if planar:
            losses.append(trainer.step(noisy, clean, channels_first=True))
        else:
            losses.append(trainer.step(noisy.permute(0, 2, 3, 1).contiguous().cpu(), clean.permute(0, 2, 3, 1).contiguous().cpu()))
    assert np.isfinite(losses[0]) and losses[0] == losses[1], losses


def test_run_trains_on_a_device_resident_curriculum(G, pictures, tmp_path):
    folder, csv_path, _ = pictures
    stage = lambda size, batch, **extra: dict(
        name=f"Training-data-{size}", type="ImageSuperResolution", device_resident=True,
        dataset_args=dict(csv_path=csv_path, root_folder=folder, dist_mode="addictive_noise_scale", lambda_noise=25.0,
                          use_data_aug=True, patch_size=[size, size], max_num_patchs=8, **extra),
        dataloader_args=dict(batch_size=batch, num_workers=4))
    conf = dict(name="device_resident", manual_seed=2204, path=dict(root_dir=str(tmp_path)),
                datasets=dict(train=[stage(16, 4), stage(32, 2, seed=2224)]),
                model=dict(type="GLRImageFilter", args=dict(n_channels_in=3, n_channels_out=3, ngraphs=4, n_cgd_iters=1)),
                train=dict(total_iters=3, checkpoint_every=3, verbose_every=1))
    tr = G.T.run(conf, device=torch.device("cuda:0"))
    assert tr.i == 3
    assert all(isinstance(st, G.T.DevicePatchLoader) for st in
               (s.loader for s in G.T.build_train_stages(conf)))
    assert len(tr.train_history) == 3 and all(np.isfinite(v) for row in tr.train_history for v in row)
    saved = torch.load(os.path.join(G.T.checkpoint_dir(conf), "checkpoint_iter00000003.pt"), weights_only=True)
    assert saved["i"] == 3 and all(np.isfinite(v.float().cpu().numpy()).all() for v in saved["model"].values())
