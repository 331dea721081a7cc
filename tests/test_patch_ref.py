"""CPU checks of the v2 patch dataset and of the numpy restatement of grr_patch_batch (tests/patch_ref.py):
Philox4x32-10 against Random123's known answers, the normals' moments, the mirror index, and
training.ImageSuperResolution against the plan and the samples recorded from the reference
(tests/golden/make_golden_patches.py -> tests/golden/patches_v2.npz)."""
import logging

import numpy as np
import pytest

from irdu_amd import training
from irdu_amd.training import DevicePatchLoader, ImageSuperResolution  # noqa: F401  (what this file is about)
from tests import patch_ref
from tests.golden_io import load_golden


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = patch_ref.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_normals_moments():
    """2^20 normals of one sample id: the mean of N unit normals has deviation 1 / sqrt(N), their sample variance
    sqrt(2 / N); five of each."""
    n = 1 << 20
    z = patch_ref.normals(2204, 5, n)
    assert z.shape == (n,) and np.isfinite(z).all()
    mean_sig, var_sig = z.mean() * np.sqrt(n), (z.var() - 1.0) / np.sqrt(2.0 / n)
    print(f"mean {mean_sig:+.2f} sigma, variance {var_sig:+.2f} sigma")
    assert abs(mean_sig) <= 5 and abs(var_sig) <= 5
    # element e is lane e % 4 of block e // 4, whatever the count
    assert np.array_equal(patch_ref.normals(2204, 5, 7), z[:7])
    assert not np.array_equal(patch_ref.normals(2204, 6, 8), z[:8])
    assert not np.array_equal(patch_ref.normals(2205, 5, 8), z[:8])
    assert not np.array_equal(patch_ref.normals(2204, 5 + (1 << 32), 8), z[:8])


def test_sym_is_numpy_symmetric_padding():
    for n in (1, 2, 5, 7):
        a = np.arange(n)
        padded = np.pad(a, (0, 4 * n + 3), mode="symmetric")
        assert [patch_ref.sym(r, n) for r in range(len(padded))] == padded.tolist()


def test_transform_is_the_kernels_index_rule():
    """patch_ref.transform (np.rot90, np.flipud) puts pixel (i, j) where kernels.dihedral_index says."""
    from irdu_amd import kernels as K
    a = np.arange(3 * 5).reshape(3, 5, 1)
    for m in range(8):
        t = patch_ref.transform(a, m)
        for i in range(3):
            for j in range(5):
                p, q = K.dihedral_index(m, 3, 5, i, j)
                assert t[p, q, 0] == a[i, j, 0], (m, i, j)
        assert np.array_equal(t, training.data_augmentation(a, m))


def test_patch_batch_ref_is_the_definition_pixel_by_pixel():
    """np.pad / np.rot90 / np.flipud against include/grr.h's words: sym on the image's own sides, then
    kernels.dihedral_index, the noise indexed in the output patch's HWC order."""
    from irdu_amd import kernels as K
    img = patch_ref.picture(1, 5, 7, 3)
    rows = [(0, 4, 6, 3), (0, 0, 0, 0), (0, 2, 5, 6), (0, 4, 0, 1)]
    ids, sigma, ph, pw = [7, 8, (1 << 32) | 9, 10], [0.1, 0.0, 0.2, 0.05], 12, 12
    clean, noisy, noise = patch_ref.patch_batch_ref([img], rows, ids, sigma, 99, ph, pw)
    for s, (_, row, col, mode) in enumerate(rows):
        z = patch_ref.normals(99, ids[s], ph * pw * 3)
        for i in range(ph):
            for j in range(pw):
                p, q = K.dihedral_index(mode, ph, pw, i, j)
                px = img[patch_ref.sym(row + i, 5), patch_ref.sym(col + j, 7)]
                assert np.array_equal(clean[s, :, p, q], px.astype(np.float32) / np.float32(255.0)), (s, i, j)
        for c in range(3):
            e = (np.arange(ph)[:, None] * pw + np.arange(pw)[None, :]) * 3 + c
            assert np.array_equal(noise[s, c], (np.float64(np.float32(sigma[s])) * z[e]).astype(np.float32))
    assert np.array_equal(noisy, clean + noise) and np.array_equal(noisy[1], clean[1])


@pytest.fixture(scope="module")
def pictures(tmp_path_factory):
    folder = tmp_path_factory.mktemp("pictures")
    csv_path, pics = patch_ref.write_pictures(str(folder))
    return str(folder), csv_path, pics


def dataset(pictures, name, **over):
    folder, csv_path, _ = pictures
    conf = dict(patch_ref.GOLDEN_CONFIGS[name])
    conf.update(over)
    return training.ImageSuperResolution(csv_path=csv_path, root_folder=folder, logger=logging.getLogger("test"), **conf)


def plan_of(ds):
    return np.array([(img, r, c, int(pad)) for r, c, pad, img in ds.patchs_data], dtype=np.int64)


@pytest.mark.parametrize("name", sorted(patch_ref.GOLDEN_CONFIGS))
def test_dataset_reproduces_the_reference(pictures, name):
    gold = load_golden("patches_v2.npz")
    ds = dataset(pictures, name)
    assert len(ds) == patch_ref.GOLDEN_CONFIGS[name]["max_num_patchs"]
    assert np.array_equal(plan_of(ds), gold[name + "/plan"])
    if name == "vary64":
        assert gold[name + "/plan"][:6, 3].any(), "the fixture's samples hold a mirrored patch"
    for i in range(gold[name + "/noisy"].shape[0]):
        noisy, clean = ds[i]
        assert noisy.dtype == clean.dtype and clean.numpy().dtype == np.float32
        assert np.array_equal(clean.numpy(), gold[name + "/clean"][i]), i
        assert np.array_equal(noisy.numpy(), gold[name + "/noisy"][i]), i


def test_host_mirror_fill_longer_than_the_side(pictures):
    """A 64-pixel patch of the 40 x 56 picture: rows 40..63 mirror rows 39..16, columns 56..63 columns 55..48."""
    ds = dataset(pictures, "vary64")
    k = next(i for i, r in enumerate(ds.patchs_data) if r[3] == 0)
    _, clean = ds[k]
    want = patch_ref.clean_patch(pictures[2][0], 0, 0, 64, 64).astype(np.float32) / np.float32(255.0)
    assert np.array_equal(clean.numpy(), want)


def test_random_permute_is_a_function_of_its_seed(pictures):
    a, b = dataset(pictures, "aug16"), dataset(pictures, "aug16")
    first = plan_of(a)
    b[0], b[1]                                   # the host stream's position must not matter
    a.random_permute(seed=2024 + 3)
    b.random_permute(seed=2024 + 1)
    b.random_permute(seed=2024 + 3)
    assert a.epoch == b.epoch == 3
    assert np.array_equal(plan_of(a), plan_of(b))
    assert not np.array_equal(plan_of(a), first)
    all_rows = a.patchs_data_all
    ind = np.random.RandomState(2027).permutation(len(all_rows))[:a.max_num_patchs]
    assert a.patchs_data == [all_rows[i] for i in ind]


def test_registered_and_int_patch_size(pictures):
    assert training.DATASETS["ImageSuperResolution"] is training.ImageSuperResolution
    ds = dataset(pictures, "aug16", patch_size=16)
    assert ds.patch_size == (16, 16) and np.array_equal(plan_of(ds), plan_of(dataset(pictures, "aug16")))


def test_value_errors(pictures, tmp_path):
    with pytest.raises(ValueError, match="square"):
        dataset(pictures, "aug16", patch_size=(16, 32))
    dataset(pictures, "vary64", patch_size=(16, 32))           # fine without the augmentation
    ds = dataset(pictures, "aug16", n_channels=1)
    with pytest.raises(ValueError, match=r"pic\d\.png"):
        ds[0]
    grey_csv, _ = patch_ref.write_pictures(str(tmp_path), shapes=((20, 24),), c=1)
    grey = training.ImageSuperResolution(csv_path=grey_csv, root_folder=str(tmp_path),
                                         dist_mode="addictive_noise", lambda_noise=25.0, patch_size=16)
    with pytest.raises(ValueError, match=r"pic0\.png"):
        grey[0]


def test_device_loader_draws_are_a_function_of_seed_and_epoch(pictures):
    """DevicePatchLoader's per-epoch modes and levels (no GPU: the draws only)."""
    ds = dataset(pictures, "aug16")
    sampler = training.ResumeableSampler(ds, 4)
    loader = training.DevicePatchLoader(ds, sampler, 4)
    assert loader.channels_first and len(loader) == 10
    m0, s0 = loader.epoch_draws(0)
    m1, _ = loader.epoch_draws(1)
    rs = np.random.RandomState((2204 * 1000003 + 0) % 2 ** 32)
    assert np.array_equal(m0, rs.randint(0, 8, len(ds))) and set(m0.tolist()) == set(range(8))
    assert not np.array_equal(m0, m1)
    assert s0.dtype == np.float32 and np.array_equal(s0, np.full(len(ds), np.float32(25.0 / 255.0)))
    dv = dataset(pictures, "vary64")
    lv = training.DevicePatchLoader(dv, training.ResumeableSampler(dv, 4), 4, drop_last=True)
    assert len(lv) == 7
    mv, sv = lv.epoch_draws(2)
    rs = np.random.RandomState((77 * 1000003 + 2) % 2 ** 32)
    want = rs.choice([15.0, 25.0, 50.0], p=[0.3, 0.4, 0.3], size=len(dv))
    assert not mv.any() and np.array_equal(sv, (want / 255.0).astype(np.float32))


def test_loader_packs_in_chunks_checks_once_and_shares_explicitly(pictures, monkeypatch):
    """DevicePatchLoader without a GPU (the launch stubbed out): the arena holds the files, staged in several
    chunks; the pack is checked when it is made, not per batch; loaders share an arena only through the dict
    they are given; the tables of a batch are the plan's rows."""
    import torch
    from irdu_amd import kernels as K
    calls, sent = [], []
    check = K._check_pack
    monkeypatch.setattr(K, "_check_pack", lambda *a, **k: calls.append(1) or check(*a, **k))
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    monkeypatch.setattr(K, "_patch_batch", lambda pack, n_img, c, table, ids, sigma, *rest: sent.append(
        (table.numpy().copy(), ids.numpy().copy(), sigma.numpy().copy(), rest)) or (None, None))
    monkeypatch.setattr(training.DevicePatchLoader, "CHUNK_BYTES", 20000)      # pictures 0..2 are 6.7, 21 and 58 KB
    ds = dataset(pictures, "aug16")
    shared = {}
    cpu = torch.device("cpu")
    a = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, 4), 4, device=cpu, shared=shared)
    pack = a.prepare()
    assert a.prepare() is pack and len(pack) == 4 and pack.arena.dtype == torch.uint8
    for i, pic in enumerate(pictures[2]):
        assert np.array_equal(pack.image(i).numpy(), pic)
    ds.random_permute(2024 + 1)
    got = list(a)
    assert len(got) == 10 and len(calls) == 1, "the pack is checked once, not per batch"
    modes, sigma = a.epoch_draws(1)
    rows = np.concatenate([s[0] for s in sent])
    assert np.array_equal(rows[:, :3], plan_of(ds)[:, :3]) and np.array_equal(rows[:, 3], modes)
    assert np.array_equal(np.concatenate([s[1] for s in sent]), (1 << 32) | np.arange(40))
    assert np.array_equal(np.concatenate([s[2] for s in sent]), sigma) and sent[0][3] == (2204, 16, 16)
    b = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, 4), 4, device=cpu, shared=shared)
    c = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, 4), 4, device=cpu)
    assert b.prepare() is pack and c.prepare() is not pack and len(shared) == 1
    assert not hasattr(training.DevicePatchLoader, "_PACKS")


def test_stages_share_one_arena_dict_per_build(pictures, tmp_path):
    folder, csv_path, _ = pictures
    stage = lambda size: dict(type="ImageSuperResolution", device_resident=True, dataloader_args=dict(batch_size=2),
                              dataset_args=dict(csv_path=csv_path, root_folder=folder, dist_mode="addictive_noise",
                                                lambda_noise=25.0, patch_size=size, max_num_patchs=8))
    conf = dict(datasets=dict(train=[stage(16), stage(32)]))
    first, second = training.build_train_stages(conf), training.build_train_stages(conf)
    assert all(isinstance(st.loader, training.DevicePatchLoader) for st in first)
    assert first[0].loader.shared is first[1].loader.shared is not second[0].loader.shared
    with pytest.raises(ValueError, match="device_resident"):
        training.build_train_stages(dict(datasets=dict(train=dict(
            type="SyntheticNoisyPatches", device_resident=True, dataset_args={}, dataloader_args={}))))


def test_loader_refuses_a_picture_the_csv_misdescribes(pictures, tmp_path, monkeypatch):
    import torch
    from irdu_amd import kernels as K
    monkeypatch.setattr(K, "_check_placed", lambda *a: None)
    csv_path, _ = patch_ref.write_pictures(str(tmp_path), shapes=((20, 24), (18, 30)))
    text = open(csv_path).read().replace("1,pic1.png,18,30,3", "1,pic1.png,30,18,3")
    open(csv_path, "w").write(text)
    ds = training.ImageSuperResolution(csv_path=csv_path, root_folder=str(tmp_path), dist_mode="addictive_noise",
                                       lambda_noise=25.0, patch_size=16, max_num_patchs=4)
    loader = training.DevicePatchLoader(ds, training.ResumeableSampler(ds, 2), 2, device=torch.device("cpu"))
    with pytest.raises(ValueError, match=r"pic1\.png.*csv"):
        loader.prepare()
