"""The blur of include/grr.h without a GPU: the two forms of the oracle tests/blur_ref.py against each other, the numpy
path training.blur_degrade_u8 against the oracle bit for bit, the quantiser's properties, the kernel builders, the
refusals of parse_blur_spec, and the host path of the GaussianMotionDeblurring dataset.

``KERNELS`` and ``SHAPES`` are also what tests/test_gpu_blur.py runs the device kernel on."""
import logging
import os

import numpy as np
import pytest

from tests import blur_ref as ref, patch_ref

# sides chosen for a kernel that stages a 16 x 64 tile with a halo of up to 15 and gives each lane 4 bytes of a row:
# below, at and above a tile in both directions, more than one tile, pictures narrower than a kernel's radius
HEIGHTS = (1, 2, 3, 7, 15, 16, 17, 31, 33)
WIDTHS = (1, 2, 5, 63, 64, 65, 129)
SHAPES = [(h, w) for h in HEIGHTS for w in WIDTHS]
CHANNELS = (1, 3, 4)


def _kernels():
    rs = np.random.RandomState(17)
    shift = ref.lone_tap(3, 3, 0, 2)            # the lone tap at (row 0, column 2): out[y, x] = src[y + 1, x - 1]
    distinct = ref.quantise(np.arange(1, 16, dtype=np.float64).reshape(3, 5) ** 1.5)
    return {"identity": ref.lone_tap(1, 1, 0, 0), "shift": shift, "distinct3x5": distinct,
            "row1x31": ref.random_table(rs, 1, 31), "column31x1": ref.random_table(rs, 31, 1),
            "random31x31": ref.random_table(rs, 31, 31), "gaussian:25:1.6": None, "motion:15:30": None}


KERNELS = _kernels()


def table_of(name):
    """The int32 table of a kernel of KERNELS: the oracle's own, or the library's builder for the two specs."""
    if KERNELS[name] is not None:
        return KERNELS[name]
    from irdu_amd import training as T
    return np.array(T.parse_blur_spec(name).table)


def picture(seed, h, w, c):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, c)).astype(np.uint8)


@pytest.mark.parametrize("boundary", ref.BOUNDARIES)
def test_the_two_oracle_forms_agree_byte_for_byte(boundary):
    rs = np.random.RandomState(3)
    for (h, w, c) in ((1, 1, 1), (2, 2, 3), (1, 5, 4), (3, 2, 1), (5, 7, 3), (2, 9, 2)):
        a = picture(h * 31 + w, h, w, c)
        for table in (ref.lone_tap(1, 1, 0, 0), ref.lone_tap(3, 3, 0, 2), ref.lone_tap(3, 5, 2, 0),
                      ref.random_table(rs, 3, 5), ref.random_table(rs, 7, 1), ref.random_table(rs, 1, 9),
                      ref.random_table(rs, 11, 13)):
            assert np.array_equal(ref.blur(a, table, boundary), ref.blur_loops(a, table, boundary)), (h, w, c, table.shape)
    # the index rule alone, far outside a side shorter than any radius (several folds)
    for n in (1, 2, 3, 5):
        assert [ref.index_of(t, n, boundary) for t in range(-40, 40)] == ref.indices(-40, 40, n, boundary).tolist()


def test_the_oracle_on_values_computed_by_hand():
    a = np.arange(12, dtype=np.uint8).reshape(3, 4, 1) * 10
    # the lone tap at (0, 2) of a 3 x 3 table: out[y, x] = src[y + 1, x - 1] -- a correlation would give src[y - 1, x + 1]
    got = ref.blur(a, ref.lone_tap(3, 3, 0, 2), "wrap")[:, :, 0]
    assert got.tolist() == np.roll(a[:, :, 0], (-1, 1), axis=(0, 1)).tolist()
    got = ref.blur(a, ref.lone_tap(3, 3, 0, 2), "replicate")[:, :, 0]
    assert got.tolist() == [[40, 40, 50, 60], [80, 80, 90, 100], [80, 80, 90, 100]]
    got = ref.blur(a, ref.lone_tap(3, 3, 0, 2), "reflect")[:, :, 0]
    assert got.tolist() == [[50, 40, 50, 60], [90, 80, 90, 100], [50, 40, 50, 60]]
    half = np.array([[32768, 32768, 0]], np.int32)          # taps at dx = +1 and 0 of the flipped kernel: src[x + 1], src[x]
    got = ref.blur(np.array([[[0], [255], [10]]], np.uint8), half, "replicate")[0, :, 0]
    assert got.tolist() == [(0 + 255 + 1) >> 1, (255 + 10 + 1) >> 1, 10]


@pytest.mark.parametrize("boundary", ref.BOUNDARIES)
def test_the_numpy_degradation_is_the_oracle_bit_for_bit(boundary):
    from irdu_amd import training as T
    for n, name in enumerate(KERNELS):
        table = table_of(name)
        for (h, w) in ((1, 1), (2, 2), (7, 5), (17, 65), (33, 20)):
            c = CHANNELS[(n + h) % 3]
            a = picture(n * 100 + h, h, w, c)
            got = T.blur_degrade_u8(a, table, boundary)
            assert got.dtype == np.uint8 and np.array_equal(got, ref.blur(a, table, boundary)), (name, h, w, c)
        flat = picture(n, 9, 11, 1)
        assert np.array_equal(T.blur_degrade_u8(flat[:, :, 0], table, T.BLUR_BOUNDARIES.index(boundary)),
                              ref.blur(flat, table, boundary)[:, :, 0])
    for value in (0, 255):          # a constant picture gives itself back
        a = np.full((9, 12, 3), value, np.uint8)
        assert np.array_equal(T.blur_degrade_u8(a, "gaussian:25:1.6", boundary), a)


def test_quantiser_properties():
    from irdu_amd import training as T
    rs = np.random.RandomState(23)
    for k in (rs.rand(5, 7), rs.rand(31, 31) ** 8, np.ones((3, 3)), np.ones((1, 1)) * 0.3, rs.rand(1, 31), np.eye(5),
              rs.randint(0, 9, (7, 3))):
        w = T.quantise_blur_kernel(k)
        assert w.dtype == np.int32 and w.shape == k.shape and int(w.sum()) == 65536 and w.min() >= 0
        assert np.array_equal(w, ref.quantise(k))
        assert np.abs(w - np.asarray(k, np.float64) / np.asarray(k, np.float64).sum() * 65536).max() < 1
    # an exact table passes through, integer or float
    exact = ref.random_table(rs, 7, 9)
    assert np.array_equal(T.quantise_blur_kernel(exact), exact) and np.array_equal(T.quantise_blur_kernel(exact * 1.0), exact)
    assert np.array_equal(T.quantise_blur_kernel(ref.lone_tap(3, 3, 2, 1)), ref.lone_tap(3, 3, 2, 1))
    # ties go to the lower flat index: 65536 = 9 * 7281 + 7, so the first 7 taps of a 3 x 3 box get the units left
    assert T.quantise_blur_kernel(np.ones((3, 3))).ravel().tolist() == [7282] * 7 + [7281] * 2
    assert T.box_kernel(3).table.ravel().tolist() == [7282] * 7 + [7281] * 2
    # so a box and a gaussian are symmetric up to the one unit the tie rule hands out, and exactly where no unit is left
    for k in [T.box_kernel(s) for s in (1, 3, 5, 31)] + [T.gaussian_kernel(s, g) for s, g in ((3, 0.5), (9, 1.6), (25, 1.6), (31, 4.0))]:
        w = k.table.astype(np.int64)
        assert int(w.sum()) == 65536 and w.min() >= 0 and k.kh == k.kw == w.shape[0]
        for other in (w.T, w[::-1], w[:, ::-1]):
            assert np.abs(w - other).max() <= 1, k.spec
    assert T.box_kernel(1).table.tolist() == [[65536]]
    real = np.exp(-(np.arange(-4, 5)[:, None] ** 2 + np.arange(-4, 5)[None, :] ** 2) / (2 * 1.6 ** 2))
    assert np.array_equal(T.gaussian_kernel(9, 1.6).table, ref.quantise(real))
    assert np.array_equal(T.parse_blur_spec("gaussian:9:1.6").table, T.gaussian_kernel(9, 1.6).table)
    for bad in (np.zeros((3, 3)), -np.ones((3, 3)), np.ones((2, 3)), np.ones((3, 33)), np.ones(3), np.full((3, 3), np.nan),
                np.full((3, 3), np.inf), np.ones((3, 3), dtype=complex)):
        with pytest.raises(ValueError, match="quantise_blur_kernel"):
            T.quantise_blur_kernel(bad)


def test_motion_kernels():
    from irdu_amd import training as T
    for length in (1, 2, 5, 8, 15, 31):
        k0, k90 = T.motion_kernel(length, 0), T.motion_kernel(length, 90)
        side = length if length % 2 else length + 1
        assert k0.table.shape == (side, side) and int(k0.table.sum()) == 65536
        assert np.array_equal(k0.table.T, k90.table), length              # transposes of each other
        assert np.count_nonzero(k0.table[side // 2]) == np.count_nonzero(k0.table)      # one row
        assert np.array_equal(T.motion_kernel(length, 180).table, k0.table)
        assert np.array_equal(T.motion_kernel(length, -90).table, k90.table)
    assert T.motion_kernel(1, 77).table.tolist() == [[65536]]
    # counter-clockwise with y down: at 30 degrees the line rises to the right
    w = T.motion_kernel(15, 30).table
    assert w[:7, 8:].sum() > 20000 and w[8:, :7].sum() > 20000 and w[:7, :7].sum() == 0 and w[8:, 8:].sum() == 0
    assert w[7, 7] > 0 and T.motion_kernel(15, 30).spec == "motion:15:30"
    assert "fspecial" in T.motion_kernel.__doc__
    assert np.array_equal(T.parse_blur_spec("motion:15:30").table, w)


def test_specs_and_their_refusals(tmp_path):
    from irdu_amd import training as T
    k = T.parse_blur_spec("box:5")
    assert isinstance(k, T.BlurKernel) and (k.kh, k.kw, k.spec) == (5, 5, "box:5") and T.parse_blur_spec(k) is k
    assert k == T.box_kernel(5) and hash(k) == hash(T.box_kernel(5)) and k != T.box_kernel(3)
    assert len({k, T.box_kernel(5), T.parse_blur_spec(np.ones((5, 5)))}) == 1          # equal tables are equal kernels
    with pytest.raises(AttributeError):
        k.kh = 3
    with pytest.raises(ValueError):
        k.table[0, 0] = 1           # read-only
    np.save(str(tmp_path / "psf.npy"), np.random.RandomState(1).rand(5, 3))
    np.save(str(tmp_path / "even.npy"), np.ones((4, 3)))
    np.save(str(tmp_path / "big.npy"), np.ones((33, 3)))
    np.save(str(tmp_path / "ints.npy"), ref.lone_tap(3, 3, 1, 1))
    f = T.parse_blur_spec(f"file:{tmp_path / 'psf.npy'}")
    assert (f.kh, f.kw) == (5, 3) and np.array_equal(f.table, ref.quantise(np.random.RandomState(1).rand(5, 3)))
    assert np.array_equal(T.parse_blur_spec(f"file:{tmp_path / 'ints.npy'}").table, ref.lone_tap(3, 3, 1, 1))
    array = T.parse_blur_spec(np.random.RandomState(2).rand(3, 7))
    assert array.spec.startswith("array:3x7:") and (array.kh, array.kw) == (3, 7)
    bad = ["", "gauss:5:1", "gaussian", "gaussian:5", "gaussian:4:1.0", "gaussian:33:1.0", "gaussian:5:0", "gaussian:5:-1",
           "gaussian:5:nan", "gaussian:5.0:1", "gaussian:5:1:2", "box", "box:2", "box:0", "box:33", "box:3:3", "box:x",
           "motion:0:10", "motion:32:10", "motion:5", "motion:5:inf", "motion:5.5:10", "file:psf.txt",
           f"file:{tmp_path / 'missing.npy'}", f"file:{tmp_path / 'even.npy'}", f"file:{tmp_path / 'big.npy'}",
           5, None, 1.5, [[1]], np.ones((2, 2)), np.ones(3)]
    for spec in bad:
        with pytest.raises(ValueError):
            T.parse_blur_spec(spec)
    for spec in bad[:6]:
        with pytest.raises(ValueError, match="blur_degrade_u8|parse_blur_spec|gaussian_kernel"):
            T.blur_degrade_u8(np.zeros((4, 4, 3), np.uint8), spec)
    for boundary in ("circular", 3, -1, True, None):
        with pytest.raises(ValueError, match="blur_degrade_u8: the boundary"):
            T.blur_degrade_u8(np.zeros((4, 4, 3), np.uint8), "box:3", boundary)
    for a in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 5), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError, match="blur_degrade_u8: expected a uint8"):
            T.blur_degrade_u8(a, "box:3")


def test_the_host_dataset_draws_one_kernel_per_file_and_cuts_both_patches_alike(tmp_path):
    from irdu_amd import training as T
    shapes_ = ((70, 90), (33, 47), (130, 64), (40, 25))
    csv_path, pics = patch_ref.write_pictures(str(tmp_path), shapes_)
    log = logging.getLogger("test")
    common = dict(csv_path=csv_path, root_folder=str(tmp_path), patch_size=32, max_num_patchs=9, seed=5, logger=log)
    specs = [["gaussian:9:1.6", "motion:15:30", "box:3", KERNELS["distinct3x5"]], [0.1, 0.2, 0.3, 0.4]]
    for kernel, boundary in (("motion:7:45", "wrap"), (specs, "reflect")):
        ds = T.GaussianMotionDeblurring(kernel=kernel, boundary=boundary, **common)
        assert isinstance(ds, T.ImageSuperResolution) and T.DATASETS["GaussianMotionDeblurring"] is T.GaussianMotionDeblurring
        assert ds.dist_mode == "none" and ds.boundary == boundary and len(ds) == 9
        if isinstance(kernel, str):
            assert ds.kernels == [T.parse_blur_spec(kernel)] * 4
        else:       # one draw per file, in file order, from RandomState(seed): a function of (seed, file)
            want = np.random.RandomState(5).choice(4, p=specs[1], size=4)
            assert ds.kernels == [T.parse_blur_spec(specs[0][int(k)]) for k in want] and len(set(ds.kernels)) > 1
            again = T.GaussianMotionDeblurring(kernel=kernel, boundary=boundary, **dict(common, max_num_patchs=3))
            assert again.kernels == ds.kernels
            other = T.GaussianMotionDeblurring(kernel=kernel, boundary=boundary, **dict(common, seed=6))
            assert other.kernels != ds.kernels
        parent = T.ImageSuperResolution(dist_mode="addictive_noise", lambda_noise=5.0, **common)
        assert ds.patchs_data == parent.patchs_data                # the plan is the parent's
        degraded = [ref.blur(p, np.array(k.table), boundary) for p, k in zip(pics, ds.kernels)]
        for idx in range(len(ds)):
            row, col, pad, img = ds.patchs_data[idx]
            inp, tgt = ds[idx]
            assert inp.shape == tgt.shape == (32, 32, 3) and inp.dtype == tgt.dtype
            want_in = patch_ref.clean_patch(degraded[img], row, col, 32, 32).astype(np.float32) / 255.0
            want_tgt = patch_ref.clean_patch(pics[img], row, col, 32, 32).astype(np.float32) / 255.0
            assert np.array_equal(inp.numpy(), want_in) and np.array_equal(tgt.numpy(), want_tgt)
        assert len(ds._degraded) <= ds.CACHE
        key = ds.synthetic_key([0, 2])
        assert key == ("blur", (ds.kernels[0], ds.kernels[2]), boundary) and hash(key) == hash(ds.synthetic_key([0, 2]))
    assert T.GaussianMotionDeblurring(kernel="box:3", **common).boundary == "wrap"
    noisy = T.GaussianMotionDeblurring(kernel="box:3", dist_mode="addictive_noise", lambda_noise=10.0, **common)
    plain = T.GaussianMotionDeblurring(kernel="box:3", **common)
    (n_in, n_tgt), (p_in, p_tgt) = noisy[0], plain[0]
    assert np.array_equal(n_tgt.numpy(), p_tgt.numpy()) and not np.array_equal(n_in.numpy(), p_in.numpy())
    too_many = [["box:3"] * 17, [1 / 17] * 17]
    for bad in ("gauss:3:1", 0, None, [["box:3", "box:5"], [1.0]], [["box:3", "box:4"], [0.5, 0.5]], [[], []],
                ["box:3", "box:5", "box:7"], ["box:3", [1.0]], too_many):
        with pytest.raises(ValueError):
            T.GaussianMotionDeblurring(kernel=bad, **common)
    for bad in ("circular", 0, True, None):
        with pytest.raises(ValueError, match="boundary"):
            T.GaussianMotionDeblurring(kernel="box:3", boundary=bad, **common)
    with pytest.raises(ValueError, match="n_channels"):
        T.GaussianMotionDeblurring(kernel="box:3", n_channels=4, **common)


def test_the_example_yaml_names_registered_types():
    from irdu_amd import training as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = T.parse(os.path.join(root, "experiment_conf", "deblur_gauss_example.yaml"))
    stages = T.train_stage_confs(conf)
    assert stages and all(st["type"] == "GaussianMotionDeblurring" and st["device_resident"] for st in stages)
    for st in stages:
        assert st["type"] in T.DATASETS and T.parse_blur_spec(st["dataset_args"]["kernel"]).kh == 25
    assert len({st["dataset_args"]["csv_path"] for st in stages}) == 1          # one csv: the stages share the arenas
    val = conf["datasets"]["val"]
    assert val["type"] == "TestImagesCSV" and T.parse_blur_spec(val["blur"]).kh == 25 and conf["train"]["val_every"] > 0
    assert "sigma" not in val and val["noise_sigma"] > 0
