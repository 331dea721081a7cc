"""PSNR and SSIM on the Y channel on the GPU (csrc/metric_ops.hip through kernels.u8_luma_sse / u8_luma_ssim and
their _images forms, restore.psnr_y_u8 / ssim_y_u8, the "_y" metrics of evaluate_metrics / evaluate_pairs /
validate_pairs and restore.py --y-channel) against the numpy restatement (tests/luma_ref.py).

The SSE is an integer and is compared for equality.  The bound of the SSIM against the restatement is 2^-32 on the
mean, as for the RGB SSIM: each value is quantised to the nearest multiple of 2^-32, so it moves by at most half a
step, 2^-33, and so does the mean; the float64 rounding of a value in either evaluation order is below 3e-13
(tests/test_luma_ref.py measures it on these inputs), far inside the other half."""
import os
import re

import numpy as np
import pytest
import torch

from tests import luma_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUND = 2.0 ** -32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def irdu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    return irdu_amd


def smooth(h, w, c):
    yy, xx = np.mgrid[0:h, 0:w]
    v = 127.5 + 90.0 * np.sin(xx / 7.0)[..., None] * np.cos(yy / 5.0)[..., None] + 10.0 * np.arange(c)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def pair(kind, shape, seed=5):
    """The three input kinds of tests/test_gpu_ssim.py: a smooth pattern against itself plus N(0, 25) noise; random a
    against 255 - a; 0 against 255."""
    h, w, c = shape
    rs = np.random.RandomState(seed + h * 131 + w * 7 + c)
    if kind == "noisy":
        a = smooth(h, w, c)
        return a, np.clip(np.rint(a + rs.normal(0, 25.0, a.shape)), 0, 255).astype(np.uint8)
    if kind == "negated":
        a = rs.randint(0, 256, shape).astype(np.uint8)
        return a, (255 - a).astype(np.uint8)
    assert kind == "extremes"
    return np.zeros(shape, dtype=np.uint8), np.full(shape, 255, dtype=np.uint8)


def dev_at(img, off=0):
    """A contiguous device copy of img that starts ``off`` bytes into a fresh allocation."""
    buf = torch.zeros(off + img.size + 16, dtype=torch.uint8, device=DEV)
    view = buf[off:off + img.size].view(img.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off
    return view


def count(shape):
    return (shape[0] - 10) * (shape[1] - 10)


KINDS = ["noisy", "negated", "extremes"]
LARGE = (300, 700, 3)       # several tiles both ways


def sse_shapes(K):
    """The fixed shapes, then one pixel count below, at and above what a lane and what a workgroup take per step."""
    group, lane = K.LUMA_SSE_BLOCK
    shapes = [(1, 1, 3), (1, 2, 3), (3, 5, 3), (11, 11, 3), (37, 53, 3), (100, 140, 3), LARGE]
    shapes += [(1, lane + d, 3) for d in (-1, 0, 1)]
    shapes += [(1, group // lane + d, 3) for d in (-1, 0, 1)]         # the lanes of a workgroup
    shapes += [(1, group + d, 3) for d in (-1, 0, 1)]
    shapes += [(3, group + 1, 3)]                                     # several workgroups, the last one partial
    return shapes


def ssim_shapes(K):
    """The fixed shapes, then rows R + 10 + d and pixel columns Cc + 10 + d of the kernel's tile, d in -1, 0, 1."""
    rows, cols = K.LUMA_SSIM_TILE
    shapes = [(11, 11, 3), (11, 29, 3), (29, 11, 3), (37, 53, 3), (100, 140, 3), LARGE]
    shapes += [(rows + 10 + d, 13, 3) for d in (-1, 0, 1)]
    shapes += [(12, cols + 10 + d, 3) for d in (-1, 0, 1)]
    shapes += [(rows + 10 + d, cols + 10 + d, 3) for d in (-1, 1)]
    return shapes


# ---- 1. the SSE, as integer equality with the restatement
@pytest.mark.parametrize("kind", KINDS)
def test_sse_is_the_restatements_integer(irdu, kind):
    K, restore = irdu.kernels, irdu.restore
    for shape in sse_shapes(K):
        a, b = pair(kind, shape)
        want = luma_ref.luma_sse(a, b)
        got = K.u8_luma_sse(dev_at(a), dev_at(b))
        assert got == want, (kind, shape, got, want)
        assert want > 0 or kind == "noisy"
        assert restore.psnr_y_u8(a, b) == luma_ref.psnr_y(a, b) == restore.psnr_y_u8(torch.from_numpy(a).to(DEV), b)
        assert restore.psnr_y_u8(a, a.copy()) == float("inf")


def test_sse_beyond_64_bits(irdu):
    """0 against 255 over 80 x 80 pixels: 6400 x 55845000^2 > 2^64, which one 64-bit sum gets wrong."""
    K = irdu.kernels
    a, b = pair("extremes", (80, 80, 3))
    want = 6400 * 55845000 ** 2
    assert want > 1 << 64 and luma_ref.luma_sse(a, b) == want
    assert K.u8_luma_sse(dev_at(a), dev_at(b)) == want
    assert irdu.psnr_y_u8(a, b) == luma_ref.psnr_y(a, b)
    assert abs(irdu.psnr_y_u8(a, b) - 20.0 * np.log10(255.0 / 219.0)) <= 1e-12


def test_sse_where_the_workgroups_stride_over_the_image(irdu):
    """More pixels than LUMA_SSE_MAX_BLOCKS workgroups take in one step each."""
    K = irdu.kernels
    group, _ = K.LUMA_SSE_BLOCK
    shape = (K.LUMA_SSE_MAX_BLOCKS + 1, group + 1, 3)
    assert shape[0] * shape[1] > K.LUMA_SSE_MAX_BLOCKS * group
    a, b = pair("noisy", shape)
    assert K.u8_luma_sse(dev_at(a), dev_at(b, 5)) == luma_ref.luma_sse(a, b)


# ---- 2. coefficients and channel order
def test_one_raised_channel_gives_its_coefficient_squared(irdu):
    K = irdu.kernels
    rs = np.random.RandomState(3)
    a = rs.randint(0, 200, (37, 53, 3)).astype(np.uint8)
    assert K.LUMA_WEIGHTS == (65481, 128553, 24966) and K.LUMA_SCALE == 255000
    for ch, coeff in enumerate((65481, 128553, 24966)):
        d = rs.randint(0, 56, a.shape[:2])
        b = a.copy()
        b[:, :, ch] = (a[:, :, ch].astype(np.int64) + d).astype(np.uint8)
        want = coeff ** 2 * int((d.astype(np.int64) ** 2).sum())
        assert K.u8_luma_sse(dev_at(a), dev_at(b)) == want == K.u8_luma_sse(dev_at(b), dev_at(a)), ch


def test_grey_pictures_give_219000_squared_times_the_plane_sse(irdu):
    K = irdu.kernels
    rs = np.random.RandomState(4)
    pa, pb = (rs.randint(0, 256, (45, 61)).astype(np.uint8) for _ in range(2))
    a, b = (np.repeat(p[:, :, None], 3, axis=2) for p in (pa, pb))
    assert K.u8_luma_sse(dev_at(a), dev_at(b)) == 219000 ** 2 * K.u8_sse(dev_at(pa), dev_at(pb))


# ---- 3. the SSIM against the restatement
@pytest.mark.parametrize("kind", KINDS)
def test_ssim_mean_is_within_one_step_of_the_restatement(irdu, kind):
    K, restore = irdu.kernels, irdu.restore
    assert K.luma_ssim_count(11, 11) == 1
    worst = 0.0
    for shape in ssim_shapes(K):
        a, b = pair(kind, shape)
        ref = luma_ref.ssim_y(a, b)
        q = K.u8_luma_ssim(dev_at(a), dev_at(b))
        got = restore._ssim(q, count(shape))
        err = abs(got - ref)
        worst = max(worst, err)
        print(f"{kind} {shape}: ref {ref:.12f} got {got:.12f} err {err:.3e}")
        assert err <= BOUND, (kind, shape, ref, got)
        assert restore.ssim_y_u8(a, b) == got == restore.ssim_y_u8(torch.from_numpy(a).to(DEV), b)
        if kind == "noisy" and min(shape[:2]) > 11:
            assert 0.2 < ref < 0.8
        if kind == "negated" and count(shape) > 100:
            assert ref < -0.5 and q < 0
        if kind == "extremes":
            # every position has the one value (2 x 16 x 235 + C1) / (16^2 + 235^2 + C1), so the mean carries that
            # value's whole quantisation error (here 6.2e-11 of the 2^-33 allowed) and is compared to 1e-12 with the
            # restatement's quantised mean, not with its float64 mean
            quantised = luma_ref.quantised_sum_y(a, b) / (2.0 ** 32 * count(shape))
            assert abs(ref - 0.135643201818) <= 1e-12 and abs(got - quantised) <= 1e-12
    print(f"{kind}: worst {worst:.3e} of {BOUND:.3e}")


def test_one_changed_byte_in_a_flat_image_needs_a_float64_luma(irdu):
    """200 against 200 with one G byte at 201: a luma held in float32 misses the mean by 1.6e-9, seven times the
    bound."""
    a = np.full((20, 20, 3), 200, dtype=np.uint8)
    b = a.copy()
    b[10, 10, 1] = 201
    ref = luma_ref.ssim_y(a, b)
    got = irdu.ssim_y_u8(a, b)
    print(f"flat: ref {ref:.12f} got {got:.12f} err {abs(got - ref):.3e}")
    assert abs(ref - 0.99995820398) <= 1e-10
    assert abs(got - ref) <= BOUND
    assert abs(irdu.ssim_y_u8(b, a) - ref) <= BOUND


# ---- 4. exactness, all as integer equality
PACK_SIZES = [(13, 15), (37, 53), (11, 11), (45, 271), (75, 33)]     # odd sizes: later images start at odd bytes


def test_identical_images_sum_to_n_times_one_and_zero(irdu):
    K = irdu.kernels
    for shape in [s for s in ssim_shapes(K) if s != LARGE]:
        for kind in ("noisy", "negated"):
            a, _ = pair(kind, shape)
            n = count(shape)
            assert K.u8_luma_ssim(dev_at(a), dev_at(a)) == n * K.SSIM_ONE == n << 32, (shape, kind)
            assert K.u8_luma_ssim(dev_at(a, 1), dev_at(a, 16 + 3)) == n << 32            # views off the 16-byte grid
            assert K.u8_luma_sse(dev_at(a, 1), dev_at(a, 16 + 3)) == 0
            assert irdu.ssim_y_u8(a, a.copy()) == 1.0


def test_the_same_call_twice_gives_the_same_integers(irdu):
    K = irdu.kernels
    a, b = pair("noisy", LARGE)
    ta, tb = dev_at(a), dev_at(b)
    for fn in (K.u8_luma_ssim, K.u8_luma_sse):
        first = fn(ta, tb)
        assert fn(ta, tb) == first
        assert fn(tb, ta) == first      # symmetric in exact arithmetic and here: x y and y x round alike


def test_every_image_of_a_pack_equals_the_single_image_call(irdu):
    K = irdu.kernels
    pairs = [pair("noisy" if i % 2 == 0 else "negated", (h, w, 3), seed=i) for i, (h, w) in enumerate(PACK_SIZES)]
    pa = irdu.pack_images([a for a, _ in pairs], DEV)
    pb = irdu.pack_images([b for _, b in pairs], DEV)
    assert any(off % 2 == 1 for off, _, _ in pa.host_table) and any(off % 4 != 0 for off, _, _ in pa.host_table)
    order = [3, 0, 4, 2, 1]
    ra = irdu.pack_images([pairs[i][0] for i in order], DEV)
    rb = irdu.pack_images([pairs[i][1] for i in order], DEV)
    one = (irdu.pack_images([pairs[1][0]], DEV), irdu.pack_images([pairs[1][1]], DEV))
    for single, packed in ((K.u8_luma_ssim, K.u8_luma_ssim_images), (K.u8_luma_sse, K.u8_luma_sse_images)):
        singles = [single(dev_at(a), dev_at(b)) for a, b in pairs]
        got = packed(pa, pb)
        assert got == singles
        assert packed(pa, pb) == got
        # a pack of one and a pack in another order: what else the arena holds changes nothing
        assert packed(ra, rb) == [singles[i] for i in order]
        assert packed(*one) == [singles[1]]
    assert all(K.u8_luma_sse(dev_at(a), dev_at(b)) == luma_ref.luma_sse(a, b) for a, b in pairs)


def test_a_pack_whose_images_start_at_offsets_not_divisible_by_three(irdu):
    """restore.ImagePack rows of the arena entry points, laid out by hand with gaps of 1 and 2 bytes between
    images whose sizes are multiples of 3."""
    from types import SimpleNamespace
    K = irdu.kernels
    pairs = [pair("noisy", (h, w, 3), seed=i) for i, (h, w) in enumerate(PACK_SIZES[:4])]
    rows, end = [], 0
    for gap, (a, _) in zip((1, 1, 2, 1), pairs):
        rows.append((end + gap, a.shape[0], a.shape[1]))
        end += gap + a.size
    assert all(off % 3 != 0 for off, _, _ in rows)
    arenas = []
    for side in (0, 1):
        arena = np.full(end + 7, 77, dtype=np.uint8)
        for (off, _, _), p in zip(rows, pairs):
            arena[off:off + p[side].size] = p[side].reshape(-1)
        arenas.append(torch.from_numpy(arena).to(DEV))
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    packs = [SimpleNamespace(arena=arena, table=table, host_table=tuple(rows), c=3) for arena in arenas]
    assert K.u8_luma_sse_images(*packs) == [luma_ref.luma_sse(a, b) for a, b in pairs]
    assert K.u8_luma_ssim_images(*packs) == [K.u8_luma_ssim(dev_at(a), dev_at(b)) for a, b in pairs]


def test_byte_offsets_of_the_two_images_change_nothing(irdu):
    K = irdu.kernels
    for shape in [(37, 53, 3), (45, 271, 3)]:
        a, b = pair("noisy", shape)
        for fn in (K.u8_luma_ssim, K.u8_luma_sse):
            want = fn(dev_at(a), dev_at(b))
            for oa, ob in [(1, 0), (0, 7), (3, 5), (15, 17), (16, 2)]:
                assert fn(dev_at(a, oa), dev_at(b, ob)) == want, (shape, oa, ob)


def test_sums_are_additive_over_rows_and_columns(irdu):
    """The valid pixels of rows [0, k + 10) and of rows [k, H) partition the whole image's, so the integer sums add
    up exactly -- unless a pixel's value depends on the tile row or lane it falls in.  Columns likewise.  The SSE is
    additive over any row split."""
    K = irdu.kernels
    rows, cols = K.LUMA_SSIM_TILE
    for shape, kr, kc in [((100, 140, 3), rows + 5, 29), ((50, cols + 60, 3), 7, cols + 16),
                          ((2 * rows + 21, 290, 3), rows - 3, 101)]:
        assert kr % rows != 0 and kc % cols != 0
        a, b = pair("noisy", shape)
        whole = K.u8_luma_ssim(dev_at(a), dev_at(b))
        top = K.u8_luma_ssim(dev_at(a[:kr + 10]), dev_at(b[:kr + 10]))
        bottom = K.u8_luma_ssim(dev_at(a[kr:]), dev_at(b[kr:]))
        assert whole == top + bottom, shape
        left = K.u8_luma_ssim(dev_at(a[:, :kc + 10]), dev_at(b[:, :kc + 10]))
        right = K.u8_luma_ssim(dev_at(a[:, kc:]), dev_at(b[:, kc:]))
        assert whole == left + right, shape
        sse = K.u8_luma_sse(dev_at(a), dev_at(b))
        for k in (1, kr, shape[0] - 1):
            assert sse == K.u8_luma_sse(dev_at(a[:k]), dev_at(b[:k])) + K.u8_luma_sse(dev_at(a[k:]), dev_at(b[k:])), (shape, k)


# ---- 5. the evaluation path
EVAL_SIZES = [(40, 56), (37, 53), (100, 140), (64, 64)]      # 37 x 53: no multiple of 16; 100 x 140: larger than tile
ALL = ("psnr", "ssim", "psnr_y", "ssim_y")
TILING = dict(factor=16, tile=64, halo=16, device=DEV)


def blur(x):
    """A fixed 3 x 3 box blur: batch-independent, any window size."""
    return torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)


@pytest.mark.parametrize("ensemble", [1, (0, 1)])
def test_evaluate_metrics_is_the_per_image_loop_and_the_restatement(irdu, ensemble):
    restore = irdu.restore
    images = [smooth(h, w, 3).astype(np.float32) / np.float32(255.0) for h, w in EVAL_SIZES]
    args = dict(sigma=25.0, seed=2204, ensemble=ensemble, **TILING)
    per = irdu.evaluate_metrics(blur, images, metrics=ALL, **args)
    across = irdu.evaluate_metrics(blur, images, metrics=ALL, across_images=True, **args)
    assert tuple(per) == ALL and per == across
    today = irdu.evaluate_metrics(blur, images, **args)               # the default metrics, unchanged
    assert set(today) == {"psnr", "ssim"} and today == {m: per[m] for m in ("psnr", "ssim")}
    assert per["psnr"] == irdu.evaluate(blur, images, **args)
    for across_images in (False, True):
        for m in ("psnr_y", "ssim_y"):
            assert irdu.evaluate_metrics(blur, images, metrics=(m,), across_images=across_images, **args) == {m: per[m]}
        assert irdu.evaluate_metrics(blur, images, metrics="psnr_y", across_images=across_images, **args) == {"psnr_y": per["psnr_y"]}
    rs = np.random.RandomState(seed=2204)
    for i, clean in enumerate(images):
        restored = irdu.restore_image(blur, restore._noisy(clean, 25.0, rs), ensemble=ensemble, **TILING)
        clean_u8 = restore._clean_u8(clean)
        assert restored.dtype == np.uint8 and restored.shape == clean_u8.shape
        assert per["psnr_y"][1][i] == irdu.psnr_y_u8(restored, clean_u8) == luma_ref.psnr_y(restored, clean_u8)
        assert per["ssim_y"][1][i] == irdu.ssim_y_u8(restored, clean_u8)
        assert abs(per["ssim_y"][1][i] - luma_ref.ssim_y(restored, clean_u8)) <= BOUND
        assert 0.0 < per["ssim_y"][1][i] < 1.0 and 10.0 < per["psnr_y"][1][i] < 60.0
    for m in ("psnr_y", "ssim_y"):
        assert len(per[m][1]) == len(images) and per[m][0] == float(np.mean(per[m][1]))


@pytest.mark.parametrize("ensemble", [1, (0, 1)])
def test_evaluate_pairs_and_validate_pairs_on_uint8_pairs(irdu, ensemble):
    from irdu_amd import training
    restore = irdu.restore
    targets = [smooth(h, w, 3) for h, w in EVAL_SIZES]
    inputs = [pair("noisy", (h, w, 3))[1] for h, w in EVAL_SIZES]
    args = dict(ensemble=ensemble, **TILING)
    per = restore.evaluate_pairs(blur, inputs, targets, metrics=ALL, **args)
    assert tuple(per) == ALL and per == restore.evaluate_pairs(blur, inputs, targets, metrics=ALL, across_images=True, **args)
    assert restore.evaluate_pairs(blur, inputs, targets, **args) == {"psnr": per["psnr"]}          # the default, unchanged
    assert restore.evaluate_pairs(blur, inputs, targets, metrics=("psnr", "ssim"), **args) == {m: per[m] for m in ("psnr", "ssim")}
    for across_images in (False, True):
        for m in ("psnr_y", "ssim_y"):
            assert restore.evaluate_pairs(blur, inputs, targets, metrics=(m,), across_images=across_images, **args) == {m: per[m]}
    for i, (a, b) in enumerate(zip(inputs, targets)):
        restored = irdu.restore_image(blur, a, ensemble=ensemble, **TILING)
        assert per["psnr_y"][1][i] == irdu.psnr_y_u8(restored, b) == luma_ref.psnr_y(restored, b)
        assert per["ssim_y"][1][i] == irdu.ssim_y_u8(restored, b)
        assert abs(per["ssim_y"][1][i] - luma_ref.ssim_y(restored, b)) <= BOUND
    pairs = list(zip(inputs, targets))
    tiling = dict(tile=64, halo=16, ensemble=ensemble)
    assert training.validate_pairs(blur, pairs, factor=16, device=DEV, metric="psnr_y", **tiling) == per["psnr_y"][0]
    assert training.validate_pairs(blur, pairs, factor=16, device=DEV, metric="psnr_y", across_images=True, **tiling) == per["psnr_y"][0]
    assert training.validate_pairs(blur, pairs, factor=16, device=DEV, **tiling) == per["psnr"][0]


# ---- 6. the tool
MODEL_YAML = """name: luma_tool
manual_seed: 2204
model:
  type: GLRImageFilter
  args: {n_channels_in: 3, n_channels_out: 3, ngraphs: 4, n_cgd_iters: 1}
"""


def test_restore_tool_prints_the_y_channel_scores_of_the_files_it_writes(irdu, tmp_path, capsys):
    from PIL import Image
    from tests.test_restore_ref import _cli
    yaml_path = tmp_path / "rgb.yaml"
    yaml_path.write_text(MODEL_YAML)
    src, ref, dst = tmp_path / "in", tmp_path / "ref", tmp_path / "out"
    src.mkdir()
    ref.mkdir()
    clean = {"a": smooth(37, 53, 3), "b": smooth(48, 40, 3)}
    for name, img in clean.items():
        Image.fromarray(img).save(ref / f"{name}.png")
        Image.fromarray(pair("noisy", img.shape)[1]).save(src / f"{name}.png")
    base = ["-yaml_path", str(yaml_path), "--input", str(src), "--output", str(dst), "--reference", str(ref), "--tile",
            "64", "--halo", "16"]
    cli = _cli()
    outs, written = {}, {}
    for key, extra in (("plain", []), ("ssim", ["--ssim"]), ("y", ["--y-channel", "--ssim"]),
                       ("y_psnr", ["--y-channel"]), ("y_batch", ["--y-channel", "--ssim", "--batch-images"]),
                       ("y_ens", ["--y-channel", "--ssim", "--ensemble-modes", "0,1"])):
        torch.manual_seed(3)
        cli.main(base + extra)
        outs[key] = capsys.readouterr().out
        written[key] = {name: np.array(Image.open(dst / f"{name}.png")) for name in clean}
    for key in ("plain", "ssim", "y_psnr", "y_batch"):          # the scores change nothing that is written
        assert all(np.array_equal(written[key][name], written["y"][name]) for name in clean), key

    # without the flag: no "-Y" anywhere, the lines of today
    assert "-Y" not in outs["plain"] and "-Y" not in outs["ssim"] and "SSIM" not in outs["plain"]
    lines = [ln for ln in outs["ssim"].splitlines() if " -> " in ln]
    rgb = []
    for line, name in zip(lines, ("a", "b")):
        m = re.search(r"  reference (\S+)  PSNR (\d+\.\d{4}) dB  SSIM (-?\d\.\d{4})$", line)
        assert m and m.group(1) == str(ref / f"{name}.png"), line
        rgb.append((irdu.psnr_u8(written["ssim"][name], clean[name]), irdu.ssim_u8(written["ssim"][name], clean[name])))
        assert (m.group(2), m.group(3)) == (f"{rgb[-1][0]:.4f}", f"{rgb[-1][1]:.4f}")
    assert outs["ssim"].splitlines()[-2:] == [f"mean PSNR over 2 image(s): {float(np.mean([p for p, _ in rgb])):.4f} dB",
                                              f"mean SSIM over 2 image(s): {float(np.mean([s for _, s in rgb])):.4f}"]
    assert [re.sub(r"  SSIM -?\d\.\d{4}$", "", ln) for ln in outs["ssim"].splitlines()[:-1]] == outs["plain"].splitlines()

    # with it: PSNR-Y and SSIM-Y of the files written, in place of the RGB values
    lines = [ln for ln in outs["y"].splitlines() if " -> " in ln]
    assert len(lines) == 2 and outs["y"].count("-Y") == 6 and not re.search(r"(PSNR|SSIM) ", outs["y"])
    ys = []
    for line, plain, name in zip(lines, [ln for ln in outs["plain"].splitlines() if " -> " in ln], ("a", "b")):
        m = re.search(r"^(.*)  PSNR-Y (\d+\.\d{4}) dB  SSIM-Y (-?\d\.\d{4})$", line)
        assert m and plain.startswith(m.group(1) + "  PSNR "), line
        ys.append((irdu.psnr_y_u8(written["y"][name], clean[name]), irdu.ssim_y_u8(written["y"][name], clean[name])))
        assert (m.group(2), m.group(3)) == (f"{ys[-1][0]:.4f}", f"{ys[-1][1]:.4f}"), line
        assert ys[-1][0] == luma_ref.psnr_y(written["y"][name], clean[name])
    assert outs["y"].splitlines()[-2:] == [f"mean PSNR-Y over 2 image(s): {float(np.mean([p for p, _ in ys])):.4f} dB",
                                           f"mean SSIM-Y over 2 image(s): {float(np.mean([s for _, s in ys])):.4f}"]
    assert outs["y_batch"] == outs["y"]
    assert [re.sub(r"  SSIM-Y -?\d\.\d{4}$", "", ln) for ln in outs["y"].splitlines()[:-1]] == outs["y_psnr"].splitlines()
    assert outs["y_ens"].count("PSNR-Y") == 3 and outs["y_ens"].count("SSIM-Y") == 3

    # nothing to compare with; a one-channel model; a grey file
    with pytest.raises(SystemExit):
        cli.main([a for a in base if a not in ("--reference", str(ref))] + ["--y-channel"])
    capsys.readouterr()
    with pytest.raises(SystemExit, match="--y-channel: the model"):
        cli.main(["-yaml_path", os.path.join(ROOT, "experiment_conf", "example.yaml")] + base[2:] + ["--y-channel"])
    for folder in (src, ref):
        Image.fromarray(clean["b"][:, :, 0]).save(folder / "b.png")
    with pytest.raises(SystemExit, match=r"--y-channel: .*b\.png has 1 channel"):
        cli.main(base + ["--y-channel"])
    capsys.readouterr()
