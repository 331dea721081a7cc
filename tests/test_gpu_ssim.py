"""SSIM on the GPU (csrc/metric_ops.hip through kernels.u8_ssim / u8_ssim_images, restore.ssim_u8,
restore.evaluate_metrics and restore.py --ssim) against the numpy float64 restatement (tests/ssim_ref.py), and its
exactness properties as integer equalities.

The bound against the restatement is 2^-32 on the mean: each value is quantised to the nearest multiple of 2^-32,
so it moves by at most half a step, 2^-33, and so does the mean of the quantised values; the float64 rounding of a
value in either evaluation order is about 1e-12 (tests/test_ssim_ref.py derives it), far inside the other half."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ssim_ref

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
    """The issue's three input kinds: a smooth pattern against itself plus N(0, 25) noise; random a against
    255 - a (a negative mean: the signed sum); 0 against 255."""
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
    return (shape[0] - 10) * (shape[1] - 10) * shape[2]


def tile_shapes(K):
    """One below, at and one above "tile + 10" in each direction of the kernel's tile: rows of SSIM_TILE[0]
    output rows, columns of SSIM_TILE[1] interleaved output bytes ((W - 10) C per row)."""
    rows, cols = K.SSIM_TILE
    shapes = [(rows + 10 + d, 13, 3) for d in (-1, 0, 1)]
    shapes += [(12, cols + 10 + d, 1) for d in (-1, 0, 1)]
    shapes += [(12, cols // 4 + 10 + d, 4) for d in (-1, 0, 1)]
    shapes += [(12, cols // 3 + 10 + d, 3) for d in (0, 1)]            # 3 (W - 10) = cols - 1, cols + 2
    shapes += [(2 * rows + 10 + d, cols // 2 + 10 + d, 2) for d in (-1, 0, 1)]
    return shapes


FIXED = [(11, 11, 1), (11, 29, 3), (29, 11, 2), (12, 12, 4), (37, 53, 3), (64, 70, 4), (100, 140, 3)]
LARGE = (300, 700, 3)       # several tiles both ways


# ---- 1. against the restatement
@pytest.mark.parametrize("kind", ["noisy", "negated", "extremes"])
def test_mean_is_within_one_step_of_the_restatement(irdu, kind):
    K, restore = irdu.kernels, irdu.restore
    assert K.ssim_count(1, 11, 11) == 1        # (11, 11, 1) has one valid pixel
    worst = 0.0
    for shape in FIXED + tile_shapes(K) + [LARGE]:
        a, b = pair(kind, shape)
        ref = ssim_ref.ssim(a, b)
        q = K.u8_ssim(dev_at(a), dev_at(b))
        got = restore._ssim(q, count(shape))
        err = abs(got - ref)
        worst = max(worst, err)
        print(f"{kind} {shape}: ref {ref:.12f} got {got:.12f} err {err:.3e}")
        assert err <= BOUND, (kind, shape, ref, got)
        assert restore.ssim_u8(a, b) == got == restore.ssim_u8(torch.from_numpy(a).to(DEV), b)
        if kind == "noisy" and min(shape[:2]) > 11:
            assert 0.3 < ref < 0.7
        if kind == "negated" and count(shape) > 100:
            assert ref < -0.9 and q < 0
        if kind == "extremes":
            assert abs(ref - 9.999000099991e-05) <= 1e-15
    print(f"{kind}: worst {worst:.3e} of {BOUND:.3e}")


def test_one_changed_byte_in_a_flat_image_needs_float64(irdu):
    """A constant 200 image against the same with one byte at 201: E[x^2] - mx^2 cancels at 40000 against
    C2 = 58.5, and a float32 evaluation misses the mean by about 8e-6."""
    a = np.full((20, 20, 3), 200, dtype=np.uint8)
    b = a.copy()
    b[10, 10, 1] = 201
    ref = ssim_ref.ssim(a, b)
    got = irdu.ssim_u8(a, b)
    print(f"flat: ref {ref:.12f} got {got:.12f} err {abs(got - ref):.3e}")
    assert 0.9999 < ref < 1.0
    assert abs(got - ref) <= BOUND
    assert abs(irdu.ssim_u8(b, a) - ref) <= BOUND


# ---- 2. identical images
def test_identical_images_sum_to_n_times_one_exactly(irdu):
    K = irdu.kernels
    for shape in FIXED + tile_shapes(K):
        for kind in ("noisy", "negated"):
            a, _ = pair(kind, shape)
            n = count(shape)
            assert K.u8_ssim(dev_at(a), dev_at(a)) == n * K.SSIM_ONE == n << 32, (shape, kind)
            assert K.u8_ssim(dev_at(a, 1), dev_at(a, 16 + 3)) == n << 32            # views off the 16-byte grid
            assert irdu.ssim_u8(a, a.copy()) == 1.0


# ---- 3. exactness, all as integer equality
PACK_SIZES = [(13, 15), (37, 53), (11, 11), (45, 271), (75, 33)]     # odd sizes: later images start at odd bytes


def test_the_same_call_twice_gives_the_same_integers(irdu):
    K = irdu.kernels
    a, b = pair("noisy", LARGE)
    ta, tb = dev_at(a), dev_at(b)
    first = K.u8_ssim(ta, tb)
    assert K.u8_ssim(ta, tb) == first
    assert K.u8_ssim(tb, ta) == first      # symmetric in exact arithmetic and here: x y and y x round alike


@pytest.mark.parametrize("c", [3, 1])
def test_every_image_of_a_pack_equals_the_single_image_call(irdu, c):
    K = irdu.kernels
    pairs = [pair("noisy" if i % 2 == 0 else "negated", (h, w, c), seed=i) for i, (h, w) in enumerate(PACK_SIZES)]
    singles = [K.u8_ssim(dev_at(a), dev_at(b)) for a, b in pairs]
    pa = irdu.pack_images([a for a, _ in pairs], DEV)
    pb = irdu.pack_images([b for _, b in pairs], DEV)
    assert any(off % 2 == 1 for off, _, _ in pa.host_table)
    got = K.u8_ssim_images(pa, pb)
    assert got == singles
    assert K.u8_ssim_images(pa, pb) == got
    # a pack of one and a pack in another order: what else the arena holds changes nothing
    order = [3, 0, 4, 2, 1]
    ra = irdu.pack_images([pairs[i][0] for i in order], DEV)
    rb = irdu.pack_images([pairs[i][1] for i in order], DEV)
    assert K.u8_ssim_images(ra, rb) == [singles[i] for i in order]
    assert K.u8_ssim_images(irdu.pack_images([pairs[1][0]], DEV), irdu.pack_images([pairs[1][1]], DEV)) == [singles[1]]
    for want, (a, b) in zip(singles, pairs):
        assert abs(irdu.restore._ssim(want, count(a.shape)) - ssim_ref.ssim(a, b)) <= BOUND


def test_byte_offsets_of_the_two_images_change_nothing(irdu):
    K = irdu.kernels
    for shape in [(37, 53, 3), (45, 271, 1)]:
        a, b = pair("noisy", shape)
        want = K.u8_ssim(dev_at(a), dev_at(b))
        for oa, ob in [(1, 0), (0, 7), (3, 5), (15, 17), (16, 2)]:
            assert K.u8_ssim(dev_at(a, oa), dev_at(b, ob)) == want, (shape, oa, ob)


def test_sums_are_additive_over_rows_and_columns(irdu):
    """The valid pixels of rows [0, k + 10) and of rows [k, H) partition the whole image's, so the integer sums add
    up exactly -- unless a pixel's value depends on the tile row or lane it falls in.  Columns likewise."""
    K = irdu.kernels
    rows, cols = K.SSIM_TILE
    for shape, kr, kc in [((100, 140, 3), rows + 5, 29), ((50, 300, 3), 7, cols // 3 + 16), ((2 * rows + 21, 290, 1), rows - 3, 101)]:
        assert kr % rows != 0 and (kc * shape[2]) % cols != 0
        a, b = pair("noisy", shape)
        whole = K.u8_ssim(dev_at(a), dev_at(b))
        top = K.u8_ssim(dev_at(a[:kr + 10]), dev_at(b[:kr + 10]))
        bottom = K.u8_ssim(dev_at(a[kr:]), dev_at(b[kr:]))
        assert whole == top + bottom, shape
        left = K.u8_ssim(dev_at(a[:, :kc + 10]), dev_at(b[:, :kc + 10]))
        right = K.u8_ssim(dev_at(a[:, kc:]), dev_at(b[:, kc:]))
        assert whole == left + right, shape


# ---- 4. the evaluation path
EVAL_SIZES = [(40, 56), (37, 53), (100, 140), (64, 64)]      # 37 x 53: no multiple of 16; 100 x 140: larger than tile


def blur(x):
    """A fixed 3 x 3 box blur: batch-independent, any window size."""
    return torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), 3, 1)


@pytest.mark.parametrize("ensemble", [1, (0, 1)])
def test_evaluate_metrics_is_the_per_image_loop_and_the_restatement(irdu, ensemble):
    restore = irdu.restore
    images = [smooth(h, w, 3).astype(np.float32) / np.float32(255.0) for h, w in EVAL_SIZES]
    args = dict(sigma=25.0, factor=16, seed=2204, tile=64, halo=16, device=DEV, ensemble=ensemble)
    per = irdu.evaluate_metrics(blur, images, **args)
    across = irdu.evaluate_metrics(blur, images, across_images=True, **args)
    assert set(per) == {"psnr", "ssim"} and per == across
    assert per["psnr"] == irdu.evaluate(blur, images, **args)
    assert across["psnr"] == irdu.evaluate(blur, images, across_images=True, **args)
    assert irdu.evaluate_metrics(blur, images, metrics=("ssim",), across_images=True, **args) == {"ssim": per["ssim"]}
    assert irdu.evaluate_metrics(blur, images, metrics=("psnr",), **args) == {"psnr": per["psnr"]}
    mean, values = per["ssim"]
    assert len(values) == len(images) and mean == float(np.mean(values))
    rs = np.random.RandomState(seed=2204)
    for clean, value in zip(images, values):
        restored = irdu.restore_image(blur, restore._noisy(clean, 25.0, rs), factor=16, tile=64, halo=16, device=DEV,
                                      ensemble=ensemble)
        clean_u8 = restore._clean_u8(clean)
        assert restored.dtype == np.uint8 and restored.shape == clean_u8.shape
        assert value == irdu.ssim_u8(restored, clean_u8)
        assert abs(value - ssim_ref.ssim(restored, clean_u8)) <= BOUND
        assert 0.0 < value < 1.0


# ---- 5. the tool
def test_restore_tool_prints_the_ssim_of_the_files_it_writes(irdu, tmp_path, capsys):
    from PIL import Image
    from tests.test_restore_ref import _cli
    yaml_path = os.path.join(ROOT, "experiment_conf", "example.yaml")       # a one-channel model, no checkpoint
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    images = {"a": smooth(37, 53, 1)[:, :, 0], "b": smooth(48, 40, 1)[:, :, 0]}
    for name, img in images.items():
        Image.fromarray(img).save(src / f"{name}.png")
    base = ["-yaml_path", yaml_path, "--input", str(src), "--output", str(dst), "--sigma", "25", "--tile", "64",
            "--halo", "16"]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "restore.py")] + base + ["--ssim"], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln for ln in run.stdout.splitlines() if " -> " in ln]
    assert len(lines) == 2
    printed = []
    for line, name in zip(lines, ("a", "b")):
        m = re.search(r"  PSNR (\d+\.\d{4}) dB  SSIM (-?\d\.\d{4})$", line)
        assert m, line
        written = np.array(Image.open(dst / f"{name}.png"))
        want = irdu.ssim_u8(written[:, :, None], images[name][:, :, None])
        assert m.group(2) == f"{want:.4f}", (line, want)
        assert m.group(1) == f"{irdu.psnr_u8(written, images[name]):.4f}"
        printed.append(want)
    tail = run.stdout.splitlines()[-2:]
    assert re.fullmatch(r"mean PSNR over 2 image\(s\): \d+\.\d{4} dB", tail[0]), tail
    assert tail[1] == f"mean SSIM over 2 image(s): {float(np.mean(printed)):.4f}", tail

    # in this process: no --ssim, no "SSIM"; --batch-images prints the lines of the per-file run
    cli = _cli()
    outs = {}
    for key, extra in (("plain", []), ("ssim", ["--ssim"]), ("batch", ["--ssim", "--batch-images"])):
        torch.manual_seed(3)
        cli.main(base + extra)
        outs[key] = capsys.readouterr().out
    assert "SSIM" not in outs["plain"] and outs["ssim"].count("SSIM") == 3
    assert outs["batch"] == outs["ssim"]
    assert [re.sub(r"  SSIM -?\d\.\d{4}$", "", ln) for ln in outs["ssim"].splitlines()[:-1]] == outs["plain"].splitlines()
    with pytest.raises(SystemExit):
        cli.main([a for a in base if a not in ("--sigma", "25")] + ["--ssim"])
    capsys.readouterr()
