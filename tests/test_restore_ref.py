"""CPU checks of the whole-image restoration plan and of its numpy restatement (tests/restore_ref.py)."""
import numpy as np
import pytest
import torch
from torch import nn

from irdu_amd import restore
from tests import restore_ref as R

# (h, w, tile, halo): w <= tile < h, sides that are multiples already, sides of 17 and 31, one window, many
PLAN_CASES = [(100, 40, 48, 16), (40, 100, 48, 16), (64, 96, 32, 0), (17, 31, 48, 16), (31, 17, 16, 0),
              (17, 100, 32, 0), (100, 140, 48, 16), (150, 203, 128, 32), (16, 16, 48, 16), (97, 33, 64, 16),
              (481, 321, 256, 32)]


def test_restatement_padding_equals_torch_reflect_with_validates_size_rule():
    rs = np.random.RandomState(1)
    factor = 16
    for h in range(16, 50):
        for w in range(16, 50):
            img = rs.rand(h, w, 2).astype(np.float32)
            x = torch.from_numpy(img).permute(2, 0, 1).unsqueeze(0)
            H, W = ((h + factor) // factor) * factor, ((w + factor) // factor) * factor     # validate()'s lines
            padh = H - h if h % factor != 0 else 0
            padw = W - w if w % factor != 0 else 0
            want = nn.functional.pad(x, (0, padw, 0, padh), "reflect")[0].permute(1, 2, 0).numpy()
            got = R.pad_reflect(img, factor)
            assert got.shape == want.shape and np.array_equal(got, want), (h, w)
            p = restore.plan(h, w, factor, 48, 16)
            assert (p.hp, p.wp) == got.shape[:2], (h, w)


@pytest.mark.parametrize("h,w,tile,halo", PLAN_CASES)
def test_plan_cores_partition_the_padded_image_and_windows_lie_inside(h, w, tile, halo):
    p = restore.plan(h, w, 16, tile, halo)
    assert (p.hp, p.wp) == (R.padded_size(h, 16), R.padded_size(w, 16))
    assert (p.th, p.tw) == (min(tile, p.hp), min(tile, p.wp))
    count = np.zeros((p.hp, p.wp), np.int64)
    for wr, wc, r0, r1, c0, c1 in p.windows:
        assert 0 <= wr and wr + p.th <= p.hp and 0 <= wc and wc + p.tw <= p.wp          # window inside
        assert wr <= r0 < r1 <= wr + p.th and wc <= c0 < c1 <= wc + p.tw                # core inside its window
        assert wr % 16 == 0 and wc % 16 == 0
        count[r0:r1, c0:c1] += 1
    assert np.array_equal(count, np.ones_like(count))
    assert (R.owner_map(p) >= 0).all()


def test_plan_raises_as_specified():
    with pytest.raises(ValueError, match="reflect"):
        restore.plan(5, 64, factor=16)          # pad 11 >= side 5: torch's reflect pad raises too
    with pytest.raises(RuntimeError):
        nn.functional.pad(torch.zeros(1, 1, 5, 64), (0, 0, 0, 11), "reflect")
    with pytest.raises(ValueError, match="reflect"):
        restore.plan(64, 7, factor=16)
    restore.plan(9, 64, factor=16)              # pad 7 < 9 is fine
    with pytest.raises(ValueError):
        restore.plan(100, 100, factor=16, tile=40, halo=16)     # tile no multiple of factor
    with pytest.raises(ValueError):
        restore.plan(100, 100, factor=16, tile=48, halo=8)      # halo no multiple of factor
    with pytest.raises(ValueError):
        restore.plan(100, 100, factor=16, tile=32, halo=16)     # tile <= 2 halo
    with pytest.raises(ValueError):
        restore.plan(100, 100, factor=16, tile=64, halo=32)


def test_uint8_round_trip_values():
    k = np.arange(256, dtype=np.uint8)
    f = k.astype(np.float32) / np.float32(255)
    assert np.array_equal(np.rint(f * np.float32(255)).astype(np.int64), np.arange(256))
    # the product with 1/255 is a different float for many values: the kernels must divide
    assert int((f != k.astype(np.float32) * np.float32(1.0 / 255.0)).sum()) == 126


@pytest.mark.parametrize("h,w,tile,halo", PLAN_CASES[:8])
def test_identity_round_trip_through_the_restatement(h, w, tile, halo):
    rs = np.random.RandomState(h * 1000 + w)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img.reshape(-1)[:256] = np.arange(256)
    p = restore.plan(h, w, 16, tile, halo)
    assert np.array_equal(R.restore(lambda x: x, img, p), img)
    f = rs.rand(h, w, 3).astype(np.float32)
    assert np.array_equal(R.restore(lambda x: x, f, p, quantise=False), f)


def test_restore_image_refuses_bad_images_without_a_gpu():
    """Shape and dtype are checked before the image goes anywhere."""
    ident = lambda x: x  # noqa: E731
    with pytest.raises(ValueError):
        restore.restore_image(ident, np.zeros((32, 32, 5), np.uint8))
    with pytest.raises(ValueError):
        restore.restore_image(ident, np.zeros((32, 32, 3), np.int16))
    with pytest.raises(ValueError):
        restore.restore_image(ident, torch.zeros(8, 32, 32))          # CHW: read as 32 channels
    with pytest.raises(ValueError):
        restore.restore_image(ident, np.zeros((5, 32, 3), np.uint8))
    with pytest.raises(ValueError):
        restore.restore_image(ident, np.zeros((32, 32), np.uint8))


def _cli():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("restore_cli", os.path.join(root, "restore.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_lists_its_inputs(tmp_path):
    cli = _cli()
    with pytest.raises(SystemExit):
        cli.input_files(str(tmp_path / "missing.png"))
    with pytest.raises(SystemExit):
        cli.input_files(str(tmp_path))                      # a directory without images
    for name in ("b.png", "a.JPG", "notes.txt"):
        (tmp_path / name).write_bytes(b"")
    assert [p.split("/")[-1] for p in cli.input_files(str(tmp_path))] == ["a.JPG", "b.png"]
    assert cli.input_files(str(tmp_path / "b.png")) == [str(tmp_path / "b.png")]
    with pytest.raises(SystemExit):
        cli.main(["--input", str(tmp_path), "--output", str(tmp_path)])     # -yaml_path is required
