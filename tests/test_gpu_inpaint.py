"""grr_patch_mask_batch and grr_u8_mask_fill on the GPU against the oracle tests/inpaint_ref.py, bit for bit: the
definition has no floating point before the last float(byte) / 255.0f, so every comparison is np.array_equal.

The arena holds a 40 x 90, a 3 x 5 (both sides below the halo: the mirror folds several times) and a 33 x 37 picture for
each of C = 1, 3, 4.  Patches of 5 x 7 (less than one tile, pw % 4 != 0), 16 x 64, 17 x 65 and 33 x 67 (two tiles each
way, both remainders) and 16 x 16 (all 8 modes); origins at the corner, inside and at the far edge, so that the patch and
its halo stick out on every side; tables of 1 x 1, 3 x 3, 15 x 15, 3 x 15, 15 x 3 and asymmetric random ones; known
shares of 0, 2^24, 2^23 and 2^24 / 5."""
import numpy as np
import pytest
import torch

from tests import inpaint_ref as ref, patch_ref

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1
ONE = ref.ONE
SHAPES = ((40, 90), (3, 5), (33, 37))
KEEPS = (ONE // 2, ONE // 5, 0, ONE, ONE // 2, ONE // 5)
_RS = np.random.RandomState(5)
TABLES = {
    "1x1": np.full((1, 1), 255, np.uint8),
    "3x3": np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.uint8),
    "15x15": np.full((15, 15), 255, np.uint8),
    "3x15": _RS.randint(0, 256, (3, 15)).astype(np.uint8),
    "15x3": _RS.randint(0, 256, (15, 3)).astype(np.uint8),
    "asym7": _RS.randint(0, 256, (7, 7)).astype(np.uint8),
    "asym5x9": _RS.randint(0, 256, (5, 9)).astype(np.uint8),
}
TABLES["asym7"][0, :] = 0               # a transposed or flipped tap index changes the sums
TABLES["asym5x9"][:, 8] = 0


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore
    return type("G", (), dict(K=kernels, R=restore))


_PICS, _SRC = {}, {}


def pictures(c):
    if c not in _PICS:
        _PICS[c] = [patch_ref.picture(k + c, h, w, c) for k, (h, w) in enumerate(SHAPES)]
    return _PICS[c]


def source(G, c):
    if c not in _SRC:
        _SRC[c] = G.K.patch_source(G.R.pack_images(pictures(c), "cuda"))
    return _SRC[c]


def rows_for(ph, pw, modes):
    """(img, row, col, mode): the corner, inside, the far edges (the patch sticks out at the bottom / right, the halo at
    the top / left), the 3 x 5 picture and the 33 x 37 one."""
    origins = [(0, 0, 0), (0, 11, 23), (0, 39, 89), (0, 30, 0), (1, 0, 0), (1, 2, 4), (2, 5, 9), (2, 32, 36)]
    return [(im, r, c, modes[i % len(modes)]) for i, (im, r, c) in enumerate(origins)]


def run(G, c, rows, ids, keeps, ph, pw, table, fill, hole, with_mask=True):
    t, i, m = G.K.patch_mask_batch(source(G, c), rows, np.asarray(ids, np.int64), np.asarray(keeps, np.int64), SEED, ph, pw,
                                   TABLES[table], fill, hole, with_mask)
    return t.cpu().numpy(), i.cpu().numpy(), None if m is None else m.cpu().numpy()


CASES = [
    # C, ph, pw, table, fill, hole, modes
    (3, 5, 7, "3x3", "conv", 0, (0, 1, 4, 5)),
    (3, 16, 64, "15x15", "conv", 200, (0, 1, 4, 5)),
    (1, 17, 65, "3x15", "conv", 200, (0, 1, 4, 5)),
    (4, 33, 67, "15x3", "conv", 0, (0, 1, 4, 5)),
    (3, 17, 65, "asym5x9", "conv", 200, (0, 1, 4, 5)),
    (3, 33, 67, "1x1", "conv", 200, (0, 1, 4, 5)),
    (4, 16, 64, "asym7", "zero", 0, (0, 1, 4, 5)),
    (1, 5, 7, "15x15", "conv", 0, (0, 1, 4, 5)),
    (3, 16, 16, "asym7", "conv", 200, tuple(range(8))),
    (4, 16, 16, "3x15", "conv", 0, tuple(range(8))),
    (1, 16, 16, "asym5x9", "zero", 200, tuple(range(8))),
    (3, 33, 67, "asym7", "conv", 0, (0, 1, 4, 5)),
]


@pytest.mark.parametrize("case", CASES, ids=[f"C{c[0]}-{c[1]}x{c[2]}-{c[3]}-{c[4]}-{c[5]}" for c in CASES])
def test_the_patch_form_is_the_oracle_bit_for_bit(G, case):
    c, ph, pw, table, fill, hole, modes = case
    rows = rows_for(ph, pw, modes)
    ids = [7 + 3 * s + ((s % 3) << 33) for s in range(len(rows))]
    keeps = [KEEPS[s % len(KEEPS)] for s in range(len(rows))]
    want = ref.mask_fill_patch(pictures(c), rows, ids, keeps, SEED, ph, pw, TABLES[table], fill, hole)
    got = run(G, c, rows, ids, keeps, ph, pw, table, fill, hole)
    for name, g, w in zip(("target", "input", "mask"), got, want):
        assert g.shape == w.shape and g.dtype == np.float32
        print(f"{case}: {name} differs in {np.count_nonzero(g != w)} of {w.size}")
        assert np.array_equal(g, w), name
    assert 0 < got[2][0].mean() < 1                     # the first share is a half: the mask is not trivial
    none = run(G, c, rows, ids, keeps, ph, pw, table, fill, hole, with_mask=False)
    assert none[2] is None and np.array_equal(none[0], want[0]) and np.array_equal(none[1], want[1])


def test_the_mask_does_not_depend_on_the_table_or_the_fill(G):
    rows, ids, keeps = rows_for(17, 65, (0, 5)), list(range(8)), [ONE // 2] * 8
    masks = [run(G, 3, rows, ids, keeps, 17, 65, table, fill, 128)[2]
             for table, fill in (("1x1", "conv"), ("15x15", "conv"), ("3x15", "conv"), ("asym7", "zero"))]
    assert all(np.array_equal(m, masks[0]) for m in masks[1:])
    other = run(G, 3, rows, [i + 1 for i in ids], keeps, 17, 65, "1x1", "conv", 128)[2]
    assert not np.array_equal(other, masks[0])


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def test_device_tables_are_clamped_and_odd_turns_of_a_non_square_patch_are_read_as_mode_and_5(G):
    """Device tables are taken as they are: modes 2, 3, 6, 7 on a 17 x 65 patch, shares outside [0, 2^24], an image
    index, a row and a column outside their ranges."""
    c, ph, pw = 3, 17, 65
    rows = [(0, 3, 4, 2), (0, 11, 23, 3), (2, 5, 9, 6), (1, 1, 1, 7), (7, 2, 2, 10), (0, 1000, 5, 0), (2, 3, -4, 13), (-3, 1, 2, 4)]
    keeps = [ONE // 2, ONE // 5, -5, ONE + 100, ONE // 2, ONE // 5, ONE // 2, ONE // 2]
    ids = [100 + s for s in range(8)]
    clamped = []
    for im, r, col, mode in rows:
        im = min(max(im, 0), len(SHAPES) - 1)
        h, w = SHAPES[im]
        clamped.append((im, min(max(r, 0), h - 1), min(max(col, 0), w - 1), mode))
    want = ref.mask_fill_patch(pictures(c), clamped, ids, keeps, SEED, ph, pw, TABLES["asym7"], "conv", 9)
    t, i, m = G.K.patch_mask_batch(source(G, c), dev(np.array(rows), torch.int32), dev(np.array(ids), torch.int64),
                                   dev(np.array(keeps), torch.int32), SEED, ph, pw, TABLES["asym7"], "conv", 9)
    for g, w in zip((t, i, m), want):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("c,ph,pw", [(1, 5, 7), (3, 16, 16), (4, 33, 67)])
def test_with_every_pixel_known_input_target_and_the_clean_patch_are_equal(G, c, ph, pw):
    rows = rows_for(ph, pw, tuple(range(8)) if ph == pw else (0, 1, 4, 5))
    ids = list(range(len(rows)))
    clean, _ = G.K.patch_batch(source(G, c), rows, np.asarray(ids, np.int64), np.zeros(len(rows), np.float32), SEED, ph, pw)
    for fill in ("zero", "conv"):
        t, i, m = run(G, c, rows, ids, [ONE] * len(rows), ph, pw, "asym7", fill, 0)
        assert np.array_equal(t, clean.cpu().numpy()) and np.array_equal(i, t) and (m == 1).all()
    t, i, m = run(G, c, rows, ids, [0] * len(rows), ph, pw, "asym7", "conv", 200)          # nothing known: the hole
    assert np.array_equal(t, clean.cpu().numpy()) and (m == 0).all()
    assert np.array_equal(i, np.full_like(i, np.float32(200) / np.float32(255)))
    t, i, m = run(G, c, rows, ids, [0] * len(rows), ph, pw, "asym7", "zero", 200)
    assert (i == 0).all() and (m == 0).all()


def test_a_sample_does_not_depend_on_its_batch(G):
    c, ph, pw = 3, 17, 65
    rows = rows_for(ph, pw, (0, 1, 4, 5))[:5]
    ids, keeps = [11, 12, 13, 14, 15], [ONE // 2, ONE // 5, ONE // 2, ONE // 5, ONE // 2]
    batch = run(G, c, rows, ids, keeps, ph, pw, "asym5x9", "conv", 128)
    for s in range(5):
        alone = run(G, c, rows[s:s + 1], ids[s:s + 1], keeps[s:s + 1], ph, pw, "asym5x9", "conv", 128)
        assert all(np.array_equal(a[0], b[s]) for a, b in zip(alone, batch))


def odd(t):
    """A copy of a uint8 device tensor at an odd byte address."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 2 == 1
    return out


@pytest.mark.parametrize("c", [1, 3, 4])
def test_the_one_picture_form_draws_the_patch_forms_mask(G, c):
    """Every picture whole, sample ids -3.., against the oracle and against the patch form of the whole picture; src at
    an odd byte address."""
    for k, img in enumerate(pictures(c)):
        h, w = img.shape[:2]
        sid, keep, table = k - 3, (ONE // 2, ONE // 5, ONE // 3)[k], ("asym7", "3x15", "15x3")[k]
        out, mask_out = G.K.u8_mask_fill(odd(torch.from_numpy(img).cuda()), None, keep, TABLES[table], "conv", 77, SEED, sid)
        want, code = ref.mask_fill_image(img, None, keep, SEED, sid, TABLES[table], "conv", 77)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(mask_out.cpu().numpy(), code)
        t, i, m = run(G, c, [(k, 0, 0, 0)], [sid], [keep], h, w, table, "conv", 77)
        assert np.array_equal(m[0, 0], (code == 1).astype(np.float32))
        assert np.array_equal(i[0], (want.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
        zero, zmask = G.K.u8_mask_fill(torch.from_numpy(img).cuda(), None, keep, None, "zero", 77, SEED, sid)
        assert np.array_equal(zmask.cpu().numpy(), (code == 1).astype(np.uint8))
        assert np.array_equal(zero.cpu().numpy(), want * (code == 1)[:, :, None])


def test_a_given_mask_with_a_wide_hole_closes_in_passes_at_odd_byte_addresses(G):
    """A 20-pixel-wide hole under a 7 x 7 table: a pass grows the filled region by 3 pixels from either side, so one
    pass leaves zeros in mask_out and four passes leave none; src, mask_in, dst and mask_out at odd byte addresses,
    through the library directly."""
    K = G.K
    img = pictures(3)[0]
    h, w = img.shape[:2]
    mask = np.ones((h, w), np.uint8)
    mask[:, 30:50] = 0
    mask[5:9, 2:4] = 0
    mask[mask > 0] = 1 + (np.arange(h * w).reshape(h, w)[mask > 0] % 3) * 100          # 1, 101, 201: carried through
    table = TABLES["asym7"] | 1                                                          # every tap positive
    wd = torch.from_numpy(np.ascontiguousarray(table)).cuda()
    src, m_in = odd(torch.from_numpy(img).cuda()), odd(torch.from_numpy(mask).cuda())
    want_img, want_mask = img, mask
    for p in range(4):
        dst, m_out = odd(torch.zeros_like(src)), odd(torch.zeros_like(m_in))
        K._launch("u8_mask_fill", 0, "grr_u8_mask_fill", src.data_ptr(), m_in.data_ptr(), h, w, 3, 0, SEED, 0, wd.data_ptr(),
                  7, 7, 1, 128, dst.data_ptr(), m_out.data_ptr(), K._stream(src.device))
        want_img, want_mask = ref.mask_fill_image(want_img, want_mask, 0, SEED, 0, table, "conv", 128)
        assert np.array_equal(dst.cpu().numpy(), want_img) and np.array_equal(m_out.cpu().numpy(), want_mask), p
        assert np.array_equal(want_mask[mask > 0], mask[mask > 0])
        left = int((m_out == 0).sum())
        assert (left > 0) == (p < 3), (p, left)
        src, m_in = dst, m_out
    assert set(np.unique(want_mask)) == {1, 2, 101, 201}
    # the wrapper's own pass: the same first pass
    out, m_out = K.u8_mask_fill(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), 0, table, "conv", 128)
    first = ref.mask_fill_image(img, mask, 0, SEED, 0, table, "conv", 128)
    assert np.array_equal(out.cpu().numpy(), first[0]) and np.array_equal(m_out.cpu().numpy(), first[1])
