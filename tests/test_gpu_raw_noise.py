"""grr_patch_raw_batch and grr_u8_raw_noise_demosaic on the GPU against the oracle tests/raw_noise_ref.py, bit for bit.

The definition ends in exact integers and rounds once, from float64, and tests/test_raw_noise_ref.py holds every fixture
used here at least 1e-6 away from that rounding's ties, so np.array_equal is the bound on target and input alike.  The
arena: pictures of 1 x 7, 2 x 2, 5 x 3, 40 x 56 and 100 x 70, one Bayer pattern each, all four in every call; 40 samples
per call with origins of every parity, all legal modes and the noise pairs (0, 0), (0, b), (a, 0), (a, b); patches of
16 x 16 (every fill, depth and clip), 6 x 6, 16 x 32 and 20 x 70."""
import numpy as np
import pytest
import torch

from tests import raw_noise_ref as ref

pytestmark = pytest.mark.gpu

CASE_IDS = [f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-{int(c[4])}" for c in ref.GPU_CASES]


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels, restore
    return type("G", (), dict(K=kernels, R=restore))


_SOURCES = {}


def source_of(G, shift):
    """The arena of the fixtures' pictures under the patterns of ``shift``, packed once."""
    if "pack" not in _SOURCES:
        _SOURCES["pack"] = G.R.pack_images(ref.pictures(), "cuda")
    if shift % 4 not in _SOURCES:
        _SOURCES[shift % 4] = G.K.patch_raw_source(_SOURCES["pack"], ref.patterns_of(shift))
    return _SOURCES[shift % 4]


def run(G, case, idx=None, seed=ref.SEED, ids=None, noise="fixture"):
    ph, pw, fill, bits, clip, shift = case
    k = ref.gpu_case(case)
    idx = list(range(ref.N)) if idx is None else list(idx)
    ids = k["ids"] if ids is None else ids
    noise = k["noise"][idx] if isinstance(noise, str) else noise
    target, inp = G.K.patch_raw_batch(source_of(G, shift), [k["rows"][i] for i in idx], ids[idx], noise, seed, ph, pw, fill,
                                      bits, clip)
    return target.cpu().numpy(), inp.cpu().numpy()


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=CASE_IDS)
def test_target_and_input_are_the_oracle_bit_for_bit(G, case):
    k = ref.gpu_case(case)
    assert k["margin"] >= ref.TIE_MARGIN            # a condition on the inputs, not a tolerance
    target, inp = run(G, case)
    assert target.shape == inp.shape == (ref.N, 3, case[0], case[1]) and target.dtype == inp.dtype == np.float32
    print(f"{case}: target differs in {np.count_nonzero(target != k['target'])}, input in "
          f"{np.count_nonzero(inp != k['input'])} of {inp.size}")
    assert np.array_equal(target, k["target"])
    assert np.array_equal(inp, k["input"])


@pytest.mark.parametrize("case", [ref.GPU_CASES[17], ref.GPU_CASES[18], ref.GPU_CASES[21], ref.GPU_CASES[23]],
                         ids=["16x16", "6x6", "16x32", "20x70"])
def test_a_sample_does_not_depend_on_its_batch(G, case):
    k = ref.gpu_case(case)
    again = run(G, case)
    assert np.array_equal(again[0], k["target"]) and np.array_equal(again[1], k["input"])             # two runs
    for s in (0, 9, 38, 39):
        alone = run(G, case, [s])                                                                     # n = 1
        assert np.array_equal(alone[0][0], k["target"][s]) and np.array_equal(alone[1][0], k["input"][s])
    order = list(np.random.RandomState(1).permutation(ref.N))
    mixed = run(G, case, order)
    assert np.array_equal(mixed[0], k["target"][order]) and np.array_equal(mixed[1], k["input"][order])
    noisy = [s for s in range(ref.N) if k["noise"][s].any()]
    quiet = [s for s in range(ref.N) if not k["noise"][s].any()]
    for other in (run(G, case, seed=ref.SEED + 1), run(G, case, ids=k["ids"] + 1), run(G, case, ids=k["ids"] + (1 << 32))):
        assert np.array_equal(other[0], k["target"])
        assert all(not np.array_equal(other[1][s], k["input"][s]) for s in noisy)
        assert np.array_equal(other[1][quiet], k["input"][quiet])           # a = b = 0: no random number is used


@pytest.mark.parametrize("case", [ref.GPU_CASES[16], ref.GPU_CASES[24]], ids=["16x16", "20x70"])
def test_no_noise_table_is_a_table_of_zeros(G, case):
    ph, pw, fill, bits, clip, shift = case
    k = ref.gpu_case(case)
    want = ref.batch(k["images"], k["patterns"], k["rows"], k["ids"], None, ref.SEED, ph, pw, fill, bits, clip)
    none, zeros = run(G, case, noise=None), run(G, case, noise=np.zeros((ref.N, 2), np.float32))
    for got in (none, zeros):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_device_tables_are_taken_as_they_are(G):
    case = ref.GPU_CASES[17]
    k = ref.gpu_case(case)
    dev = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    target, inp = G.K.patch_raw_batch(source_of(G, case[5]), dev(np.array(k["rows"]), torch.int32), dev(k["ids"], torch.int64),
                                      dev(k["noise"], torch.float32), ref.SEED, 16, 16, case[2], case[3], case[4])
    assert np.array_equal(target.cpu().numpy(), k["target"]) and np.array_equal(inp.cpu().numpy(), k["input"])


@pytest.mark.parametrize("pattern,fill,bits,clip", ref.WHOLE_CASES)
def test_the_one_image_form_is_the_patch_form_of_the_whole_picture(G, pattern, fill, bits, clip):
    """Pictures of 40 x 56 and 100 x 70 (both tile seams) and the 5 x 3, 2 x 2 and 1 x 7 ones, sample ids 0..4: HWC here,
    planar there; and the oracle where the CPU test holds the margin."""
    a, b = ref.SHOT, ref.read_b(ref.READ)
    pack = G.R.pack_images(ref.pictures(), "cuda")
    src = G.K.patch_raw_source(pack, pattern)
    for i, img in enumerate(ref.pictures()):
        h, w = img.shape[:2]
        sid = i - 3
        one = G.K.u8_raw_noise_demosaic(torch.from_numpy(img).cuda(), pattern, fill, a, b, bits, clip, ref.SEED, sid)
        assert tuple(one.shape) == (h, w, 3) and one.dtype == torch.float32
        _, inp = G.K.patch_raw_batch(src, [(i, 0, 0, 0)], np.array([sid], np.int64), np.array([[a, b]], np.float32), ref.SEED,
                                     h, w, fill, bits, clip)
        assert np.array_equal(one.cpu().numpy().transpose(2, 0, 1), inp[0].cpu().numpy())
        if i >= 3:
            want = ref.sample(img, pattern, 0, 0, 0, h, w, a, b, ref.SEED, sid, fill, bits, clip)
            assert want[3] >= ref.TIE_MARGIN and np.array_equal(inp[0].cpu().numpy(), want[1])
            same = G.R.raw_noise_demosaic_u8(img, pattern, fill, ref.SHOT, ref.READ, bits, clip, ref.SEED, sid)
            assert isinstance(same, np.ndarray) and np.array_equal(same, one.cpu().numpy())
