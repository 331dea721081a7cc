"""The feature CNN kernels' output bits on gfx950, pinned: SHA-256 digests of the fp32 bytes of lnb_fused16_kernel,
lnb_rep_kernel and feat_edge_kernel outputs against tests/golden/feature_cnn_bits_gfx950.json, which
scripts/record_feature_bits.py wrote from the build of the commit named in the file.  A change that is meant to
keep the arithmetic (an instruction-selection or scheduling change) passes unchanged; one that moves a bit has to
re-record the fixture deliberately.  The accuracy of the same kernels is tests/test_gpu_lnb_tiles.py's and
tests/test_gpu_feature_edges.py's business, not this file's.

  fused LNB     out and the kept gate g at lnb_ref.CASES[1] (C 20, hid 24: a partial last chunk, lanes with
                pj >= hid) and CASES[5] (C 96, hid 256: the headline instance), B = 2 of lnb_ref's 20 x 70 images
                (nine tiles, partial right and bottom), NCHW, skip = lnb_ref.SKIP
  fused LNB c8  out with channel-blocked input and output (io 3) at CASES[5]
  replicated    lnb_rep_kernel at lnb_ref.REPLICATED[0]
  edges         all three outputs of feature_edges at (b, G, H, W) = (2, 5, 9, 29) (G < 32, narrower than one
                strip) and (1, 32, 40, 64) (two strips, halo columns on both sides)
"""
import hashlib
import json
import os

import pytest
import torch

from tests import lnb_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARCH = "gfx950"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_cnn_bits_gfx950.json")
EDGE_SHAPES = [(2, 5, 9, 29), (1, 32, 40, 64)]


def device_arch():
    return torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]


def sha(t):
    assert t.dtype == torch.float32
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _case_inputs(case):
    x, _, p = L.inputs(case, 2)
    return x.to(DEV), L.Params(*[t.to(DEV).contiguous() for t in p]), torch.tensor(L.SKIP, dtype=torch.float32, device=DEV)


def lnb_fused_digests(K, idx):
    case = L.CASES[idx]
    x, p, sk = _case_inputs(case)
    out, gate = K.lnb_forward_keep(x, p.ln_w, p.w1, p.wdw, p.w2, sk)
    torch.cuda.synchronize()
    tag = f"lnb_fused/{L.IDS[idx]}"
    return {f"{tag}/out": sha(out), f"{tag}/g": sha(gate)}


def lnb_fused_c8_digests(K):
    case = L.CASES[5]
    x, p, sk = _case_inputs(case)
    out = K.lnb_forward_c8(K.to_c8(x), case.c, p.ln_w, p.w1, p.wdw, p.w2, sk, True, True)
    torch.cuda.synchronize()
    return {f"lnb_fused/{L.IDS[5]}/io3/out": sha(out)}


def lnb_rep_digests(K):
    case = L.REPLICATED[0]
    x, p, sk = _case_inputs(case)
    out = K.lnb_forward_rep(x[:, :case.rep].contiguous(), None, p.ln_w, p.w1, p.wdw, p.w2, sk)
    torch.cuda.synchronize()
    return {f"lnb_rep/Cs{case.rep}-R{case.c // case.rep}-hid{case.hid}/out": sha(out)}


def edge_digests(K, shape):
    b, g, h, w = shape
    c = 3 * g
    gen = torch.Generator().manual_seed(b * 100 + g + h + w)
    x = (torch.randn(b, c, h, w, generator=gen) * torch.rand(b, 1, h, w, generator=gen) * 3).to(DEV)   # per-pixel scales vary
    wt = (torch.randn(2 * c, c, 1, 1, generator=gen) * 0.2).to(DEV)
    mG = (0.5 + torch.rand(g, 3, generator=gen)).to(DEV)
    mL = (0.5 + torch.rand(g, 3, generator=gen)).to(DEV)
    wG, cG, wL = K.feature_edges(x, False, wt, g, 3, mG, mL)
    torch.cuda.synchronize()
    tag = f"feature_edges/b{b}-G{g}-{h}x{w}"
    return {f"{tag}/wG": sha(wG), f"{tag}/cG": sha(cG), f"{tag}/wL": sha(wL)}


GROUPS = {
    "lnb_fused-" + L.IDS[1]: lambda K: lnb_fused_digests(K, 1),
    "lnb_fused-" + L.IDS[5]: lambda K: lnb_fused_digests(K, 5),
    "lnb_fused-c8": lnb_fused_c8_digests,
    "lnb_rep": lnb_rep_digests,
    "edges-G5": lambda K: edge_digests(K, EDGE_SHAPES[0]),
    "edges-G32": lambda K: edge_digests(K, EDGE_SHAPES[1]),
}


def all_digests(K):
    """Every pinned digest, {name: hex} (scripts/record_feature_bits.py writes these into the fixture)."""
    out = {}
    for fn in GROUPS.values():
        out.update(fn(K))
    return out


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if device_arch() != ARCH:
        pytest.skip(f"the digests are {ARCH}'s (this device: {device_arch()})")
    import irdu_amd
    irdu_amd.load_native()
    from irdu_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["arch"] == ARCH and len(fx["commit"]) == 40, fx
    return fx


def test_fixture_names_every_digest(golden):
    names = set(golden["digests"])
    assert len(names) == 12 and all(len(v) == 64 for v in golden["digests"].values())


@pytest.mark.parametrize("group", list(GROUPS))
def test_bits_unchanged(K, golden, group):
    got = GROUPS[group](K)
    for name, digest in got.items():
        print(f"{name}: {digest}  (recorded at {golden['commit'][:12]}: {golden['digests'].get(name)})")
    bad = [name for name, digest in got.items() if golden["digests"].get(name) != digest]
    assert not bad, f"bits moved against commit {golden['commit'][:12]}: {bad}"
