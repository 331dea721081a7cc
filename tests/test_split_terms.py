"""The pack-time three-term bf16 split (csrc/grr_split.h, split_term) against torch's RNE bfloat16 (CPU).

The weight-pack kernels round with integer arithmetic on the bit pattern; the kernels' split3x8 uses the
hardware conversion and the tests' references use torch's.  A small stand-alone host program
(tests/split_terms_main.hip, compiled with hipcc for the host only) prints split_term(v, q), q = 0, 1, 2,
for a fixed list of finite fp32 values; every bit must equal tests/gemm_ref.py::split3, which alone defines
the expected terms.

All inputs are finite, but not every term is: the largest finite float (+-0x7f7fffff) rounds to bf16 infinity,
so its terms are (Inf, -Inf, NaN) in the reference and in split_term alike.  The infinities agree bit for bit
(7f80 / ff80).  The NaN does not (split_term ffc0: the host's default NaN through the integer rounding;
torch ffff), and RNE defines no NaN payload, so where the reference's term is a NaN the test requires a NaN
and compares no payload.  These are 2 terms of 3518 x 3; every other term, 0x7f7f7fff (the largest float whose
split is finite) included, is compared bit for bit.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import gemm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "imagerestoration-development-unrolling_amd", "csrc")
OUT = os.path.join(ROOT, "build", "split_terms")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def _build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "split_terms")
    main = os.path.join(ROOT, "tests", "split_terms_main.hip")
    deps = [main] + [os.path.join(CSRC, h) for h in ("grr_split.h", "grr_device.h", "grr_common.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(exe) < os.path.getmtime(d) for d in deps):
        r = subprocess.run([_hipcc(), "--cuda-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                            main, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return exe


def _inputs():
    """Finite fp32 bit patterns (uint32): normals over exponents -100..100, bf16 ties both ways, +-0, the
    largest finite float, subnormals."""
    g = torch.Generator().manual_seed(5117)
    e = torch.randint(-100, 101, (3000,), generator=g)
    normals = torch.ldexp(torch.randn(3000, generator=g), e).float()
    bits = [normals.view(torch.int32).numpy().view(np.uint32)]
    # exact ties of the first rounding: low half 0x8000 under an even (rounds down) and an odd (rounds up)
    # bf16 significand, both signs, several exponents; and the neighbours one ulp either side of the tie
    ties = []
    for ex in (1, 27, 100, 127, 128, 200, 253):
        for sig in (0x00, 0x01, 0x2A, 0x2B, 0x7E, 0x7F):
            for sign in (0, 1):
                hi = (sign << 15) | (ex << 7) | sig
                for low in (0x7FFF, 0x8000, 0x8001):
                    ties.append((hi << 16) | low)
    # ties of the second rounding: the residual after the first term is exactly half a bf16 ulp of itself
    for ex in (60, 127, 190):
        for low in (0x0080, 0x0180, 0x4080, 0x4180, 0x00C0, 0x01C0):
            ties.append((ex << 23) | low)
            ties.append((1 << 31) | (ex << 23) | low)
    bits.append(np.array(ties, dtype=np.uint32))
    bits.append(np.array([0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0xFF7F7FFF], dtype=np.uint32))
    sub = [0x00000001, 0x00000002, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00028000, 0x007FFFFF,
           0x00400000, 0x00012345]
    bits.append(np.array(sub + [s | 0x80000000 for s in sub], dtype=np.uint32))
    g2 = np.random.default_rng(5118)
    bits.append(g2.integers(1, 0x00800000, 200, dtype=np.uint32))       # random subnormals
    out = np.concatenate(bits)
    assert np.isfinite(out.view(np.float32)).all()
    return out


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_split_term_bits_match_torch_rne():
    exe = _build()
    u = _inputs()
    assert 3000 < u.size < 10000
    r = subprocess.run([exe], input="".join("%08x\n" % x for x in u), capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    got = np.array([[int(t, 16) for t in line.split()] for line in r.stdout.splitlines()], dtype=np.uint32)
    assert got.shape == (u.size, 3)
    v = torch.from_numpy(u.view(np.float32).copy())
    ref = gemm_ref.split3(v).float().view(torch.int32).numpy().view(np.uint32)   # [3, n], bf16 values as fp32
    assert (ref & 0xFFFF == 0).all()
    want = (ref >> 16).T

    def is_nan(h):   # bf16 bit patterns
        return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)

    assert is_nan(want).sum() == 2, "only the third term of +-FLT_MAX is a NaN in the reference"
    same = np.where(is_nan(want), is_nan(got), got == want)
    bad = np.nonzero(~same.all(axis=1))[0]
    msg = "; ".join("v=%08x got %s want %s" % (u[i], ["%04x" % t for t in got[i]], ["%04x" % t for t in want[i]])
                    for i in bad[:8])
    assert bad.size == 0, "%d of %d values differ: %s" % (bad.size, u.size, msg)
