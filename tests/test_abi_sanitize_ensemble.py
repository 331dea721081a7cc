"""The argument validation of the four self-ensemble entry points (grr_tile_gather_d8, grr_tiles_gather_d8,
grr_tile_scatter_mean, grr_tiles_scatter_mean) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

Built and run as tests/test_abi_sanitize.py builds and runs its driver: libgrr's sources with the sanitizers on the
HOST side only (the objects under build/asan/ are that test's, shared and rebuilt only when a source changes),
linked with the standalone driver tests/abi_sanitize_ensemble_main.cpp.  Nothing is loaded into Python.
"""
import os
import subprocess

import pytest

from tests import test_abi_sanitize as base

MAIN = os.path.join(base.ROOT, "tests", "abi_sanitize_ensemble_main.cpp")


def _build():
    base._build()                                   # the sanitized objects of every source, cached
    import importlib.util
    spec = importlib.util.spec_from_file_location("_grr_build", os.path.join(base.ROOT, "imagerestoration-development-unrolling_amd",
                                                                            "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    hipcc = base._hipcc()
    objs = [os.path.join(base.OUT, src.replace(".hip", ".o")) for src in bn.SOURCES]
    exe = os.path.join(base.OUT, "abi_sanitize_ensemble")
    if not os.path.exists(exe) or any(os.path.getmtime(exe) < os.path.getmtime(o) for o in objs + [MAIN]):
        main_o = os.path.join(base.OUT, "abi_sanitize_ensemble_main.o")
        clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
        r = subprocess.run([clang, "-x", "c++", "-O1", "-g", "-std=c++17", "-fsanitize=address", "-fsanitize=undefined",
                            "-fno-omit-frame-pointer", "-I", os.path.join(base.ROOT, "include"), "-c", MAIN, "-o", main_o],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        r = subprocess.run([hipcc, f"--offload-arch={bn.ARCH}"] + base.SAN + [main_o] + objs + ["-o", exe, "-pthread"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return exe


@pytest.mark.skipif(base._hipcc() is None, reason="hipcc not available")
def test_ensemble_abi_validation_under_asan_ubsan():
    exe = _build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failure(s)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
