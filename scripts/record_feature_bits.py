"""Write tests/golden/feature_cnn_bits_gfx950.json: the SHA-256 digests that tests/test_gpu_feature_bits.py pins,
computed on a gfx950 device from the library that is loaded (GRR_LIB, else the in-tree libgrr.so).

    python scripts/record_feature_bits.py --commit <id of the commit the library was built from> [--out FILE]

Run it on the build of the commit whose bits are to be kept -- before a change that must not move them, or,
deliberately, after one that does.  It does nothing else.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the producing commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    assert len(commit) == 40, commit

    import torch
    import irdu_amd
    from tests import test_gpu_feature_bits as T

    assert torch.cuda.is_available() and T.device_arch() == T.ARCH, f"needs a {T.ARCH} device"
    irdu_amd.load_native()
    from irdu_amd import kernels
    fixture = {"arch": T.ARCH, "commit": commit, "digests": T.all_digests(kernels)}
    out = args.out or T.FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(fixture['digests'])} digests of commit {commit[:12]}")


if __name__ == "__main__":
    main()
