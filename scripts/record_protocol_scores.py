"""Write tests/golden/protocol_scores_gfx950.json: the scores of the super-resolution, JPEG and demosaicking protocols
that tests/test_gpu_protocol_scores.py pins, computed on a gfx950 device through the public evaluate_* and validate_*
functions of the tree it runs in.

    python scripts/record_protocol_scores.py --commit <id of the commit of the tree> [--out FILE]

Run it on the commit whose scores are to be kept -- before a change to the host code that must not move them, or,
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
    from tests import test_gpu_protocol_scores as T

    assert torch.cuda.is_available() and T.device_arch() == T.ARCH, f"needs a {T.ARCH} device"
    irdu_amd.load_native()
    from irdu_amd import restore, training
    fixture = {"arch": T.ARCH, "commit": commit, "scores": T.all_scores(restore, training)}
    out = args.out or T.FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(fixture['scores'])} scores of commit {commit[:12]}")


if __name__ == "__main__":
    main()
