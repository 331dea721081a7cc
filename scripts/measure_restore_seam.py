"""Seam error of restore_image's windows for the four-level v1.0 model.

    python scripts/measure_restore_seam.py [--yaml experiment_conf/c4_train.yaml] [--size 1024] [--tile 512] [--halos 64 96]

One noisy size^2 RGB float image that fits one window is restored whole (tile = size) and in windows of
``tile`` at each halo; prints one JSON line per halo: max |tiled - whole| / max |whole| of the float
outputs, how many uint8 levels differ, and the wall time of one tiled call.  The model is the YAML's, at its initial weights, and again with
the solver scalars moved off their near-zero initial values (as __graft_entry__.smoke does) so that every
graph term acts; no trained v1.0 weights ship with the repository.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default=os.path.join(ROOT, "experiment_conf", "c4_train.yaml"))
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--halos", type=int, nargs="+", default=[64, 96])
    args = ap.parse_args()
    import irdu_amd
    from irdu_amd import training
    from bench import synthetic_patches
    irdu_amd.load_native()
    torch.manual_seed(2204)
    model = training.build_model(training.parse_options(args.yaml)["model"]).to("cuda").eval()
    _, noisy = synthetic_patches(1, seed=2204, h=args.size, w=args.size)
    img = noisy[0].permute(1, 2, 0).contiguous().numpy()
    for weights in ("initial", "solver scalars moved"):
        if weights != "initial":
            with torch.no_grad():
                for name, p in model.named_parameters():
                    leaf = name.rsplit(".", 1)[-1]
                    if leaf[:-2] in ("muys", "ro"):
                        p.fill_(-1.5)
                    elif leaf[:-2] == "gamma":
                        p.fill_(-4.0)
        whole = irdu_amd.restore_image(model, img, tile=args.size, halo=32, quantise=False)
        whole8 = irdu_amd.restore_image(model, img, tile=args.size, halo=32)
        for halo in args.halos:
            tiled = irdu_amd.restore_image(model, img, tile=args.tile, halo=halo, micro_batch=4, quantise=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tiled8 = irdu_amd.restore_image(model, img, tile=args.tile, halo=halo, micro_batch=4)
            ms = (time.perf_counter() - t0) * 1e3     # the second call at this shape; the result is on the host
            d8 = np.abs(tiled8.astype(np.int16) - whole8.astype(np.int16))
            print(json.dumps({"model": os.path.basename(args.yaml), "weights": weights, "size": args.size,
                              "tile": args.tile, "halo": halo,
                              "windows": len(irdu_amd.plan(args.size, args.size, 16, args.tile, halo).windows),
                              "rel_err_vs_whole": float(np.abs(tiled - whole).max() / np.abs(whole).max()),
                              "uint8_levels_differing": int((d8 > 0).sum()), "uint8_max_diff": int(d8.max()),
                              "pixels_x_channels": int(d8.size), "ms_per_image": round(ms, 1)}), flush=True)


if __name__ == "__main__":
    main()
