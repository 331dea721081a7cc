"""Golden plan and samples of the v2 patch dataset by running the REFERENCE (build container only).

Usage:  python tests/golden/make_golden_patches.py --ref <reference checkout>

Imports exploration/model_multiscale_mixture_GLR/lib/dataloader_v2.py with stand-in modules for the imports it
does not need here (cv2 -- copyMakeBorder(BORDER_REFLECT) is np.pad(..., "symmetric") --, torchvision, skimage),
builds ImageSuperResolution on the pictures of tests/patch_ref.py for each of its GOLDEN_CONFIGS and records,
as data only, into tests/golden/patches_v2.npz:
  <name>/plan      int64 [n, 4]: (picture, row, col, padding) of patchs_data, after the permutation
  <name>/noisy, <name>/clean   float32 [6, h, w, 3]: samples 0..5, fetched in that order right after construction
"""
import argparse
import logging
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import patch_ref  # noqa: E402

N_SAMPLES = 6


def stand_ins():
    cv2 = types.ModuleType("cv2")
    cv2.BORDER_REFLECT = 2

    def copy_make_border(a, top, bottom, left, right, kind):
        assert kind == cv2.BORDER_REFLECT
        return np.pad(a, ((top, bottom), (left, right), (0, 0)), mode="symmetric")
    cv2.copyMakeBorder = copy_make_border
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvt.ToTensor = object
    tv.transforms = tvt
    for name, mod in (("cv2", cv2), ("torchvision", tv), ("torchvision.transforms", tvt),
                      ("skimage", types.ModuleType("skimage"))):
        sys.modules.setdefault(name, mod)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    args = ap.parse_args()
    stand_ins()
    sys.path.insert(0, os.path.join(args.ref, "exploration", "model_multiscale_mixture_GLR", "lib"))
    import dataloader_v2
    out = {}
    with tempfile.TemporaryDirectory() as folder:
        csv_path, _ = patch_ref.write_pictures(folder)
        index = {os.path.join(folder, f"pic{k}.png"): k for k in range(len(patch_ref.PICTURE_SHAPES))}
        for name, conf in patch_ref.GOLDEN_CONFIGS.items():
            ds = dataloader_v2.ImageSuperResolution(csv_path=csv_path, root_folder=folder,
                                                    logger=logging.getLogger("golden"), **conf)
            pd = ds.patchs_data
            out[name + "/plan"] = np.array([(index[p], r, c, int(pad)) for r, c, pad, p in
                                            zip(pd["row"], pd["col"], pd["padding"], pd["path"])], dtype=np.int64)
            pairs = [ds[i] for i in range(N_SAMPLES)]
            out[name + "/noisy"] = np.stack([n.numpy() for n, _ in pairs]).astype(np.float32)
            out[name + "/clean"] = np.stack([c.numpy() for _, c in pairs]).astype(np.float32)
    path = os.path.join(HERE, "patches_v2.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
