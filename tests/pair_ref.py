"""Numpy restatement of grr_patch_pair_batch (include/grr.h), built from tests/patch_ref.py: the patch of the
target picture and the same patch of its degraded version, plus patch_ref's noise where a sigma is given."""
import os

import numpy as np

from tests.patch_ref import PICTURE_SHAPES, clean_patch, normals, picture, transform

DEGRADED = 17        # input picture k is patch_ref.picture(k + DEGRADED, ...): swapping the two files is visible


def pair_batch_ref(inputs, targets, rows, sample_ids, sigma, seed, ph, pw):
    """(target, input, noise) of grr_patch_pair_batch, float32 [n, C, ph, pw] each; inputs, targets: uint8
    H x W x C arrays, image i of one the degraded image i of the other; rows: (img, row, col, mode); sigma: one
    float per row, or None (no noise: input is the degraded patch over 255, noise is 0)."""
    target, inp, noise = [], [], []
    for s, ((im, row, col, mode), sid) in enumerate(zip(rows, sample_ids)):
        t = transform(clean_patch(targets[im], row, col, ph, pw), mode).astype(np.float32) / np.float32(255.0)
        d = transform(clean_patch(inputs[im], row, col, ph, pw), mode).astype(np.float32) / np.float32(255.0)
        if sigma is None:
            nz = np.zeros(d.shape, np.float32)
        else:
            z = normals(seed, sid, d.size).reshape(d.shape)            # HWC order
            nz = (np.float64(np.float32(sigma[s])) * z).astype(np.float32)
        target.append(t.transpose(2, 0, 1))
        noise.append(nz.transpose(2, 0, 1))
        inp.append((d + nz).transpose(2, 0, 1))
    return tuple(np.ascontiguousarray(np.stack(v)) for v in (target, inp, noise))


def write_pairs(folder, shapes=PICTURE_SHAPES, c=3, column=True):
    """Degraded and clean pictures as PNG files in ``folder`` with their csv (index, path, target_path, height,
    width, nchannels; column=False leaves target_path out): the csv's path, the inputs and the targets."""
    from PIL import Image
    inputs, targets = [], []
    lines = ["index,path,target_path,height,width,nchannels" if column else "index,path,height,width,nchannels"]
    for k, (h, w) in enumerate(shapes):
        targets.append(picture(k, h, w, c))
        inputs.append(picture(k + DEGRADED, h, w, c))
        for name, pic in ((f"noisy{k}.png", inputs[-1]), (f"clean{k}.png", targets[-1])):
            Image.fromarray(pic if c != 1 else pic[:, :, 0]).save(os.path.join(folder, name))
        lines.append(f"{k},noisy{k}.png,clean{k}.png,{h},{w},{c}" if column else f"{k},noisy{k}.png,{h},{w},{c}")
    csv_path = os.path.join(folder, "pairs.csv")
    with open(csv_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return csv_path, inputs, targets
