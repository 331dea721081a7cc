"""Numpy restatement of grr_patch_batch (include/grr.h): Philox4x32-10, the float64 Box-Muller normals, the
edge-repeating mirror and the patch batch itself, built from np.pad / np.rot90 / np.flipud."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 of uint32 counters [..., 4] and keys [..., 2] (broadcast against each other): [..., 4]."""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., k] for k in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def normals(seed, sample_id, count):
    """The first ``count`` float64 normals of a sample: element e is lane e % 4 of block e // 4."""
    seed, sample_id = int(seed), int(sample_id) & ((1 << 64) - 1)
    blocks = -(-count // 4)
    ctr = np.zeros((blocks, 4), np.uint64)
    ctr[:, 0] = np.arange(blocks, dtype=np.uint64)
    ctr[:, 2], ctr[:, 3] = sample_id & 0xFFFFFFFF, sample_id >> 32
    x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    z = np.empty((blocks, 4), np.float64)
    for h in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, h]))
        th = 6.283185307179586 * u[:, h + 1]
        z[:, h], z[:, h + 1] = r * np.cos(th), r * np.sin(th)
    return z.reshape(-1)[:count]


def sym(r, n):
    """Index r >= 0 of the mirror ...cba|abc...|cba... of n samples."""
    t = r % (2 * n)
    return t if t < n else 2 * n - 1 - t


def transform(a, mode):
    """T_mode of an H x W x C array: np.rot90(a, mode // 2), then np.flipud if mode is odd."""
    out = np.rot90(a, mode // 2)
    return np.flipud(out) if mode % 2 else out


def clean_patch(img, row, col, ph, pw):
    """The ph x pw x C patch at (row, col) of a uint8 image continued at the bottom / right by np.pad "symmetric":
    pixel (i, j) is image pixel (sym(row + i, H), sym(col + j, W))."""
    h, w = img.shape[:2]
    padded = np.pad(img, ((0, max(0, row + ph - h)), (0, max(0, col + pw - w)), (0, 0)), mode="symmetric")
    return padded[row:row + ph, col:col + pw]


PICTURE_SHAPES = ((40, 56), (100, 70), (130, 150), (820, 810))       # one above 800 on both sides: one 512 crop
GOLDEN_CONFIGS = {
    "aug16": dict(dist_mode="addictive_noise_scale", lambda_noise=25.0, use_data_aug=True, patch_size=(16, 16),
                  max_num_patchs=40, seed=2204),
    "vary64": dict(dist_mode="vary_addictive_noise", lambda_noise=[[15.0, 25.0, 50.0], [0.3, 0.4, 0.3]],
                   use_data_aug=False, patch_size=(64, 64), max_num_patchs=30, seed=77),
}


def picture(k, h, w, c=3):
    """Picture k of the dataset tests, uint8 h x w x c, from an integer formula."""
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((y * 7 + x * 13 + ch * 31 + ((y * x) % 17) * 5 + (y // 9) * (x // 11) + k * 11) % 256).astype(np.uint8)


def write_pictures(folder, shapes=PICTURE_SHAPES, c=3):
    """The pictures as PNG files in ``folder`` with their csv (index, path, height, width, nchannels): the csv's
    path and the pictures."""
    import os
    from PIL import Image
    pics, lines = [], ["index,path,height,width,nchannels"]
    for k, (h, w) in enumerate(shapes):
        pics.append(picture(k, h, w, c))
        Image.fromarray(pics[-1] if c != 1 else pics[-1][:, :, 0]).save(os.path.join(folder, f"pic{k}.png"))
        lines.append(f"{k},pic{k}.png,{h},{w},{c}")
    csv_path = os.path.join(folder, "info.csv")
    with open(csv_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return csv_path, pics


def patch_batch_ref(images, rows, sample_ids, sigma, seed, ph, pw):
    """(clean, noisy, noise) of grr_patch_batch, float32 [n, C, ph, pw] each; images: uint8 H x W x C arrays;
    rows: (img, row, col, mode)."""
    clean, noisy, noise = [], [], []
    for (im, row, col, mode), sid, sg in zip(rows, sample_ids, sigma):
        patch = transform(clean_patch(images[im], row, col, ph, pw), mode)
        c = patch.astype(np.float32) / np.float32(255.0)
        z = normals(seed, sid, c.size).reshape(c.shape)            # HWC order
        nz = (np.float64(np.float32(sg)) * z).astype(np.float32)
        clean.append(c.transpose(2, 0, 1))
        noise.append(nz.transpose(2, 0, 1))
        noisy.append((c + nz).transpose(2, 0, 1))
    return tuple(np.ascontiguousarray(np.stack(v)) for v in (clean, noisy, noise))
