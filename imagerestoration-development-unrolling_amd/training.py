"""Training engine: the reference's run_train.py / experiment_conf YAML surface on the HIP path.

Mirrors (reference paths):
  run_train.py:20-121                      parse_options, checkpoint discovery, logger, dataset/dataloader
  environ/utils/custom_parser.py:23-30     YAML -> dict
  environ/data/__init__.py:29-69           create_dataset (by ``type``), create_dataloader
  environ/data/data_sampler.py:6-31        ResumeableSampler (resume inside an epoch)
  environ/data/images_pair_restoration_dataset.py:15-116
                                           AddictiveGaussianNoiseImagePair (patch grid, permute, noise)
  exploration/model_multiscale_mixture_GLR/scripts_v2/run_abtract_lightformer_GGTV_GGLR_sigma25.py
    :120-151  model / losses (L1 + 0.1 MSE(enc-dec) + 0.5 MSE(latent-perturbed decode))
    :153-171  Adam(4e-4, eps 1e-8), MultiStepLR(gamma = 0.5**0.25) -> CosineAnnealingLR (SequentialLR)
    :186-224  training step, checkpoint dict {'i', 'model', 'optimizer', 'lr_scheduler'}
    :235-288  periodic validation: reflect-pad to x16, crop, clamp, img_as_ubyte, mean PSNR (validate)

The reference's run_train.py stops after building the dataloader; the YAML here adds
``model:`` and ``train:`` sections so the same entry point runs the training loop of the
v2 scripts.  Multi-GPU: one process per GPU (torchrun); every rank trains on its own
slice of each global batch and gradients are averaged with bucketed RCCL all-reduces
(sharding.OverlappedGradReducer, launched from backward hooks so they overlap the
reverse sweep) — the only collective of the path.

Datasets: no image data ships with the reference, so ``SyntheticNoisyPatches`` (seeded
procedural clean patches, the same noise law) is the default; the CSV/PNG dataset type
is kept for real data.  Samples are (noisy, clean) HWC float32 like the reference's.
``ImageSuperResolution`` is the v2 scripts' own training set (exploration/model_multiscale_mixture_GLR/
lib/dataloader_v2.py:70-242); a stage with ``device_resident: true`` reads it through ``DevicePatchLoader``,
which keeps the decoded pictures on the GPU and makes each planar batch there (csrc/image_ops.hip:
grr_patch_batch).
``PairedImageRestoration`` is the same patch plan over degraded / clean file pairs (real camera noise, JPEG
artefacts, blur, rain): nothing is synthesised unless a noise mode asks for it.  Its device-resident stage holds
two arenas under one image table (grr_patch_pair_batch), ``TestPairsCSV`` lists pairs for the periodic validation
and ``validate_pairs`` scores them with restore.evaluate_pairs.
``BicubicSuperResolution`` is that plan over clean files alone for bicubic super-resolution: the input is the picture
degraded by the exact bicubic down and up at an integer scale (``bicubic_degrade_u8`` on the host; on the device
csrc/resize_ops.hip makes the degraded arena from the clean one), and ``validate_sr`` scores the protocol on a
``TestImagesCSV`` set with restore.evaluate_sr.
``JpegArtifactRemoval`` is the same over clean files for JPEG compression-artifact removal: the input is the picture
after the JPEG round trip at a quality of 1..100 (``jpeg_degrade_u8`` on the host, Pillow's bytes; on the device
csrc/jpeg_ops.hip makes the degraded arena), and ``validate_car`` scores it on a ``TestImagesCSV`` set with a
``jpeg_quality`` key through restore.evaluate_car.
``BayerDemosaicking`` is the third of the kind, for demosaicking: the input is the picture sampled through a Bayer
colour filter array with its missing channels filled by a fixed integer filter (``demosaic_degrade_u8`` on the host;
on the device csrc/demosaic_ops.hip makes the filled arena), and ``validate_demosaic`` scores it on a
``TestImagesCSV`` set with a ``bayer`` key through restore.evaluate_demosaic.
``GaussianMotionDeblurring`` is the fourth, for deblurring: the input is the picture convolved with an integer
point-spread function -- Gaussian, box, motion or from a file (``parse_blur_spec``, ``blur_degrade_u8`` on the host; on
the device csrc/blur_ops.hip makes the blurred arena) -- and ``validate_deblur`` scores it on a ``TestImagesCSV`` set
with a ``blur`` key through restore.evaluate_deblur.
"""
from __future__ import annotations

import argparse
import json
import logging
import math
import os
import random
from typing import Callable, Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import yaml
from torch.utils.data import Dataset, Sampler

from . import losses, sharding, stream_guard

LOG = logging.getLogger("irdu_amd.train")


def miopen_training_defaults() -> None:
    """Process-wide MIOpen setting for the training entry points (run_train.py / training.main,
    bench_train.py), never applied on import: MIOPEN_DEBUG_DISABLE_FIND_DB=1 unless the environment
    already sets it.  The stock convolutions outside the graph path (the v1.0 model's embedding,
    down/up-sampling and channel combines) run on MIOpen; with MIOpen's user find-db filled by an earlier
    process its immediate mode spends host time per call -- the C4 training step (v1.0, 32 x 512^2) went
    1.03 s (fresh box) -> 2.7-4.0 s on every later run, GPU kernel time unchanged at 1.09 s; with the
    find-db off every run stays at 1.02-1.03 s (profiles/r04/miopen/).  MIOpen reads the
    variable at its first convolution, so call this before any convolution runs in the process."""
    os.environ.setdefault("MIOPEN_DEBUG_DISABLE_FIND_DB", "1")


# ---------------------------------------------------------------------------
# options (run_train.py:20-36, custom_parser.py:23-30, small_utils.py:12-18)
# ---------------------------------------------------------------------------
def parse(yaml_file_path: str) -> dict:
    with open(yaml_file_path) as f:
        return yaml.safe_load(f)


def set_random_seed(seed: int = 2204) -> None:
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def parse_options(yaml_path: str) -> dict:
    conf = parse(yaml_path)
    if conf.get("manual_seed") is None:
        conf["manual_seed"] = random.randint(1, 10000)
    set_random_seed(conf["manual_seed"])
    return conf


# ---------------------------------------------------------------------------
# data (environ/data/*)
# ---------------------------------------------------------------------------
def _noisy(patch: np.ndarray, rs: np.random.RandomState, dist_mode: str, lambda_noise) -> np.ndarray:
    """images_pair_restoration_dataset.py:101-110: additive Gaussian noise, sigma = lambda/255;
    vary_addictive_noise (model_multiscale_mixture_GLR/lib/dataloader.py:165-169): lambda_noise =
    [levels, probabilities], one level drawn per patch."""
    if dist_mode == "addictive_noise":
        noise = rs.normal(loc=0.0, scale=lambda_noise / 255.0, size=patch.shape)
    elif dist_mode == "vary_addictive_noise":
        level = rs.choice(lambda_noise[0], p=lambda_noise[1])
        noise = rs.normal(loc=0.0, scale=level / 255.0, size=patch.shape)
    elif dist_mode == "addictive_noise_scale":
        noise = rs.normal(loc=0.0, scale=1.0, size=patch.shape) * (lambda_noise / 255.0)
    else:
        raise ValueError(f"unknown dist_mode {dist_mode!r}")
    return patch + noise.astype(np.float32)


class AddictiveGaussianNoiseImagePair(Dataset):
    """CSV-indexed image patches + noise (images_pair_restoration_dataset.py:15-116).
    csv columns: index, path, height, width (as the reference's *_info.csv)."""

    def __init__(self, csv_path, dist_mode="", lambda_noise=None, patch_size=64, patch_overlap_size=32,
                 max_num_patchs=100000, root_folder="", logger_name=None, device_str="cpu", n_channels=3):
        import pandas as pd
        self.img_infos = pd.read_csv(csv_path, index_col="index")
        self.patch_size, self.patch_overlap_size = patch_size, patch_overlap_size
        self.root_folder, self.lambda_noise, self.dist_mode = root_folder, lambda_noise, dist_mode
        self.n_channels = n_channels
        rows = []
        step = patch_size - patch_overlap_size
        for i in range(self.img_infos.shape[0]):
            info = self.img_infos.iloc[i]
            path = os.path.join(root_folder, info["path"])
            for r in np.arange(0, info["height"] - patch_size, step):
                for c in np.arange(0, info["width"] - patch_size, step):
                    rows.append((int(r), int(c), path))
        self.patchs_data_all = rows
        self.max_num_patchs = min(max_num_patchs, len(rows))
        self.random_permute(seed=2204)

    def random_permute(self, seed=2204):
        self.random_state = np.random.RandomState(seed=seed)
        ind = self.random_state.permutation(self.max_num_patchs)
        self.patchs_data = [self.patchs_data_all[i] for i in ind]

    def __len__(self):
        return len(self.patchs_data)

    def __getitem__(self, idx):
        from PIL import Image
        row, col, path = self.patchs_data[idx]
        img = np.array(Image.open(path))
        patch = img[row:row + self.patch_size, col:col + self.patch_size, :]
        h, w = (patch.shape[0] // 16) * 16, (patch.shape[1] // 16) * 16
        patch = patch[:h, :w].astype(np.float32) / 255.0
        dist = _noisy(patch, self.random_state, self.dist_mode, self.lambda_noise)
        return torch.from_numpy(dist), torch.from_numpy(patch)


def synthetic_clean_patch(rs: np.random.RandomState, h: int, w: int, c: int) -> np.ndarray:
    """Piecewise-smooth clean patch on the uint8 grid (sinusoid background + rectangles), HWC."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((h, w, c), np.float32)
    for ch in range(c):
        fy, fx, ph = rs.uniform(0.5, 4.0), rs.uniform(0.5, 4.0), rs.uniform(0, 6.28)
        img = 0.5 + 0.3 * np.sin(2 * np.pi * fy * yy / h + ph) * np.cos(2 * np.pi * fx * xx / w)
        for _ in range(3):
            r0, c0 = rs.randint(0, max(1, h - h // 4)), rs.randint(0, max(1, w - w // 4))
            img[r0:r0 + rs.randint(4, max(5, h // 3)), c0:c0 + rs.randint(4, max(5, w // 3))] += rs.uniform(-0.3, 0.3)
        out[..., ch] = img
    return (np.round(np.clip(out, 0, 1) * 255.0) / 255.0).astype(np.float32)


class SyntheticNoisyPatches(Dataset):
    """Deterministic synthetic (noisy, clean) patch pairs: sample i is a function of (seed, i)."""

    def __init__(self, dist_mode="addictive_noise_scale", lambda_noise=25.0, patch_size=64, max_num_patchs=1000,
                 n_channels=3, seed=2204, **_ignored):
        self.dist_mode, self.lambda_noise = dist_mode, lambda_noise
        self.patch_size, self.n_channels, self.seed = patch_size, n_channels, seed
        self.max_num_patchs = max_num_patchs
        self.random_permute(seed=2204)

    def random_permute(self, seed=2204):
        self.order = np.random.RandomState(seed).permutation(self.max_num_patchs)

    def __len__(self):
        return self.max_num_patchs

    def __getitem__(self, idx):
        rs = np.random.RandomState((self.seed * 1000003 + int(self.order[idx])) % (2 ** 32))
        clean = synthetic_clean_patch(rs, self.patch_size, self.patch_size, self.n_channels)
        return torch.from_numpy(_noisy(clean, rs, self.dist_mode, self.lambda_noise)), torch.from_numpy(clean)


def data_augmentation(image: np.ndarray, mode: int) -> np.ndarray:
    """lib/dataloader_v2.py:23-66: mode m = 2k + f is np.rot90(image, k), then np.flipud if f."""
    out = np.rot90(image, k=mode // 2)
    return (np.flipud(out) if mode % 2 else out).copy()


class ImageSuperResolution(Dataset):
    """The v2 scripts' training set (model_multiscale_mixture_GLR/lib/dataloader_v2.py:70-242; csv columns
    index, path, height, width, nchannels): pictures with both sides above 800 are cut into 512-pixel crops every
    416 pixels (:111-153), every pass over the crops takes one random patch per crop (:155-188), and one
    RandomState(seed) then permutes and cuts the list to max_num_patchs (:190-193).  A crop no larger than the
    patch gives the patch at its origin, filled at the bottom and right by OpenCV's BORDER_REFLECT, the
    edge-repeating mirror ...cba|abc...|cba... (np.pad "symmetric").  ``__getitem__`` is the reference's host
    path (:195-242): (noisy, clean) float32 HWC, the augmentation mode and the noise drawn from that same
    stream, so a sample depends on everything drawn before it.  The reference draws the mode as randint(0, 7),
    modes 0..6; this path keeps that.  DevicePatchLoader is the path that does not depend on the draw order.

    Beyond the reference: ``n_channels`` (a picture with another channel count is a ValueError naming the file,
    where the reference fails with an index error), an int ``patch_size`` means a square, and a non-square patch
    with use_data_aug is refused (the odd quarter turns change the shape; the reference's collation would fail)."""

    IMG_SIZE, OVERLAP, MAX_SIZE = 512, 96, 800
    DIST_MODES = ("addictive_noise", "vary_addictive_noise", "addictive_noise_scale")

    def __init__(self, csv_path, dist_mode, lambda_noise, use_data_aug=False, patch_size=(64, 64),
                 max_num_patchs=100000, root_folder="", logger=None, device=None, seed=2204, n_channels=3):
        import pandas as pd
        if isinstance(patch_size, int):
            patch_size = (patch_size, patch_size)
        self.patch_size = (int(patch_size[0]), int(patch_size[1]))
        if use_data_aug and self.patch_size[0] != self.patch_size[1]:
            raise ValueError(f"ImageSuperResolution: use_data_aug needs a square patch (the odd quarter turns change "
                             f"the shape), got {self.patch_size}")
        if dist_mode not in self.DIST_MODES:
            raise ValueError(f"unknown dist_mode {dist_mode!r}")
        self.img_infos = pd.read_csv(csv_path, index_col="index")
        self.max_num_patchs = max_num_patchs
        self.device, self.root_folder, self.lambda_noise = device, root_folder, lambda_noise
        self.use_data_augmentation, self.dist_mode = bool(use_data_aug), dist_mode
        self.logger = logger if logger is not None else LOG
        self.seed, self.n_channels, self.epoch = int(seed), int(n_channels), 0
        self.create_all_images()
        self.random_state = np.random.RandomState(seed=seed)
        self.create_patchs(self.max_num_patchs)
        self.random_permute_subselect_patchs_data(self.max_num_patchs)

    def __len__(self):
        return len(self.patchs_data)

    def create_all_images(self):
        """:111-153: (row, col, height, width, nchannels, image) per crop; ``paths`` lists the files."""
        size, step = self.IMG_SIZE, self.IMG_SIZE - self.OVERLAP
        self.paths, crops = [], []
        for i in range(self.img_infos.shape[0]):
            info = self.img_infos.iloc[i]
            height, width, nchannels = int(info["height"]), int(info["width"]), int(info["nchannels"])
            self.paths.append(os.path.join(self.root_folder, info["path"]))
            if width > self.MAX_SIZE and height > self.MAX_SIZE:
                for r in np.arange(0, height - size, step):
                    for c in np.arange(0, width - size, step):
                        crops.append((int(r), int(c), size, size, nchannels, i))
            else:
                crops.append((0, 0, height, width, nchannels, i))
        self.images_data_all = crops
        self.logger.info(f"Dataset - Create total {len(crops)} cropped images")

    def create_patchs(self, max_num_patchs):
        """:155-188: rows (row, col, padding, image)."""
        ph, pw = self.patch_size
        rows = []
        for _ in range(max_num_patchs // len(self.images_data_all) + 1):
            for row, col, height, width, nchannels, img in self.images_data_all:
                if nchannels > 3:
                    continue
                if ph < height and pw < width:
                    r = row + self.random_state.randint(0, height - ph)
                    c = col + self.random_state.randint(0, width - pw)
                    rows.append((int(r), int(c), False, img))
                else:
                    rows.append((row, col, True, img))
        self.patchs_data_all = rows
        self.logger.info(f"Dataset - Create total {len(rows)} patchs")

    def _select(self, ind):
        self.patchs_data = [self.patchs_data_all[i] for i in ind]
        # the same selection as int64 [n, 3] rows (image, row, col), for the device path
        self.plan = np.array([(img, r, c) for r, c, _, img in self.patchs_data], dtype=np.int64).reshape(-1, 3)

    def random_permute_subselect_patchs_data(self, max_num_patchs):
        """:190-193, on the constructor's stream."""
        self.logger.info(f"Dataset - Permute and select {max_num_patchs}/{len(self.patchs_data_all)} patchs")
        self._select(self.random_state.permutation(len(self.patchs_data_all))[:max_num_patchs])

    def random_permute(self, seed=2204):
        """What ResumeableSampler.set_epoch_and_current_sample calls with 2024 + epoch: the selection is re-drawn
        from the fixed patch list by RandomState(seed) alone, and the epoch is kept for the device path."""
        self._select(np.random.RandomState(seed).permutation(len(self.patchs_data_all))[:self.max_num_patchs])
        self.epoch = int(seed) - 2024

    def load_image(self, img: int) -> np.ndarray:
        """File ``img`` of ``paths`` as uint8 H x W x n_channels."""
        return self._load(self.paths[img])

    def _load(self, path: str) -> np.ndarray:
        from PIL import Image
        a = np.array(Image.open(path))
        if a.ndim == 2 and self.n_channels == 1:
            a = a[:, :, None]
        if a.ndim != 3 or a.shape[2] != self.n_channels or a.dtype != np.uint8:
            raise ValueError(f"ImageSuperResolution: {path} is {a.dtype} {a.shape}, not an 8-bit picture of "
                             f"{self.n_channels} channel(s)")
        return a

    def out_size(self) -> Tuple[int, int]:
        """The sample's sides: the patch cut to multiples of 16 (:208-212)."""
        return (self.patch_size[0] // 16) * 16, (self.patch_size[1] // 16) * 16

    def _cut(self, image: np.ndarray, row: int, col: int, need_padding: bool) -> np.ndarray:
        """The sample's uint8 patch of a decoded picture (:199-212), before the augmentation."""
        ph, pw = self.patch_size
        patch = image[row:row + ph, col:col + pw, :]
        if need_padding:
            patch = np.pad(patch, ((0, ph - patch.shape[0]), (0, pw - patch.shape[1]), (0, 0)), mode="symmetric")
        h_, w_ = (patch.shape[0] // 16) * 16, (patch.shape[1] // 16) * 16
        return patch[0:h_, 0:w_]

    def __getitem__(self, idx):
        row, col, need_padding, img_i = self.patchs_data[idx]
        patch = self._cut(self.load_image(img_i), row, col, need_padding)
        if self.use_data_augmentation:
            patch = data_augmentation(patch, self.random_state.randint(0, 7))
        patch = patch.astype(np.float32) / 255.0
        dist = _noisy(patch, self.random_state, self.dist_mode, self.lambda_noise)
        return torch.from_numpy(dist), torch.from_numpy(patch)


class PairedImageRestoration(ImageSuperResolution):
    """Degraded / clean file pairs under ImageSuperResolution's crop and patch plan (csv columns index, path,
    target_path, height, width, nchannels; ``path`` is the degraded file, ``target_path`` its ground truth of the
    same size, dtype and channels).  The plan is the parent's, unchanged -- 512 crops every 416 pixels, one random
    patch per crop per pass, the permutation -- so equal seeds and sizes select the same (image, row, col) rows.
    ``dist_mode``: "none" (default) leaves the degraded picture as it is; the parent's three additive modes add
    their noise on top of it.  ``__getitem__`` makes the parent's draws in the parent's order (the mode when
    augmenting, then the noise unless "none") and returns (input, target) float32 HWC, both cut and turned alike."""

    DIST_MODES = ("none",) + ImageSuperResolution.DIST_MODES

    def __init__(self, csv_path, dist_mode="none", lambda_noise=None, use_data_aug=False, patch_size=(64, 64),
                 max_num_patchs=100000, root_folder="", logger=None, device=None, seed=2204, n_channels=3):
        super().__init__(csv_path, dist_mode, lambda_noise, use_data_aug=use_data_aug, patch_size=patch_size,
                         max_num_patchs=max_num_patchs, root_folder=root_folder, logger=logger, device=device,
                         seed=seed, n_channels=n_channels)

    def create_all_images(self):
        if "target_path" not in self.img_infos.columns:
            raise ValueError("PairedImageRestoration: the csv needs a target_path column (index, path, target_path, "
                             f"height, width, nchannels), got {list(self.img_infos.columns)}")
        super().create_all_images()
        self.target_paths = [os.path.join(self.root_folder, p) for p in self.img_infos["target_path"].tolist()]

    def load_target(self, img: int, like: Optional[np.ndarray] = None) -> np.ndarray:
        """The ground truth of file ``img`` as uint8 H x W x n_channels; it must have the dtype, shape and channels
        of its input (``like``: that input where the caller has decoded it already, else it is decoded here)."""
        from PIL import Image
        path = self.target_paths[img]
        a = np.array(Image.open(path))
        if a.ndim == 2 and self.n_channels == 1:
            a = a[:, :, None]
        if like is None:
            like = self.load_image(img)
        if a.dtype != like.dtype or a.shape != like.shape:
            raise ValueError(f"PairedImageRestoration: target {path} is {a.dtype} {a.shape}, its input "
                             f"{self.paths[img]} is {like.dtype} {like.shape}: a pair has one dtype, size and channel "
                             "count")
        return a

    def __getitem__(self, idx):
        row, col, need_padding, img_i = self.patchs_data[idx]
        degraded = self.load_image(img_i)
        inp = self._cut(degraded, row, col, need_padding)
        tgt = self._cut(self.load_target(img_i, degraded), row, col, need_padding)
        if self.use_data_augmentation:
            mode = self.random_state.randint(0, 7)
            inp, tgt = data_augmentation(inp, mode), data_augmentation(tgt, mode)
        inp, tgt = inp.astype(np.float32) / 255.0, tgt.astype(np.float32) / 255.0
        if self.dist_mode != "none":
            inp = _noisy(inp, self.random_state, self.dist_mode, self.lambda_noise)
        return torch.from_numpy(inp), torch.from_numpy(tgt)


def _bicubic_pass_u8(a: np.ndarray, s: int, up_to: Optional[int]) -> np.ndarray:
    """One 1-D pass of the exact bicubic resize along axis 0 of a uint8 [n, ...] array (include/grr.h): down to
    ceil(n / s) rows (up_to None) or up to ``up_to`` rows.  One int64 multiply-add over the whole output per tap."""
    from . import kernels
    n = a.shape[0]
    is_up = up_to is not None
    length = up_to if is_up else -(-n // s)
    sets = kernels.resize_taps(s, is_up)
    src = a.astype(np.int64)
    acc = np.zeros((length,) + a.shape[1:], np.int64)
    y = np.arange(length, dtype=np.int64)
    for p, taps in enumerate(sets):
        rows = y[y % s == p] if is_up else y
        base = rows // s if is_up else rows * s
        for off, q in taps:
            t = (base + off) % (2 * n)                                   # numpy's %: non-negative
            acc[rows] += np.int64(q) * src[np.where(t < n, t, 2 * n - 1 - t)]
    return np.clip((acc + (1 << 29)) >> 30, 0, 255).astype(np.uint8)


def _bicubic_resize_u8(a: np.ndarray, s: int, out_hw) -> np.ndarray:
    rows = _bicubic_pass_u8(a, s, None if out_hw is None else out_hw[0])
    cols = _bicubic_pass_u8(rows.transpose(1, 0, 2), s, None if out_hw is None else out_hw[1])
    return np.ascontiguousarray(cols.transpose(1, 0, 2))


def bicubic_degrade_u8(a: np.ndarray, s: int) -> np.ndarray:
    """The bicubic super-resolution input of a uint8 H x W x C picture on the CPU, at its size: the exact
    antialiased bicubic down by the integer scale ``s`` (2..8) and the bicubic back up to H x W, rows first and a
    rounding to uint8 after each 1-D pass (include/grr.h; MATLAB imresize's convention with fixed-point weights).
    The same integers as kernels.u8_bicubic_degrade, bit for bit: it serves the host DataLoader path and users
    without a GPU."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError(f"bicubic_degrade_u8: expected a uint8 H x W x C picture, got {a.dtype} {a.shape}")
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 2 <= s <= 8:
        raise ValueError(f"bicubic_degrade_u8: the scale is an integer of 2..8, got {s!r}")
    s = int(s)
    return _bicubic_resize_u8(_bicubic_resize_u8(a, s, None), s, a.shape[:2])


_JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
              14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def jpeg_quality_table(quality: int, chroma: bool = False) -> np.ndarray:
    """The int64 8 x 8 quantisation table of ``quality`` (1..100) in natural order: libjpeg's scaling of the
    Annex-K luminance (or chrominance) table, clamp((base scale + 50) / 100, 1, 255) with scale = 5000 / q below 50
    and 200 - 2 q from 50 on.  100 gives all ones, 50 the base table."""
    if isinstance(quality, (bool, np.bool_)) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_quality_table: the quality is an integer of 1..100, got {quality!r}")
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array(_JPEG_CHROMA if chroma else _JPEG_LUMA, np.int64).reshape(8, 8)
    return np.clip((base * scale + 50) // 100, 1, 255)


def _jpeg_odd(a, b, c, d):
    """The odd part jfdctint and jidctint share (include/grr.h, ODD)."""
    z5 = 9633 * (a + b + c + d)
    z1, z2, z3, z4 = -7373 * (a + d), -20995 * (b + c), z5 - 16069 * (a + c), z5 - 3196 * (b + d)
    return 2446 * a + z1 + z3, 16819 * b + z2 + z4, 25172 * c + z2 + z3, 12299 * d + z1 + z4


def _jpeg_pass(x: np.ndarray, axis: int, inverse: bool, shift: int, dc_shift: int) -> np.ndarray:
    """One 1-D pass of the integer DCT along ``axis`` (of length 8) of an int64 array: the forward pass rounds
    outputs 0 and 4 by ``dc_shift`` (negative: a left shift) and the others by ``shift``; the inverse rounds all by
    ``shift``."""
    d = np.moveaxis(x, axis, 0)
    rnd = lambda v, n: (v + (1 << (n - 1))) >> n
    out = np.empty_like(d)
    if inverse:
        z1 = 4433 * (d[2] + d[6])
        t2, t3 = z1 - 15137 * d[6], z1 + 6270 * d[2]
        t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
        even = (t0 + t3, t1 + t2, t1 - t2, t0 - t3)
        odd = _jpeg_odd(d[7], d[5], d[3], d[1])
        for k in range(4):
            out[k], out[7 - k] = rnd(even[k] + odd[3 - k], shift), rnd(even[k] - odd[3 - k], shift)
    else:
        t = [d[k] + d[7 - k] for k in range(4)] + [d[3 - k] - d[4 + k] for k in range(4)]     # t0..t3, t4..t7
        t10, t13, t11, t12 = t[0] + t[3], t[0] - t[3], t[1] + t[2], t[1] - t[2]
        for k, v in ((0, t10 + t11), (4, t10 - t11)):
            out[k] = v << -dc_shift if dc_shift < 0 else rnd(v, dc_shift)
        z1 = 4433 * (t12 + t13)
        out[2], out[6] = rnd(z1 + 6270 * t13, shift), rnd(z1 - 15137 * t12, shift)
        for k, v in zip((7, 5, 3, 1), _jpeg_odd(t[4], t[5], t[6], t[7])):
            out[k] = rnd(v, shift)
    return np.moveaxis(out, 0, axis)


def _jpeg_plane(p: np.ndarray, table: np.ndarray) -> np.ndarray:
    """An int64 [h, w] plane of samples 0..255 through the forward DCT, the quantiser and the inverse DCT."""
    h, w = p.shape
    p = np.pad(p, ((0, -h % 8), (0, -w % 8)), mode="edge") - 128
    b = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8)            # [block row, row, block column, column]
    b = _jpeg_pass(_jpeg_pass(b, 3, False, 11, -2), 1, False, 15, 2)
    tab = table[None, :, None, :]
    b = np.sign(b) * ((np.abs(b) + 4 * tab) // (8 * tab)) * tab
    b = _jpeg_pass(_jpeg_pass(b, 1, True, 11, 0), 3, True, 18, 0)
    return np.clip(b + 128, 0, 255).reshape(p.shape)[:h, :w]


def _jpeg_chroma_420(p: np.ndarray, table: np.ndarray) -> np.ndarray:
    """A full-resolution int64 chroma plane down to 4:2:0, through the codec and back up to its size."""
    h, w = p.shape
    ch, cw = -(-h // 2), -(-w // 2)
    q = np.pad(p, ((0, h % 2), (0, -w % 16)), mode="edge")
    q = q.reshape(ch, 2, q.shape[1] // 2, 2).sum(axis=(1, 3))
    q = (q + 1 + (np.arange(q.shape[1]) & 1)) >> 2
    c = _jpeg_plane(q, table)[:, :cw]
    if cw <= 2:                                                       # libjpeg's triangle filter is off
        return c.repeat(2, axis=0).repeat(2, axis=1)[:h, :w]
    above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.stack([3 * c + above, 3 * c + below], axis=1).reshape(2 * ch, cw)      # even rows look up, odd down
    left = np.concatenate([4 * s[:, :1], 3 * s[:, 1:] + s[:, :-1]], axis=1) + 8
    right = np.concatenate([3 * s[:, :-1] + s[:, 1:], 4 * s[:, -1:]], axis=1) + 7
    return (np.stack([left, right], axis=2).reshape(2 * ch, 2 * cw) >> 4)[:h, :w]


def jpeg_degrade_u8(a: np.ndarray, quality: int, subsampling: int = 0) -> np.ndarray:
    """The JPEG round trip of a uint8 H x W x C picture (C of 1 or 3) on the CPU: what decoding its baseline JPEG of
    ``quality`` (1..100) gives, in libjpeg's integer arithmetic and without a bitstream (include/grr.h) -- the bytes
    Pillow's ``save(format="JPEG", quality=q, subsampling=s)`` followed by ``open`` returns.  ``subsampling``: 0 for
    4:4:4, 2 for 4:2:0; a gray picture ignores it.  The same integers as kernels.u8_jpeg, bit for bit: it serves
    the host DataLoader path and users without a GPU."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3) or 0 in a.shape:
        raise ValueError(f"jpeg_degrade_u8: expected a uint8 H x W x 1 or H x W x 3 picture, got {a.dtype} {a.shape}")
    if isinstance(subsampling, (bool, np.bool_)) or not isinstance(subsampling, (int, np.integer)) \
            or subsampling not in (0, 2):
        raise ValueError(f"jpeg_degrade_u8: the subsampling is 0 (4:4:4) or 2 (4:2:0), got {subsampling!r}")
    try:
        luma, chroma = jpeg_quality_table(quality), jpeg_quality_table(quality, True)
    except ValueError:
        raise ValueError(f"jpeg_degrade_u8: the quality is an integer of 1..100, got {quality!r}") from None
    x = a.astype(np.int64)
    if a.shape[2] == 1:
        return _jpeg_plane(x[:, :, 0], luma).astype(np.uint8)[:, :, None]
    F = lambda v: int(v * 65536 + 0.5)
    r, g, b = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    y = (F(.299) * r + F(.587) * g + F(.114) * b + 32768) >> 16
    cb = (-F(.16874) * r - F(.33126) * g + F(.5) * b + (128 << 16) + 32767) >> 16
    cr = (F(.5) * r - F(.41869) * g - F(.08131) * b + (128 << 16) + 32767) >> 16
    code = _jpeg_chroma_420 if subsampling == 2 else _jpeg_plane
    y, cb, cr = _jpeg_plane(y, luma), code(cb, chroma) - 128, code(cr, chroma) - 128
    out = np.stack([y + ((F(1.402) * cr + 32768) >> 16), y + ((-F(.34414) * cb - F(.71414) * cr + 32768) >> 16),
                    y + ((F(1.772) * cb + 32768) >> 16)], axis=2)
    return np.clip(out, 0, 255).astype(np.uint8)


class _DegradedFromClean(ImageSuperResolution):
    """Pairs synthesised from clean files under ImageSuperResolution's csv, crop and patch plan and draws: the input
    of a sample is the same patch of the whole picture degraded (``degrade_host``), the target the clean patch.
    ``dist_mode``: "none" (default), or one of the parent's three additive modes, whose noise is added on top of the
    degraded patch as in PairedImageRestoration.  ``__getitem__`` is the host path: it degrades the decoded picture
    with numpy (the last CACHE pictures are kept), makes the parent's draws in the parent's order and returns (input,
    target) float32 HWC, cut and turned alike.  A DevicePatchLoader decodes only the clean files and makes the
    degraded arena on the GPU: ``degrade_pack`` of the clean pack, under ``synthetic_key`` in a shared store."""

    DIST_MODES = ("none",) + ImageSuperResolution.DIST_MODES
    CACHE = 4

    def __init__(self, csv_path, dist_mode, lambda_noise, **kwargs):
        self._degraded = {}          # image index -> (degraded, clean), the last CACHE decoded
        super().__init__(csv_path, dist_mode, lambda_noise, **kwargs)

    def degrade_host(self, img: int, clean: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def degrade_pack(self, pack, used: Sequence[int]):
        """The degraded pack of the clean pack of the files ``used``, sharing its image table."""
        raise NotImplementedError

    def synthetic_key(self, used: Sequence[int]) -> tuple:
        """What tells this degradation of the files ``used`` from any other."""
        raise NotImplementedError

    def load_pair(self, img: int) -> Tuple[np.ndarray, np.ndarray]:
        """(degraded, clean) of file ``img`` as uint8 H x W x n_channels."""
        if img not in self._degraded:
            while len(self._degraded) >= self.CACHE:
                self._degraded.pop(next(iter(self._degraded)))
            clean = self.load_image(img)
            self._degraded[img] = (self.degrade_host(img, clean), clean)
        return self._degraded[img]

    def __getitem__(self, idx):
        row, col, need_padding, img_i = self.patchs_data[idx]
        degraded, clean = self.load_pair(img_i)
        inp, tgt = self._cut(degraded, row, col, need_padding), self._cut(clean, row, col, need_padding)
        if self.use_data_augmentation:
            mode = self.random_state.randint(0, 7)
            inp, tgt = data_augmentation(inp, mode), data_augmentation(tgt, mode)
        inp, tgt = inp.astype(np.float32) / 255.0, tgt.astype(np.float32) / 255.0
        if self.dist_mode != "none":
            inp = _noisy(inp, self.random_state, self.dist_mode, self.lambda_noise)
        return torch.from_numpy(inp), torch.from_numpy(tgt)


class BicubicSuperResolution(_DegradedFromClean):
    """Bicubic super-resolution pairs synthesised from clean files under ImageSuperResolution's csv, crop and patch
    plan and draws: the input of a sample is the same patch of the whole picture degraded by ``scale`` (2..8) --
    the exact antialiased bicubic down and the bicubic back up to the picture's size, bicubic_degrade_u8 -- and the
    target the clean patch.  ``dist_mode``: "none" (default), or one of the parent's three additive modes, whose
    noise is added on top of the degraded patch as in PairedImageRestoration.  ``__getitem__`` is the host path:
    it degrades the decoded picture with numpy (the last CACHE pictures are kept), makes the parent's draws in the
    parent's order and returns (input, target) float32 HWC, cut and turned alike.  A DevicePatchLoader decodes only
    the clean files and makes the degraded arena on the GPU."""

    def __init__(self, csv_path, scale, dist_mode="none", lambda_noise=None, use_data_aug=False, patch_size=(64, 64),
                 max_num_patchs=100000, root_folder="", logger=None, device=None, seed=2204, n_channels=3):
        if isinstance(scale, bool) or not isinstance(scale, int) or not 2 <= scale <= 8:
            raise ValueError(f"BicubicSuperResolution: scale is an integer of 2..8, got {scale!r}")
        self.scale = scale
        super().__init__(csv_path, dist_mode, lambda_noise, use_data_aug=use_data_aug, patch_size=patch_size,
                         max_num_patchs=max_num_patchs, root_folder=root_folder, logger=logger, device=device,
                         seed=seed, n_channels=n_channels)

    def degrade_host(self, img, clean):
        return bicubic_degrade_u8(clean, self.scale)

    def degrade_pack(self, pack, used):
        from . import kernels
        return kernels.u8_bicubic_degrade_images(pack, self.scale)

    def synthetic_key(self, used):
        return ("bicubic", self.scale)


class JpegArtifactRemoval(_DegradedFromClean):
    """JPEG compression-artifact-removal pairs synthesised from clean files under ImageSuperResolution's csv, crop
    and patch plan and draws: the input of a sample is the same patch of the whole picture after the JPEG round trip
    (jpeg_degrade_u8: decode(encode(picture)) in libjpeg's integer arithmetic), the target the clean patch.
    ``quality``: an integer of 1..100 for every file, or ``[levels, probabilities]`` as ``lambda_noise`` of
    vary_addictive_noise is; the quality of file i is then drawn once, in file order, from RandomState(seed), so it
    is a function of (seed, file) alone and is fixed for the run -- it is not drawn again per epoch or per patch
    (``qualities`` lists them).  ``subsampling``: 0 (4:4:4) or 2 (4:2:0); gray pictures ignore it.  ``dist_mode``
    defaults to "none"; the additive modes add their noise on top of the degraded patch.  A DevicePatchLoader
    decodes only the clean files and makes the degraded arena on the GPU (kernels.u8_jpeg_images)."""

    def __init__(self, csv_path, quality, subsampling=0, dist_mode="none", lambda_noise=None, use_data_aug=False,
                 patch_size=(64, 64), max_num_patchs=100000, root_folder="", logger=None, device=None, seed=2204,
                 n_channels=3):
        who = "JpegArtifactRemoval"
        ok = lambda q: isinstance(q, (int, np.integer)) and not isinstance(q, (bool, np.bool_)) and 1 <= q <= 100
        if isinstance(quality, (list, tuple)):
            if len(quality) != 2 or len(quality[0]) < 1 or len(quality[0]) != len(quality[1]) \
                    or not all(ok(q) for q in quality[0]):
                raise ValueError(f"{who}: quality is an integer of 1..100 or [levels, probabilities] with as many "
                                 f"probabilities as levels of 1..100, got {quality!r}")
        elif not ok(quality):
            raise ValueError(f"{who}: quality is an integer of 1..100 or [levels, probabilities], got {quality!r}")
        if isinstance(subsampling, bool) or subsampling not in (0, 2):
            raise ValueError(f"{who}: subsampling is 0 (4:4:4) or 2 (4:2:0), got {subsampling!r}")
        if n_channels not in (1, 3):
            raise ValueError(f"{who}: JPEG is defined for 1 or 3 channels, got n_channels {n_channels}")
        self.quality, self.subsampling = quality, int(subsampling)
        super().__init__(csv_path, dist_mode, lambda_noise, use_data_aug=use_data_aug, patch_size=patch_size,
                         max_num_patchs=max_num_patchs, root_folder=root_folder, logger=logger, device=device,
                         seed=seed, n_channels=n_channels)

    def create_all_images(self):
        super().create_all_images()
        n = len(self.paths)
        if isinstance(self.quality, (list, tuple)):
            drawn = np.random.RandomState(self.seed).choice(self.quality[0], p=self.quality[1], size=n)
            self.qualities = [int(q) for q in drawn]
        else:
            self.qualities = [int(self.quality)] * n

    def degrade_host(self, img, clean):
        return jpeg_degrade_u8(clean, self.qualities[img], self.subsampling)

    def degrade_pack(self, pack, used):
        from . import kernels
        return kernels.u8_jpeg_images(pack, [self.qualities[i] for i in used], self.subsampling)

    def synthetic_key(self, used):
        return ("jpeg", tuple(self.qualities[i] for i in used), self.subsampling)


BAYER_PATTERNS = ("rggb", "grbg", "gbrg", "bggr")      # kernels.DEMOSAIC_PATTERNS: the index is the code
BAYER_FILLS = ("zero", "bilinear", "malvar")           # kernels.DEMOSAIC_FILLS


def _bayer_code(who: str, what: str, names, v) -> int:
    if isinstance(v, str) and v in names:
        return names.index(v)
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and 0 <= v < len(names):
        return int(v)
    raise ValueError(f"{who}: the {what} is one of {names} or its code 0..{len(names) - 1}, got {v!r}")


def _mirror(n: int) -> np.ndarray:
    """The indices -2 .. n + 1 of a side n reflected about its edge samples, which are not repeated."""
    i = np.arange(-2, n + 2)
    if n == 1:
        return np.zeros_like(i)
    t = i % (2 * (n - 1))
    return np.where(t < n, t, 2 * (n - 1) - t)


def demosaic_degrade_u8(a: np.ndarray, pattern, fill="malvar") -> np.ndarray:
    """The Bayer mosaic of a uint8 picture with its missing channels filled, H x W x 3, on the CPU (include/grr.h
    has the definition).  ``a``: H x W x 3 (R, G, B) or the mosaic plane itself as H x W x 1 or H x W.  ``pattern``:
    "rggb", "grbg", "gbrg", "bggr" or the code 0..3; ``fill``: "zero", "bilinear", "malvar" or 0..2.  The same
    integers as kernels.u8_demosaic, bit for bit: it serves the host DataLoader path and users without a GPU."""
    who = "demosaic_degrade_u8"
    a = np.asarray(a)
    a = a[:, :, None] if a.ndim == 2 else a
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3) or 0 in a.shape:
        raise ValueError(f"{who}: expected a uint8 H x W x 3, H x W x 1 or H x W picture, got {a.dtype} {a.shape}")
    code, fill = _bayer_code(who, "pattern", BAYER_PATTERNS, pattern), _bayer_code(who, "fill", BAYER_FILLS, fill)
    h, w = a.shape[:2]
    ry, rx = code >> 1, code & 1
    red, blue = (slice(ry, None, 2), slice(rx, None, 2)), (slice(1 - ry, None, 2), slice(1 - rx, None, 2))
    m = a[:, :, a.shape[2] // 2].astype(np.int32)                      # G everywhere, or the plane itself
    if a.shape[2] == 3:
        m[red], m[blue] = a[:, :, 0][red], a[:, :, 2][blue]
    p = m[_mirror(h)][:, _mirror(w)]                                    # the plane with its reflected 2-sample frame
    at = lambda dy, dx: p[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
    ctr = at(0, 0)
    if fill == 0:
        green = other = inrow = incol = np.zeros_like(ctr)
    else:
        h1, v1 = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
        diag = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
        if fill == 1:
            green, other, inrow, incol = 4 * (h1 + v1), 4 * diag, 8 * h1, 8 * v1
        else:
            h2, v2 = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
            green = 8 * ctr + 4 * (h1 + v1) - 2 * (h2 + v2)
            other = 12 * ctr + 4 * diag - 3 * (h2 + v2)
            inrow = 10 * ctr + 8 * h1 - 2 * diag - 2 * h2 + v2
            incol = 10 * ctr + 8 * v1 - 2 * diag - 2 * v2 + h2
    s = np.empty((h, w, 3), np.int32)                                   # sixteenths
    s[:, :, 1] = green
    s[:, :, 0], s[:, :, 2] = other, other
    for rows, cols, of_row, of_col in ((red[0], blue[1], 0, 2), (blue[0], red[1], 2, 0)):      # the two kinds of G site
        s[rows, cols, of_row], s[rows, cols, of_col] = inrow[rows, cols], incol[rows, cols]
        s[rows, cols, 1] = 16 * ctr[rows, cols]
    s[red + (0,)], s[blue + (2,)] = 16 * ctr[red], 16 * ctr[blue]
    return np.clip((s + 8) >> 4, 0, 255).astype(np.uint8)


class BayerDemosaicking(_DegradedFromClean):
    """Demosaicking pairs synthesised from clean RGB files under ImageSuperResolution's csv, crop and patch plan and
    draws: the input of a sample is the same patch of the whole picture sampled through a Bayer colour filter array
    and filled (demosaic_degrade_u8), the target the clean patch.  ``pattern``: "rggb", "grbg", "gbrg" or "bggr" for
    every file, or ``[names, probabilities]``; the pattern of file i is then drawn once, in file order, from
    RandomState(seed), so it is a function of (seed, file) alone and is fixed for the run (``patterns`` lists the
    names drawn).  ``fill``: "zero", "bilinear" or "malvar".  It needs ``n_channels == 3``.  A DevicePatchLoader
    decodes only the clean files and makes the filled arena on the GPU (kernels.u8_demosaic_images).

    Two properties to know.  Patches are cut from the filled whole picture at any origin, odd ones included, and the
    8 augmentation modes turn them, so the model sees every phase of the colour filter array under one pattern.  An
    additive ``dist_mode`` (default "none") adds its noise on top of the filled patch, as the sibling datasets do:
    noise on the mosaic before the fill (joint denoising and demosaicking) is NoisyBayerDemosaicking's."""

    def __init__(self, csv_path, pattern="rggb", fill="malvar", dist_mode="none", lambda_noise=None,
                 use_data_aug=False, patch_size=(64, 64), max_num_patchs=100000, root_folder="", logger=None,
                 device=None, seed=2204, n_channels=3):
        _check_bayer_args("BayerDemosaicking", pattern, fill, n_channels)
        self.pattern, self.fill = pattern, fill
        super().__init__(csv_path, dist_mode, lambda_noise, use_data_aug=use_data_aug, patch_size=patch_size,
                         max_num_patchs=max_num_patchs, root_folder=root_folder, logger=logger, device=device,
                         seed=seed, n_channels=n_channels)

    def create_all_images(self):
        super().create_all_images()
        self.patterns = _draw_patterns(self.pattern, self.seed, len(self.paths))

    def degrade_host(self, img, clean):
        return demosaic_degrade_u8(clean, self.patterns[img], self.fill)

    def degrade_pack(self, pack, used):
        from . import kernels
        return kernels.u8_demosaic_images(pack, [self.patterns[i] for i in used], self.fill)

    def synthetic_key(self, used):
        return ("bayer", tuple(self.patterns[i] for i in used), self.fill)


RAW_NOISE_BITS = (8, 16)      # kernels.RAW_NOISE_BITS


def _reflect_any(i: np.ndarray, n: int) -> np.ndarray:
    """Any indices reflected about the edge samples of a side n, which are not repeated (_mirror for any index)."""
    if n == 1:
        return np.zeros_like(i)
    t = i % (2 * (n - 1))
    return np.where(t < n, t, 2 * (n - 1) - t)


def raw_noise_demosaic_patch(a: np.ndarray, pattern, row: int, col: int, ph: int, pw: int, shot_a: float, read_b: float,
                             z: Optional[np.ndarray], fill="malvar", bits: int = 16, clip: bool = True):
    """(target, input) float32 ph x pw x 3 of the joint denoising and demosaicking degradation on the CPU, before
    T_mode (include/grr.h has the definition): the (ph + 4) x (pw + 4) window of the uint8 H x W x 3 picture ``a`` at
    (row - 2, col - 2), continued by the reflection that keeps the colour filter array's parity, sampled through
    ``pattern``, given noise sqrt(shot_a x + read_b) z (``z``: float64 normals [ph + 4, pw + 4], or None for none),
    clipped, quantised to ``bits`` bits and filled by ``fill``.  With kernels.patch_raw_batch's normals it gives the
    kernel's floats; the host DataLoader path draws its own."""
    who = "raw_noise_demosaic_patch"
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or 0 in a.shape:
        raise ValueError(f"{who}: expected a uint8 H x W x 3 picture, got {a.dtype} {a.shape}")
    code, fill = _bayer_code(who, "pattern", BAYER_PATTERNS, pattern), _bayer_code(who, "fill", BAYER_FILLS, fill)
    h, w = a.shape[:2]
    ry, rx = code >> 1, code & 1
    ys, xs = _reflect_any(row - 2 + np.arange(ph + 4), h), _reflect_any(col - 2 + np.arange(pw + 4), w)
    py, px = ((ys ^ ry) & 1)[:, None], ((xs ^ rx) & 1)[None, :]       # 0 in an R row / column
    x = a[ys[:, None], xs[None, :], py + px].astype(np.float64) / 255.0
    full = float((1 << bits) - 1)
    var = float(np.float32(shot_a)) * x + float(np.float32(read_b))
    t = x if z is None else np.where(var != 0, x + np.sqrt(var) * np.asarray(z, dtype=np.float64), x)
    if clip:
        t = np.clip(t, 0.0, 1.0)
    q = np.clip(np.nan_to_num(np.rint(t * full), nan=0.0), -2.0 ** 24, 2.0 ** 24).astype(np.int64)
    at = lambda dy, dx: q[2 + dy:2 + dy + ph, 2 + dx:2 + dx + pw]
    ctr = at(0, 0)
    if fill == 0:
        green = other = inrow = incol = np.zeros_like(ctr)
    else:
        h1, v1 = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
        diag = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
        if fill == 1:
            green, other, inrow, incol = 4 * (h1 + v1), 4 * diag, 8 * h1, 8 * v1
        else:
            h2, v2 = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
            green = 8 * ctr + 4 * (h1 + v1) - 2 * (h2 + v2)
            other = 12 * ctr + 4 * diag - 3 * (h2 + v2)
            inrow = 10 * ctr + 8 * h1 - 2 * diag - 2 * h2 + v2
            incol = 10 * ctr + 8 * v1 - 2 * diag - 2 * v2 + h2
    cy, cx = py[2:-2], px[:, 2:-2]
    site, g = cy + cx, cy != cx
    s = np.stack([np.where(g, np.where(cy == 1, incol, inrow), other), green,
                  np.where(g, np.where(cy == 1, inrow, incol), other)], axis=2)                # sixteenths
    s = np.where(site[:, :, None] == np.arange(3), 16 * ctr[:, :, None], s)
    target = a[ys[2:-2, None], xs[None, 2:-2]].astype(np.float32) / np.float32(255.0)
    return target, (s.astype(np.float64) / (16.0 * full)).astype(np.float32)


def _check_bayer_args(who: str, pattern, fill, n_channels) -> None:
    """BayerDemosaicking's refusals of pattern, fill and n_channels."""
    ok = lambda p: isinstance(p, str) and p in BAYER_PATTERNS
    if isinstance(pattern, (list, tuple)):
        if len(pattern) != 2 or isinstance(pattern[0], str) or len(pattern[0]) < 1 \
                or len(pattern[0]) != len(pattern[1]) or not all(ok(p) for p in pattern[0]):
            raise ValueError(f"{who}: pattern is one of {BAYER_PATTERNS} or [names, probabilities] with as many "
                             f"probabilities as names, got {pattern!r}")
    elif not ok(pattern):
        raise ValueError(f"{who}: pattern is one of {BAYER_PATTERNS} or [names, probabilities], got {pattern!r}")
    if not (isinstance(fill, str) and fill in BAYER_FILLS):
        raise ValueError(f"{who}: fill is one of {BAYER_FILLS}, got {fill!r}")
    if n_channels != 3:
        raise ValueError(f"{who}: a Bayer mosaic is made from R, G, B pictures, got n_channels {n_channels}")


def _draw_patterns(pattern, seed: int, n: int) -> List[str]:
    """The pattern name of each of n files: the one name, or drawn once, in file order, from RandomState(seed)."""
    if isinstance(pattern, (list, tuple)):
        drawn = np.random.RandomState(seed).choice(len(pattern[0]), p=pattern[1], size=n)
        return [str(pattern[0][int(k)]) for k in drawn]
    return [pattern] * n


def _check_levels(who: str, what: str, v, top: float) -> None:
    """A noise level: a number of 0..top, or [levels, probabilities] as lambda_noise of vary_addictive_noise is."""
    ok = lambda q: isinstance(q, (int, float, np.integer, np.floating)) and not isinstance(q, (bool, np.bool_)) \
        and np.isfinite(q) and 0 <= q <= top
    if isinstance(v, (list, tuple)):
        if len(v) != 2 or not isinstance(v[0], (list, tuple)) or len(v[0]) < 1 or len(v[0]) != len(v[1]) \
                or not all(ok(q) for q in v[0]):
            raise ValueError(f"{who}: {what} is a number of 0..{top:g} or [levels, probabilities] with as many "
                             f"probabilities as levels, got {v!r}")
    elif not ok(v):
        raise ValueError(f"{who}: {what} is a number of 0..{top:g} or [levels, probabilities], got {v!r}")


def _draw_levels(rs: np.random.RandomState, v, n: int) -> np.ndarray:
    """n levels of a _check_levels value as float64: drawn from ``rs`` if it is a distribution, else repeated."""
    if isinstance(v, (list, tuple)):
        return np.asarray(rs.choice(v[0], p=v[1], size=n), dtype=np.float64)
    return np.full(n, float(v))


def raw_noise_pairs(shot: np.ndarray, read: np.ndarray) -> np.ndarray:
    """The kernel's float32 [n, 2] noise pairs (a, b) of shot gains and read levels (8-bit units, as lambda_noise):
    a = float32(shot), b = float32((read / 255)^2)."""
    shot, read = np.asarray(shot, dtype=np.float64), np.asarray(read, dtype=np.float64)
    return np.stack([shot.astype(np.float32), ((read / 255.0) ** 2).astype(np.float32)], axis=1)


class NoisyBayerDemosaicking(ImageSuperResolution):
    """Joint denoising and demosaicking pairs synthesised from clean RGB files under ImageSuperResolution's csv, crop
    and patch plan: the input of a sample is the patch sampled through a Bayer colour filter array, given sensor noise
    ON THE MOSAIC -- variance ``shot`` x + (``read`` / 255)^2 for a signal x in [0, 1] -- clipped to [0, 1] if ``clip``,
    quantised to ``bits`` bits and only then filled (raw_noise_demosaic_patch; include/grr.h has the definition), so
    the fill spreads and correlates the noise as a camera pipeline does; the target is the clean patch.  ``pattern``
    and ``fill`` as BayerDemosaicking takes them, with the same per-file draw.  ``shot`` (0..1) and ``read`` (0..255,
    8-bit levels like ``lambda_noise``): a number, or ``[levels, probabilities]`` drawn per sample.  ``dist_mode`` must
    be "none": the noise is the sensor's.  A patch that sticks out of its picture is continued by the reflection that
    keeps the array's parity, not by the siblings' edge-repeating mirror.

    The noise is fresh per sample and per epoch and lies under the fill, so there is no degraded arena: a
    DevicePatchLoader holds the clean arena and the files' pattern codes, and a batch is one kernels.patch_raw_batch
    call.  ``__getitem__`` is the host path: the same formula in numpy with normals from the dataset's RandomState
    (after the mode and the level draws); its noise is not the device's."""

    DIST_MODES = ("none",)

    def __init__(self, csv_path, pattern="rggb", fill="malvar", shot=0.0, read=0.0, bits=16, clip=True, dist_mode="none",
                 lambda_noise=None, use_data_aug=False, patch_size=(64, 64), max_num_patchs=100000, root_folder="",
                 logger=None, device=None, seed=2204, n_channels=3):
        who = "NoisyBayerDemosaicking"
        _check_bayer_args(who, pattern, fill, n_channels)
        _check_levels(who, "shot", shot, 1.0)
        _check_levels(who, "read", read, 255.0)
        if isinstance(bits, bool) or not isinstance(bits, int) or not RAW_NOISE_BITS[0] <= bits <= RAW_NOISE_BITS[1]:
            raise ValueError(f"{who}: bits is an integer of {RAW_NOISE_BITS[0]}..{RAW_NOISE_BITS[1]}, got {bits!r}")
        if not isinstance(clip, bool):
            raise ValueError(f"{who}: clip is true or false, got {clip!r}")
        if dist_mode != "none":
            raise ValueError(f"{who}: dist_mode must be 'none' (the noise is shot and read, on the mosaic), got "
                             f"{dist_mode!r}")
        self.pattern, self.fill, self.shot, self.read, self.bits, self.clip = pattern, fill, shot, read, bits, clip
        super().__init__(csv_path, dist_mode, lambda_noise, use_data_aug=use_data_aug, patch_size=patch_size,
                         max_num_patchs=max_num_patchs, root_folder=root_folder, logger=logger, device=device,
                         seed=seed, n_channels=n_channels)

    def create_all_images(self):
        super().create_all_images()
        self.patterns = _draw_patterns(self.pattern, self.seed, len(self.paths))

    @property
    def noise_free(self) -> bool:
        """shot and read are both the number 0: no generator runs."""
        return not isinstance(self.shot, (list, tuple)) and not isinstance(self.read, (list, tuple)) \
            and self.shot == 0 and self.read == 0

    def __getitem__(self, idx):
        row, col, _, img_i = self.patchs_data[idx]
        h, w = self.out_size()
        rs = self.random_state
        mode = rs.randint(0, 7) if self.use_data_augmentation else 0
        pair = raw_noise_pairs(_draw_levels(rs, self.shot, 1), _draw_levels(rs, self.read, 1))[0]
        z = None if self.noise_free else rs.standard_normal((h + 4, w + 4))
        tgt, inp = raw_noise_demosaic_patch(self.load_image(img_i), self.patterns[img_i], row, col, h, w, pair[0], pair[1],
                                            z, self.fill, self.bits, self.clip)
        return torch.from_numpy(data_augmentation(inp, mode)), torch.from_numpy(data_augmentation(tgt, mode))


MASK_FILLS = ("zero", "conv")                           # kernels.MASK_FILLS: the index is the code
MASK_HALO = 7                 # GRR_MASK_HALO


def _mask_sym(n_from: int, count: int, n: int) -> np.ndarray:
    """sym(r, n) of r = n_from .. n_from + count - 1: the edge-repeating mirror for any index."""
    t = np.arange(n_from, n_from + count) % (2 * n)
    return np.where(t < n, t, 2 * n - 1 - t)


def mask_fill_patch(a: np.ndarray, row: int, col: int, ph: int, pw: int, known: np.ndarray, weights, fill="conv",
                    hole: int = 128) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(target, input, mask) of one inpainting sample before the augmentation (include/grr.h has the definition):
    uint8 ph x pw x C twice and the bool ph x pw plane of the known pixels.  ``a``: the uint8 H x W x C picture;
    ``known``: the bool (ph + 14) x (pw + 14) bits of the window, whose position (wy, wx) is picture pixel
    (sym(row + wy - 7), sym(col + wx - 7)); ``weights``: the uint8 table of the conv fill.  A known pixel passes
    through; a missing one is 0 under the zero fill and (2 num + den) / (2 den) under conv -- den and num the sums of
    w k and w k v under the table -- or ``hole`` where den is 0.  With kernels.patch_mask_batch's bits it gives the
    kernel's bytes; the host DataLoader path draws its own."""
    who = "mask_fill_patch"
    fill = _bayer_code(who, "fill", MASK_FILLS, fill)
    known = np.asarray(known, dtype=bool)
    if known.shape != (ph + 2 * MASK_HALO, pw + 2 * MASK_HALO):
        raise ValueError(f"{who}: the known bits are ({ph} + 14) x ({pw} + 14), got {known.shape}")
    win = a[np.ix_(_mask_sym(row - MASK_HALO, ph + 2 * MASK_HALO, a.shape[0]),
                   _mask_sym(col - MASK_HALO, pw + 2 * MASK_HALO, a.shape[1]))]
    core = (slice(MASK_HALO, MASK_HALO + ph), slice(MASK_HALO, MASK_HALO + pw))
    target, kc = win[core], known[core]
    if fill == 0:
        return target, target * kc[:, :, None].astype(np.uint8), kc
    w = np.asarray(weights)
    if w.ndim != 2 or w.dtype != np.uint8 or any(s % 2 == 0 or s > 2 * MASK_HALO + 1 for s in w.shape):
        raise ValueError(f"{who}: a weight table is uint8 with odd sides of at most 15, got {w.dtype} {w.shape}")
    k = known.astype(np.int64)
    vk = win.astype(np.int64) * k[:, :, None]
    den, num = np.zeros((ph, pw), np.int64), np.zeros(target.shape, np.int64)
    for i in range(w.shape[0]):
        for j in range(w.shape[1]):
            ys, xs = MASK_HALO + i - w.shape[0] // 2, MASK_HALO + j - w.shape[1] // 2
            den += int(w[i, j]) * k[ys:ys + ph, xs:xs + pw]
            num += int(w[i, j]) * vk[ys:ys + ph, xs:xs + pw]
    d = den[:, :, None]
    filled = np.where(d > 0, (2 * num + d) // (2 * np.maximum(d, 1)), int(hole))
    return target, np.where(kc[:, :, None], target, filled).astype(np.uint8), kc


class RandomMaskInpainting(ImageSuperResolution):
    """Inpainting pairs synthesised from clean files under ImageSuperResolution's csv, crop and patch plan: the input
    of a sample is the patch with a random share of its pixels missing -- one Bernoulli bit per pixel, shared by the
    channels -- and the missing ones filled (mask_fill_patch; include/grr.h has the definition); the target is the
    clean patch.  ``keep``: the known share of 0..1, a number, or ``[levels, probabilities]`` drawn per sample.
    ``fill``: "zero", or "conv", the normalised convolution of the known pixels under a ``fill_side`` x ``fill_side``
    table (odd, at most 15) that is flat, or a Gaussian of ``fill_sigma`` (kernels.mask_weights), with ``hole`` (a
    byte) where no known pixel lies under the table.  ``dist_mode`` must be "none": noise on top is not made.

    The mask is fresh per sample and per epoch and lies under the fill, so there is no degraded arena: a
    DevicePatchLoader holds the clean arena alone and a batch is one kernels.patch_mask_batch call.  ``__getitem__``
    is the host path: the same formula in numpy with bits from the dataset's RandomState (after the mode and the
    level draws: random_sample((h + 14, w + 14)) < keep); its mask is not the device's."""

    DIST_MODES = ("none",)

    def __init__(self, csv_path, keep=0.5, fill="conv", fill_side=7, fill_sigma=None, hole=128, dist_mode="none",
                 lambda_noise=None, use_data_aug=False, patch_size=(64, 64), max_num_patchs=100000, root_folder="",
                 logger=None, device=None, seed=2204, n_channels=3):
        from . import kernels
        who = "RandomMaskInpainting"
        _check_levels(who, "keep", keep, 1.0)
        if fill not in MASK_FILLS:
            raise ValueError(f"{who}: fill is one of {MASK_FILLS}, got {fill!r}")
        try:
            self.weights = kernels.mask_weights(fill_side, fill_sigma)
            hole = kernels._check_hole(who, hole)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        if dist_mode != "none":
            raise ValueError(f"{who}: dist_mode must be 'none' (noise on top of the masked input is not made), got "
                             f"{dist_mode!r}")
        self.keep, self.fill, self.fill_side, self.fill_sigma, self.hole = keep, fill, fill_side, fill_sigma, hole
        super().__init__(csv_path, dist_mode, lambda_noise, use_data_aug=use_data_aug, patch_size=patch_size,
                         max_num_patchs=max_num_patchs, root_folder=root_folder, logger=logger, device=device,
                         seed=seed, n_channels=n_channels)

    def __getitem__(self, idx):
        row, col, _, img_i = self.patchs_data[idx]
        h, w = self.out_size()
        rs = self.random_state
        mode = rs.randint(0, 7) if self.use_data_augmentation else 0
        keep = float(_draw_levels(rs, self.keep, 1)[0])
        known = rs.random_sample((h + 2 * MASK_HALO, w + 2 * MASK_HALO)) < keep
        tgt, inp, _ = mask_fill_patch(self.load_image(img_i), row, col, h, w, known, self.weights, self.fill, self.hole)
        as_f32 = lambda p: data_augmentation(p, mode).astype(np.float32) / np.float32(255.0)      # noqa: E731
        return torch.from_numpy(as_f32(inp)), torch.from_numpy(as_f32(tgt))


BLUR_BOUNDARIES = ("wrap", "replicate", "reflect")      # kernels.BLUR_BOUNDARIES: the index is the code
MAX_BLUR_SIDE = 31            # GRR_BLUR_MAX_SIDE
BLUR_ONE = 65536              # GRR_BLUR_ONE
MAX_BLUR_KERNELS = 16         # kernels.MAX_BLUR_KERNELS: distinct kernels of one degraded arena


def quantise_blur_kernel(k) -> np.ndarray:
    """The int32 weight table of a non-negative real kernel ``k`` of positive sum (include/grr.h has the rule), in
    float64: q = k / sum(k) * 65536 with sum(k) the correctly rounded sum (math.fsum, so it does not depend on an
    order of summation), W = floor(q), and the 65536 - sum(W) units left go one each to the taps of largest
    fractional part, ties to the lower flat index.  An integer table that already sums to 65536 passes through
    unchanged."""
    who = "quantise_blur_kernel"
    k = np.asarray(k)
    if k.ndim != 2 or k.size == 0 or k.dtype.kind not in "iuf":
        raise ValueError(f"{who}: a blur kernel is a 2-D array of real numbers, got {k.dtype} {k.shape}")
    if any(s % 2 == 0 or s > MAX_BLUR_SIDE for s in k.shape):
        raise ValueError(f"{who}: a blur kernel's sides are odd and at most {MAX_BLUR_SIDE}, got {k.shape}")
    if k.dtype.kind in "iu" and k.min() >= 0 and int(k.astype(np.int64).sum()) == BLUR_ONE:
        return np.ascontiguousarray(k, dtype=np.int32)
    k = k.astype(np.float64)
    total = math.fsum(k.ravel().tolist())
    if not np.all(np.isfinite(k)) or k.min() < 0 or not total > 0:
        raise ValueError(f"{who}: a blur kernel is finite and non-negative with a positive sum")
    q = k / total * float(BLUR_ONE)
    w = np.floor(q)
    left = BLUR_ONE - int(w.sum())
    order = np.argsort(-(q - w).ravel(), kind="stable")      # largest fraction first, ties in flat order
    w = w.astype(np.int64).ravel()
    if not 0 <= left <= w.size:      # rounding of q cannot move the sum further than one unit per tap
        raise ValueError(f"{who}: the kernel cannot be quantised ({left} units left for {w.size} taps)")
    w[order[:left]] += 1
    return np.ascontiguousarray(w.reshape(k.shape), dtype=np.int32)


class BlurKernel:
    """A blur kernel as the device takes it: ``table`` (int32 [kh, kw], read-only; odd sides up to 31, non-negative,
    of sum 65536), ``kh``, ``kw`` and ``spec``, the string it was built from (for an array, its sides and a digest of
    the table).  Immutable and hashable: equal kernels have equal tables."""
    __slots__ = ("table", "kh", "kw", "spec", "_key")

    def __init__(self, weights, spec: Optional[str] = None):
        table = quantise_blur_kernel(weights).copy()
        table.setflags(write=False)
        key = (table.shape, table.tobytes())
        if spec is None:
            import hashlib
            spec = f"array:{table.shape[0]}x{table.shape[1]}:{hashlib.sha1(key[1]).hexdigest()[:12]}"
        for name, v in (("table", table), ("kh", int(table.shape[0])), ("kw", int(table.shape[1])), ("spec", str(spec)),
                        ("_key", key)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a BlurKernel is immutable")

    def __eq__(self, other):
        return isinstance(other, BlurKernel) and self._key == other._key

    def __hash__(self):
        return hash(self._key)

    def __repr__(self):
        return f"BlurKernel({self.spec!r}, {self.kh} x {self.kw})"


def _blur_side(who: str, what: str, v, odd: bool = True) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_BLUR_SIDE \
            or (odd and v % 2 == 0):
        raise ValueError(f"{who}: {what} is an{' odd' if odd else ''} integer of 1..{MAX_BLUR_SIDE}, got {v!r}")
    return int(v)


def gaussian_kernel(side: int, sigma: float) -> BlurKernel:
    """``gaussian:SIDE:SIGMA``: exp(-(dy^2 + dx^2) / (2 sigma^2)) on a SIDE x SIDE grid about its centre, quantised."""
    side = _blur_side("gaussian_kernel", "the side", side)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) \
            or not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"gaussian_kernel: sigma is a positive number, got {sigma!r}")
    d = np.arange(side, dtype=np.float64) - (side - 1) / 2
    return BlurKernel(np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * float(sigma) ** 2)),
                      f"gaussian:{side}:{float(sigma):g}")


def box_kernel(side: int) -> BlurKernel:
    """``box:SIDE``: the mean over a SIDE x SIDE window, quantised."""
    side = _blur_side("box_kernel", "the side", side)
    return BlurKernel(np.ones((side, side)), f"box:{side}")


def motion_kernel(length: int, angle: float) -> BlurKernel:
    """``motion:LENGTH:ANGLE``: a straight line of LENGTH pixels (an integer of 1..31) through the centre of an s x s
    grid, s = LENGTH if that is odd, else LENGTH + 1, at ANGLE degrees counter-clockwise with y pointing down.
    N = 8 LENGTH + 1 points (one for LENGTH 1) at t evenly spaced on [-(LENGTH - 1) / 2, (LENGTH - 1) / 2] are placed
    at (x, y) = (c + t cos a, c - t sin a), c = (s - 1) / 2, and each adds its bilinear weights to its four
    neighbouring taps; a neighbour outside the grid gets nothing.  The sum is quantised.

    This is this project's definition, not MATLAB's ``fspecial('motion')``: the two differ in how the line is sampled
    and weighted.  Two details make it reproducible: the cosine and sine of a multiple of 90 degrees are exact (0 or
    +-1), and every tap is the correctly rounded sum (math.fsum) of its contributions, so a kernel does not depend on
    the order of the points: the kernels at 0 and at 90 degrees are transposes of each other."""
    who = "motion_kernel"
    length = _blur_side(who, "the length", length, odd=False)
    if isinstance(angle, bool) or not isinstance(angle, (int, float, np.integer, np.floating)) or not math.isfinite(angle):
        raise ValueError(f"{who}: the angle is a finite number of degrees, got {angle!r}")
    s = length if length % 2 else length + 1
    c = (s - 1) // 2
    quarter = (float(angle) % 360.0) / 90.0
    if quarter == int(quarter):
        cos_a, sin_a = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter)]
    else:
        cos_a, sin_a = math.cos(math.radians(float(angle))), math.sin(math.radians(float(angle)))
    # t_i = (i - 4 LENGTH) (LENGTH - 1) / (8 LENGTH): exactly antisymmetric about the middle point
    ts = [0.0] if length == 1 else [(i - 4 * length) * (length - 1) / (8.0 * length) for i in range(8 * length + 1)]
    parts = [[[] for _ in range(s)] for _ in range(s)]
    for t in ts:
        x, y = c + t * cos_a, c - t * sin_a
        x0, y0 = math.floor(x), math.floor(y)
        fx, fy = x - x0, y - y0
        for yy, wy in ((y0, 1.0 - fy), (y0 + 1, fy)):
            for xx, wx in ((x0, 1.0 - fx), (x0 + 1, fx)):
                if 0 <= yy < s and 0 <= xx < s:
                    parts[yy][xx].append(wy * wx)
    k = np.array([[math.fsum(p) for p in row] for row in parts], dtype=np.float64)
    return BlurKernel(k, f"motion:{length}:{float(angle):g}")


def parse_blur_spec(spec) -> BlurKernel:
    """The kernel of a spec: a BlurKernel (returned as it is), a 2-D array (quantised), or one of the strings
    ``gaussian:SIDE:SIGMA``, ``box:SIDE``, ``motion:LENGTH:ANGLE`` and ``file:PATH.npy`` (a 2-D float or integer
    array with odd sides of at most 31).  ValueError for anything else."""
    who = "parse_blur_spec"
    if isinstance(spec, BlurKernel):
        return spec
    if isinstance(spec, np.ndarray):
        return BlurKernel(spec)
    if not isinstance(spec, str):
        raise ValueError(f"{who}: a blur spec is a string, a 2-D array or a BlurKernel, got {type(spec).__name__}")
    name, _, rest = spec.partition(":")
    if name == "file":
        if not rest.endswith(".npy"):
            raise ValueError(f"{who}: file:PATH.npy names a .npy file, got {spec!r}")
        try:
            k = np.load(rest, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise ValueError(f"{who}: {spec!r} cannot be read: {e}") from None
        return BlurKernel(k, spec)
    forms = {"gaussian": (gaussian_kernel, (int, float)), "box": (box_kernel, (int,)), "motion": (motion_kernel, (int, float))}
    if name not in forms:
        raise ValueError(f"{who}: a blur spec is gaussian:SIDE:SIGMA, box:SIDE, motion:LENGTH:ANGLE or file:PATH.npy, "
                         f"got {spec!r}")
    build, types = forms[name]
    fields = rest.split(":") if rest else []
    if len(fields) != len(types):
        raise ValueError(f"{who}: {name} takes {len(types)} field(s) after its name, got {spec!r}")
    try:
        values = [t(f) for t, f in zip(types, fields)]
    except ValueError:
        raise ValueError(f"{who}: the fields of {spec!r} are not numbers of the kinds {name} takes") from None
    return build(*values)


def _blur_index(t: np.ndarray, n: int, mode: int) -> np.ndarray:
    """b(t, n) of include/grr.h for any integers t: 0 wrap, 1 replicate, 2 reflect without the edge sample."""
    if mode == 0:
        return t % n
    if mode == 1:
        return np.clip(t, 0, n - 1)
    if n == 1:
        return np.zeros_like(t)
    m = t % (2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def blur_degrade_u8(a: np.ndarray, kernel, boundary="wrap") -> np.ndarray:
    """The uint8 picture ``a`` (H x W x C with C of 1..4, or H x W) convolved with a blur kernel on the CPU, in the
    integers of include/grr.h.  ``kernel``: a spec as parse_blur_spec takes it; ``boundary``: "wrap", "replicate",
    "reflect" or the code 0..2.  The same bytes as kernels.u8_blur, bit for bit: it serves the host DataLoader path
    and users without a GPU.  One pass over the picture per non-zero tap: seconds for a 25 x 25 kernel."""
    who = "blur_degrade_u8"
    kernel = parse_blur_spec(kernel)
    mode = _bayer_code(who, "boundary", BLUR_BOUNDARIES, boundary)
    a = np.asarray(a)
    flat = a.ndim == 2
    a = a[:, :, None] if flat else a
    if a.dtype != np.uint8 or a.ndim != 3 or not 1 <= a.shape[2] <= 4 or 0 in a.shape:
        raise ValueError(f"{who}: expected a uint8 H x W x C (C of 1..4) or H x W picture, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    kh, kw, table = kernel.kh, kernel.kw, kernel.table
    rows = _blur_index(np.arange(-(kh // 2), h + kh // 2), h, mode)
    cols = _blur_index(np.arange(-(kw // 2), w + kw // 2), w, mode)
    p = a[rows][:, cols].astype(np.int32)              # the picture with its frame: p[r, c] is the sample at (r - kh/2, c - kw/2)
    acc = np.full(a.shape, 32768, np.int32)            # at most 32768 + 255 * 65536 < 2^31
    for i, j in zip(*np.nonzero(table)):
        acc += int(table[i, j]) * p[kh - 1 - i:kh - 1 - i + h, kw - 1 - j:kw - 1 - j + w]
    out = (acc >> 16).astype(np.uint8)
    return out[:, :, 0] if flat else out


class GaussianMotionDeblurring(_DegradedFromClean):
    """Deblurring pairs synthesised from clean files under ImageSuperResolution's csv, crop and patch plan and draws:
    the input of a sample is the same patch of the whole picture blurred (blur_degrade_u8), the target the clean
    patch.  ``kernel``: one spec for every file (parse_blur_spec: "gaussian:25:1.6", "motion:15:30", "box:5",
    "file:psf.npy", an array or a BlurKernel), or ``[specs, probabilities]`` with at most 16 specs; the kernel of file
    i is then drawn once, in file order, from RandomState(seed), so it is a function of (seed, file) alone and is
    fixed for the run (``kernels`` lists the BlurKernels drawn).  ``boundary``: "wrap" (the circular convolution of
    the deblurring tables, default), "replicate" or "reflect"; it acts on the whole picture, before a patch is cut.
    ``dist_mode`` defaults to "none"; the parent's additive modes put their noise on top of the blurred patch, which
    is the blur-plus-noise setting of the tables.  A DevicePatchLoader decodes only the clean files and makes the
    blurred arena on the GPU (kernels.u8_blur_images)."""

    def __init__(self, csv_path, kernel, boundary="wrap", dist_mode="none", lambda_noise=None, use_data_aug=False,
                 patch_size=(64, 64), max_num_patchs=100000, root_folder="", logger=None, device=None, seed=2204,
                 n_channels=3):
        who = "GaussianMotionDeblurring"
        if isinstance(kernel, (list, tuple)):
            if len(kernel) != 2 or isinstance(kernel[0], (str, np.ndarray, BlurKernel)) \
                    or not 1 <= len(kernel[0]) <= MAX_BLUR_KERNELS or len(kernel[0]) != len(kernel[1]):
                raise ValueError(f"{who}: kernel is one spec or [specs, probabilities] with 1..{MAX_BLUR_KERNELS} specs "
                                 f"and as many probabilities, got {kernel!r}")
            self.kernel_choices, self.kernel_p = [parse_blur_spec(k) for k in kernel[0]], list(kernel[1])
        else:
            self.kernel_choices, self.kernel_p = [parse_blur_spec(kernel)], None
        if not (isinstance(boundary, str) and boundary in BLUR_BOUNDARIES):
            raise ValueError(f"{who}: boundary is one of {BLUR_BOUNDARIES}, got {boundary!r}")
        if n_channels not in (1, 3):
            raise ValueError(f"{who}: pictures are decoded to 1 or 3 channels, got n_channels {n_channels}")
        self.kernel, self.boundary = kernel, boundary
        super().__init__(csv_path, dist_mode, lambda_noise, use_data_aug=use_data_aug, patch_size=patch_size,
                         max_num_patchs=max_num_patchs, root_folder=root_folder, logger=logger, device=device,
                         seed=seed, n_channels=n_channels)

    def create_all_images(self):
        super().create_all_images()
        n = len(self.paths)
        if self.kernel_p is not None:
            drawn = np.random.RandomState(self.seed).choice(len(self.kernel_choices), p=self.kernel_p, size=n)
            self.kernel_index = [int(k) for k in drawn]
        else:
            self.kernel_index = [0] * n
        self.kernels = [self.kernel_choices[k] for k in self.kernel_index]

    def degrade_host(self, img, clean):
        return blur_degrade_u8(clean, self.kernels[img], self.boundary)

    def degrade_pack(self, pack, used):
        from . import kernels
        return kernels.u8_blur_images(pack, self.kernel_choices, [self.kernel_index[i] for i in used], self.boundary)

    def synthetic_key(self, used):
        return ("blur", tuple(self.kernels[i] for i in used), self.boundary)


class DevicePatchLoader:
    """Batches of an ImageSuperResolution dataset made on the device: yields (noisy, clean) float32
    [B, C, h, w], planar (``channels_first``), in place of a DataLoader.  On first use (or in ``prepare``) every file
    a patch reads is decoded once into one uint8 arena laid out as restore.pack_images lays it out (a
    restore.ImagePack; every rank holds all of it), sent in chunks so the host holds little of it at a time, and the
    pack is checked once; a batch is then three small tables and one kernels.patch_batch call, whose host cost
    does not grow with the number of files.

    Per epoch e, vectorised in dataset order from RandomState((dataset.seed 1000003 + e) mod 2^32):
    modes = randint(0, 8, n) -- all 8 flips and quarter turns; the host path keeps the reference's randint(0, 7),
    modes 0..6 -- or zeros without use_data_aug, then for vary_addictive_noise choice(levels, p, size=n); the other
    two modes use lambda_noise (on the device they are one distribution).  Position p of the epoch's selection has
    sample id (e << 32) | p and the kernel's noise is a function of (dataset.seed, sample id, element), so a sample
    is a function of (dataset seed, epoch, position) alone: batch size, rank count and the resume point cannot
    change it.

    A PairedImageRestoration dataset yields (input, target): the degraded and the clean files are decoded in one
    pass into two arenas under one image table and a batch is one kernels.patch_pair_batch call.  The draws are the
    same ones -- dist_mode "none" draws no level and its sigma is zero, so the kernel computes no noise -- and a
    sample stays a function of (dataset seed, epoch, position).  The device holds both arenas: twice the bytes of
    the unpaired loader over the same pictures.

    A BicubicSuperResolution dataset yields (input, target) by the paired path as well, but only its clean files are
    decoded: the degraded arena is made from the clean one on the device (kernels.u8_bicubic_degrade_images, once, in
    ``prepare``) and shares its image table.  The host never holds a degraded picture.  A JpegArtifactRemoval dataset
    goes the same way with kernels.u8_jpeg_images at each file's quality: the switch is the datasets' common base
    class, whose ``degrade_pack`` makes the arena and whose ``synthetic_key`` tells one degradation from another in a
    shared store.  A BayerDemosaicking dataset is a third of the kind (kernels.u8_demosaic_images, each file's
    pattern), a GaussianMotionDeblurring dataset a fourth (kernels.u8_blur_images, each file's kernel).

    A NoisyBayerDemosaicking dataset yields (input, target) from the clean arena alone: its degradation -- noise on the
    mosaic, then the fill -- is made per batch inside kernels.patch_raw_batch, so the device holds one arena (shared
    with any other stage over the same files) and the files' pattern codes.  After the draws above the epoch stream
    gives the per-sample shot and then read levels where they are distributions (``epoch_noise``).

    A RandomMaskInpainting dataset goes the same way: the clean arena alone, and a batch is one
    kernels.patch_mask_batch call that draws the mask and fills the missing pixels.  After the draws above the epoch
    stream gives the per-sample known shares where ``keep`` is a distribution (``epoch_keep``, in units of 2^-24).  The
    loader still yields (input, target); the mask of the last batch, float32 [B, 1, h, w] with 1 for a known pixel, is
    kept as ``last_mask`` for a masked loss."""
    channels_first = True
    CHUNK_BYTES = 256 << 20      # decoded pictures staged on the host per transfer

    def __init__(self, dataset, sampler, batch_size: int, drop_last: bool = False, device=None, shared=None):
        """shared: a dict that loaders over the same files and device put their arena in and take it from (the
        stages of a curriculum read one csv; training.build_train_stages owns the dict, so the arena lives as
        long as the stages do).  None: this loader's own arena."""
        if not isinstance(dataset, ImageSuperResolution):
            raise ValueError("DevicePatchLoader: needs an ImageSuperResolution dataset")
        if batch_size < 1:
            raise ValueError(f"DevicePatchLoader: batch_size must be positive (got {batch_size})")
        self.dataset, self.sampler, self.batch_size, self.drop_last = dataset, sampler, int(batch_size), bool(drop_last)
        self.device = device
        self.shared = shared
        self.synthetic = isinstance(dataset, _DegradedFromClean)         # the input arena is made on the device
        self.paired = self.synthetic or isinstance(dataset, PairedImageRestoration)
        self.raw = isinstance(dataset, NoisyBayerDemosaicking)          # the degradation is made per batch
        self.source = None           # kernels.PatchSource (PatchPairSource if paired): the arena(s), checked once
        self.raw_source = None       # raw: kernels.PatchRawSource over source's pack
        self.masked = isinstance(dataset, RandomMaskInpainting)         # so is the mask and its fill
        self.last_mask = None        # masked: the mask of the last batch, float32 [B, 1, h, w]
        self._draws = (None, None, None, None)

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _pack(self, used: Sequence[int], dev):
        """The files ``used`` of the dataset in one uint8 arena on ``dev``, sized from the csv's heights and
        widths: decoded one by one and sent in chunks of about CHUNK_BYTES, so the host never holds more than two
        chunks of decoded pictures.  Returns the packs: one, or for a paired dataset (input, target), every file
        decoded once and both arenas under one image table."""
        from . import restore
        ds, c = self.dataset, self.dataset.n_channels
        shapes = [(int(ds.img_infos.iloc[i]["height"]), int(ds.img_infos.iloc[i]["width"])) for i in used]
        host_table, total = restore._host_table(shapes, c)
        from_files = self.paired and not self.synthetic             # both arenas are decoded
        arenas = [torch.empty(total, dtype=torch.uint8, device=dev) for _ in range(2 if from_files else 1)]
        held, held_bytes, at = [[] for _ in arenas], 0, 0

        def flush():
            nonlocal held, held_bytes, at
            if held_bytes:
                for arena, parts in zip(arenas, held):
                    arena[at:at + held_bytes].copy_(torch.cat(parts))
                at += held_bytes
                held, held_bytes = [[] for _ in arenas], 0
        for i, shape in zip(used, shapes):
            a = ds.load_image(i)
            if a.shape[:2] != shape:
                raise ValueError(f"ImageSuperResolution: {ds.paths[i]} is {a.shape[0]} x {a.shape[1]}, the csv says "
                                 f"{shape[0]} x {shape[1]}")
            for parts, picture in zip(held, (a, ds.load_target(i, a)) if from_files else (a,)):
                parts.append(torch.from_numpy(np.ascontiguousarray(picture)).reshape(-1))
            held_bytes += a.size
            if held_bytes >= self.CHUNK_BYTES:
                flush()
        flush()
        table = torch.tensor(host_table, dtype=torch.int64).to(dev)
        return tuple(restore.ImagePack(arena, table, host_table, c, ("numpy",) * len(used)) for arena in arenas)

    def prepare(self):
        """Decode and pack the pictures now (otherwise the first batch does) and check the pack once; returns the
        restore.ImagePack, or for a paired dataset the (input, target) packs.  Serial PIL decodes: for a training
        set of thousands of files this takes minutes."""
        if self.source is None:
            from . import kernels
            dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            ds = self.dataset
            used = sorted({r[3] for r in ds.patchs_data_all})                # files no patch reads stay on disk
            slot = np.full(len(ds.paths), -1, dtype=np.int64)
            slot[used] = np.arange(len(used))
            self._slot = slot
            key = (tuple(ds.paths[i] for i in used), ds.n_channels, str(dev))
            if self.synthetic:
                key += ds.synthetic_key(used)
            elif self.paired:    # both arenas under one key: a curriculum decodes each file once
                key += (tuple(ds.target_paths[i] for i in used),)
            store = self.shared if self.shared is not None else {}
            if key not in store:
                packs = self._pack(used, dev)
                if self.synthetic:
                    packs = (ds.degrade_pack(packs[0], used), packs[0])
                store[key] = kernels.patch_pair_source(*packs) if self.paired else kernels.patch_source(*packs)
            self.source = store[key]
            if self.raw:             # the one clean arena, under its plain key, and this dataset's pattern codes
                raw_key = key + ("raw", tuple(ds.patterns[i] for i in used))
                if raw_key not in store:
                    store[raw_key] = kernels.patch_raw_source(self.source.pack, [ds.patterns[i] for i in used])
                self.raw_source = store[raw_key]
        return (self.source.input, self.source.target) if self.paired else self.source.pack

    def epoch_draws(self, epoch: int) -> Tuple[np.ndarray, np.ndarray]:
        """(modes int64 [n], sigma float32 [n]) of the epoch, in dataset order."""
        ds = self.dataset
        if self._draws[0] != (epoch, len(ds)):
            rs = np.random.RandomState((ds.seed * 1000003 + epoch) % (2 ** 32))
            n = len(ds)
            modes = rs.randint(0, 8, n) if ds.use_data_augmentation else np.zeros(n, np.int64)
            if ds.dist_mode == "vary_addictive_noise":
                levels = rs.choice(ds.lambda_noise[0], p=ds.lambda_noise[1], size=n)
            elif ds.dist_mode == "none":
                levels = np.zeros(n)
            else:
                levels = np.full(n, ds.lambda_noise)
            sigma = (np.asarray(levels, dtype=np.float64) / 255.0).astype(np.float32)
            noise = raw_noise_pairs(_draw_levels(rs, ds.shot, n), _draw_levels(rs, ds.read, n)) if self.raw else None
            if self.masked:          # the known shares in the kernel's units, in the noise pairs' place
                noise = np.rint(_draw_levels(rs, ds.keep, n) * float(1 << 24)).astype(np.int64)
            self._draws = ((epoch, n), modes.astype(np.int64), sigma, noise)
        return self._draws[1], self._draws[2]

    def epoch_noise(self, epoch: int) -> np.ndarray:
        """The float32 [n, 2] noise pairs (a, b) of the epoch of a NoisyBayerDemosaicking dataset, in dataset order:
        drawn from the epoch's stream after epoch_draws' own draws, the shot levels first."""
        self.epoch_draws(epoch)
        return self._draws[3]

    def epoch_keep(self, epoch: int) -> np.ndarray:
        """The int64 [n] known shares of the epoch of a RandomMaskInpainting dataset in units of 2^-24, in dataset
        order: round(keep 2^24), the levels drawn from the epoch's stream after epoch_draws' own draws."""
        self.epoch_draws(epoch)
        return self._draws[3]

    def batch(self, positions: Sequence[int]):
        """(noisy, clean) -- (input, target) of a paired dataset -- of the samples at these positions of the current
        epoch's selection."""
        from . import kernels
        ds = self.dataset
        epoch = int(ds.epoch)
        modes, sigma = self.epoch_draws(epoch)
        pos = np.asarray(positions, dtype=np.int64)
        self.prepare()
        plan = ds.plan[pos]
        rows = np.stack([self._slot[plan[:, 0]], plan[:, 1], plan[:, 2], modes[pos]], axis=1)
        h, w = ds.out_size()
        ids = (np.int64(epoch) << 32) | pos
        if self.raw:
            target, inp = kernels.patch_raw_batch(self.raw_source, rows, ids,
                                                  None if ds.noise_free else self.epoch_noise(epoch)[pos], ds.seed, h, w,
                                                  ds.fill, ds.bits, ds.clip)
            return inp, target
        if self.masked:
            target, inp, self.last_mask = kernels.patch_mask_batch(self.source, rows, ids, self.epoch_keep(epoch)[pos],
                                                                   ds.seed, h, w, ds.weights, ds.fill, ds.hole)
            return inp, target
        if self.paired:
            target, inp = kernels.patch_pair_batch(self.source, rows, ids, None if ds.dist_mode == "none" else sigma[pos],
                                                   ds.seed, h, w)
            return inp, target
        clean, noisy = kernels.patch_batch(self.source, rows, ids, sigma[pos], ds.seed, h, w)
        return noisy, clean

    def __iter__(self):
        held: List[int] = []
        for p in self.sampler:
            held.append(p)
            if len(held) == self.batch_size:
                yield self.batch(held)
                held = []
        if held and not self.drop_last:
            yield self.batch(held)


DATASETS = {c.__name__: c for c in (AddictiveGaussianNoiseImagePair, SyntheticNoisyPatches, ImageSuperResolution,
                                    PairedImageRestoration, BicubicSuperResolution, JpegArtifactRemoval,
                                    BayerDemosaicking, NoisyBayerDemosaicking, GaussianMotionDeblurring,
                                    RandomMaskInpainting)}


# ---------------------------------------------------------------------------
# periodic validation (scripts_v2/run_abtract_lightformer_GGTV_GGLR_sigma25.py:235-288)
# ---------------------------------------------------------------------------
class TestImagesCSV:
    """Whole clean test images listed in a csv (column ``path``, as the reference's
    dataset/CBSD68_testing_data_info.csv), HWC float32 in [0, 1] on the uint8 grid (:250-258)."""

    def __init__(self, csv_path, root_folder="", **_ignored):
        import pandas as pd
        self.paths = [os.path.join(root_folder, p) for p in pd.read_csv(csv_path, index_col="index")["path"].tolist()]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, idx):
        from PIL import Image
        return np.array(Image.open(self.paths[idx])).astype(np.float32) / 255.0


class SyntheticTestImages:
    """Deterministic synthetic clean test images (no image data ships with the reference); the default
    sizes are not multiples of 16, so the reflect padding of the recipe is exercised."""

    def __init__(self, n_images=4, height=100, width=140, n_channels=3, seed=68, **_ignored):
        self.n, self.h, self.w, self.c, self.seed = n_images, height, width, n_channels, seed

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        return synthetic_clean_patch(np.random.RandomState(self.seed * 7919 + idx), self.h, self.w, self.c)


class TestPairsCSV:
    """Whole degraded / clean test pictures listed in a csv (columns index, path, target_path): item i is the
    (input, target) pair as uint8 H x W x C arrays, as restore.evaluate_pairs takes them."""
    __test__ = False        # a dataset, not a pytest class

    def __init__(self, csv_path, root_folder="", **_ignored):
        import pandas as pd
        infos = pd.read_csv(csv_path, index_col="index")
        for column in ("path", "target_path"):
            if column not in infos.columns:
                raise ValueError(f"TestPairsCSV: {csv_path} needs the columns path and target_path, got "
                                 f"{list(infos.columns)}")
        self.paths = [os.path.join(root_folder, p) for p in infos["path"].tolist()]
        self.target_paths = [os.path.join(root_folder, p) for p in infos["target_path"].tolist()]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, idx):
        from PIL import Image
        pair = []
        for path in (self.paths[idx], self.target_paths[idx]):
            a = np.array(Image.open(path))
            if a.dtype != np.uint8:
                raise ValueError(f"TestPairsCSV: {path} is {a.dtype}; only 8-bit pictures are supported")
            pair.append(a[:, :, None] if a.ndim == 2 else a)
        if pair[0].shape != pair[1].shape:
            raise ValueError(f"TestPairsCSV: {self.paths[idx]} is {pair[0].shape} and its target "
                             f"{self.target_paths[idx]} is {pair[1].shape}")
        return pair[0], pair[1]


VAL_DATASETS = {c.__name__: c for c in (TestImagesCSV, SyntheticTestImages, TestPairsCSV)}


def _img_as_ubyte(x: np.ndarray) -> np.ndarray:
    """skimage.util.img_as_ubyte of a float32 image in [0, 1] (the reference's :279): skimage's
    float -> uint8 ``_convert`` multiplies in the smallest float type of at least the input's size that
    holds the output (float32 here: ``np.multiply(x, 255, dtype=float32)``), rounds half to even
    (``np.rint``), clips to [0, 255] and casts.  The float32 product matters at ties: a value whose
    float64 product lies just below k + 0.5 can round to k + 0.5 in float32 and go to the even k."""
    y = np.multiply(np.asarray(x, dtype=np.float32), np.float32(255.0), dtype=np.float32)
    np.rint(y, out=y)
    np.clip(y, 0, 255, out=y)
    return y.astype(np.uint8)


@torch.no_grad()
def validate(model: nn.Module, images, sigma: float = 25.0, factor: int = 16, seed: int = 2204,
             device=None) -> float:
    """The reference's test loop (:235-288): per image, add N(0, sigma/255) noise from one
    RandomState(seed) stream, reflect-pad the bottom / right to a multiple of ``factor`` (only a side
    that is not already one), filter, crop, clamp to [0, 1], quantise with img_as_ubyte, MSE against
    the clean image x 255, PSNR = 20 log10(255 / sqrt(MSE)); returns the mean PSNR over the images.

    Several ranks: each filters a contiguous share of the images -- the noise draws follow the global
    image order, as one rank would make them -- and the PSNR sum and count are all-reduced."""
    rank, world = sharding.world()
    was_training = model.training
    model.eval()
    if device is None:
        device = next(model.parameters()).device
    rs = np.random.RandomState(seed=seed)
    s, e = sharding.shard_range(len(images), rank, world)
    psnrs = []
    for i in range(len(images)):
        img_true = np.asarray(images[i], dtype=np.float32)
        noisy_raw = img_true.copy()
        noisy_raw += rs.normal(0, sigma / 255.0, img_true.shape)     # float32 += float64 draws (:258)
        if not s <= i < e:
            continue
        noisy = torch.from_numpy(noisy_raw).permute(2, 0, 1).unsqueeze(0)
        h, w = noisy.shape[2], noisy.shape[3]
        H, W = ((h + factor) // factor) * factor, ((w + factor) // factor) * factor
        padh = H - h if h % factor != 0 else 0
        padw = W - w if w % factor != 0 else 0
        noisy = nn.functional.pad(noisy, (0, padw, 0, padh), "reflect")
        restored = model(noisy.to(device).contiguous())[:, :, :h, :w]
        restored = torch.clamp(restored, 0, 1).cpu().permute(0, 2, 3, 1).squeeze(0).numpy()
        restored = _img_as_ubyte(restored).astype(np.float32)
        img_true_255 = np.rint(img_true.astype(np.float64) * 255.0).astype(np.float32)   # the uint8 image (:253)
        mse = np.square(img_true_255 - restored).mean()                                  # float32, as :273
        psnrs.append(float(20 * np.log10(np.float32(255.0) / np.sqrt(mse))))
    if was_training:
        model.train()
    return _mean_over_ranks(psnrs, world, device)


def _mean_over_ranks(values, world: int, device) -> float:
    """The mean of per-image values over all ranks: this rank's float64 [sum, count], moved to ``device`` under NCCL,
    all-reduced; the one tail of validate and of every validate_* below."""
    acc = torch.tensor([float(np.sum(values)), float(len(values))], dtype=torch.float64)
    if world > 1:
        if torch.distributed.get_backend() == "nccl":
            acc = acc.to(device)
        torch.distributed.all_reduce(acc)
    return float(acc[0] / acc[1])


def _clean_share_u8(images, rank: int, world: int) -> list:
    """This rank's share (sharding.shard_range) of a clean test set as uint8 H x W x C arrays: a 2-D picture gets its
    channel axis, a float one in [0, 1] on the uint8 grid (as TestImagesCSV yields them) becomes rint(x 255)."""
    s, e = sharding.shard_range(len(images), rank, world)
    mine = []
    for i in range(s, e):
        a = np.asarray(images[i])
        a = a[:, :, None] if a.ndim == 2 else a
        mine.append(a if a.dtype == np.uint8 else np.rint(a.astype(np.float64) * 255.0).astype(np.uint8))
    return mine


def _validate_degraded(name: str, val_metrics, evaluate: Callable, model, images, device, metric: str, **args) -> float:
    """The one body of validate_sr, validate_car and validate_demosaic: the metric checked first, this rank's share
    of the pictures through ``evaluate`` (a restore.evaluate_* with its protocol's ``args``), the mean over ranks."""
    if metric not in val_metrics:
        raise ValueError(f"{name}: metric is one of {val_metrics}, got {metric!r}")
    rank, world = sharding.world()
    if device is None:
        device = next(model.parameters()).device
    mine = _clean_share_u8(images, rank, world)
    scores = evaluate(model, mine, device=device, metrics=(metric,), **args)[metric][1] if mine else []
    return _mean_over_ranks(scores, world, device)


VAL_PAIR_METRICS = ("psnr", "psnr_y")


def validate_pairs(model: nn.Module, pairs, factor: int = 16, device=None, metric: str = "psnr", **tiling_args) -> float:
    """Mean PSNR of ``model`` over degraded / clean pairs (``pairs[i]`` = (input, target), uint8 H x W x C, a
    TestPairsCSV for instance): restore.evaluate_pairs on this rank's share.  Nothing is drawn: each input is
    restored as it is and scored against its target from the exact integer SSE.  ``metric``: "psnr", or "psnr_y"
    for the PSNR on the Y channel of RGB pairs (restore.psnr_y_u8), the number deraining and super-resolution
    tables print.  tiling_args: tile, halo, micro_batch, ensemble, across_images.

    Several ranks: each takes sharding.shard_range's share of the pairs and the PSNR sum and count are all-reduced,
    as validate does."""
    from . import restore
    if metric not in VAL_PAIR_METRICS:
        raise ValueError(f"validate_pairs: metric is one of {VAL_PAIR_METRICS}, got {metric!r}")
    rank, world = sharding.world()
    if device is None:
        device = next(model.parameters()).device
    s, e = sharding.shard_range(len(pairs), rank, world)
    mine = [pairs[i] for i in range(s, e)]
    psnrs = restore.evaluate_pairs(model, [p[0] for p in mine], [p[1] for p in mine], factor=factor, device=device,
                                   metrics=(metric,), **tiling_args)[metric][1] if mine else []
    return _mean_over_ranks(psnrs, world, device)


VAL_SR_METRICS = ("psnr", "psnr_y")


def validate_sr(model: nn.Module, images, scale: int, shave: Optional[int] = None, factor: int = 16, device=None,
                metric: str = "psnr_y", **tiling_args) -> float:
    """Mean PSNR of ``model`` on the bicubic super-resolution protocol over clean test pictures (``images[i]``: uint8
    H x W x C, or float32 in [0, 1] on the uint8 grid as TestImagesCSV yields them): restore.evaluate_sr on this
    rank's share -- mod-crop, degrade by ``scale`` on the device, restore, shave ``shave`` (default ``scale``)
    border pixels, score.  ``metric``: "psnr_y" (default, the tables' number) or "psnr".  Nothing is drawn.
    tiling_args: tile, halo, micro_batch, ensemble.

    Several ranks: sharded and all-reduced as validate_pairs does."""
    from . import restore
    return _validate_degraded("validate_sr", VAL_SR_METRICS, restore.evaluate_sr, model, images, device, metric,
                              scale=scale, shave=shave, factor=factor, **tiling_args)


VAL_CAR_METRICS = ("psnr", "psnr_y", "psnrb")


def validate_car(model: nn.Module, images, jpeg_quality: int, subsampling: int = 0, factor: int = 16, device=None,
                 metric: str = "psnr", **tiling_args) -> float:
    """Mean score of ``model`` on JPEG compression-artifact removal over clean test pictures (``images[i]``: uint8
    H x W x C, or float32 in [0, 1] on the uint8 grid as TestImagesCSV yields them): restore.evaluate_car on this
    rank's share -- the JPEG round trip at ``jpeg_quality`` on the device, restore, score against the clean picture.
    ``metric``: "psnr" (default), "psnr_y" or "psnrb" (PSNR-B).  Nothing is drawn.  tiling_args: tile, halo,
    micro_batch, ensemble.

    Several ranks: sharded and all-reduced as validate_pairs does."""
    from . import restore
    return _validate_degraded("validate_car", VAL_CAR_METRICS, restore.evaluate_car, model, images, device, metric,
                              quality=jpeg_quality, subsampling=subsampling, factor=factor, **tiling_args)


VAL_DEMOSAIC_METRICS = ("psnr", "psnr_y", "ssim")


def validate_demosaic(model: nn.Module, images, bayer="rggb", fill="malvar", shave: int = 0, factor: int = 16,
                      device=None, metric: str = "psnr", **tiling_args) -> float:
    """Mean score of ``model`` on Bayer demosaicking over clean RGB test pictures (``images[i]``: uint8 H x W x 3, or
    float32 in [0, 1] on the uint8 grid as TestImagesCSV yields them): restore.evaluate_demosaic on this rank's
    share -- mosaic with the pattern ``bayer`` and ``fill`` on the device, restore, cut ``shave`` pixels from each
    side, score against the clean picture.  ``metric``: "psnr" (default: over the three channels, the CPSNR),
    "psnr_y" or "ssim".  Nothing is drawn.  tiling_args: tile, halo, micro_batch, ensemble.

    Several ranks: sharded and all-reduced as validate_pairs does."""
    from . import restore
    return _validate_degraded("validate_demosaic", VAL_DEMOSAIC_METRICS, restore.evaluate_demosaic, model, images, device,
                              metric, pattern=bayer, fill=fill, shave=shave, factor=factor, **tiling_args)


def validate_jdd(model: nn.Module, images, raw_noise=(0.0, 0.0), bayer="rggb", fill="malvar", bits: int = 16,
                 clip: bool = True, seed: int = 2204, shave: int = 0, factor: int = 16, device=None, metric: str = "psnr",
                 **tiling_args) -> float:
    """Mean score of ``model`` on joint denoising and demosaicking over clean RGB test pictures (``images[i]``: uint8
    H x W x 3, or float32 in [0, 1] on the uint8 grid as TestImagesCSV yields them): restore.evaluate_jdd on this
    rank's share -- mosaic with the pattern ``bayer``, sensor noise ``raw_noise`` = (shot, read) on the mosaic, ``bits``
    bits, ``fill``, all on the device, restore, cut ``shave`` pixels from each side, score against the clean picture.
    ``metric``: "psnr" (default, the CPSNR), "psnr_y" or "ssim".  The noise of a picture is a function of (seed, its
    index in this rank's share); nothing is drawn on the host.  tiling_args: tile, halo, micro_batch, ensemble.

    Several ranks: sharded and all-reduced as validate_pairs does."""
    from . import restore
    if not isinstance(raw_noise, (list, tuple)) or len(raw_noise) != 2:
        raise ValueError(f"validate_jdd: raw_noise is (shot, read), got {raw_noise!r}")
    return _validate_degraded("validate_jdd", VAL_DEMOSAIC_METRICS, restore.evaluate_jdd, model, images, device, metric,
                              pattern=bayer, fill=fill, shot=raw_noise[0], read=raw_noise[1], bits=bits, clip=clip,
                              seed=seed, shave=shave, factor=factor, **tiling_args)


VAL_INPAINT_METRICS = ("psnr", "psnr_y", "ssim", "psnr_missing")


def validate_inpaint(model: nn.Module, images, inpaint_keep: float = 0.5, fill="conv", fill_side: int = 7,
                     fill_sigma: Optional[float] = None, hole: int = 128, seed: int = 2204, passes: int = 1,
                     shave: int = 0, factor: int = 16, device=None, metric: str = "psnr", **tiling_args) -> float:
    """Mean score of ``model`` on inpainting over clean test pictures (``images[i]``: uint8 H x W x C, or float32 in
    [0, 1] on the uint8 grid as TestImagesCSV yields them): restore.evaluate_inpaint on this rank's share -- a pixel
    is known with probability ``inpaint_keep``, the missing ones are filled by ``fill`` (``fill_side``, ``fill_sigma``,
    ``hole``, ``passes``), all on the device, the filled picture is restored, the known pixels are put back, ``shave``
    pixels are cut from each side and the result is scored against the clean picture.  ``metric``: "psnr" (default),
    "psnr_y", "ssim" or "psnr_missing" (the PSNR over the missing pixels alone).  The mask of a picture is a function
    of (seed, its index in this rank's share); nothing is drawn on the host.  tiling_args: tile, halo, micro_batch,
    ensemble.

    Several ranks: sharded and all-reduced as validate_pairs does."""
    from . import restore
    return _validate_degraded("validate_inpaint", VAL_INPAINT_METRICS, restore.evaluate_inpaint, model, images, device,
                              metric, keep=inpaint_keep, fill=fill, fill_side=fill_side, fill_sigma=fill_sigma, hole=hole,
                              seed=seed, passes=passes, shave=shave, factor=factor, **tiling_args)


VAL_DEBLUR_METRICS = ("psnr", "psnr_y", "ssim")


def validate_deblur(model: nn.Module, images, blur, boundary="wrap", noise_sigma: float = 0.0, seed: int = 2204,
                    shave: int = 0, factor: int = 16, device=None, metric: str = "psnr", **tiling_args) -> float:
    """Mean score of ``model`` on deblurring over clean test pictures (``images[i]``: uint8 H x W x C, or float32 in
    [0, 1] on the uint8 grid as TestImagesCSV yields them): restore.evaluate_deblur on this rank's share -- blur with
    the kernel spec ``blur`` under ``boundary`` on the device, add N(0, noise_sigma / 255) noise where ``noise_sigma``
    is positive (drawn on the host from RandomState(seed), in the order of this rank's pictures), restore, cut
    ``shave`` pixels from each side, score against the clean picture.  ``metric``: "psnr" (default), "psnr_y" or
    "ssim".  tiling_args: tile, halo, micro_batch, ensemble.

    Several ranks: sharded and all-reduced as validate_pairs does."""
    from . import restore
    return _validate_degraded("validate_deblur", VAL_DEBLUR_METRICS, restore.evaluate_deblur, model, images, device,
                              metric, kernel=blur, boundary=boundary, noise_sigma=noise_sigma, seed=seed, shave=shave,
                              factor=factor, **tiling_args)


def _val_blur_spec(v) -> str:
    """``datasets.val.blur``: a kernel spec string, parsed once here so that a bad one is refused with the config."""
    if not isinstance(v, str):
        raise ValueError(f"datasets.val.blur is a kernel spec string such as 'gaussian:25:1.6', got {v!r}")
    parse_blur_spec(v)
    return v


def _val_raw_noise(v) -> List[float]:
    """``datasets.val.raw_noise``: [shot, read], checked here so that a bad pair is refused with the config."""
    from . import kernels
    if not isinstance(v, (list, tuple)) or len(v) != 2:
        raise ValueError(f"datasets.val.raw_noise is [shot, read] (a gain of 0..1, 8-bit levels of 0..255), got {v!r}")
    kernels.raw_noise_pair("datasets.val.raw_noise", v[0], v[1])
    return [float(v[0]), float(v[1])]


class _ValProtocol(NamedTuple):
    """A row of _VAL_PROTOCOLS: how a ``datasets.val`` section selects a validator, and which of its keys the
    validator gets (beside factor, tile, halo, micro_batch and metric, which every row has)."""
    key: Optional[str]              # the YAML key that selects the row on a set of ``dataset``; None: the set alone does
    dataset: type
    convert: Optional[Callable]     # the selecting key's value as the validator takes it
    int_keys: Tuple[str, ...]       # the row's own optional integer keys
    choices: dict                   # its string keys, the selecting one included, with their allowed values
    metrics: Tuple[str, ...]
    validator: Callable
    float_keys: Tuple[str, ...] = ()    # the row's own optional float keys


_VAL_PROTOCOLS = (      # in order of precedence; a section that selects no row is the noise protocol, validate's
    _ValProtocol("jpeg_quality", TestImagesCSV, int, ("subsampling",), {}, VAL_CAR_METRICS, validate_car),
    _ValProtocol("bayer", TestImagesCSV, str, ("shave",), {"bayer": BAYER_PATTERNS, "fill": BAYER_FILLS},
                 VAL_DEMOSAIC_METRICS, validate_demosaic),
    _ValProtocol("scale", TestImagesCSV, int, ("shave",), {}, VAL_SR_METRICS, validate_sr),
    _ValProtocol("blur", TestImagesCSV, _val_blur_spec, ("shave",), {"boundary": BLUR_BOUNDARIES}, VAL_DEBLUR_METRICS,
                 validate_deblur, ("noise_sigma",)),
    _ValProtocol(None, TestPairsCSV, None, (), {}, VAL_PAIR_METRICS, validate_pairs),
)


# Joint denoising and demosaicking refines the ``bayer`` row: a section with a ``raw_noise`` key is taken here, directly
# before that row, and a section without one never sees this record
_VAL_RAW_NOISE = _ValProtocol("raw_noise", TestImagesCSV, _val_raw_noise, ("shave", "bits"),
                              {"bayer": BAYER_PATTERNS, "fill": BAYER_FILLS}, VAL_DEMOSAIC_METRICS, validate_jdd)


def _val_keep(v) -> float:
    """``datasets.val.inpaint_keep``: the known share, checked here so that a bad one is refused with the config."""
    from . import kernels
    try:
        kernels.keep_units(v)
    except ValueError:
        raise ValueError(f"datasets.val.inpaint_keep is the known share of the pixels, a number of 0..1, got {v!r}") from None
    return float(v)


# Inpainting stands before every other row: a section with an ``inpaint_keep`` key is taken here, and a section without
# one never sees this record
_VAL_INPAINT = _ValProtocol("inpaint_keep", TestImagesCSV, _val_keep, ("shave", "fill_side", "hole", "passes", "seed"),
                            {"fill": MASK_FILLS}, VAL_INPAINT_METRICS, validate_inpaint, ("fill_sigma",))


def _val_rows() -> Iterator[_ValProtocol]:
    """Every row a ``datasets.val`` section is matched against, in order of precedence: _VAL_INPAINT, then
    _val_protocols' rows."""
    yield _VAL_INPAINT
    yield from _val_protocols()


def _val_protocols() -> Iterator[_ValProtocol]:
    """The rows a ``datasets.val`` section is matched against, in order of precedence: _VAL_PROTOCOLS with
    _VAL_RAW_NOISE directly before the ``bayer`` row."""
    for p in _VAL_PROTOCOLS:
        if p.key == "bayer":
            yield _VAL_RAW_NOISE
        yield p


def val_check(val_set, val_args: dict) -> Callable:
    """The validator of what create_val_dataset returned: ``val_check(val_set, val_args)(model, val_set, device=device,
    **val_args)`` is the validation run() makes."""
    for p in _val_rows():
        if (p.key in val_args) if p.key else isinstance(val_set, p.dataset):
            return p.validator
    return validate


def create_val_dataset(conf: dict):
    """``datasets.val`` of the YAML ({type, dataset_args, sigma, factor}), or None.  A paired set (TestPairsCSV)
    takes {type, dataset_args, factor, tile, halo, micro_batch, metric}: validate_pairs' arguments, no sigma; without
    ``metric`` validate_pairs' default, the RGB PSNR, is scored.  TestImagesCSV with a ``scale`` key is the bicubic
    super-resolution protocol: {type, dataset_args, scale, shave, factor, tile, halo, micro_batch, metric},
    validate_sr's arguments, no sigma.  TestImagesCSV with a ``jpeg_quality`` key is JPEG artifact removal:
    {type, dataset_args, jpeg_quality, subsampling, factor, tile, halo, micro_batch, metric}, validate_car's
    arguments, no sigma.  TestImagesCSV with a ``bayer`` key (a pattern name) is demosaicking:
    {type, dataset_args, bayer, fill, shave, factor, tile, halo, micro_batch, metric}, validate_demosaic's arguments,
    no sigma.  With a ``raw_noise`` key ([shot, read]) as well, or alone, it is joint denoising and demosaicking:
    {type, dataset_args, raw_noise, bayer, fill, shave, bits, factor, tile, halo, micro_batch, metric}, validate_jdd's
    arguments; ``raw_noise`` takes precedence over ``bayer``.  TestImagesCSV with a ``blur`` key (a kernel spec string) is deblurring:
    {type, dataset_args, blur, boundary, noise_sigma, shave, factor, tile, halo, micro_batch, metric},
    validate_deblur's arguments; the noise on the blurred picture is ``noise_sigma``, not ``sigma``.  TestImagesCSV with
    an ``inpaint_keep`` key (the known share of 0..1) is inpainting and takes precedence over all of them:
    {type, dataset_args, inpaint_keep, fill, fill_side, fill_sigma, hole, passes, seed, shave, factor, tile, halo,
    micro_batch, metric}, validate_inpaint's arguments."""
    vconf = conf.get("datasets", {}).get("val")
    if not vconf:
        return None, {}
    cls = VAL_DATASETS.get(vconf["type"])
    if cls is None:
        raise ValueError(f"Validation dataset {vconf['type']} is not found.")
    for p in _val_rows():
        if cls is not p.dataset or (p.key is not None and vconf.get(p.key) is None):
            continue
        for k, allowed in p.choices.items():
            if vconf.get(k) is not None and vconf[k] not in allowed:
                raise ValueError(f"datasets.val.{k} is one of {allowed}, got {vconf[k]!r}")
        args = {k: int(vconf[k]) for k in ("tile", "halo", "micro_batch") + p.int_keys if vconf.get(k) is not None}
        args.update({k: float(vconf[k]) for k in p.float_keys if vconf.get(k) is not None})
        args.update({k: str(vconf[k]) for k in p.choices if k != p.key and vconf.get(k) is not None})
        if vconf.get("metric") is not None:
            if vconf["metric"] not in p.metrics:
                raise ValueError(f"datasets.val.metric is one of {p.metrics}, got {vconf['metric']!r}")
            args["metric"] = str(vconf["metric"])
        dataset = cls(**vconf.get("dataset_args", {}))
        if p.key is not None:
            args[p.key] = p.convert(vconf[p.key])
        return dataset, dict(args, factor=int(vconf.get("factor", 16)))
    return cls(**vconf.get("dataset_args", {})), {"sigma": float(vconf.get("sigma", 25.0)),
                                                   "factor": int(vconf.get("factor", 16))}


class ResumeableSampler(Sampler):
    """Deterministic in-order sampling that resumes after ``current_sample`` (data_sampler.py:6-31).
    With world_size > 1 each rank yields its own contiguous slice of every global batch, and the
    epoch is cut to whole global batches (the tail of num_samples % (batch_size * world_size) is
    dropped) so every rank runs the same number of full steps — a rank with one more batch would
    block forever in the gradient all-reduce."""

    def __init__(self, dataset, batch_size: int = 1, rank: int = 0, world_size: int = 1):
        self.dataset = dataset
        self.epoch = 0
        self.current_sample = -1
        self.batch_size, self.rank, self.world_size = batch_size, rank, world_size
        n = len(dataset)
        self.num_samples = n if world_size == 1 else n - n % (batch_size * world_size)

    def _mine(self, i: int) -> bool:
        if self.world_size == 1:
            return True
        gb = self.batch_size * self.world_size
        return (i % gb) // self.batch_size == self.rank

    def __iter__(self) -> Iterator[int]:
        for sample_i in range(self.num_samples):
            if sample_i > self.current_sample:
                self.current_sample += 1
                if self._mine(sample_i):
                    yield sample_i

    def __len__(self):
        return self.num_samples // self.world_size

    def set_epoch_and_current_sample(self, current_epoch, current_sample):
        self.epoch = self.current_epoch = current_epoch
        self.current_sample = current_sample
        self.dataset.random_permute(seed=2024 + current_epoch)

    def steps_per_epoch(self, drop_last: bool = False) -> int:
        """Optimisation steps one epoch holds: a partial last batch counts unless the loader drops
        it (dataloader_args.drop_last); with world_size > 1 there is none (whole global batches)."""
        local = self.num_samples // self.world_size
        return local // self.batch_size if drop_last else -(-local // self.batch_size)


def create_dataset(dataset_conf: dict, environ_conf: dict):
    cls = DATASETS.get(dataset_conf["type"])
    if cls is None:
        raise ValueError(f"Dataset {dataset_conf['type']} is not found (the datasets are {sorted(DATASETS)}).")
    return cls(**dataset_conf["dataset_args"])


def create_dataloader(dataset, sampler, dataset_conf: dict, environ_conf: dict):
    args = dict(dataset_conf["dataloader_args"])
    return torch.utils.data.DataLoader(dataset=dataset, sampler=sampler, **args)


class TrainStage:
    """One loader of the training curriculum: dataset + resumable sampler + dataloader, and the
    optimisation steps it holds per epoch."""

    def __init__(self, index: int, ds_conf: dict, environ_conf: dict, rank: int, world: int, shared=None):
        self.index = index
        self.dataset = create_dataset(ds_conf, environ_conf)
        self.batch_size = int(ds_conf["dataloader_args"].get("batch_size", 1))
        self.drop_last = bool(ds_conf["dataloader_args"].get("drop_last", False))
        self.sampler = ResumeableSampler(self.dataset, self.batch_size, rank, world)
        if ds_conf.get("device_resident"):
            # batches made on the device from a packed arena; dataloader_args' num_workers is ignored
            if not isinstance(self.dataset, ImageSuperResolution):
                raise ValueError(f"training stage {index}: device_resident needs type ImageSuperResolution, "
                                 "PairedImageRestoration, BicubicSuperResolution, JpegArtifactRemoval, BayerDemosaicking, "
                                 "NoisyBayerDemosaicking or GaussianMotionDeblurring, got "
                                 f"{ds_conf['type']}")
            self.loader = DevicePatchLoader(self.dataset, self.sampler, self.batch_size, self.drop_last,
                                            shared=shared)
        else:
            self.loader = create_dataloader(self.dataset, self.sampler, ds_conf, environ_conf)
        self.steps = self.sampler.steps_per_epoch(self.drop_last)
        if self.steps <= 0:
            raise ValueError(f"training stage {index}: dataset of {len(self.dataset)} samples holds no batch of "
                             f"{self.batch_size} x {world} ranks")


def train_stage_confs(conf: dict) -> List[dict]:
    """``datasets.train`` as a list of stage configurations: one dict (one loader), or a list of them --
    the v2 script's curriculum, four loaders chained per epoch (128^2 x 4, 192^2 x 3, 256^2 x 2,
    384^2 x 1; scripts_v2/run_abtract_lightformer_GGTV_GGLR_sigma25.py:50-115, :185)."""
    tr = conf["datasets"]["train"]
    return list(tr) if isinstance(tr, (list, tuple)) else [tr]


def build_train_stages(conf: dict, rank: int = 0, world: int = 1) -> List[TrainStage]:
    """The stages of an epoch, in order.  Data-parallel policy: a stage's ``batch_size`` is per rank (its
    global batch is batch_size x world) and each stage's epoch is cut to whole global batches, so every
    rank runs the same number of steps in every stage and all ranks stay in one all-reduce sequence --
    the 384^2 x 1 stage on 8 GPUs is a global batch of 8, one patch per rank."""
    shared: dict = {}     # the device-resident stages' arena, one per set of files: it lives as long as the stages
    return [TrainStage(k, dc, conf, rank, world, shared) for k, dc in enumerate(train_stage_confs(conf))]


# ---------------------------------------------------------------------------
# model / optimiser / schedule (v2 script :120-171)
# ---------------------------------------------------------------------------
def build_model(model_conf: dict) -> nn.Module:
    import irdu_amd
    kind = model_conf.get("type", "AbtractMultiScaleGraphFilter")
    from irdu_amd import window_graph, window_graph_v1
    cls = {"AbtractMultiScaleGraphFilter": irdu_amd.AbtractMultiScaleGraphFilter,
           "MultiScaleGraphFilter": irdu_amd.MultiScaleGraphFilter,
           "GLRImageFilter": irdu_amd.GLRImageFilter,
           "MultiScaleGLRImageFilter": irdu_amd.MultiScaleGLRImageFilter,
           # window-graph denoisers of the multiblocks scripts (REF7 v7 / REF1 v1)
           "MultiScaleSequenceDenoiser": window_graph.MultiScaleSequenceDenoiser,
           "MultiScaleSequenceDenoiserV1": window_graph_v1.MultiScaleSequenceDenoiser}.get(kind)
    if cls is None:
        raise ValueError(f"model type {kind!r} has no training path")
    return cls(**model_conf.get("args", {}))


def build_optimizer(model: nn.Module, tconf: dict):
    """Adam + MultiStepLR(gamma=sqrt(sqrt(0.5))) -> CosineAnnealingLR (base lr 5e-5) via SequentialLR;
    ``lr_schedule: multistep`` is the multiblocks scripts' Adam + MultiStepLR(milestones, lr_gamma)
    (run_lightformer_GGTV_GGLR_multiblocks.py:166-174)."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, MultiStepLR, SequentialLR
    opt = torch.optim.Adam(model.parameters(), lr=tconf.get("lr", 4e-4), eps=tconf.get("eps", 1e-8))
    if tconf.get("lr_schedule", "v2") == "multistep":
        return opt, MultiStepLR(opt, milestones=list(tconf.get("milestones", [200000, 500000, 650000])),
                                gamma=float(tconf.get("lr_gamma", 0.5)))
    switch = tconf.get("cosine_from", 600000)
    s1 = MultiStepLR(opt, milestones=list(tconf.get("milestones", range(50000, 600001, 50000))),
                     gamma=float(np.sqrt(np.sqrt(0.5))))
    s2 = CosineAnnealingLR(opt, T_max=tconf.get("cosine_T_max", 701000), eta_min=tconf.get("eta_min", 1e-6))
    s2.base_lrs = [tconf.get("cosine_base_lr", 5e-5) for _ in opt.param_groups]
    return opt, SequentialLR(opt, schedulers=[s1, s2], milestones=[switch])


class Trainer:
    """One optimisation step = the v2 script's loop body (:186-207) + the DDP gradient average."""

    def __init__(self, model: nn.Module, tconf: dict, device):
        self.model, self.device = model.to(device), device
        self.optimizer, self.lr_scheduler = build_optimizer(self.model, tconf)
        self.w_encdec = float(tconf.get("loss02_weight", 0.1))
        self.w_perturb = float(tconf.get("loss03_weight", 0.5))
        self.latent_noise = float(tconf.get("latent_noise", 0.05))
        self.bucket_mb = float(tconf.get("allreduce_bucket_mb", 32.0))
        # train.ssim_weight w > 0: the loss gains w (1 - SSIM(out, clean)) on the HIP kernels (losses.ssim_loss);
        # 0 or absent: the op is never called
        self.w_ssim = float(tconf.get("ssim_weight", 0.0) or 0.0)
        if not (math.isfinite(self.w_ssim) and self.w_ssim >= 0.0):
            raise ValueError(f"train.ssim_weight must be a finite number >= 0 (got {tconf.get('ssim_weight')!r})")
        # train.native_convs: the v1.0 model's plain convolutions on libgrr (graph_filter.NATIVE_CONVS); absent:
        # the process-wide switch (GRR_NATIVE_CONVS, default off) is left as it is
        if tconf.get("native_convs") is not None:
            from . import graph_filter
            graph_filter.native_convs(bool(int(tconf["native_convs"])))
        # all-reduces overlapped with the reverse sweep (post-accumulate-grad hooks); inert on one rank
        self.reducer = sharding.OverlappedGradReducer(self.model.parameters(), bucket_mb=self.bucket_mb)
        self.i = 0
        self.val_history: List[Tuple[int, float]] = []     # (iteration, mean test PSNR)
        # training-time PSNR / MSE (:212-223): per step the batch's squared-error sum (float64, on the
        # device, no host sync) and its element count; summarised by train_metrics()
        self.track_metrics = bool(tconf.get("train_metrics", True))
        self._sse: List[torch.Tensor] = []
        self._n: List[int] = []
        self.train_history: List[Tuple[int, float, float]] = []   # (iteration, mean PSNR, mean MSE)

    def loss(self, noisy: torch.Tensor, clean: torch.Tensor, _out: Optional[list] = None) -> torch.Tensor:
        m = self.model
        out = m(noisy)
        if _out is not None:
            _out.append(out)
        loss = nn.functional.l1_loss(out, clean)
        if self.w_ssim:
            loss = loss + self.w_ssim * losses.ssim_loss(out, clean)
        if hasattr(m, "encode") and (self.w_encdec or self.w_perturb):
            latent = m.encode(clean)
            rec = m.decode(latent)
            disturbed = m.decode(tuple(t + torch.normal(0.0, self.latent_noise, size=t.shape, device=t.device)
                                       for t in latent))
            loss = loss + self.w_encdec * nn.functional.mse_loss(rec, clean)
            loss = loss + self.w_perturb * nn.functional.mse_loss(rec, disturbed)
        return loss

    def step(self, noisy_hwc: torch.Tensor, clean_hwc: torch.Tensor, channels_first: bool = False) -> float:
        """noisy/clean: [B,H,W,C] batches as the dataset yields them (permuted like :191-193), or, with
        channels_first, the planar [B,C,H,W] batches of a DevicePatchLoader, taken as they are."""
        self.model.train()
        self.optimizer.zero_grad(set_to_none=True)
        self.reducer.prepare()
        noisy = noisy_hwc.to(self.device, non_blocking=True)
        clean = clean_hwc.to(self.device, non_blocking=True)
        if not channels_first:
            noisy = noisy.permute(0, 3, 1, 2).contiguous()
            clean = clean.permute(0, 3, 1, 2).contiguous()
        outs: list = []
        with stream_guard.maybe_guard():       # GRR_STREAM_GUARD=1: check the internal-stream invariant
            loss = self.loss(noisy, clean, outs)
            loss.backward()
        self.reducer.finish()
        self.optimizer.step()
        self.lr_scheduler.step()
        if self.track_metrics:
            # :212-214: both images clipped to [0, 1], squared error in float64 (summed here, divided at
            # summary time, so several ranks' shares add up to the global batch's MSE)
            with torch.no_grad():
                d = outs[0].detach().clamp(0.0, 1.0).double() - clean.clamp(0.0, 1.0).double()
                self._sse.append(torch.sum(d * d))
            self._n.append(d.numel())
            del self._sse[:-100], self._n[:-100]
        self.i += 1
        return float(loss.detach())

    def train_metrics(self) -> Tuple[float, float]:
        """Mean PSNR and mean MSE over the last <= 100 steps (the reference's running window, :221-223):
        step k's MSE = its squared-error sum / element count over the global batch (summed over ranks,
        one all-reduce of the window), PSNR_k = 10 log10(1 / MSE_k).  Every rank must call it at the same
        iteration (it is collective when world > 1)."""
        if not self._sse:
            return float("nan"), float("nan")
        acc = torch.stack([torch.stack(self._sse), torch.tensor(self._n, dtype=torch.float64,
                                                                 device=self._sse[0].device)])
        rank, world = sharding.world()
        if world > 1:
            torch.distributed.all_reduce(acc)
        mse = (acc[0] / acc[1]).cpu().numpy()
        return float(np.mean(10.0 * np.log10(1.0 / mse))), float(np.mean(mse))

    def state_dict(self) -> dict:
        return {"i": self.i, "model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(),
                "lr_scheduler": self.lr_scheduler.state_dict()}

    def load_state_dict(self, ckpt: dict) -> None:
        self.model.load_state_dict(ckpt["model"])
        self.optimizer.load_state_dict(ckpt["optimizer"])
        self.lr_scheduler.load_state_dict(ckpt["lr_scheduler"])
        self.i = int(ckpt["i"])


def checkpoint_dir(conf: dict) -> str:
    return os.path.join(conf["path"]["root_dir"], "experiments", conf["name"], "learning_checkpoints")


def latest_checkpoint(conf: dict) -> Optional[str]:
    """run_train.py:42-55: the last file of the sorted checkpoint folder."""
    d = checkpoint_dir(conf)
    files = sorted(os.listdir(d)) if os.path.isdir(d) else []
    return os.path.join(d, files[-1]) if files else None


def run(conf: dict, device=None, max_iters: Optional[int] = None) -> Trainer:
    """Build everything from the YAML dict, resume from the latest checkpoint, train."""
    rank, world = sharding.world()
    if device is None:
        device = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}") if torch.cuda.is_available() \
            else torch.device("cpu")
    tconf = conf.get("train", {})
    stages = build_train_stages(conf, rank, world)
    for st in stages:
        if isinstance(st.loader, DevicePatchLoader) and st.loader.device is None:
            st.loader.device = device      # the arena lives where the model trains
    trainer = Trainer(build_model(conf.get("model", {})), tconf, device)
    ckpt_path = conf["path"].get("latest_checkpoint_path") or latest_checkpoint(conf)
    if world > 1:
        # every rank resumes rank 0's choice of checkpoint (ranks never pick their own latest file:
        # without a shared view they could resume at different iterations and block forever in the
        # gradient all-reduce)
        choice = [ckpt_path]
        torch.distributed.broadcast_object_list(choice, src=0)
        ckpt_path = choice[0]
    spe = sum(st.steps for st in stages)
    if ckpt_path:
        trainer.load_state_dict(torch.load(ckpt_path, map_location=device, weights_only=True))
        LOG.info("resumed from %s at iteration %d", ckpt_path, trainer.i)
    if world > 1:
        its = [None] * world
        torch.distributed.all_gather_object(its, trainer.i)
        if len(set(its)) != 1:
            raise RuntimeError(f"ranks resumed at different iterations {its} from {ckpt_path!r}")
    # replicas start identical whatever each rank's seed was (data-parallel averaging never
    # reconciles diverged weights); rank 0's weights are the ones checkpointed
    sharding.broadcast_module(trainer.model)
    os.makedirs(checkpoint_dir(conf), exist_ok=True)
    total = max_iters if max_iters is not None else int(tconf.get("total_iters", spe))
    every = int(tconf.get("checkpoint_every", 5000))
    verbose = int(tconf.get("verbose_every", 100))
    val_set, val_args = create_val_dataset(conf)
    val_every = int(tconf.get("val_every", 0)) if val_set is not None else 0   # the reference's VERBOSE_RATE

    def save():
        if rank == 0:
            torch.save(trainer.state_dict(), os.path.join(checkpoint_dir(conf), f"checkpoint_iter{trainer.i:08d}.pt"))

    # epoch e visits every stage's dataset permuted with seed 2024 + e (data_sampler.py:28-31), for a
    # fresh run and a resumed one alike, so resuming at iteration i continues exactly the order the
    # uninterrupted run would have seen (the reference permutes a fresh run with 2204 instead,
    # images_pair_restoration_dataset.py:41, which makes its resume skip a different order).  An epoch
    # runs the stages in order (the reference's itertools.chain of its loaders, :185); iteration i of
    # the epoch lies in the first stage whose cumulative step count exceeds it.
    epoch, done_in_epoch = divmod(trainer.i, spe)
    start_i, saved_at = trainer.i, None
    while trainer.i < total:
        for st in stages:
            if trainer.i >= total:
                break
            if done_in_epoch >= st.steps:
                done_in_epoch -= st.steps
                continue
            st.sampler.set_epoch_and_current_sample(epoch, done_in_epoch * st.batch_size * world - 1)
            stepped = False
            for noisy, clean in st.loader:
                if trainer.i >= total:
                    break
                loss = trainer.step(noisy, clean, channels_first=getattr(st.loader, "channels_first", False))
                stepped = True
                if trainer.i % verbose == 0:
                    psnr_tr, mse_tr = trainer.train_metrics() if trainer.track_metrics else (float("nan"),) * 2
                    trainer.train_history.append((trainer.i, psnr_tr, mse_tr))
                    if rank == 0:
                        LOG.info("iter=%d loss=%.6f lr=%.3e psnr=%.4f mse=%.6e", trainer.i, loss,
                                 trainer.optimizer.param_groups[0]["lr"], psnr_tr, mse_tr)
                if trainer.i % every == 0:
                    save()
                    saved_at = trainer.i
                if val_every and trainer.i % val_every == 0:
                    psnr = val_check(val_set, val_args)(trainer.model, val_set, device=device, **val_args)
                    trainer.val_history.append((trainer.i, psnr))
                    if rank == 0:
                        LOG.info("FINISH VAL EPOCH %d - iter=%d - psnr_testing=%.4f", epoch, trainer.i, psnr)
            if not stepped and trainer.i < total:
                raise RuntimeError(f"epoch {epoch} stage {st.index} yielded no batch (dataset {len(st.dataset)}, "
                                   f"batch {st.batch_size}, {world} ranks, drop_last {st.drop_last})")
            done_in_epoch = 0
        epoch, done_in_epoch = epoch + 1, 0
    if trainer.i > start_i and saved_at != trainer.i:     # the final state is always on disk
        save()
    return trainer


def log_files_dir(conf: dict) -> str:
    return os.path.join(conf["path"]["root_dir"], "experiments", conf["name"], "log_files")


def plumbing(conf: dict) -> dict:
    """The reference's run_train.py main (:38-121) as it stands, for config C1 on a host without a GPU:
    find the latest checkpoint of the experiment (only its path: nothing is unpickled), create the
    checkpoint and log-file folders of a fresh run, log the configuration to
    experiments/<name>/log_files/run_train_<name>.log, and build the training dataset, the resumable
    sampler and the dataloader.  Like the reference it builds no model; returns the pieces."""
    ckpt = latest_checkpoint(conf)
    if ckpt:
        conf["path"]["latest_checkpoint_path"] = ckpt
    else:
        os.makedirs(checkpoint_dir(conf), exist_ok=True)
        conf["path"]["checkpoints_folder"] = checkpoint_dir(conf)
        os.makedirs(log_files_dir(conf), exist_ok=True)
        conf["path"]["log_files_folder"] = log_files_dir(conf)
    logger = logging.getLogger(conf["name"])
    logger.setLevel(logging.INFO)
    log_dir = conf["path"].get("log_files_folder") or log_files_dir(conf)
    os.makedirs(log_dir, exist_ok=True)
    fh = logging.FileHandler(os.path.join(log_dir, f"run_train_{conf['name']}.log"))
    fh.setFormatter(logging.Formatter("%(asctime)s %(levelname)s: %(message)s"))
    logger.addHandler(fh)
    try:
        logger.info("environ_conf=%s", json.dumps(conf, indent=1, default=str))
        stages = build_train_stages(conf)
        for st in stages:
            logger.info("train dataset: %d samples", len(st.dataset))
    finally:
        logger.removeHandler(fh)
        fh.close()
    st = stages[0]
    return {"latest_checkpoint_path": ckpt, "dataset": st.dataset, "sampler": st.sampler, "dataloader": st.loader,
            "stages": stages}


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("-yaml_path", type=str, required=True, help="Path to option YAML file.")
    ap.add_argument("-max_iters", type=int, default=None)
    ap.add_argument("-plumbing_only", action="store_true",
                    help="the reference run_train.py's steps only (no model); the default without a GPU")
    args = ap.parse_args(argv)
    miopen_training_defaults()
    conf = parse_options(args.yaml_path)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s: %(message)s")
    if args.plumbing_only or not torch.cuda.is_available():
        # config C1 (PyTorch-CPU plumbing): the reference's script stops before any model;
        # the HIP model itself needs an MI355X
        parts = plumbing(conf)
        LOG.info("plumbing only (%s): %d training samples, latest checkpoint %s",
                 "no GPU" if not torch.cuda.is_available() else "-plumbing_only", len(parts["dataset"]),
                 parts["latest_checkpoint_path"])
        return None
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1 and not torch.distributed.is_initialized():
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        torch.distributed.init_process_group(backend)
    run(conf, max_iters=args.max_iters)
