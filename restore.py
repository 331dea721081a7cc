"""Restore image files with a trained model (irdu_amd.restore; single process, one GPU).

    python restore.py -yaml_path CONF.yaml --ckpt CHECKPOINT.pt --input FILE_OR_DIR --output DIR \\
           [--sigma S --seed N [--ssim] [--y-channel] | --reference DIR [--ssim] [--y-channel]
            | --scale S [--shave N] [--ssim] [--y-channel] | --upscale S
            | --jpeg-quality Q [--jpeg-subsampling 444|420] [--psnrb] [--ssim] [--y-channel]
            | --bayer PATTERN [--demosaic-fill FILL] [--shave N] [--ssim] [--y-channel]
              [--raw-noise SHOT,READ [--raw-bits N] [--raw-no-clip] [--raw-seed N]]
            | --raw PATTERN [--demosaic-fill FILL]
            | --blur SPEC [--blur-boundary B] [--blur-noise S] [--shave N] [--ssim] [--y-channel]
            | --inpaint-keep F [--mask-seed N] [--ssim] [--y-channel]]
           [--mask MASK_DIR [--mask-white-missing] [--reference DIR]]
           [--mask-fill zero|conv --mask-fill-side N --mask-fill-sigma S --mask-fill-passes P --no-keep-known]
           [--tile T --halo H --factor F] [--batch-images]
           [--self-ensemble | --ensemble-modes 0,1,4,5]

The model is ``training.build_model(conf["model"])``; the checkpoint is the training loop's dict (its
"model" entry).  Without --ckpt the initial weights run, and the tool says so.  Images of any size are read
and written with PIL.  With --sigma each input is taken as clean: N(0, sigma/255) noise is drawn on the host
from one RandomState(seed) stream in file order (as ``irdu_amd.evaluate`` and ``training.validate`` do), the
noisy image is restored and its PSNR against the input printed, with the mean at the end.  Without --sigma
the input is restored as it is.  With --batch-images all inputs are read first and restored by
``irdu_amd.restore_images``, windows of different files sharing the model's batches (files of one mode, all
RGB or all grey); the noise is still drawn in file order, and the lines printed and the files written are
the same.  With --self-ensemble every window is restored under all 8 flips and quarter turns and the results,
turned back, are averaged (``ensemble=8``; about 8 times the work); --ensemble-modes takes a subset of the modes
0..7 (m = 2k + f: k quarter turns counter-clockwise, then an upside-down flip if f), ascending and separated by
commas.  Both work with --batch-images; the lines printed and the files written keep their formats.  With --ssim
(with --sigma or --reference) each line also carries the SSIM of the restored image against the input, or the
reference (``irdu_amd.ssim_u8``: 11 x 11 Gaussian window, both sides at least 11 pixels) and the mean SSIM follows
the mean PSNR.  With --reference DIR (not with --sigma) the inputs are degraded pictures that have a ground truth:
each is restored as it is and scored against the file of the same stem in DIR, which must have the input's size
and channels; PSNR per file and the mean are printed as with --sigma.  A reference that is missing, ambiguous or of
another size is reported before anything runs.  It works with --batch-images and the ensemble options.  With
--y-channel (with --sigma or --reference; RGB files and a 3-channel model) the scores are taken on the Y channel of
YCbCr, as the tables of deraining, deblurring and super-resolution papers are: ITU-R BT.601 luma in [16, 235], not
rounded (MATLAB's rgb2ycbcr, BasicSR's test_y_channel; ``irdu_amd.psnr_y_u8`` / ``ssim_y_u8``).  The lines then read
PSNR-Y and SSIM-Y in place of PSNR and SSIM; the files written are the same.
With --scale S (2..8; not with --sigma or --reference) the inputs are clean high-resolution files and the bicubic
super-resolution protocol runs on each: it is cropped at the top left to multiples of S, degraded on the GPU by the
exact antialiased bicubic down and the bicubic back up (``irdu_amd.bicubic_degrade_u8``), restored, and scored against
the cropped input after --shave N border pixels (default S) are cut from both; the restored picture is written at the
cropped size.  --ssim and --y-channel apply as above (the tables print PSNR-Y / SSIM-Y).  With --upscale S the inputs
are low-resolution files: each is brought to S times its size by the bicubic (``irdu_amd.bicubic_up_u8``), restored
and written at that size; nothing is scored.  Both work with --batch-images and the ensemble options.
With --jpeg-quality Q (1..100; not with the other scored modes) the inputs are clean files and JPEG compression-artifact
removal runs on each: it goes through the JPEG round trip at quality Q on the GPU (``irdu_amd.jpeg_degrade_u8``: what
decoding its JPEG gives, Pillow's bytes, no file is written), the degraded picture is restored and scored against the
input.  --jpeg-subsampling 444 (default) or 420 chooses the chroma subsampling of RGB files.  With --psnrb (with
--jpeg-quality or --reference; both sides at least 16 pixels) each line also carries PSNR-B, the PSNR with the
blocking effect factor of the restored picture (``irdu_amd.psnrb_u8``), and its mean follows the others; it is always
taken on all channels, also with --y-channel.
With --bayer PATTERN (rggb, grbg, gbrg or bggr; not with the other scored modes) the inputs are clean RGB files and the
demosaicking protocol runs on each: it is sampled through the Bayer colour filter array and its missing channels are
filled on the GPU (``irdu_amd.demosaic_u8``; --demosaic-fill zero, bilinear or malvar, the default), the filled picture
is restored and scored against the input after --shave N border pixels (default 0) are cut from both.  The PSNR over
the three channels is the CPSNR of the demosaicking tables; --ssim and --y-channel apply as above.  With --raw-noise
SHOT,READ beside --bayer the protocol is joint denoising and demosaicking (``irdu_amd.evaluate_jdd``): sensor noise of
variance SHOT x + (READ / 255)^2 -- SHOT a gain of 0..1, READ in 8-bit levels -- is put on the mosaic, which is clipped
to [0, 1] (unless --raw-no-clip), quantised to --raw-bits N bits (8..16, default 16) and only then filled
(``irdu_amd.raw_noise_demosaic_u8``); the model's input is that float32 picture.  File i has sample id i under
--raw-seed N (default 2204), so its noise does not depend on the other files.  With --raw PATTERN
the inputs are 1-channel mosaic files as a sensor gives them: each is filled to RGB the same way, restored and written
as RGB; nothing is scored.  Both need a 3-channel model and work with --batch-images and the ensemble options.
With --blur SPEC (gaussian:SIDE:SIGMA, box:SIDE, motion:LENGTH:ANGLE or file:PATH.npy; not with the other scored modes)
the inputs are clean files and the deblurring protocol runs on each: it is convolved with the kernel on the GPU in exact
integers (``irdu_amd.blur_u8``; --blur-boundary wrap, the default and the circular convolution of the deblurring tables,
replicate or reflect), with --blur-noise S noise of N(0, S/255) is added to the blurred picture (drawn on the host from
RandomState(--seed) in file order; the model's input is then float32 and is not quantised), the result is restored and
scored against the input after --shave N border pixels (default 0) are cut from both.  --ssim and --y-channel apply as
above; it works with --batch-images and the ensemble options.
With --inpaint-keep F (0..1; not with the other scored modes) the inputs are clean files and the inpainting protocol
runs on each: a pixel is known with probability F -- file i has sample id i under --mask-seed N (default 2204), so its
mask does not depend on the other files -- the missing pixels are filled on the GPU (``irdu_amd.mask_fill_u8``:
--mask-fill conv, the default, a normalised convolution of the known pixels under a flat --mask-fill-side N table (odd,
at most 15, default 7) or a Gaussian of --mask-fill-sigma S, or zero; --mask-fill-passes P repeats the fill, each pass
taking the filled pixels as known), the filled picture is restored, the known pixels are put back (unless
--no-keep-known) and the result is scored against the input; each line also carries PSNR-missing, the PSNR over the
missing pixels alone.  With --mask MASK_DIR the inputs are pictures with holes: the 1-channel file of the same stem and
size in MASK_DIR says which pixels are known -- nonzero, or zero with --mask-white-missing -- the others are filled the
same way, the picture is restored, the known pixels are put back and the result is written; with --reference DIR it is
also scored.  Both work with --batch-images and the ensemble options.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PATTERNS = ("rggb", "grbg", "gbrg", "bggr")     # irdu_amd.kernels.DEMOSAIC_PATTERNS
FILLS = ("zero", "bilinear", "malvar")          # irdu_amd.kernels.DEMOSAIC_FILLS
BOUNDARIES = ("wrap", "replicate", "reflect")   # irdu_amd.kernels.BLUR_BOUNDARIES
MASK_FILLS = ("zero", "conv")                   # irdu_amd.kernels.MASK_FILLS
EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".ppm", ".pgm", ".webp")


def input_files(path: str):
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(EXTENSIONS))
        if not files:
            raise SystemExit(f"no image files in {path}")
        return files
    if not os.path.isfile(path):
        raise SystemExit(f"{path}: no such file or directory")
    return [path]


def reference_files(files, ref_dir: str):
    """The reference of each input file: the one image file of ``ref_dir`` with the input's stem (any of
    EXTENSIONS).  SystemExit naming the input where there is none, or more than one."""
    if not os.path.isdir(ref_dir):
        raise SystemExit(f"--reference: {ref_dir} is not a directory")
    by_stem = {}
    for f in sorted(os.listdir(ref_dir)):
        if f.lower().endswith(EXTENSIONS):
            by_stem.setdefault(os.path.splitext(f)[0], []).append(os.path.join(ref_dir, f))
    refs = []
    for path in files:
        stem = os.path.splitext(os.path.basename(path))[0]
        found = by_stem.get(stem, [])
        if len(found) != 1:
            raise SystemExit(f"--reference: {path} has {'no' if not found else len(found)} reference(s) named "
                             f"{stem}.* in {ref_dir}" + (f" ({', '.join(found)})" if found else ""))
        refs.append(found[0])
    return refs


def check_references(files, refs) -> None:
    """SystemExit for the first reference whose size or channels differ from its input's (headers only)."""
    from PIL import Image
    for path, ref in zip(files, refs):
        with Image.open(path) as a, Image.open(ref) as b:
            if a.size != b.size or len(a.getbands()) != len(b.getbands()):
                raise SystemExit(f"--reference: {ref} is {b.size[1]}x{b.size[0]}x{len(b.getbands())}, its input {path} "
                                 f"is {a.size[1]}x{a.size[0]}x{len(a.getbands())}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-yaml_path", type=str, required=True, help="option YAML file (its model: section is used)")
    ap.add_argument("--ckpt", type=str, default=None, help="training checkpoint (dict with a 'model' entry)")
    ap.add_argument("--input", type=str, required=True, help="an image file, or a directory of them")
    ap.add_argument("--output", type=str, required=True, help="directory for the restored images (PNG)")
    scored = ap.add_mutually_exclusive_group()
    scored.add_argument("--sigma", type=float, default=None, help="treat inputs as clean: add this noise, report PSNR")
    scored.add_argument("--reference", type=str, default=None, metavar="DIR",
                        help="inputs are degraded: restore them as they are, report PSNR against the file of the same "
                             "stem in DIR")
    scored.add_argument("--scale", type=int, default=None, metavar="S",
                        help="inputs are clean: mod-crop, degrade by the bicubic at scale S (2..8), restore, report PSNR "
                             "against the cropped input")
    scored.add_argument("--upscale", type=int, default=None, metavar="S",
                        help="inputs are low-resolution: bring each to S times its size with the bicubic, restore, write")
    scored.add_argument("--jpeg-quality", type=int, default=None, metavar="Q",
                        help="inputs are clean: JPEG round trip at quality Q (1..100) on the GPU, restore, report PSNR "
                             "against the input")
    scored.add_argument("--bayer", type=str, default=None, metavar="PATTERN", choices=PATTERNS,
                        help="inputs are clean RGB: Bayer mosaic with this pattern (rggb, grbg, gbrg, bggr) and fill on the "
                             "GPU, restore, report PSNR (CPSNR) against the input")
    scored.add_argument("--raw", type=str, default=None, metavar="PATTERN", choices=PATTERNS,
                        help="inputs are 1-channel Bayer mosaics with this pattern: fill to RGB, restore, write")
    scored.add_argument("--blur", type=str, default=None, metavar="SPEC",
                        help="inputs are clean: blur with this kernel (gaussian:SIDE:SIGMA, box:SIDE, motion:LENGTH:ANGLE, "
                             "file:PATH.npy) on the GPU, restore, report PSNR against the input")
    scored.add_argument("--inpaint-keep", type=float, default=None, metavar="F",
                        help="inputs are clean: keep each pixel with probability F (0..1), fill the others on the GPU, "
                             "restore, report PSNR against the input")
    ap.add_argument("--mask", type=str, default=None, metavar="MASK_DIR",
                    help="inputs have holes: the 1-channel file of the same stem in MASK_DIR is nonzero where a pixel is "
                         "known; fill the others, restore, put the known pixels back, write")
    ap.add_argument("--mask-white-missing", action="store_true", help="with --mask: nonzero means missing")
    ap.add_argument("--mask-fill", type=str, default=None, choices=MASK_FILLS,
                    help="with --inpaint-keep or --mask: how the missing pixels are filled before the model (default conv)")
    ap.add_argument("--mask-fill-side", type=int, default=None, metavar="N",
                    help="with --mask-fill conv: the side of the weight table, odd, 1..15 (default 7)")
    ap.add_argument("--mask-fill-sigma", type=float, default=None, metavar="S",
                    help="with --mask-fill conv: a Gaussian table of this sigma (default: a flat table)")
    ap.add_argument("--mask-fill-passes", type=int, default=None, metavar="P",
                    help="with --inpaint-keep or --mask: fill P times, each pass taking the filled pixels as known "
                         "(default 1)")
    ap.add_argument("--mask-seed", type=int, default=None, metavar="N", help="with --inpaint-keep: the mask seed (default 2204)")
    ap.add_argument("--no-keep-known", action="store_true",
                    help="with --inpaint-keep or --mask: do not put the known pixels back into the restored picture")
    ap.add_argument("--blur-boundary", type=str, default=None, choices=BOUNDARIES,
                    help="with --blur: how the picture continues beyond its sides (default wrap)")
    ap.add_argument("--blur-noise", type=float, default=None, metavar="S",
                    help="with --blur: add N(0, S/255) noise to the blurred picture (default 0: none)")
    ap.add_argument("--demosaic-fill", type=str, default=None, choices=FILLS,
                    help="with --bayer or --raw: how the missing channels are filled before the model (default malvar)")
    ap.add_argument("--raw-noise", type=str, default=None, metavar="SHOT,READ",
                    help="with --bayer: joint denoising and demosaicking -- noise of variance SHOT x + (READ / 255)^2 on the "
                         "mosaic, before the fill (SHOT 0..1, READ in 8-bit levels 0..255)")
    ap.add_argument("--raw-bits", type=int, default=None, metavar="N",
                    help="with --raw-noise: the depth of the raw samples, 8..16 (default 16)")
    ap.add_argument("--raw-no-clip", action="store_true", help="with --raw-noise: do not clip the noisy mosaic to [0, 1]")
    ap.add_argument("--raw-seed", type=int, default=None, metavar="N", help="with --raw-noise: the noise seed (default 2204)")
    ap.add_argument("--jpeg-subsampling", type=str, default=None, choices=("444", "420"),
                    help="with --jpeg-quality: the chroma subsampling of RGB files (default 444)")
    ap.add_argument("--psnrb", action="store_true",
                    help="with --jpeg-quality or --reference: report PSNR-B beside the PSNR")
    ap.add_argument("--shave", type=int, default=None, metavar="N",
                    help="with --scale, --bayer or --blur: border pixels cut from both pictures before scoring (default: S "
                         "with --scale, 0 with --bayer and --blur)")
    ap.add_argument("--seed", type=int, default=2204)
    ap.add_argument("--ssim", action="store_true",
                    help="with --sigma, --reference, --scale, --jpeg-quality, --bayer or --blur: report the SSIM beside the "
                         "PSNR")
    ap.add_argument("--y-channel", action="store_true",
                    help="with --sigma, --reference, --scale, --jpeg-quality, --bayer or --blur: score on the Y channel of "
                         "YCbCr (BT.601 luma of RGB images): PSNR-Y, and with --ssim SSIM-Y, in place of the RGB values")
    ap.add_argument("--tile", type=int, default=None)
    ap.add_argument("--halo", type=int, default=None)
    ap.add_argument("--factor", type=int, default=16)
    ap.add_argument("--batch-images", action="store_true",
                    help="read all inputs first and restore them in shared window batches (restore_images)")
    group = ap.add_mutually_exclusive_group()
    group.add_argument("--self-ensemble", action="store_true",
                       help="average the restorations under all 8 flips and quarter turns (ensemble=8)")
    group.add_argument("--ensemble-modes", type=str, default=None, metavar="M,M,...",
                       help="average over these modes of 0..7 only, ascending (e.g. 0,1,4,5)")
    args = ap.parse_args(argv)
    args.scored = args.sigma is not None or args.reference is not None or args.scale is not None \
        or args.jpeg_quality is not None or args.bayer is not None or args.blur is not None \
        or args.inpaint_keep is not None
    if args.ssim and not args.scored:
        ap.error("--ssim needs --sigma, --reference, --scale, --jpeg-quality, --bayer or --blur: there is nothing to compare a restored image with otherwise")
    if args.y_channel and not args.scored:
        ap.error("--y-channel needs --sigma, --reference, --scale, --jpeg-quality, --bayer or --blur: there is nothing to compare a restored image with "
                 "otherwise")
    if args.jpeg_quality is not None and not 1 <= args.jpeg_quality <= 100:
        ap.error(f"--jpeg-quality: the quality is an integer of 1..100, got {args.jpeg_quality}")
    if args.jpeg_subsampling is not None and args.jpeg_quality is None:
        ap.error("--jpeg-subsampling needs --jpeg-quality")
    args.jpeg_subsampling = 2 if args.jpeg_subsampling == "420" else 0
    if args.psnrb and args.jpeg_quality is None and args.reference is None:
        ap.error("--psnrb needs --jpeg-quality or --reference")
    for flag, value in (("--scale", args.scale), ("--upscale", args.upscale)):
        if value is not None and not 2 <= value <= 8:
            ap.error(f"{flag}: the scale is an integer of 2..8, got {value}")
    if args.demosaic_fill is not None and args.bayer is None and args.raw is None:
        ap.error("--demosaic-fill needs --bayer or --raw")
    args.demosaic_fill = args.demosaic_fill or "malvar"
    if args.raw_noise is not None:
        if args.bayer is None:
            ap.error("--raw-noise needs --bayer")
        try:
            shot, read = (float(v) for v in args.raw_noise.split(","))
        except ValueError:
            ap.error(f"--raw-noise: expected SHOT,READ, two numbers separated by a comma, got {args.raw_noise!r}")
        if not (0 <= shot <= 1 and 0 <= read <= 255):
            ap.error(f"--raw-noise: SHOT is a gain of 0..1 and READ a level of 0..255, got {args.raw_noise!r}")
        args.raw_noise = (shot, read)
    for flag, value in (("--raw-bits", args.raw_bits), ("--raw-no-clip", args.raw_no_clip or None),
                        ("--raw-seed", args.raw_seed)):
        if value is not None and args.raw_noise is None:
            ap.error(f"{flag} needs --raw-noise")
    if args.raw_bits is not None and not 8 <= args.raw_bits <= 16:
        ap.error(f"--raw-bits: the depth is an integer of 8..16, got {args.raw_bits}")
    if args.raw_seed is not None and not 0 <= args.raw_seed < 2 ** 64:
        ap.error(f"--raw-seed: the seed is an integer of 0..2^64 - 1, got {args.raw_seed}")
    args.raw_bits = 16 if args.raw_bits is None else args.raw_bits
    args.raw_seed = 2204 if args.raw_seed is None else args.raw_seed
    for flag, value in (("--blur-boundary", args.blur_boundary), ("--blur-noise", args.blur_noise)):
        if value is not None and args.blur is None:
            ap.error(f"{flag} needs --blur")
    if args.blur_noise is not None and not 0 <= args.blur_noise < float("inf"):
        ap.error(f"--blur-noise: the noise level is a non-negative number, got {args.blur_noise}")
    args.blur_boundary, args.blur_noise = args.blur_boundary or "wrap", args.blur_noise or 0.0
    if args.shave is not None and ((args.scale is None and args.bayer is None and args.blur is None) or args.shave < 0):
        ap.error("--shave is a non-negative number of pixels and needs --scale, --bayer or --blur")
    if args.scale is not None and args.shave is None:
        args.shave = args.scale
    if (args.bayer is not None or args.blur is not None) and args.shave is None:
        args.shave = 0
    if args.inpaint_keep is not None and not 0 <= args.inpaint_keep <= 1:
        ap.error(f"--inpaint-keep: the known share is a number of 0..1, got {args.inpaint_keep}")
    if args.mask is not None:
        for flag, value in (("--sigma", args.sigma), ("--scale", args.scale), ("--upscale", args.upscale),
                            ("--jpeg-quality", args.jpeg_quality), ("--bayer", args.bayer), ("--raw", args.raw),
                            ("--blur", args.blur), ("--inpaint-keep", args.inpaint_keep)):
            if value is not None:
                ap.error(f"--mask: not allowed with {flag}")
    args.inpaint = args.inpaint_keep is not None or args.mask is not None
    for flag, value in (("--mask-fill", args.mask_fill), ("--mask-fill-side", args.mask_fill_side),
                        ("--mask-fill-sigma", args.mask_fill_sigma), ("--mask-fill-passes", args.mask_fill_passes),
                        ("--no-keep-known", args.no_keep_known or None)):
        if value is not None and not args.inpaint:
            ap.error(f"{flag} needs --inpaint-keep or --mask")
    if args.mask_white_missing and args.mask is None:
        ap.error("--mask-white-missing needs --mask")
    if args.mask_seed is not None and args.inpaint_keep is None:
        ap.error("--mask-seed needs --inpaint-keep")
    if args.mask_seed is not None and not 0 <= args.mask_seed < 2 ** 64:
        ap.error(f"--mask-seed: the seed is an integer of 0..2^64 - 1, got {args.mask_seed}")
    args.mask_fill = args.mask_fill or "conv"
    for flag, value in (("--mask-fill-side", args.mask_fill_side), ("--mask-fill-sigma", args.mask_fill_sigma)):
        if value is not None and args.mask_fill != "conv":
            ap.error(f"{flag} needs --mask-fill conv")
    if args.mask_fill_side is not None and not (1 <= args.mask_fill_side <= 15 and args.mask_fill_side % 2 == 1):
        ap.error(f"--mask-fill-side: the side is an odd integer of 1..15, got {args.mask_fill_side}")
    if args.mask_fill_sigma is not None and not 0 < args.mask_fill_sigma < float("inf"):
        ap.error(f"--mask-fill-sigma: sigma is a positive number, got {args.mask_fill_sigma}")
    if args.mask_fill_passes is not None and args.mask_fill_passes < 1:
        ap.error(f"--mask-fill-passes: the number of passes is a positive integer, got {args.mask_fill_passes}")
    args.mask_fill_side = 7 if args.mask_fill_side is None else args.mask_fill_side
    args.mask_fill_passes = 1 if args.mask_fill_passes is None else args.mask_fill_passes
    args.mask_seed = 2204 if args.mask_seed is None else args.mask_seed
    args.ensemble = 8 if args.self_ensemble else 1
    if args.ensemble_modes is not None:
        try:
            args.ensemble = tuple(int(m) for m in args.ensemble_modes.split(","))
        except ValueError:
            ap.error(f"--ensemble-modes: expected integers separated by commas, got {args.ensemble_modes!r}")
    return args


def main(argv=None) -> None:
    args = parse_args(argv)
    ensemble = args.ensemble

    import numpy as np
    import torch
    from PIL import Image
    import irdu_amd
    from irdu_amd import restore, training

    try:
        restore._ensemble_modes("--ensemble-modes", ensemble)
    except ValueError as e:
        raise SystemExit(str(e))
    files = input_files(args.input)
    refs = {}
    if args.reference is not None:
        found = reference_files(files, args.reference)
        check_references(files, found)
        refs = dict(zip(files, found))
    masks = {}
    if args.mask is not None:
        if not os.path.isdir(args.mask):
            raise SystemExit(f"--mask: {args.mask} is not a directory")
        try:
            masks = dict(zip(files, reference_files(files, args.mask)))
        except SystemExit as e:
            raise SystemExit(str(e).replace("--reference", "--mask").replace("reference(s)", "mask(s)"))
        for path, mask_path in masks.items():
            with Image.open(path) as a, Image.open(mask_path) as b:
                if a.size != b.size or len(b.getbands()) != 1:
                    raise SystemExit(f"--mask: {mask_path} is {b.size[1]}x{b.size[0]}x{len(b.getbands())}, its input {path} "
                                     f"is {a.size[1]}x{a.size[0]}; a mask is a 1-channel file of the input's size")
    conf = training.parse_options(args.yaml_path)

    def need_three_channels(flag, model_needs, bands, files_need):
        """Before anything runs: SystemExit for a model of the YAML that is not 3-channel, or a file without ``bands``."""
        model_args = conf.get("model", {}).get("args", {})
        for key in ("n_channels_in", "n_channels_out"):
            if model_args.get(key) is not None and int(model_args[key]) != 3:
                raise SystemExit(f"{flag}: the model of {args.yaml_path} has {key} {model_args[key]}; {model_needs}")
        for path in files:
            with Image.open(path) as im:
                if len(im.getbands()) != bands:
                    raise SystemExit(f"{flag}: {path} has {len(im.getbands())} channel(s) ({im.mode}); {files_need}")

    if args.y_channel:
        need_three_channels("--y-channel", "the Y channel is defined for 3-channel (RGB) models", 3,
                            "the Y channel is defined for 3-channel (RGB) images")
    if args.bayer is not None:
        need_three_channels("--bayer", "a demosaicked picture has 3 channels (R, G, B)", 3,
                            "the protocol takes clean 3-channel (RGB) images")
    if args.raw is not None:
        need_three_channels("--raw", "a demosaicked picture has 3 channels (R, G, B)", 1, "a raw mosaic is a 1-channel image")
    # the degrade-from-clean protocol asked for, if any: read, input_of and finish take its crop, degradation, shave
    # and label from the record (parse_args has checked the values)
    try:
        protocol = (restore._sr_protocol("--scale", args.scale, args.shave) if args.scale is not None else
                    restore._car_protocol("--jpeg-quality", args.jpeg_quality, args.jpeg_subsampling)
                    if args.jpeg_quality is not None else
                    restore._jdd_protocol("--bayer", args.bayer, args.demosaic_fill, args.raw_noise[0], args.raw_noise[1],
                                          args.raw_bits, not args.raw_no_clip, args.raw_seed, args.shave)
                    if args.raw_noise is not None else
                    restore._demosaic_protocol("--bayer", args.bayer, args.demosaic_fill, args.shave)
                    if args.bayer is not None else
                    restore._deblur_protocol("--blur", args.blur, args.blur_boundary, args.blur_noise, args.seed,
                                             args.shave)
                    if args.blur is not None else None)
    except ValueError as e:          # a kernel spec is only parsed here
        raise SystemExit(str(e))
    if not torch.cuda.is_available():
        raise SystemExit("restore.py needs a GPU: the HIP engine has no CPU path")
    irdu_amd.load_native()
    model = training.build_model(conf.get("model", {}))
    if args.ckpt:
        model.load_state_dict(torch.load(args.ckpt, map_location="cpu")["model"])
        print(f"weights: {args.ckpt}")
    else:
        print("weights: none given (--ckpt), running the model's initial weights")
    model = model.to("cuda").eval()
    tile = restore.TILE if args.tile is None else args.tile
    halo = restore.HALO if args.halo is None else args.halo
    os.makedirs(args.output, exist_ok=True)
    rs = np.random.RandomState(seed=args.seed)
    psnrs, ssims, psnrbs, missing = [], [], [], []
    psnr_of, ssim_of, tag = ((irdu_amd.psnr_y_u8, irdu_amd.ssim_y_u8, "-Y") if args.y_channel else
                             (irdu_amd.psnr_u8, irdu_amd.ssim_u8, ""))

    def decode(path):
        img = np.array(Image.open(path))
        if img.dtype != np.uint8:
            raise SystemExit(f"{path}: only 8-bit images are supported (got {img.dtype})")
        return img[:, :, None] if img.ndim == 2 else img

    def read(path):
        """The picture the model's input is made of and, when scoring without a reference, compared with."""
        img = decode(path)
        if protocol is not None:
            h, w = protocol.crop(img.shape[0], img.shape[1])
            if min(h, w) <= 2 * protocol.shave:
                raise SystemExit(f"{path}: nothing is left of {img.shape[0]}x{img.shape[1]} {protocol.left_after}")
            img = np.ascontiguousarray(img[:h, :w])
        elif args.upscale is not None:
            img = irdu_amd.bicubic_up_u8(img, args.upscale)
        elif args.raw is not None:
            img = irdu_amd.demosaic_u8(img, args.raw, args.demosaic_fill)
        return img

    known_of = {}       # inpainting: the 0 / 1 plane of the known pixels of each file
    mask_table = irdu_amd.kernels.mask_weights(args.mask_fill_side, args.mask_fill_sigma) if args.inpaint else None

    def input_of(img, path):
        if args.sigma is not None:
            return noisy_of(img)
        if args.inpaint:
            given = None
            if args.mask is not None:
                given = np.array(Image.open(masks[path]))
                given = (given == 0) if args.mask_white_missing else (given != 0)
            try:
                filled, known_of[path] = irdu_amd.mask_fill_u8(
                    img, mask=given, keep=args.inpaint_keep, fill=args.mask_fill, weights=mask_table,
                    seed=args.mask_seed, sample_id=files.index(path), passes=args.mask_fill_passes)
            except ValueError as e:
                raise SystemExit(f"{path}: {e}")
            return filled
        if protocol is None:
            return img
        try:
            return restore._resized_u8(protocol.who, img, protocol.degrade)
        except ValueError as e:
            raise SystemExit(f"{protocol.who}: {e}")

    def noisy_of(img):
        noisy = img.astype(np.float32) / 255.0
        noisy += rs.normal(0, args.sigma / 255.0, noisy.shape)
        return noisy

    def finish(path, img, out):
        out_path = os.path.join(args.output, os.path.splitext(os.path.basename(path))[0] + ".png")
        if path in known_of and not args.no_keep_known and out.shape == img.shape:
            out = np.where(known_of[path][:, :, None] != 0, img, out)
        if not args.scored:
            print(f"{path} -> {out_path}  {img.shape[0]}x{img.shape[1]}x{img.shape[2]}")
        else:
            if out.shape != img.shape:
                raise SystemExit(f"{path}: the model returns {out.shape[2]} channels for {img.shape[2]}; no PSNR")
            truth = img if args.reference is None else decode(refs[path])
            if truth.shape != out.shape:
                raise SystemExit(f"--reference: {refs[path]} decodes to {truth.shape}, the restored {path} is {out.shape}")
            scored = out
            if protocol is not None:
                scored, truth = np.ascontiguousarray(protocol.shaved(out)), np.ascontiguousarray(protocol.shaved(truth))
            try:
                psnrs.append(psnr_of(scored, truth))
            except ValueError as e:
                raise SystemExit(f"{path}: {e}")
            against = (protocol.label if protocol is not None else
                       f"inpaint keep {args.inpaint_keep:g} {args.mask_fill} seed {args.mask_seed}"
                       if args.inpaint_keep is not None else
                       f"sigma {args.sigma:g}" if args.reference is None else f"reference {refs[path]}")
            line = f"{path} -> {out_path}  {against}  PSNR{tag} {psnrs[-1]:.4f} dB"
            if args.ssim:
                try:
                    ssims.append(ssim_of(scored, truth))
                except ValueError as e:
                    raise SystemExit(f"{path}: {e}")
                line += f"  SSIM{tag} {ssims[-1]:.4f}"
            if path in known_of:
                missing.append(irdu_amd.psnr_missing_u8(scored, truth, known_of[path]))
                line += f"  PSNR-missing {missing[-1]:.4f} dB"
            if args.psnrb:
                try:
                    psnrbs.append(irdu_amd.psnrb_u8(scored, truth))
                except ValueError as e:
                    raise SystemExit(f"{path}: {e}")
                line += f"  PSNR-B {psnrbs[-1]:.4f} dB"
            print(line)
        Image.fromarray(out[:, :, 0] if out.shape[2] == 1 else out).save(out_path)

    if args.batch_images:
        imgs = [read(path) for path in files]
        inputs = [input_of(img, path) for img, path in zip(imgs, files)]               # draws in file order
        try:
            outs = irdu_amd.restore_images(model, inputs, factor=args.factor, tile=tile, halo=halo, ensemble=ensemble)
        except ValueError as e:
            raise SystemExit(f"--batch-images: {e}")
        for path, img, out in zip(files, imgs, outs):
            finish(path, img, out)
    else:
        for path in files:
            img = read(path)
            out = irdu_amd.restore_image(model, input_of(img, path), factor=args.factor,
                                         tile=tile, halo=halo, ensemble=ensemble)
            finish(path, img, out)
    if psnrs:
        print(f"mean PSNR{tag} over {len(psnrs)} image(s): {float(np.mean(psnrs)):.4f} dB")
    if ssims:
        print(f"mean SSIM{tag} over {len(ssims)} image(s): {float(np.mean(ssims)):.4f}")
    if missing:
        print(f"mean PSNR-missing over {len(missing)} image(s): {float(np.mean(missing)):.4f} dB")
    if psnrbs:
        print(f"mean PSNR-B over {len(psnrbs)} image(s): {float(np.mean(psnrbs)):.4f} dB")


if __name__ == "__main__":
    main()
