"""Restore image files with a trained model (irdu_amd.restore; single process, one GPU).

    python restore.py -yaml_path CONF.yaml --ckpt CHECKPOINT.pt --input FILE_OR_DIR --output DIR \\
           [--sigma S --seed N] [--tile T --halo H --factor F]

The model is ``training.build_model(conf["model"])``; the checkpoint is the training loop's dict (its
"model" entry).  Without --ckpt the initial weights run, and the tool says so.  Images of any size are read
and written with PIL.  With --sigma each input is taken as clean: N(0, sigma/255) noise is drawn on the host
from one RandomState(seed) stream in file order (as ``irdu_amd.evaluate`` and ``training.validate`` do), the
noisy image is restored and its PSNR against the input printed, with the mean at the end.  Without --sigma
the input is restored as it is.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

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


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-yaml_path", type=str, required=True, help="option YAML file (its model: section is used)")
    ap.add_argument("--ckpt", type=str, default=None, help="training checkpoint (dict with a 'model' entry)")
    ap.add_argument("--input", type=str, required=True, help="an image file, or a directory of them")
    ap.add_argument("--output", type=str, required=True, help="directory for the restored images (PNG)")
    ap.add_argument("--sigma", type=float, default=None, help="treat inputs as clean: add this noise, report PSNR")
    ap.add_argument("--seed", type=int, default=2204)
    ap.add_argument("--tile", type=int, default=None)
    ap.add_argument("--halo", type=int, default=None)
    ap.add_argument("--factor", type=int, default=16)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from PIL import Image
    import irdu_amd
    from irdu_amd import restore, training

    files = input_files(args.input)
    conf = training.parse_options(args.yaml_path)
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
    psnrs = []
    for path in files:
        img = np.array(Image.open(path))
        if img.dtype != np.uint8:
            raise SystemExit(f"{path}: only 8-bit images are supported (got {img.dtype})")
        gray = img.ndim == 2
        if gray:
            img = img[:, :, None]
        out_path = os.path.join(args.output, os.path.splitext(os.path.basename(path))[0] + ".png")
        if args.sigma is None:
            out = irdu_amd.restore_image(model, img, factor=args.factor, tile=tile, halo=halo)
            print(f"{path} -> {out_path}  {img.shape[0]}x{img.shape[1]}x{img.shape[2]}")
        else:
            noisy = img.astype(np.float32) / 255.0
            noisy += rs.normal(0, args.sigma / 255.0, noisy.shape)
            out = irdu_amd.restore_image(model, noisy, factor=args.factor, tile=tile, halo=halo)
            if out.shape != img.shape:
                raise SystemExit(f"{path}: the model returns {out.shape[2]} channels for {img.shape[2]}; no PSNR")
            psnrs.append(irdu_amd.psnr_u8(out, img))
            print(f"{path} -> {out_path}  sigma {args.sigma:g}  PSNR {psnrs[-1]:.4f} dB")
        Image.fromarray(out[:, :, 0] if out.shape[2] == 1 else out).save(out_path)
    if psnrs:
        print(f"mean PSNR over {len(psnrs)} image(s): {float(np.mean(psnrs)):.4f} dB")


if __name__ == "__main__":
    main()
