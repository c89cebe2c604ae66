"""`python -m hgr_net_amd.baseline.extract_features`: images -> the feature file `evaluate_dgp --features FILE.npz` reads
(`dgp_eval.load_features`: one [n_i, K] array per wnid), through the DGP baseline's ResNet on the device (`resnet.ResNetFeatures`).
Extraction and scoring can so run apart; `evaluate_dgp --cnn ... --image-dir ...` runs them in one go on the same code.

--cnn FILE.pth is a `make_resnet50_base().state_dict()` checkpoint as the reference's evaluate_imagenet.py loads it (`--version` for
another depth); `--cnn synthetic` is a seeded net (synth.resnet_state_dict).  --image-dir DIR holds one sub-folder per wnid.  Files
are decoded on the host (PIL) and transformed on the device by preprocess.BatchPreprocessor - Resize(short side = --image-size,
bicubic) + CenterCrop + Normalize with the ImageNet mean / std of train_resnet_fit.py:32-33.  The reference's own evaluation transform
lives in its `datasets/imagenet.py`, which is NOT part of its checkout: its resize and crop are unknown, and this transform is ours,
not a restatement.  --synthetic N generates the images instead (1 - 9 per class of a generated N-node graph's test split)."""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

IMAGE_EXT = (".jpg", ".jpeg", ".png", ".bmp", ".webp")
SYNTHETIC_SIZE = 64                      # edge of the generated images when --image-size is not given


class ImageRows:
    """The images of one class: `len()` and `batch(o, n)` -> fp32 device tensor [<= n, 3, R, R] of images o .. o + n - 1."""

    def __len__(self) -> int:
        raise NotImplementedError

    def batch(self, o: int, n: int, device) -> torch.Tensor:
        raise NotImplementedError


class FileRows(ImageRows):
    def __init__(self, paths: Sequence[str], pre):
        self.paths, self.pre = list(paths), pre

    def __len__(self) -> int:
        return len(self.paths)

    def batch(self, o: int, n: int, device) -> torch.Tensor:
        from PIL import Image
        return self.pre([np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p in self.paths[o:o + n]])


class TensorRows(ImageRows):
    def __init__(self, images: torch.Tensor):
        self.images = images

    def __len__(self) -> int:
        return self.images.shape[0]

    def batch(self, o: int, n: int, device) -> torch.Tensor:
        return self.images[o:o + n].to(device, non_blocking=True)


def image_dir_rows(root: str, size: int, device, wnids: Optional[Sequence[str]] = None) -> Dict[str, ImageRows]:
    """{wnid: FileRows} of `root`/<wnid>/*: every sub-folder (or those of `wnids` that exist), files in sorted order."""
    from ..preprocess import BatchPreprocessor
    from .resnet import IMAGENET_MEAN, IMAGENET_STD
    if not os.path.isdir(root):
        raise SystemExit(f"--image-dir {root}: not a directory")
    pre = BatchPreprocessor(size, device, mean=IMAGENET_MEAN, std=IMAGENET_STD)
    names = sorted(os.listdir(root)) if wnids is None else list(wnids)
    out: Dict[str, ImageRows] = {}
    for w in names:
        d = os.path.join(root, w)
        if os.path.isdir(d):
            files = sorted(f for f in os.listdir(d) if f.lower().endswith(IMAGE_EXT))
            if files:
                out[w] = FileRows([os.path.join(d, f) for f in files], pre)
    return out


def synthetic_rows(wnids: Sequence[str], seed: int, size: int, max_rows: int = 9) -> Dict[str, ImageRows]:
    from .. import synth
    counts = synth.randint(seed, "dgp.cnn.rows", len(wnids), 1, max_rows + 1)
    return {w: TensorRows(synth.images(int(counts[i]), size, seed=synth.fnv1a64(f"{seed}.{w}") % (1 << 31))) for i, w in enumerate(wnids)}


def load_cnn(spec: str, version: str = "resnet50", seed: int = 0, device="cuda:0"):
    """`ResNetFeatures` of the checkpoint `spec` (a base state_dict, as evaluate_imagenet.py:198-199 loads it) or of the seeded net."""
    from .. import synth
    from .resnet import ResNetFeatures, make_resnet_base
    net = make_resnet_base(version)
    if spec == "synthetic":
        if version not in synth.RESNET_LAYERS:
            raise SystemExit(f"--cnn synthetic: --version must be one of {sorted(synth.RESNET_LAYERS)}")
        sd = synth.resnet_state_dict(version, seed)
    else:
        if not os.path.isfile(spec):
            raise SystemExit(f"--cnn {spec}: no such file")
        sd = torch.load(spec, map_location="cpu")
    net.load_state_dict(sd)
    return ResNetFeatures(net.to(device))


def extract(cnn, rows: Dict[str, ImageRows], batch_size: int = 256, device="cuda:0") -> Dict[str, np.ndarray]:
    """{wnid: fp16 [n_i, K]}: every class through `cnn`, `batch_size` images at a time, one host read per class."""
    out = {}
    for w, r in rows.items():
        parts: List[torch.Tensor] = [cnn(r.batch(o, batch_size, device)).clone() for o in range(0, len(r), batch_size)]
        if parts:
            out[w] = torch.cat(parts).cpu().numpy()
    return out


def save_features(path, features: Dict[str, np.ndarray]) -> None:
    """The `--features` format: `np.savez(path, **{wnid: rows})`, every array a float [n_i, K] of one width."""
    widths = {np.asarray(a).shape[1] for a in features.values() if np.asarray(a).ndim == 2}
    if not features or len(widths) != 1 or any(np.asarray(a).ndim != 2 or np.asarray(a).dtype.kind != "f" for a in features.values()):
        raise ValueError("features must be a non-empty {wnid: float [n, K]} mapping of one width")
    with open(path, "wb") as f:                                         # a file object: np.savez appends no '.npz' to the name
        np.savez(f, **{w: np.ascontiguousarray(a) for w, a in features.items()})


def add_cnn_options(parser: argparse.ArgumentParser) -> None:
    """The image options, shared with `evaluate_dgp`."""
    parser.add_argument("--cnn", default=None, metavar="FILE.pth|synthetic",
                        help="ResNet base checkpoint (the reference's option), or 'synthetic' for a seeded net")
    parser.add_argument("--version", default="resnet50", choices=["resnet50", "resnet101", "resnet152"], help="depth of the --cnn checkpoint")
    parser.add_argument("--image-dir", default=None, metavar="DIR", help="one sub-folder of image files per wnid")
    parser.add_argument("--image-size", type=int, default=None, metavar="R",
                        help="images become R x R: short side resized to R (bicubic), centre crop, ImageNet mean / std. The reference's own "
                             "resize and crop (its datasets/imagenet.py) are not in its checkout and are not known; default 224 "
                             f"({SYNTHETIC_SIZE} for generated images)")


def check_cnn_args(args: argparse.Namespace, synthetic: bool) -> None:
    if args.image_size is not None and args.image_size < 32:
        raise SystemExit("--image-size must be at least 32")
    if args.cnn is None:
        if args.image_dir is not None:
            raise SystemExit("--image-dir needs --cnn FILE.pth")
        return
    if args.cnn == "synthetic" and not synthetic and args.image_dir is None:
        raise SystemExit("--cnn synthetic needs --synthetic N (generated images) or --image-dir DIR")
    if args.image_dir is None and not synthetic:
        raise SystemExit("--cnn needs images: --image-dir DIR (or --synthetic N)")
    if args.image_dir is not None and synthetic:
        raise SystemExit("--image-dir and --synthetic exclude each other")


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(prog="python -m hgr_net_amd.baseline.extract_features", description=__doc__.split("\n\n")[0])
    add_cnn_options(parser)
    parser.add_argument("--output", default=None, metavar="FILE.npz", help="the feature file to write")
    parser.add_argument("--synthetic", type=int, default=None, metavar="N", help="generated images for the test split of a generated N-node graph")
    parser.add_argument("--seed", type=int, default=0, help="seed of the --synthetic material and of --cnn synthetic")
    parser.add_argument("--batch-size", type=int, default=256)
    args = parser.parse_args(argv)
    if args.cnn is None:
        raise SystemExit("--cnn FILE.pth (or 'synthetic') is required")
    if args.output is None:
        raise SystemExit("--output FILE.npz is required")
    if args.batch_size < 1:
        raise SystemExit("--batch-size must be at least 1")
    check_cnn_args(args, args.synthetic is not None)
    return args


def main(argv=None) -> Dict[str, np.ndarray]:
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("extract_features needs the GPU: the product path has no CPU fallback")
    dev = "cuda:0"
    if args.synthetic is not None:
        from . import evaluate_dgp
        _, splits, _, _ = evaluate_dgp.synthetic_material(args.synthetic, args.seed, dim=8)
        rows = synthetic_rows(splits["rest"], args.seed, args.image_size or SYNTHETIC_SIZE)
    else:
        rows = image_dir_rows(args.image_dir, args.image_size or 224, dev)
    if not rows:
        raise SystemExit("no images found")
    feats = extract(load_cnn(args.cnn, args.version, args.seed, dev), rows, args.batch_size, dev)
    save_features(args.output, feats)
    print("wrote {}: {} classes, {} rows".format(args.output, len(feats), sum(len(a) for a in feats.values())))
    return feats


if __name__ == "__main__":
    main()
