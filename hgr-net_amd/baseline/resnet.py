"""The DGP baseline's feature extractor on the device: the torchvision-style ResNet of the reference's baseline/DGP/models/resnet.py
(`make_resnet_base`, `ResNet`), which evaluate_imagenet.py pushes every image through before it scores the features.  It is NOT
CLIP's ModifiedResNet (clip/model.py): a 7 x 7 / stride 2 stem, a 3 x 3 / stride 2 max-pool, the stride of the first block of layers
2 - 4 on its 3 x 3 convolution and on a strided 1 x 1 `downsample`, and a global mean.

Module tree, constructor arguments and `state_dict` keys are the reference's (`conv1.weight`, `bn1.*`, `layerL.J.conv{1,2,3}.weight`,
`layerL.J.bnK.*`, `layerL.J.downsample.0/1.*`; `resnet_base.*` / `fc.*` on `ResNet`), so its checkpoints load as they are.

`model.eval()(images)` runs on libhgr: activations NHWC in the 16-bit MFMA type, BatchNorm folded into the convolution in front of it
(once per weights generation), every 1 x 1 convolution a `gemm_nt`, every 3 x 3 the implicit-GEMM `conv3x3_nhwc`, the stem
`hgr_stem7_pool` (or, with HGR_TV_STEM_FUSED=0, im2col + GEMM + max-pool), the strided 1 x 1 a row gather + `gemm_nt`, the head
`hgr_meanpool_nhwc`.  No host synchronisation: a forward can be captured in a HIP graph.  `model.train()(x)` raises - training-mode
BatchNorm and its backward (train_resnet_fit.py) are not built.  The BasicBlock versions (resnet18 / resnet34) build and load, but
their forward raises: the 3 x 3 kernel has no residual epilogue."""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..clip.model import _Workspace, _fold
from ..ops import EPI_BIAS, EPI_BIAS_ADD16_RELU, EPI_BIAS_RELU

__all__ = ["ResNetBase", "make_resnet_base", "ResNet", "ResNetFeatures", "BasicBlock", "Bottleneck", "VERSIONS", "IMAGENET_MEAN", "IMAGENET_STD"]

# HGR_TV_STEM_FUSED=0: the stem runs as hgr_stem7_im2col -> gemm_nt(BIAS_RELU) -> hgr_maxpool3s2_nhwc (three launches, the conv map
# written and read back) instead of the one-launch hgr_stem7_pool - for A/B runs and tests; same bits on inputs whose sums are exact.
STEM_FUSED = os.environ.get("HGR_TV_STEM_FUSED", "1") != "0"

IMAGENET_MEAN = (0.485, 0.456, 0.406)          # train_resnet_fit.py:32-33
IMAGENET_STD = (0.229, 0.224, 0.225)

VERSIONS = {"resnet18": ("basic", (2, 2, 2, 2)), "resnet34": ("basic", (3, 4, 6, 3)), "resnet50": ("bottleneck", (3, 4, 6, 3)),
            "resnet101": ("bottleneck", (3, 4, 23, 3)), "resnet152": ("bottleneck", (3, 8, 36, 3))}


class BasicBlock(nn.Module):
    """Two 3 x 3 convolutions and a residual add (resnet18 / resnet34): parameters only, no device forward."""
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample, self.stride = downsample, stride


class Bottleneck(nn.Module):
    """1 x 1 -> 3 x 3 (carries the stride) -> 1 x 1 to 4 x planes, residual add, ReLU."""
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample, self.stride = downsample, stride


class _Block16:
    """Folded 16-bit weights of one Bottleneck."""

    def __init__(self, blk: Bottleneck, dt: torch.dtype):
        self.c1, self.c2, self.c3 = _fold(blk.conv1, blk.bn1, dt), _fold(blk.conv2, blk.bn2, dt), _fold(blk.conv3, blk.bn3, dt)
        self.down = _fold(blk.downsample[0], blk.downsample[1], dt) if blk.downsample is not None else None
        self.stride, self.planes, self.out = blk.stride, blk.conv1.weight.shape[0], blk.conv3.weight.shape[0]


class ResNetBase(nn.Module):
    """`ResNetBase(block, layers)` as in the reference; `dtype` ("f16" | "bf16") is the MFMA input type of the device forward."""

    def __init__(self, block, layers, dtype: str = "f16"):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.out_channels = 512 * block.expansion
        self.block = block
        self.compute_dtype = ops.TORCH16[ops.dtype_code(dtype)]
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
        self._ws = _Workspace()
        self._prep: dict = {}

    def _make_layer(self, block, planes: int, blocks: int, stride: int = 1) -> nn.Sequential:
        out = planes * block.expansion
        down = None
        if stride != 1 or self.inplanes != out:
            down = nn.Sequential(nn.Conv2d(self.inplanes, out, 1, stride=stride, bias=False), nn.BatchNorm2d(out))
        seq = [block(self.inplanes, planes, stride, down)] + [block(out, planes) for _ in range(1, blocks)]
        self.inplanes = out
        return nn.Sequential(*seq)

    # -- device forward -----------------------------------------------------------------------------------------------------------
    def _fingerprint(self):
        """(storage, torch version counter) of every parameter and BatchNorm buffer + ops.WEIGHTS_GEN, as CLIP._fingerprint."""
        return (ops.WEIGHTS_GEN[0], self.compute_dtype) + tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def _prepared(self) -> dict:
        fp = self._fingerprint()
        if self._prep.get("fp") != fp:
            dt = self.compute_dtype
            self._prep = {"fp": fp, "stem": _fold(self.conv1, self.bn1, dt),
                          "blocks": [_Block16(b, dt) for li in (1, 2, 3, 4) for b in getattr(self, f"layer{li}")]}
        return self._prep

    def _check(self, x: torch.Tensor) -> None:
        if self.training:
            raise NotImplementedError("training-mode BatchNorm: this build runs the ResNet for inference (model.eval()); "
                                      "train_resnet_fit.py is out of scope")
        if self.block is not Bottleneck:
            raise NotImplementedError("BasicBlock versions (resnet18 / resnet34) build and load, but have no device forward: a BasicBlock "
                                      "ends in a 3 x 3 convolution + residual add, and hgr_conv3x3_nhwc has no residual epilogue")
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == x.shape[3]
                and x.dtype == torch.float32 and x.shape[0] >= 1 and x.shape[2] >= 32):
            raise ops._lib.HgrError("images must be a device tensor [B, 3, R, R] in fp32 with R >= 32 (no CPU path)")

    @torch.no_grad()
    def features(self, x: torch.Tensor, out_dtype: torch.dtype = torch.float32, taps: Optional[dict] = None) -> torch.Tensor:
        """[B, out_channels] in `out_dtype` (fp32 or the compute type, rounded once).  `taps`, if a dict, receives 'pool' = the
        post-max-pool NHWC tensor (a view of a workspace buffer)."""
        self._check(x)
        p, ws, dt, dev = self._prepared(), self._ws, self.compute_dtype, x.device
        x = x.contiguous()
        b, r = x.shape[0], x.shape[2]
        w1, b1 = p["stem"]
        hc, h = ops.stem7_geometry(r)
        a = ws.get("tv.x0", (b * h * h, 64), dt, dev)
        if STEM_FUSED:
            ops.stem7_pool(x, w1, b1, a)
        else:
            col = ws.get("tv.col", (b * hc * hc, w1.shape[1]), dt, dev)
            ops.stem7_im2col(x, col)
            c1 = ws.get("tv.c1", (b * hc * hc, 64), dt, dev)
            ops.gemm_nt(col, w1, c1, bias=b1, epilogue=EPI_BIAS_RELU, tag="tv.stem")
            ops.maxpool3s2_nhwc(c1, a, b, hc, hc, 64)
        if taps is not None:
            taps["pool"] = a.view(b, h, h, 64)
        cin, flip = 64, 0
        for k in p["blocks"]:
            m, pl = b * h * h, k.planes
            t1 = ws.get("tv.t1", (m, pl), dt, dev)
            ops.gemm_nt(a, k.c1[0], t1, bias=k.c1[1], epilogue=EPI_BIAS_RELU, tag="tv.c1")
            ho = (h - 1) // k.stride + 1
            mo = b * ho * ho
            t2 = ws.get("tv.t2", (mo, pl), dt, dev)
            ops.conv3x3_nhwc(t1, k.c2[0], k.c2[1], t2, b, h, h, pl, stride=k.stride)
            idn = a
            if k.down is not None:
                xin = a
                if k.stride == 2:                              # the rows a 1 x 1 / stride 2 convolution reads
                    xin = ws.get("tv.xs", (mo, cin), dt, dev)
                    ops.subsample2_nhwc(a, xin, b, h, h, cin)
                idn = ws.get("tv.idn", (mo, k.out), dt, dev)
                ops.gemm_nt(xin, k.down[0], idn, bias=k.down[1], epilogue=EPI_BIAS, tag="tv.down")
            out = ws.get(f"tv.out{flip}", (mo, k.out), dt, dev)
            ops.gemm_nt(t2, k.c3[0], out, bias=k.c3[1], residual=idn, epilogue=EPI_BIAS_ADD16_RELU, tag="tv.c3")
            a, cin, h, flip = out, k.out, ho, flip ^ 1
        if out_dtype not in (torch.float32, dt):
            raise ValueError(f"out_dtype {out_dtype}: fp32 or the compute type {dt}")
        feat = torch.empty((b, cin), dtype=out_dtype, device=dev)
        return ops.meanpool_nhwc(a, feat, b, h, h, cin)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.features(x)


def make_resnet_base(version: str, pretrained=None, dtype: str = "f16") -> ResNetBase:
    """The reference's factory: `pretrained` names a torchvision-style checkpoint, whose `fc.*` entries are dropped."""
    if version not in VERSIONS:
        raise KeyError(f"unknown version {version!r}: one of {sorted(VERSIONS)}")
    kind, layers = VERSIONS[version]
    net = ResNetBase(BasicBlock if kind == "basic" else Bottleneck, list(layers), dtype=dtype)
    if pretrained is not None:
        sd = torch.load(pretrained, map_location="cpu")
        sd.pop("fc.weight")
        sd.pop("fc.bias")
        net.load_state_dict(sd)
    return net


class ResNet(nn.Module):
    """`resnet_base` + `fc`; `forward(x, need_features=False)` returns the logits (fp32), with `need_features` also the features."""

    def __init__(self, version: str, num_classes: int, pretrained=None, dtype: str = "f16"):
        super().__init__()
        self.resnet_base = make_resnet_base(version, pretrained=pretrained, dtype=dtype)
        self.fc = nn.Linear(self.resnet_base.out_channels, num_classes)
        self._fc: dict = {}

    @torch.no_grad()
    def forward(self, x: torch.Tensor, need_features: bool = False):
        base = self.resnet_base
        dt = base.compute_dtype
        f16 = base.features(x, out_dtype=dt)
        fp = (ops.WEIGHTS_GEN[0], dt, self.fc.weight.data_ptr(), self.fc.weight._version, self.fc.bias.data_ptr(), self.fc.bias._version)
        if self._fc.get("fp") != fp:
            n, k = self.fc.weight.shape
            self._fc = {"fp": fp, "w": self.fc.weight.detach().to(dt).contiguous(), "b": self.fc.bias.detach().float().contiguous(),
                        "ld": -(-n // 4) * 4}
        out = torch.empty((x.shape[0], self._fc["ld"]), dtype=torch.float32, device=x.device)
        ops.gemm_nt(f16, self._fc["w"], out, bias=self._fc["b"], epilogue=EPI_BIAS, n=self.fc.weight.shape[0], tag="tv.fc")
        logits = out[:, :self.fc.weight.shape[0]]
        return (logits, f16.float()) if need_features else logits


class ResNetFeatures:
    """The callable `DGPEvaluator(cnn=...)` wants: fp32 images [B, 3, R, R] -> contiguous, 16-byte aligned fp16 rows [B, out_channels]
    (with an f16 net straight from hgr_meanpool_nhwc, so the evaluator's table reads them without its staging copy)."""

    def __init__(self, model, dtype: str = "f16"):
        base = model.resnet_base if isinstance(model, ResNet) else model
        if not isinstance(base, ResNetBase):
            raise TypeError("ResNetFeatures wraps a ResNetBase or a ResNet")
        want = ops.TORCH16[ops.dtype_code(dtype)]
        if base.compute_dtype != want:
            base.compute_dtype = want
        self.base = base.eval()
        self.out_channels = base.out_channels

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        if self.base.compute_dtype == torch.float16:
            return self.base.features(images, out_dtype=torch.float16)
        return self.base.features(images).to(torch.float16)
