#!/usr/bin/env python3
"""Generates tests/golden/dgp_resnet50.npz by RUNNING the reference's baseline/DGP/models/resnet.py on the CPU in fp32.  The module
is imported from the reference checkout at run time (it only needs torch); nothing of it is copied.  The fixture holds

  keys, shapes     the key list and shapes of `make_resnet_base('resnet50').state_dict()`
  seeds            (weights seed, image seed): inputs are synth.resnet_state_dict('resnet50', 0), synth.images(3, 64, 1234) and
                   synth.images(2, 72, 1234) - R = 72 gives odd maps (18, 9, 5, 3) in layers 3 and 4
  feat64, feat72   the reference's features [3, 2048] / [2, 2048]
  pool64           its post-max-pool tensor of image 0 at R = 64, NHWC [16, 16, 64]
  err_model_*      the maximum error of a CPU ROUNDING MODEL of the device route against those outputs, per 16-bit type and per
                   resolution (and for pool64): folded weights (clip/model.py `_fold`) rounded to the type, the image rounded to the
                   type, every layer's output (after bias, ReLU and the residual add) rounded to the type once, fp32 arithmetic
                   between the roundings, the identity branch rounded before it is added, the final mean left in fp32.
                   It is the distance between two correct implementations that the GPU tests size their bounds by."""
import importlib.util
import json
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("HGR_REFERENCE", REPO.parent / "reference")) / "baseline" / "DGP" / "models" / "resnet.py"   # the reference checkout
sys.path.insert(0, str(REPO))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
import torch.nn.functional as F                                        # noqa: E402

from hgr_net_amd import synth                                          # noqa: E402

GOLD = REPO / "tests" / "golden" / "dgp_resnet50.npz"
W_SEED, IMG_SEED = 0, 1234
CASES = ((3, 64), (2, 72))


def load_reference():
    spec = importlib.util.spec_from_file_location("dgp_reference_resnet", str(REF))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fold(sd, conv, bn, dt):
    """(w, b) of conv + inference BatchNorm, the weight rounded to dt (clip/model.py `_fold`)."""
    s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-5)
    b = sd[bn + ".bias"] - sd[bn + ".running_mean"] * s
    return (sd[conv + ".weight"] * s.view(-1, 1, 1, 1)).to(dt).float(), b


def rounding_model(sd, x, dt, taps=None):
    rnd = lambda t: t.to(dt).float()
    w, b = fold(sd, "conv1", "bn1", dt)
    a = rnd(F.relu(F.conv2d(rnd(x), w, b, stride=2, padding=3)))
    a = F.max_pool2d(a, 3, 2, 1)
    if taps is not None:
        taps["pool"] = a
    for li in (1, 2, 3, 4):
        j = 0
        while f"layer{li}.{j}.conv1.weight" in sd:
            p = f"layer{li}.{j}"
            stride = 2 if (li > 1 and j == 0) else 1
            w, b = fold(sd, p + ".conv1", p + ".bn1", dt)
            t = rnd(F.relu(F.conv2d(a, w, b)))
            w, b = fold(sd, p + ".conv2", p + ".bn2", dt)
            t = rnd(F.relu(F.conv2d(t, w, b, stride=stride, padding=1)))
            idn = a
            if p + ".downsample.0.weight" in sd:
                w, b = fold(sd, p + ".downsample.0", p + ".downsample.1", dt)
                idn = rnd(F.conv2d(a, w, b, stride=stride))
            w, b = fold(sd, p + ".conv3", p + ".bn3", dt)
            a = rnd(F.relu(F.conv2d(t, w, b) + idn))
            j += 1
    return a.flatten(2).mean(2)


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    ref = load_reference()
    net = ref.make_resnet_base("resnet50")
    sd = synth.resnet_state_dict("resnet50", W_SEED)
    net.load_state_dict(sd)
    net.eval()
    ref_sd = net.state_dict()
    out = {"keys": np.array(list(ref_sd.keys())), "shapes": np.array(json.dumps([list(v.shape) for v in ref_sd.values()])),
           "seeds": np.array([W_SEED, IMG_SEED], np.int64)}
    grabbed = {}
    net.maxpool.register_forward_hook(lambda m, i, o: grabbed.__setitem__("pool", o.detach().clone()))
    for b, r in CASES:
        x = synth.images(b, r, IMG_SEED)
        feat = net(x)
        out[f"feat{r}"] = feat.numpy().astype(np.float32)
        print(f"R={r}: max|ref| = {feat.abs().max():.3f}, mean|ref| = {feat.abs().mean():.3f}")
        if r == 64:
            out["pool64"] = np.ascontiguousarray(grabbed["pool"][0].permute(1, 2, 0).numpy().astype(np.float32))
        for name, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            taps = {}
            err = float((rounding_model(sd, x, dt, taps) - feat).abs().max())
            out[f"err_model_{name}_{r}"] = np.float64(err)
            print(f"  err_model {name}: {err:.5f}")
            if r == 64:
                perr = float((taps["pool"][0] - grabbed["pool"][0]).abs().max())
                out[f"err_model_pool_{name}_64"] = np.float64(perr)
                print(f"  err_model pool {name}: {perr:.5f} (max|ref| = {grabbed['pool'][0].abs().max():.3f})")
    np.savez_compressed(GOLD, **out)
    print(f"wrote {GOLD} ({GOLD.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
