"""Host side of the DGP baseline's ResNet (baseline/resnet.py): the module's `state_dict` schema against the reference's
(tests/golden/dgp_resnet50.npz, recorded by tools/make_golden_dgp_resnet.py), the `pretrained` route, what refuses to run, the stem's
geometry, the command lines' argument checks and the feature file's round trip.  `torch_forward` is the fp32 torch restatement of the
net that the GPU tests also use; here it is held against the reference's recorded features."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hgr_net_amd import ops, synth
from hgr_net_amd.baseline import dgp_eval, evaluate_dgp, extract_features, resnet

_FIX = {}


def fixture(golden_dir):
    if not _FIX:
        with np.load(golden_dir / "dgp_resnet50.npz") as z:
            _FIX.update({k: z[k] for k in z.files})
        _FIX["sd"] = synth.resnet_state_dict("resnet50", int(_FIX["seeds"][0]))
    return _FIX


def torch_forward(sd, x, taps=None):
    """models/resnet.py:139-151 with inference BatchNorm, in torch's own fp32 operations on the CPU."""
    def cbn(t, conv, bn, stride=1, padding=0):
        t = F.conv2d(t, sd[conv + ".weight"], None, stride=stride, padding=padding)
        return F.batch_norm(t, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, 1e-5)
    a = F.max_pool2d(F.relu(cbn(x, "conv1", "bn1", 2, 3)), 3, 2, 1)
    if taps is not None:
        taps["pool"] = a
    for li in (1, 2, 3, 4):
        j = 0
        while f"layer{li}.{j}.conv1.weight" in sd:
            p, stride = f"layer{li}.{j}", 2 if (li > 1 and j == 0) else 1
            t = F.relu(cbn(a, p + ".conv1", p + ".bn1"))
            t = F.relu(cbn(t, p + ".conv2", p + ".bn2", stride, 1))
            idn = cbn(a, p + ".downsample.0", p + ".downsample.1", stride) if p + ".downsample.0.weight" in sd else a
            a = F.relu(cbn(t, p + ".conv3", p + ".bn3") + idn)
            j += 1
    return a.flatten(2).mean(2)


def test_state_dict_schema_is_the_references(golden_dir):
    fx = fixture(golden_dir)
    keys, shapes = [str(k) for k in fx["keys"]], json.loads(str(fx["shapes"]))
    assert len(keys) == len(shapes) == 318 and keys[0] == "conv1.weight" and "layer2.0.downsample.1.running_var" in keys
    net = resnet.make_resnet_base("resnet50")
    mine = net.state_dict()
    assert list(mine.keys()) == keys and [list(v.shape) for v in mine.values()] == shapes
    sd = fx["sd"]
    assert list(sd.keys()) == keys and [list(v.shape) for v in sd.values()] == shapes
    assert all(torch.equal(v, v.half().float()) for v in sd.values() if v.dtype == torch.float32)       # fp16-representable
    net.load_state_dict(sd)
    assert net.out_channels == 2048 and net.compute_dtype == torch.float16
    assert resnet.make_resnet_base("resnet50", dtype="bf16").compute_dtype == torch.bfloat16
    assert synth.RESNET_LAYERS == {v: layers for v, (kind, layers) in resnet.VERSIONS.items() if kind == "bottleneck"}
    assert sum(1 for k in resnet.make_resnet_base("resnet101").state_dict() if k.endswith(".conv3.weight")) == 33
    with pytest.raises(KeyError):
        resnet.make_resnet_base("resnet51")


def test_torch_restatement_matches_the_recorded_reference(golden_dir):
    fx = fixture(golden_dir)
    taps = {}
    got = torch_forward(fx["sd"], synth.images(3, 64, int(fx["seeds"][1])), taps).numpy()
    assert np.abs(got - fx["feat64"]).max() <= 1e-4 * np.abs(fx["feat64"]).max()
    assert np.abs(taps["pool"][0].permute(1, 2, 0).numpy() - fx["pool64"]).max() <= 1e-5 * np.abs(fx["pool64"]).max()
    assert fx["feat64"].shape == (3, 2048) and fx["feat72"].shape == (2, 2048) and fx["pool64"].shape == (16, 16, 64)


def test_pretrained_drops_fc_and_resnet_wraps_the_base(golden_dir, tmp_path):
    sd = dict(fixture(golden_dir)["sd"])
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(10, 2048), torch.zeros(10)
    path = tmp_path / "resnet50.pth"
    torch.save(sd, path)
    net = resnet.make_resnet_base("resnet50", pretrained=str(path))
    assert torch.equal(net.layer4[2].bn3.running_var, sd["layer4.2.bn3.running_var"]) and "fc.weight" not in net.state_dict()
    torch.save({k: v for k, v in sd.items() if not k.startswith("fc.")}, path)
    with pytest.raises(KeyError):                                      # the reference pops them unconditionally
        resnet.make_resnet_base("resnet50", pretrained=str(path))
    full = resnet.ResNet("resnet18", 7)
    keys = list(full.state_dict().keys())
    assert keys[0] == "resnet_base.conv1.weight" and keys[-2:] == ["fc.weight", "fc.bias"] and full.fc.weight.shape == (7, 512)
    assert "resnet_base.layer2.0.downsample.0.weight" in keys and "resnet_base.layer1.0.downsample.0.weight" not in keys
    assert not any(".conv3." in k for k in keys)


def test_what_does_not_run_says_why():
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="residual epilogue"):
        resnet.make_resnet_base("resnet18").eval()(x)
    with pytest.raises(NotImplementedError, match="residual epilogue"):
        resnet.ResNet("resnet34", 5).eval()(x)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        resnet.make_resnet_base("resnet50").train()(x)
    with pytest.raises(ops._lib.HgrError, match="no CPU path"):
        resnet.make_resnet_base("resnet50").eval()(x)
    with pytest.raises(TypeError):
        resnet.ResNetFeatures(torch.nn.Linear(2, 2))


@pytest.mark.parametrize("r, hc, hp", [(32, 16, 8), (33, 17, 9), (64, 32, 16), (70, 35, 18), (72, 36, 18), (224, 112, 56)])
def test_stem_geometry(r, hc, hp):
    assert ops.stem7_geometry(r) == (hc, hp)
    x = torch.zeros(1, 3, r, r)
    c = F.conv2d(x, torch.zeros(1, 3, 7, 7), stride=2, padding=3)
    assert c.shape[-1] == hc and F.max_pool2d(c, 3, 2, 1).shape[-1] == hp


def test_command_line_argument_errors():
    a = evaluate_dgp.parse_args(["--synthetic", "40", "--cnn", "synthetic"])
    assert (a.cnn, a.image_dir, a.image_size, a.version) == ("synthetic", None, None, "resnet50")
    a = evaluate_dgp.parse_args(["--cnn", "w.pth", "--image-dir", "d", "--image-size", "96", "--version", "resnet101"])
    assert (a.cnn, a.image_dir, a.image_size, a.version) == ("w.pth", "d", 96, "resnet101")
    for bad in (["--cnn", "w.pth"], ["--cnn", "synthetic"], ["--image-dir", "d"], ["--cnn", "w.pth", "--image-dir", "d", "--features", "f.npz"],
                ["--cnn", "w.pth", "--image-dir", "d", "--synthetic", "40"], ["--synthetic", "40", "--cnn", "synthetic", "--image-size", "16"],
                ["--synthetic", "40", "--cnn", "synthetic", "--version", "resnet18"]):
        with pytest.raises(SystemExit):
            evaluate_dgp.parse_args(bad)
    a = extract_features.parse_args(["--cnn", "synthetic", "--synthetic", "40", "--output", "f.npz"])
    assert (a.cnn, a.synthetic, a.output, a.batch_size) == ("synthetic", 40, "f.npz", 256)
    for bad in ([], ["--cnn", "w.pth", "--image-dir", "d"], ["--cnn", "w.pth", "--output", "f.npz"], ["--image-dir", "d", "--output", "f.npz"],
                ["--cnn", "synthetic", "--synthetic", "40", "--output", "f.npz", "--batch-size", "0"]):
        with pytest.raises(SystemExit):
            extract_features.parse_args(bad)
    help_text = " ".join(evaluate_dgp.__doc__.split()) + " ".join(extract_features.__doc__.split())
    assert "unknown" in help_text and "datasets/imagenet.py" in help_text


def test_feature_file_round_trip(tmp_path):
    feats = {"n00000001": np.arange(12, dtype=np.float16).reshape(3, 4), "n00000002": np.ones((1, 4), np.float16)}
    path = tmp_path / "feat.npz"
    extract_features.save_features(path, feats)
    back = dgp_eval.load_features(path)
    assert list(back) == list(feats) and all(back[w].dtype == np.float16 and np.array_equal(back[w], feats[w]) for w in feats)
    for bad in ({}, {"a": np.ones((2, 4), np.float16), "b": np.ones((2, 5), np.float16)}, {"a": np.ones(4, np.float32)}, {"a": np.ones((2, 4), np.int32)}):
        with pytest.raises(ValueError):
            extract_features.save_features(tmp_path / "bad.npz", bad)
    rows = extract_features.synthetic_rows(["n1", "n2", "n3"], 0, 32)
    assert all(1 <= len(r) <= 9 and r.batch(0, 4, "cpu").shape[1:] == (3, 32, 32) for r in rows.values())
    assert not torch.equal(rows["n1"].batch(0, 1, "cpu"), rows["n2"].batch(0, 1, "cpu"))
