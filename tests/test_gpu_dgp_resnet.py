"""GPU: the DGP baseline's ResNet (baseline/resnet.py, csrc/hgr_resnet_tv.hip).

Kernel tests run on GRID inputs: image values multiples of 1/8 in [-4, 4], weights multiples of 1/64 in [-1/4, 1/4], biases multiples
of 1/8.  Every product is a multiple of 1/512 and every sum stays far below 2^24 / 512, so each fp32 sum is exact in any order and the
only rounding is the final one: the expected value is torch's float64 conv2d / max_pool2d / mean rounded ONCE to the output type, and
equality is required.  The whole net is pinned to the reference's recorded features (tests/golden/dgp_resnet50.npz) within
2e-3 x max(1, max|ref|) - the bar test_gpu_model.py holds the 16-bit towers to - which must be at least 3 x the fixture's `err_model`
(the error of a CPU rounding model of the device route, tools/make_golden_dgp_resnet.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_dgp_resnet_host import fixture, torch_forward

from hgr_net_amd import ops, synth
from hgr_net_amd.baseline import dgp_eval, evaluate_dgp, resnet

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def grid(rng, shape, step, lim):
    """float64 multiples of `step` in [-lim, lim]."""
    n = int(round(lim / step))
    return torch.from_numpy(rng.integers(-n, n + 1, shape).astype(np.float64) * step)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def fold7(w4, dt):
    """[64, 3, 7, 7] -> the folded layout [64, 192] in (ky, kx, c) order."""
    w = torch.zeros(64, 192, dtype=dt)
    w[:, :147] = w4.permute(0, 2, 3, 1).reshape(64, 147).to(dt)
    return w.to(DEV)


# ---- the stem, fused and unfused -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("b, r", [(1, 30), (3, 30), (1, 70), (3, 70), (1, 64), (3, 64)])
def test_stem_fused_and_unfused_are_exact(b, r, dtype):
    dt = DTYPES[dtype]
    rng = np.random.default_rng(1000 * r + b)
    img, w4, bias = grid(rng, (b, 3, r, r), 1 / 8, 4.0), grid(rng, (64, 3, 7, 7), 1 / 64, 0.25), grid(rng, (64,), 1 / 8, 2.0)
    hc, hp = ops.stem7_geometry(r)
    conv = F.relu(F.conv2d(img, w4, bias, stride=2, padding=3)).to(dt)                 # rounded once, after bias and ReLU
    want = F.max_pool2d(conv.double(), 3, 2, 1).to(dt).permute(0, 2, 3, 1).contiguous()
    assert conv.shape[-1] == hc and want.shape[1] == hp and float(conv.float().max()) > 8.0
    x, w, bq = img.float().to(DEV), fold7(w4, dt), bias.float().to(DEV)
    fused = ops.stem7_pool(x, w, bq, torch.full((b * hp * hp, 64), -7.0, dtype=dt, device=DEV))
    col = ops.stem7_im2col(x, torch.full((b * hc * hc, 192), -7.0, dtype=dt, device=DEV))
    c1 = ops.gemm_nt(col, w, torch.empty((b * hc * hc, 64), dtype=dt, device=DEV), bias=bq, epilogue=ops.EPI_BIAS_RELU)
    unfused = ops.maxpool3s2_nhwc(c1, torch.full((b * hp * hp, 64), -7.0, dtype=dt, device=DEV), b, hc, hc, 64)
    torch.cuda.synchronize()
    # the im2col matrix itself: the taps in (ky, kx, c) order, zero beyond 147
    cols = F.unfold(img.to(dt).double(), 7, padding=3, stride=2).view(b, 3, 49, hc * hc).permute(0, 3, 2, 1).reshape(b * hc * hc, 147)
    assert torch.equal(col[:, :147].cpu().double(), cols) and not col[:, 147:].any()
    assert torch.equal(bits(c1), bits(conv.permute(0, 2, 3, 1).reshape(-1, 64)))
    assert torch.equal(bits(unfused), bits(want.view(-1, 64)))
    assert torch.equal(bits(fused), bits(want.view(-1, 64)))
    assert torch.equal(bits(fused), bits(unfused))


# ---- max-pool alone: negative maps, so that a padded zero would be seen to win ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("h, w", [(1, 1), (2, 5), (15, 15)])
def test_maxpool_ignores_taps_outside_the_map(h, w, dtype):
    dt = DTYPES[dtype]
    rng = np.random.default_rng(10 * h + w)
    x = (-0.125 - grid(rng, (2, 64, h, w), 1 / 8, 4.0).abs()).to(dt)                   # every value negative
    want = F.max_pool2d(x.double(), 3, 2, 1).to(dt).permute(0, 2, 3, 1).contiguous()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert want.shape == (2, ho, wo, 64) and float(want.double().max()) < 0
    out = ops.maxpool3s2_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), torch.zeros((2 * ho * wo, 64), dtype=dt, device=DEV), 2, h, w, 64)
    assert torch.equal(bits(out), bits(want.view(-1, 64)))


# ---- the strided 1 x 1 convolution of `downsample` -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("h", [9, 8])
def test_strided_1x1_is_gather_plus_gemm(h, dtype):
    dt = DTYPES[dtype]
    b, cin, cout, ho = 2, 256, 512, (h - 1) // 2 + 1
    rng = np.random.default_rng(h)
    x, w4, bias = grid(rng, (b, cin, h, h), 1 / 8, 4.0), grid(rng, (cout, cin, 1, 1), 1 / 64, 0.25), grid(rng, (cout,), 1 / 8, 2.0)
    want = F.conv2d(x, w4, bias, stride=2).to(dt).permute(0, 2, 3, 1).reshape(-1, cout)
    assert want.shape[0] == b * ho * ho
    xd = x.to(dt).permute(0, 2, 3, 1).contiguous().to(DEV)
    w, bq = w4.view(cout, cin).to(dt).to(DEV), bias.float().to(DEV)
    rows = ops.subsample2_nhwc(xd, torch.full((b * ho * ho, cin), 9.0, dtype=dt, device=DEV), b, h, h, cin)
    got = ops.gemm_nt(rows, w, torch.empty((b * ho * ho, cout), dtype=dt, device=DEV), bias=bq, epilogue=ops.EPI_BIAS)
    gathered = xd[:, ::2, ::2, :].contiguous().view(-1, cin)                           # torch's own gather, then the same GEMM
    ref = ops.gemm_nt(gathered, w, torch.empty((b * ho * ho, cout), dtype=dt, device=DEV), bias=bq, epilogue=ops.EPI_BIAS)
    assert torch.equal(bits(rows), bits(gathered))
    assert torch.equal(bits(got), bits(ref)) and torch.equal(bits(got), bits(want))


# ---- the global mean ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("h, w", [(1, 1), (2, 2), (3, 3)])
def test_meanpool_all_output_types(h, w, dtype):
    dt = DTYPES[dtype]
    b, c = 3, 2048
    x = grid(np.random.default_rng(h), (b, h, w, c), 1 / 8, 4.0)
    mean32 = (x.view(b, h * w, c).sum(1).float() / float(h * w))                       # an exact fp32 sum, one IEEE division
    assert torch.equal(mean32.double(), (x.view(b, h * w, c).sum(1) / (h * w)).float().double())    # = the float64 mean rounded once
    xd = x.to(dt).to(DEV)
    for out_dt in (dt, torch.float32):
        out = ops.meanpool_nhwc(xd, torch.full((b, c), 5.0, dtype=out_dt, device=DEV), b, h, w, c)
        assert out.data_ptr() % 16 == 0
        assert torch.equal(out.cpu(), mean32.to(out_dt))
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    with pytest.raises(AssertionError):
        ops.meanpool_nhwc(xd, torch.empty((b, c), dtype=other, device=DEV), b, h, w, c)


def test_bad_arguments_are_refused():
    from hgr_net_amd import _lib
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(_lib.HgrError, match="Kp"):
        ops.stem7_im2col(x, torch.empty((256, 144), dtype=torch.float16, device=DEV))
    with pytest.raises(_lib.HgrError, match="bad geometry"):
        ops.maxpool3s2_nhwc(torch.zeros(1, 2, 2, 12, dtype=torch.float16, device=DEV), torch.zeros(1, 1, 1, 12, dtype=torch.float16, device=DEV), 1, 2, 2, 12)
    with pytest.raises(_lib.HgrError, match="misaligned"):
        buf = torch.zeros(8 * 64 + 8, dtype=torch.float16, device=DEV)
        ops.subsample2_nhwc(buf[4:4 + 256].view(1, 2, 2, 64), torch.zeros(1, 1, 1, 64, dtype=torch.float16, device=DEV), 1, 2, 2, 64)


# ---- the whole net, pinned to the reference -------------------------------------------------------------------------------------------------
_NET = {}


def net(golden_dir, dtype="f16"):
    if dtype not in _NET:
        m = resnet.make_resnet_base("resnet50", dtype=dtype)
        m.load_state_dict(fixture(golden_dir)["sd"])
        _NET[dtype] = m.to(DEV).eval()
    return _NET[dtype]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("b, r", [(3, 64), (2, 72)])
def test_features_are_pinned_to_the_reference(golden_dir, monkeypatch, b, r, fused):
    fx = fixture(golden_dir)
    ref, err_model = fx[f"feat{r}"], float(fx[f"err_model_f16_{r}"])
    bound = 2e-3 * max(1.0, float(np.abs(ref).max()))
    assert err_model <= bound / 3, (err_model, bound)
    monkeypatch.setattr(resnet, "STEM_FUSED", fused)
    taps = {}
    got = net(golden_dir).features(synth.images(b, r, int(fx["seeds"][1])).to(DEV), taps=taps)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"R={r} fused={fused}: max |feature - reference| = {err:.5f} (err_model {err_model:.5f}, bound {bound:.5f})")
    assert err <= bound
    if r == 64:
        pref, perr_model = fx["pool64"], float(fx["err_model_pool_f16_64"])
        pbound = 2e-3 * max(1.0, float(np.abs(pref).max()))
        assert perr_model <= pbound / 3, (perr_model, pbound)
        perr = float(np.abs(taps["pool"][0].float().cpu().numpy() - pref).max())
        print(f"  post-pool tensor: max |err| = {perr:.5f} (err_model {perr_model:.5f}, bound {pbound:.5f})")
        assert taps["pool"].shape == (b, 16, 16, 64) and perr <= pbound


def test_bf16_against_the_torch_restatement(golden_dir):
    """bf16 carries 8 significant bits: its bound is 3 x the rounding model's bf16 error, as the f16 bound is about 3 x its own."""
    fx = fixture(golden_dir)
    x = synth.images(3, 64, int(fx["seeds"][1]))
    taps_ref, taps = {}, {}
    ref = torch_forward(fx["sd"], x, taps_ref).numpy()
    got = net(golden_dir, "bf16").features(x.to(DEV), taps=taps).cpu().numpy()
    err, bound = float(np.abs(got - ref).max()), 3 * float(fx["err_model_bf16_64"])
    perr = float((taps["pool"][0].float().cpu() - taps_ref["pool"][0].permute(1, 2, 0)).abs().max())
    pbound = 3 * float(fx["err_model_pool_bf16_64"])
    print(f"bf16: max |feature - torch| = {err:.4f} (bound {bound:.4f}); post-pool {perr:.4f} (bound {pbound:.4f})")
    assert err <= bound and perr <= pbound


def test_resnet_head_runs_fc_through_gemm(golden_dir):
    fx = fixture(golden_dir)
    m = resnet.ResNet("resnet50", 10)
    m.resnet_base.load_state_dict(fx["sd"])
    with torch.no_grad():
        m.fc.weight.copy_(torch.from_numpy(synth.normal(3, "fc.w", 10 * 2048).reshape(10, 2048).astype(np.float32) * 0.02).half().float())
        m.fc.bias.copy_(torch.arange(10.0) / 8)
    m = m.to(DEV).eval()
    logits, feat = m(synth.images(3, 64, int(fx["seeds"][1])).to(DEV), need_features=True)
    assert logits.shape == (3, 10) and feat.shape == (3, 2048) and torch.equal(m(synth.images(3, 64, int(fx["seeds"][1])).to(DEV)), logits)
    want = feat.double().cpu() @ m.fc.weight.detach().double().cpu().T + m.fc.bias.detach().double().cpu()
    assert float((logits.double().cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    assert float(np.abs(feat.cpu().numpy() - fx["feat64"]).max()) <= 2e-3 * float(np.abs(fx["feat64"]).max()) + 2 ** -6   # + the f16 rounding of the rows


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------------
def test_forward_replays_from_a_graph(golden_dir):
    m = net(golden_dir)
    imgs = [synth.images(2, 72, seed).to(DEV) for seed in (5, 6, 7)]
    eager = [m(x).clone() for x in imgs]
    static = imgs[0].clone()
    m(static)                                                          # buffers of this shape exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(static)
    for x, want in zip(imgs[1:], eager[1:]):
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    assert not torch.equal(eager[1], eager[2])


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_with_cnn_equals_evaluator_fed_features(golden_dir):
    cnn = resnet.ResNetFeatures(net(golden_dir))
    edges, splits, pred, _ = evaluate_dgp.synthetic_material(40, 0, dim=2048)
    nodes, ns = splits["train"] + splits["rest"], len(splits["train"])
    a = dgp_eval.DGPEvaluator(edges, nodes, ns, pred, device=DEV, cnn=cnn)
    b = dgp_eval.DGPEvaluator(edges, nodes, ns, pred, device=DEV)
    for i in range(4):
        x = synth.images(1 + i, 64, 20 + i).to(DEV)
        f = cnn(x).clone()
        assert f.dtype == torch.float16 and f.is_contiguous() and f.data_ptr() % 16 == 0 and f.shape == (1 + i, 2048)
        a.add(x, ns + i)
        b.add(f, ns + i)
    assert torch.equal(a.acc, b.acc) and float(a.acc[:, 8].sum()) == 10.0


def test_cli_scores_generated_images_end_to_end(capsys):
    res = evaluate_dgp.main(["--synthetic", "40", "--cnn", "synthetic"])
    printed = capsys.readouterr().out.strip().splitlines()
    from hgr_net_amd.baseline import extract_features
    _, splits, _, _ = evaluate_dgp.synthetic_material(40, 0, dim=8)
    fed = sum(len(r) for r in extract_features.synthetic_rows(splits["rest"], 0, extract_features.SYNTHETIC_SIZE).values())
    assert printed[-1].startswith("summary: ") and printed[-1].split()[-2:] == ["total", str(fed)] and res["tot"] == fed > len(splits["rest"])


def test_extract_features_writes_what_evaluate_reads(tmp_path, capsys):
    from hgr_net_amd.baseline import extract_features
    path = tmp_path / "feat.npz"
    feats = extract_features.main(["--cnn", "synthetic", "--synthetic", "40", "--output", str(path), "--batch-size", "4"])
    back = dgp_eval.load_features(path)
    assert list(back) == list(feats) and all(np.array_equal(back[w], feats[w]) and back[w].shape[1] == 2048 for w in feats)
    direct = evaluate_dgp.main(["--synthetic", "40", "--cnn", "synthetic", "--batch-size", "4"])
    edges, splits, pred, _ = evaluate_dgp.synthetic_material(40, 0, dim=2048)
    apart = evaluate_dgp.evaluate(edges, splits["train"], splits["rest"], pred, back, batch_size=4, device=DEV, log=lambda s: None)
    assert apart["hits"] == direct["hits"] and apart["tot"] == direct["tot"]
