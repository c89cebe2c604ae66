"""CPU: the FREE baseline's host side - the modules' state_dict schema, the host twins against the fixtures the reference's own code
recorded (tools/make_golden_free.py: err32 is the measured distance between its fp32 and fp64 runs; a twin must stay within
4 x err32 of fp64, the rule of tests/test_cnzsl_host.py), next_batch's index sequences with the wrap, the counter normal's moments,
the argument checks of the five entry points (they return before any launch, so no device is needed) and the command line."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _free():
    from hgr_net_amd.baseline import free
    return free


def load(golden_dir, name):
    with np.load(golden_dir / name) as z:
        return {k: z[k] for k in z.files}


def fixture_opt(fx):
    a, ngh, _, n_seen = (int(v) for v in fx["dims"][:4])
    return _free().make_opt(attSize=a, ngh=ngh, latensize=ngh // 2, nclass_seen=n_seen, decoder_hidden=ngh)


def fixture_inputs(fx, counts=None):
    """What tools/make_golden_free.py `inputs` builds by seed: attributes, the loader's real rows and labels, the test rows, the
    classifier's initial weight - and the two networks' state dicts."""
    free = _free()
    from hgr_net_amd import synth
    seed = int(fx["seed"])
    a, ngh, n_nodes, n_seen, num, real_rows, _, loader, _ = (int(v) for v in fx["dims"])
    k = free.RES + ngh + a
    opt = fixture_opt(fx)
    att = free.synth_rows(seed, "free.att", n_nodes, a)
    att = (att / np.sqrt((att.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)
    real = [np.abs(0.5 * free.synth_rows(seed, f"free.real.{i}", real_rows, free.RES)) for i in range(loader)]
    labels = [synth.randint(seed, f"free.labels.{i}", real_rows, 0, n_seen).astype(np.int64) for i in range(loader)]
    sd_g, sd_fr = free.synth_state(seed, opt, "netG", float(fx["att_gain"])), free.synth_state(seed, opt, "netFR")
    out = dict(seed=seed, opt=opt, att=att, real=real, labels=labels, sd_g=sd_g, sd_fr=sd_fr, w0=0.02 * free.synth_rows(seed, "free.cls.w", n_nodes, k),
               z=[free.synth_rows(seed, f"free.z.{i}", num, a) for i in range(n_nodes - n_seen)])
    if counts is not None:
        tcls = np.repeat(np.arange(n_seen, n_nodes), counts)
        tz = np.concatenate([out["z"][i][:c] for i, c in enumerate(counts)], 0)
        out["test"] = free.generator_host(sd_g, tz, att[tcls]).numpy()
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_state_dict_schema_matches_the_reference(golden_dir):
    free = _free()
    fx = load(golden_dir, "free_forward_small.npz")
    opt = fixture_opt(fx)
    for mod, tag in ((free.Generator(opt), "netG"), (free.FR(opt, opt.attSize), "netFR")):
        sd = mod.state_dict()
        assert list(sd) == [str(k) for k in fx["keys_" + tag]]
        assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == fx["shapes_" + tag].tolist()
    assert list(free.Encoder(opt).state_dict()) == [p + s for p in ("fc1", "fc3", "linear_means", "linear_log_var") for s in (".weight", ".bias")]
    assert list(free.Discriminator(opt).state_dict()) == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    cls = free.LinearLogSoftmaxClassifier(2240, 96)
    assert {k: tuple(v.shape) for k, v in cls.state_dict().items()} == {"fc.weight": (96, 2240), "fc.bias": (96,)}
    assert float(free.Generator(opt).fc1.bias.data.abs().max()) == 0.0 and 0.015 < float(free.Generator(opt).fc1.weight.data.std()) < 0.025     # weights_init


def test_training_mode_and_gan_modules_name_train_free():
    free = _free()
    opt = free.make_opt(attSize=64, ngh=128, latensize=64, nclass_seen=4, decoder_hidden=128)
    x = torch.zeros(2, 64)
    for call in (lambda: free.Encoder(opt).eval()(x), lambda: free.Discriminator(opt).eval()(x, x), lambda: free.Generator(opt).train()(x, x),
                 lambda: free.FR(opt, 64).train()(torch.zeros(2, 2048))):
        with pytest.raises(NotImplementedError, match="train_free.py"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        free.Generator(opt).eval()(x, x)


def test_host_twins_match_the_reference_forward(golden_dir):
    free = _free()
    fx = load(golden_dir, "free_forward_small.npz")
    m = fixture_inputs(fx)
    seed, rows, a = m["seed"], fx["x32"].shape[0], int(fx["dims"][0])
    z, eps = free.synth_rows(seed, "free.fwd.z", rows, a), free.synth_rows(seed, "free.fwd.eps", rows, a)
    tol = 4 * float(fx["err32"])
    x = free.generator_host(m["sd_g"], z, m["att"][fx["cls"]]).numpy()
    f = free.fr_host(m["sd_fr"], m["real"][0][:rows], eps)
    big = free.features_host(m["sd_fr"], m["real"][0][:rows], eps).numpy()
    errs = {"x": rel(x, fx["x64"]), "hidden": rel(f["hidden"].numpy(), fx["hidden64"]), "h": rel(f["h"].numpy(), fx["h64"]), "mus": rel(f["mus"].numpy(), fx["mus64"])}
    print(errs, "tol", tol)
    assert max(errs.values()) <= tol
    assert np.array_equal(big[:, :free.RES], m["real"][0][:rows]) and rel(big[:, free.RES:], np.concatenate((fx["hidden64"], fx["h64"]), 1)) <= tol
    assert rel(f["stds"].numpy(), fx["stds32"]) <= tol and rel(f["encoder_out"].numpy(), fx["enc32"]) <= tol


def test_fit_step_host_matches_the_reference(golden_dir):
    free = _free()
    fx = load(golden_dir, "free_fit_small.npz")
    m = fixture_inputs(fx)
    a, _, n_nodes, n_seen, num, real_rows, syn_b = (int(v) for v in fx["dims"][:7])
    tol = 4 * float(fx["err32"])
    te = np.arange(n_seen, n_nodes)
    syn = np.concatenate([free.generator_host(m["sd_g"], m["z"][i], np.repeat(m["att"][[c]], num, 0)).numpy() for i, c in enumerate(te)], 0)
    syn_label = np.repeat(te, num)
    st = free.fit_state_host({"fc.weight": m["w0"], "fc.bias": np.zeros(n_nodes, np.float32)})
    cols = fx["cols"]
    for i in range(2):
        idx = fx["index"][i]
        x = np.concatenate((m["real"][i % 2], syn[idx]), 0)
        y = np.concatenate((m["labels"][i % 2], syn_label[idx]))
        big = free.features_host(m["sd_fr"], x, free.synth_rows(m["seed"], f"free.eps.fit.{i}", real_rows + syn_b, a))
        loss, g, _ = free.fit_step_host(st, big, y)
        assert abs(float(loss) - fx["losses64"][i]) / fx["losses64"][i] <= tol and rel(g["fc.bias"].numpy(), fx["gb64"][i]) <= tol
        if i == 0:
            assert rel(g["fc.weight"].numpy()[:, cols], fx["gw1_64"]) <= tol
    keep = fx["gmin"] >= float(fx["gfloor"])
    moved = st["sd"]["fc.weight"].numpy()[:, cols] - m["w0"][:, cols]
    moved64 = fx["w_final64"] - m["w0"][:, cols].astype(np.float64)
    assert 1.0 - keep.mean() <= 0.02
    assert np.abs(moved - moved64)[keep].max() / np.abs(moved64).max() <= 4 * float(fx["err32_w"])


def test_next_batch_indices_match_the_reference_including_the_wrap(golden_dir):
    free = _free()
    fx = load(golden_dir, "free_fit_small.npz")
    ntrain = int(fx["perms"].shape[1])
    perms = iter(fx["perms"])
    b = free.SynBatcher(ntrain, perm=lambda n: torch.from_numpy(next(perms).astype(np.int64)))
    syn_b = int(fx["dims"][6])
    assert ntrain % syn_b != 0
    for i, want in enumerate(fx["index"]):
        assert np.array_equal(b.next(syn_b).numpy(), want), f"call {i}"
        assert b.epochs_completed == (1 if i >= 2 else 0), "the third call wraps"
    assert b.index_in_epoch == len(fx["index"]) * syn_b - ntrain
    # the default source: torch.randperm on a host generator; every call a permutation slice, reproducible by seed
    one, two = free.SynBatcher(2100, seed=3), free.SynBatcher(2100, seed=3)
    got = [one.next(1000) for _ in range(5)]
    assert all(torch.equal(g, two.next(1000)) for g in got) and all(g.numel() == 1000 for g in got)
    assert torch.equal(torch.sort(torch.cat(got[:2] + [got[2][:100]]))[0], torch.arange(2100))


def test_normal_host_moments():
    free = _free()
    n = 1 << 20
    z = free.normal_host(7, 0, 0, 1024, 1024)
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert np.array_equal(free.normal_host(7, 0, 5, 3, 8), free.normal_host(7, 0, 0, 8, 8)[5:]) and not np.array_equal(z[:8, :8], free.normal_host(7, 1, 0, 8, 8))


def test_abi_rejects_bad_arguments_before_any_launch():
    """K not a multiple of 64 is refused by the products' own check (free.product); the entry points refuse ld < n, misaligned
    leading dimensions and null pointers with HGR_EINVAL and a message."""
    from hgr_net_amd import _lib
    free = _free()
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    p = p + (-p) % 16
    bad = []
    bad.append(lib.hgr_nll_rows16(p, 8, p, 2, 9, p, None, 0, None, 0, 0, None))                 # ld < n
    bad.append(lib.hgr_nll_rows16(p, 12, p, 2, 9, p, None, 0, None, 0, 0, None))                # ld not a multiple of 8
    bad.append(lib.hgr_nll_rows16(None, 16, p, 2, 9, p, None, 0, None, 0, 0, None))             # null logits
    bad.append(lib.hgr_nll_rows16(p, 16, p, 2, 9, None, p, 8, None, 0, 0, None))                # ld_d < ld
    bad.append(lib.hgr_nll_rows16(p, 16, None, 2, 9, p, None, 0, None, 0, 0, None))             # a loss without labels
    bad.append(lib.hgr_bias_act_rows(p, 8, p, p, 12, 0, 0, 0, 2, 8, None))                      # ld_y not a multiple of 8
    bad.append(lib.hgr_bias_act_rows(p, 8, None, p, 16, 0, 0, 0, 2, 8, None))                   # null bias
    bad.append(lib.hgr_bias_act_rows(p, 8, p, p, 16, 0, 0, 0, 2, 12, None))                     # C not a multiple of 8
    bad.append(lib.hgr_bias_act_rows(p, 8, p, p, 16, 16, 0, 0, 2, 8, None))                     # col0 + C > ld_y
    bad.append(lib.hgr_bias_act_rows(p, 8, p, p, 16, 0, 3, 0, 2, 8, None))                      # unknown out_type
    bad.append(lib.hgr_free_fr_tail(p, 8, None, None, 0, p, 16, 0, 0, None, 0, 2, 8, 0, 0, 0, None))      # ld_l < 2A
    bad.append(lib.hgr_free_fr_tail(None, 16, None, None, 0, p, 16, 0, 0, None, 0, 2, 8, 0, 0, 0, None))  # null lantent
    bad.append(lib.hgr_free_gen_input(p, 16, 0, None, 0, p, 8, 4, p, 2, 3, 7, 8, 8, 0, 0, 0, None))       # 7 rows out of 2 x 3
    bad.append(lib.hgr_free_gen_input(p, 12, 0, None, 0, p, 8, 4, p, 2, 3, 6, 8, 8, 0, 0, 0, None))       # ld_out < nz + A
    bad.append(lib.hgr_free_gen_input(p, 16, 0, None, 0, None, 8, 4, p, 2, 3, 6, 8, 8, 0, 0, 0, None))    # null attribute table
    bad.append(lib.hgr_adam_l2_cast16(p, p, 6, 2, 1.0, p, p, p, 8, 1e-3, 0.5, 0.999, 1e-8, 0.0, 1, 0, None))   # slice_stride < n
    bad.append(lib.hgr_adam_l2_cast16(p, p, 8, 1, 1.0, p, p, p, 6, 1e-3, 0.5, 0.999, 1e-8, 0.0, 1, 0, None))   # n not a multiple of 4
    bad.append(lib.hgr_adam_l2_cast16(p, p + 4, 8, 1, 1.0, p, p, p, 8, 1e-3, 0.5, 0.999, 1e-8, 0.0, 1, 0, None))  # misaligned gradient
    bad.append(lib.hgr_normal_counter(p, 6, None, 2, 8, 0, 0, 0, None))                         # ld_z < C
    assert bad == [-1] * len(bad), bad                                                          # HGR_EINVAL
    assert b"hgr_normal_counter" in lib.hgr_last_error()
    layer = torch.nn.Linear(100, 8)
    with pytest.raises(ValueError, match="multiple of 64"):
        free.product(torch.zeros(2, 100), layer, "bf16")


def test_cli_parses_and_refuses_to_run_without_a_device(monkeypatch):
    from hgr_net_amd.baseline import validate_free
    args = validate_free.parse_args(["--load_G", "g.pth", "--load_F", "f.pth", "--attributes", "a.npz", "--features", "f.npz", "--attSize", "1024",
                                     "--resSize", "2048", "--ngh", "4096", "--latensize", "2048", "--classifier_lr", "0.002", "--syn_num", "50",
                                     "--manualSeed", "9", "--batch_size", "256", "--graph", "g.json", "--splits", "s.json", "--epochs", "3",
                                     "--dtype", "f16", "--seed", "4", "--save-cls", "cls_1024"])
    assert (args.classifier_lr, args.syn_num, args.manualSeed, args.batch_size, args.epochs, args.dtype, args.save_cls) == (0.002, 50, 9, 256, 3, "f16", "cls_1024")
    assert validate_free.parse_args(["--synthetic", "300"]).synthetic == 300
    for bad in ([], ["--synthetic", "50"], ["--synthetic", "300", "--dtype", "fp32"]):
        with pytest.raises(SystemExit):
            validate_free.parse_args(bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs the GPU: the product path has no CPU fallback"):
        validate_free.main(["--synthetic", "300"])
