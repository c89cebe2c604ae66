"""GPU: the folded-LayerNorm and non-linear forms of the NT GEMM family against float64, on every route of tests/test_gemm_fold_host.py's
case table, both types.  Cases, inputs, references and bounds are that file's (its head derives every coefficient); the references are
evaluated in float64 on the device and EVERY element is compared - no sampling, no excluded share.  Every operand and output lies
between NaN guard bands (the two patterns of tests/test_gpu_row_kernels.py: one for pure inputs, one for what a kernel writes), the
statistics buffers hold exactly M * slots * 2 floats between theirs.  Each test first captures the plan of its own device call and
asserts the route the case was written for.

Time on the MI355X: the 90 tests of this file take 5 s together, the largest (p8 4096^2, tail 4252 x 4096, persist 25600 x 768) 0.1 - 0.3 s
each; the whole GPU suite takes 370 s with them (2244 tests), 365 s without (2154)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import _lib, ops

import test_gemm_fold_host as H
from test_gemm_fold_host import BF16, F16, DTS, TAG, EPS_SET, EPI_GELU, EPI_QGRAD, case_id, check_plan, knobs, seed_of, want_of
from test_gpu_row_kernels import _Band, _in, _same

DEV = "cuda"
F32 = torch.float32
BIG = 4 << 20                                # outputs beyond this many elements get fewer calls per test (the p8, tail and persist cases)
_worst = {}


def _within(got, ref64, bound, what=""):
    """test_attention_host.within on the device: |got - ref64| <= bound for every element, no non-finite output; the worst ratio."""
    assert got.shape == ref64.shape == bound.shape, (what, got.shape, ref64.shape, bound.shape)
    assert bool(torch.isfinite(got.float()).all()), (what, "non-finite output")
    worst = float(((got.double() - ref64).abs() / bound.clamp_min(1e-300)).max()) if got.numel() else 0.0
    assert worst <= 1.0, (what, "error / bound = %.3g" % worst)
    return worst


def _note(form, dt, value):
    key = (form, TAG[dt])
    _worst[key] = max(_worst.get(key, 0.0), value)
    print("worst error / bound:", "%s %s" % key, round(_worst[key], 3))


def _out(shape, dtype):
    return _Band(shape=shape, dtype=dtype)


def _dev(d, *names):
    return [d[n].to(DEV) for n in names]


def _row_stats(x32, dt):
    """hgr_row_stats16 into guard bands: the pair is the reference encoder's, the statistics inside their bound; (x16, xlo, stats) bands."""
    m, k = x32.shape
    X16, XLO, ST = _out((m, k), dt), _out((m, k), ops.PAIR_LO), _out((m, k // 64 * 2), F32)
    ops.row_stats16(_in(x32), X16.t, XLO.t, ST.t)
    rh, rl = H.pair_encode(x32, dt)
    assert _same(X16.t, rh) and _same(XLO.t, rl) and X16.intact() and XLO.intact() and ST.intact()
    sref, sbound = H.stats_bound(x32.double())
    _note("row_stats16", dt, _within(ST.t.view(m, k // 64, 2), sref, sbound, "row_stats16"))
    return X16, XLO, ST


# ---- hgr_gemm_nt_ln -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("cs", H.ALL_CONSUMER, ids=case_id)
def test_gemm_nt_ln_vs_float64(dt, cs):
    """Planted rows (eps 1e-5 and 1e-3: a kernel that ignores eps is off by 2 % on the sigma = 2^-6 rows) and random rows at scales 1 and
    3, both `act` values, against the kernel's own formula in float64; the random rows also against a float64 LayerNorm -> Linear."""
    m, n, k = cs.m, cs.n, cs.k
    big = m * n > BIG
    pl = H.plant_consumer(m, n, k, seed_of(cs))
    x, w, s, c, stats, sw, sigma = _dev(pl, "x", "w", "s", "c", "stats", "sw", "sigma")
    x16, w16, sv, cv, st = _in(x.to(dt)), _in(w.to(dt)), _in(s), _in(c), _in(stats.view(m, -1))
    with knobs(cs):
        for act in (0, 1):
            C = _out((m, n), dt)
            check_plan(want_of(cs, "consumer", act), lambda: ops.gemm_nt_ln(x16, w16, C.t, sv, cv, st, 1e-5, quickgelu=bool(act)))
        for eps, act in (((1e-5, 0), (1e-3, 1)) if big else [(e, a) for e in EPS_SET for a in (0, 1)]):
            C = _out((m, n), dt)
            ops.gemm_nt_ln(x16, w16, C.t, sv, cv, st, eps, quickgelu=bool(act))
            assert C.intact(), (case_id(cs), "planted", eps, act)
            ref, bound = H.consumer_ref(x16, w16, sv, cv, st, eps, act, dt)
            exact = sigma[:, None] * sw / torch.sqrt(sigma ** 2 + eps)[:, None] + c.double()
            exact = H.qgelu64(exact) if act else exact
            assert float((ref - exact).abs().max()) <= 1e-9 * max(1.0, float(exact.abs().max()))
            _note("ln planted %s act%d" % (cs.name, act), dt, _within(C.t, exact, bound, (case_id(cs), "planted", eps, act)))
        for scale, acts in (((1.0, (1,)), (3.0, (0,))) if big else ((1.0, (0, 1)), (3.0, (0, 1)))):
            rd = H.rand_consumer(m, n, k, scale, dt, seed_of(cs) + int(scale))
            x32, w16, s, c = _dev(rd, "x", "w", "s", "c")
            X16, _, ST = _row_stats(x32, dt)
            w16, sv, cv = _in(w16), _in(s), _in(c)
            for act in acts:
                C = _out((m, n), dt)
                ops.gemm_nt_ln(X16.t, w16, C.t, sv, cv, ST.t, 1e-5, quickgelu=bool(act))
                assert C.intact() and X16.intact() and ST.intact(), (case_id(cs), "random", scale, act)
                ref, bound = H.consumer_ref(X16.t, w16, sv, cv, ST.t, 1e-5, act, dt)
                _note("ln random %s act%d" % (cs.name, act), dt, _within(C.t, ref, bound, (case_id(cs), "random", scale, act)))
                ref2, extra = H.layernorm_ref(x32, X16.t, w16, sv, cv, 1e-5, act, dt)
                _note("ln vs LayerNorm %s act%d" % (cs.name, act), dt, _within(C.t, ref2, bound + extra, (case_id(cs), "layernorm", scale, act)))


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("b,l,heads,causal", H.LN_MHA_CASES)
def test_gemm_nt_ln_mha_consumer_half_vs_float64(dt, b, l, heads, causal):
    """hgr_gemm_nt_ln_mha = hgr_gemm_nt_ln into q | k | v + hgr_mha, bit for bit (the link, repeated here on this data); q | k | v
    against the consumer's float64 bound.  The attention half has its own in tests/test_gpu_attention.py."""
    wd, m = heads * 64, b * l
    rd = H.rand_consumer(m, 3 * wd, wd, 1.0, dt, 97 * m + wd)
    x32, w16, s, c = _dev(rd, "x", "w", "s", "c")
    w16 = (w16.float() * (wd ** -0.5 / 0.05)).to(dt)                       # scores of the order of 1
    s = w16.float().sum(1)
    X16, _, ST = _row_stats(x32, dt)
    w16, sv, cv = _in(w16), _in(s), _in(c)
    QKV, ATT, TWO = _out((m, 3 * wd), dt), _out((m, wd), dt), _out((m, wd), dt)
    ops.gemm_nt_ln(X16.t, w16, QKV.t, sv, cv, ST.t, 1e-5)
    ref, bound = H.consumer_ref(X16.t, w16, sv, cv, ST.t, 1e-5, 0, dt)
    _note("ln_mha q|k|v", dt, _within(QKV.t, ref, bound, ("qkv", b, l, heads)))
    ops.gemm_nt_ln_mha(X16.t, w16, ATT.t, sv, cv, ST.t, b, l, heads, causal, 1e-5)
    ops.mha(QKV.t, TWO.t, b, l, heads, causal)
    assert _same(ATT.t, TWO.t) and ATT.intact() and QKV.intact() and TWO.intact()


# ---- the residual producers ---------------------------------------------------------------------------------------------------------------
def _producer(cs, dt, call, scales):
    m, n, k = cs.m, cs.n, cs.k
    pl = H.plant_producer(m, n, k, seed_of(cs))
    a, w, bias, old, new = _dev(pl, "a", "w", "bias", "old", "new")
    oh, ol = H.pair_encode(old, dt)
    A, W, bv = _in(a.to(dt)), _in(w.to(dt)), _in(bias)
    XH, XL, ST = _Band(oh), _Band(ol), _out((m, n // 64 * 2), F32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    call(A, W, XH.t, XL.t, bv, ST.t, flag)
    rh, rl = H.pair_encode(new, dt)
    assert XH.intact() and XL.intact() and ST.intact() and int(flag) == 0
    assert torch.equal(ops.pair_value(XH.t, XL.t), new), "the decoded pair is the integer"
    assert _same(XH.t, rh) and _same(XL.t, rl)
    assert torch.equal(ST.t.view(m, n // 64, 2).double(), H.slot_stats64(new)), "both statistics are exact integers"
    for scale in scales:
        rd = H.rand_producer(m, n, k, scale, dt, seed_of(cs) + int(scale))
        a16, w16, bias, old = _dev(rd, "a", "w", "bias", "old")
        oh, ol = H.pair_encode(old, dt)
        old = ops.pair_value(oh, ol)
        assert torch.equal(old, H.pair_decode(oh, ol, dt))                 # the kernels' decoder and the host file's agree
        A, W, bv = _in(a16), _in(w16), _in(bias)
        XH, XL, ST = _Band(oh), _Band(ol), _out((m, n // 64 * 2), F32)
        flag.zero_()
        call(A, W, XH.t, XL.t, bv, ST.t, flag)
        assert XH.intact() and XL.intact() and ST.intact() and int(flag) == 0
        v, b_v = H.producer_ref(a16, w16, bias, old, dt)
        worst, near = H.check_pair(XH.t, XL.t, v, b_v, dt, (case_id(cs), scale), within=_within)
        _note("res_stats pair %s" % cs.name, dt, worst)
        sref, sbound = H.stats_bound(v, b_v)
        _note("res_stats statistics %s" % cs.name, dt, _within(ST.t.view(m, n // 64, 2), sref, sbound, (case_id(cs), "stats", scale)))
        _note("res_stats statistics vs own pair %s" % cs.name, dt, H.check_stats_self(XH.t, XL.t, ST.t, dt, (case_id(cs), scale), within=_within))


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("cs", H.PRODUCER_CASES, ids=case_id)
def test_gemm_nt_res_stats_guard_vs_float64(dt, cs):
    """hgr_gemm_nt_res_stats_guard (hgr_gemm_nt_res_stats is the same launch without the flag): planted integers - pair and statistics
    exact - and random operands inside the accumulation bound; the flag stays 0."""
    call = lambda a, w, xh, xl, bias, st, flag: ops.gemm_nt_res_stats(a, w, xh, xl, bias, st.view(cs.m, -1, 2), flag=flag)
    with knobs(cs):
        pl = H.plant_producer(cs.m, cs.n, cs.k, seed_of(cs))
        a, w, bias, old = _dev(pl, "a", "w", "bias", "old")
        oh, ol = H.pair_encode(old, dt)
        st, flag = torch.empty(cs.m, cs.n // 64, 2, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        check_plan(cs, lambda: ops.gemm_nt_res_stats(a.to(dt), w.to(dt), oh, ol, bias, st, flag=flag))
        _producer(cs, dt, call, (1.0,) if cs.m * cs.n > BIG else (1.0, 3.0))


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
def test_gemm_nt_res_stats_wide_vs_float64(dt):
    cs = H.WIDE_CASE
    assert ops.gemm_nt_res_stats_wide_ok(cs.m, cs.n, cs.k, cs.k, cs.k, cs.n, dt)
    before = ops.WIDE_CALLS[0]
    _producer(cs, dt, lambda a, w, xh, xl, bias, st, flag: ops.gemm_nt_res_stats_wide(a, w, xh, xl, bias, st.view(cs.m, -1, 2), flag=flag), (1.0, 3.0))
    assert ops.WIDE_CALLS[0] == before + 3


# ---- hgr_row_stats16, hgr_vit_embed_ln_stats --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", H.ROW_STATS_SHAPES)
def test_row_stats16_vs_float64(dt, shape):
    m, w = shape
    for scale in (1.0, 3.0):
        x = H.rand_rows(m, w, scale, 17 * m + w).to(DEV)
        X16, XLO, _ = _row_stats(x, dt)
        _note("row_stats16 pair", dt, _within(ops.pair_value(X16.t, XLO.t), x.double(), H.pair_step(x.double(), dt), (shape, "pair", scale)))


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("b,g,w", H.EMBED_SHAPES)
def test_vit_embed_ln_stats_vs_float64(dt, b, g, w):
    """The pair is the reference encoder's of hgr_vit_embed_ln's fp32 rows (exact, as tests/test_gpu_kernels.py asserts), the slot
    statistics of those rows inside the statistics bound."""
    gen = H._gen(b + g + w)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
    pe, cls, pos = rnd(b * g, w), rnd(w), rnd(g + 1, w)
    gamma, beta = 1.0 + 0.1 * rnd(w), 0.1 * rnd(w)
    rows = b * (g + 1)
    x1 = torch.empty(rows, w, device=DEV)
    ops.vit_embed_ln(pe, cls, pos, gamma, beta, x1, b, g)
    XH, XL, ST = _out((rows, w), dt), _out((rows, w), ops.PAIR_LO), _out((rows, w // 64 * 2), F32)
    ops.vit_embed_ln_stats(_in(pe), _in(cls), _in(pos), _in(gamma), _in(beta), XH.t, XL.t, ST.t, b, g)
    rh, rl = H.pair_encode(x1, dt)
    assert _same(XH.t, rh) and _same(XL.t, rl) and XH.intact() and XL.intact() and ST.intact()
    sref, sbound = H.stats_bound(x1.double())
    _note("vit_embed_ln_stats", dt, _within(ST.t.view(rows, w // 64, 2), sref, sbound, (b, g, w)))


# ---- hgr_gemm_nt's non-linear epilogues, the dual-output forward, the gradient with column sums -------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("cs", H.NT_CASES, ids=case_id)
def test_gemm_nt_nonlinear_epilogues_vs_float64(dt, cs):
    m, n, k = cs.m, cs.n, cs.k
    with knobs(cs):
        for scale in (1.0, 3.0):
            rd = H.rand_nt(m, n, k, scale, dt, seed_of(cs) + int(scale))
            a, w, bias, pre = (_in(t) for t in _dev(rd, "a", "w", "bias", "pre"))
            for epi, form in ((EPI_GELU, "BIAS_QUICKGELU"), (EPI_QGRAD, "QGELU_GRAD16")):
                C = _out((m, n), dt)
                call = lambda: ops.gemm_nt(a, w, C.t, bias=bias if epi == EPI_GELU else None, residual=pre if epi == EPI_QGRAD else None, epilogue=epi)
                check_plan(want_of(cs, "nt", epi=epi), call)
                call()
                assert C.intact(), (case_id(cs), form)
                ref, bound = H.nt_ref(a, w, bias, pre, epi, dt)
                _note("gemm_nt %s %s" % (form, cs.name), dt, _within(C.t, ref, bound, (case_id(cs), form, scale)))


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("cs", H.DUAL_CASES, ids=case_id)
def test_gemm_nt_bias_gelu_dual_vs_float64(dt, cs):
    m, n, k = cs.m, cs.n, cs.k
    with knobs(cs):
        for scale in ((1.0,) if m * n > BIG else (1.0, 3.0)):
            rd = H.rand_nt(m, n, k, scale, dt, seed_of(cs) + int(scale))
            a, w, bias = (_in(t) for t in _dev(rd, "a", "w", "bias"))
            PRE, POST = _out((m, n), dt), _out((m, n), dt)
            call = lambda: ops.gemm_nt_bias_gelu_dual(a, w, PRE.t, POST.t, bias)
            check_plan(cs, call)
            call()
            assert PRE.intact() and POST.intact()
            pref, bpre, qref, bpost = H.dual_ref(a, w, bias, PRE.t, dt)
            _note("bias_gelu_dual pre %s" % cs.name, dt, _within(PRE.t, pref, bpre, (case_id(cs), "pre", scale)))
            _note("bias_gelu_dual post %s" % cs.name, dt, _within(POST.t, qref, bpost, (case_id(cs), "post", scale)))


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("cs", H.COLSUM_CASES, ids=case_id)
def test_gemm_nt_qgelu_grad_colsum_vs_float64(dt, cs):
    m, n, k = cs.m, cs.n, cs.k
    units = (m + 63) // 64
    with knobs(cs):
        for scale in ((1.0,) if m * n > BIG else (1.0, 3.0)):
            rd = H.rand_nt(m, n, k, scale, dt, seed_of(cs) + int(scale))
            a, w, pre = (_in(t) for t in _dev(rd, "a", "w", "pre"))
            C, PART = _out((m, n), dt), _out((units, n), F32)
            call = lambda: ops.gemm_nt_qgelu_grad_colsum(a, w, C.t, pre, PART.t)
            check_plan(cs, call)
            call()
            assert C.intact() and PART.intact()
            ref, bound = H.nt_ref(a, w, None, pre, EPI_QGRAD, dt)
            _note("qgelu_grad_colsum dx %s" % cs.name, dt, _within(C.t, ref, bound, (case_id(cs), "dx", scale)))
            cref, cbound = H.colsum_ref(C.t)
            _note("qgelu_grad_colsum sums %s" % cs.name, dt, _within(PART.t, cref, cbound, (case_id(cs), "sums", scale)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
def test_fold_entry_points_refuse_and_write_nothing(dt):
    """K % 128 != 0 and act outside {0, 1} (hgr_gemm_nt_ln), a guard flag with guard_sumsq <= 0 (both producers): an error, and every
    output - all of it poison before the call - keeps its bits."""
    m, n = 300, 128
    dtc = ops.DT_OF[dt]
    for k, act, text in ((192, 0, "multiple of 128"), (320, 1, "multiple of 128"), (256, 2, "act must be 0"), (256, -1, "act must be 0")):
        x, w, s, c, st = _in(torch.ones(m, k, dtype=dt, device=DEV)), _in(torch.ones(n, k, dtype=dt, device=DEV)), _in(torch.ones(n, device=DEV)), \
            _in(torch.ones(n, device=DEV)), _in(torch.ones(m, k // 64 * 2, device=DEV))
        C = _out((m, n), dt)
        with pytest.raises(_lib.HgrError, match=text):
            _lib.call("hgr_gemm_nt_ln", x.data_ptr(), k, w.data_ptr(), k, C.t.data_ptr(), n, s.data_ptr(), c.data_ptr(), st.data_ptr(), 1e-5, m, n, k, dtc, act,
                      ops._stream())
        torch.cuda.synchronize()
        assert C.intact() and bool((C.t.view(torch.int16) == C.poison).all())
    for name, (m, n, k) in (("hgr_gemm_nt_res_stats_guard", (300, 128, 128)), ("hgr_gemm_nt_res_stats_wide", (640, 512, 256))):
        for guard in (0.0, -1.0):
            a, w, bias = _in(torch.ones(m, k, dtype=dt, device=DEV)), _in(torch.ones(n, k, dtype=dt, device=DEV)), _in(torch.ones(n, device=DEV))
            XH, XL, ST = _out((m, n), dt), _out((m, n), ops.PAIR_LO), _out((m, n // 64 * 2), F32)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            with pytest.raises(_lib.HgrError, match="guard_sumsq > 0"):
                _lib.call(name, a.data_ptr(), k, w.data_ptr(), k, XH.t.data_ptr(), XL.t.data_ptr(), n, bias.data_ptr(), ST.t.data_ptr(), guard, flag.data_ptr(),
                          m, n, k, dtc, ops._stream())
            torch.cuda.synchronize()
            assert XH.intact() and XL.intact() and ST.intact() and int(flag) == 0
            assert bool((XH.t.view(torch.int16) == XH.poison).all()) and bool((XL.t == XL.poison).all()) and bool((ST.t.view(torch.int32) == ST.poison).all())
