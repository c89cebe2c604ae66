"""CPU: the inputs, float64 references and error bounds that tests/test_gpu_attention.py holds the attention kernels to (hgr_mha,
hgr_mha_rows, hgr_mha_stats, hgr_mha_bwd*, hgr_attnpool_attend), tested here against an fp32 emulation of the kernels' arithmetic - a
wrong bound or an unsound planted input is found without a device, and three deliberately broken emulations show that the checks bite.
The backward entry points' argument checks (alignment, grid size) return before any launch and are tested here too.

Planted one-hot attention.  k[b,h,j] = 8 c_j with c_j in {+-1}^64, q[b,h,i] = 8 c_pi(i): the scaled target score is 8 * 8 * 64 / 8 = 512,
every other one 8 (c_i . c_j) <= 320 (`MARGIN`: the builder asserts max c_i . c_j <= 40 for the draw it keeps).  A scaled gap >= 192 is
an exp2 argument <= -277: every off-target exponential is exactly 0 in fp32, the softmax is exactly one-hot, and out[i] == v[pi(i)] bit
for bit, stats == (512, 1), dQ == dK == 0, dV[j] == the integer sum of dO[i] over pi(i) = j rounded once.  V holds integers in
[-128, 128] (exact in both types) and its rows are pairwise distinct over the whole tensor, so a row read from the wrong key, head or
sequence is another row.  A forward that exponentiates before it subtracts the row maximum overflows at 512.

Planted uniform attention.  All keys of a (b, h) are 8 c and all queries -8 c: every live score is -512 and p = 1 / n over the allowed
keys.  A zero-filled padding key or a key beyond the causal limit that is NOT masked scores 0 and takes the whole softmax.

Float64 references restate each kernel's own formula from the input bits:
    forward, attnpool_attend     softmax(q k^T / 8 [+ mask]) v
    backward, every L            P from the same softmax; dP = dO V^T; dS = P (dP - D) / 8; dV = P^T dO; dK = dS^T Q; dQ = dS K
    D, 32 < L <= 320             mha_bwd_tiled: D = rowsum(dO * O_given), O_given = the ROUNDED forward output the caller passes in
    D, L <= 32                   mha_bwd_wave:  D = rowsum(P * dP); this kernel never reads `out`
(csrc/hgr_train.hip; `definition_of_d(L)` below is that switch.)

Error bound, element-wise.  One round-to-nearest of x to the 16-bit type errs by at most r(x) = max(u |x|, t), u = 2^-8 / 2^-11 and
t = 2^-134 / 2^-25 for bf16 / f16.  The kernels round P (and dS) once before the second products, accumulate in fp32 and round the
result once:
    bound = half_ulp16(ref) + sum_j r(x_ij) |y_jd| + 2^-14 * A32
x = p (forward, dV) or dS (dQ, dK), y the other operand; A32 = the same abs-sum with |x|, for dQ / dK with
P (|dO| |V|^T + rowsum |dO| |O|) / 8 in place of |dS| (the cancellation in dP - D is done in fp32).  Every 16-bit term has coefficient 1
per rounding; only the fp32 allowance 2^-14 could ever grow, and only for a named instruction.  attnpool_attend keeps P in fp32:
its bound is half_ulp16(ref) + 2^-14 * A32.

Worst error / bound over the cases each test runs (CPU: the fp32 emulation below, L in {33, 77, 257, 320} x scale {1, 3, 5}, both
definitions of D; MI355X: tests/test_gpu_attention.py, every length it lists, scales 1 and 3):

    kernel             CPU bf16  CPU f16   MI355X bf16  MI355X f16
    forward            0.885     0.830     0.908        0.853
    backward dQ        0.887     0.667     0.918        0.672
    backward dK        0.928     0.742     0.951        0.741
    backward dV        0.978     0.876     0.988        0.910
    attnpool_attend    0.980     0.869     0.979        0.887
No ratio exceeds 1 with the coefficients above: the fp32 allowance stayed at 2^-14.  (The 16-bit terms are tight by construction - a
result that lands on a rounding tie of the type is at ratio ~ 1 - so values near 1 are expected, not a sign of a loose kernel.)
"""
import numpy as np
import pytest
import torch

from hgr_net_amd import synth

BF16, F16 = torch.bfloat16, torch.float16
DTS = [BF16, F16]
U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}               # one rounding, relative
TINY = {BF16: 2.0 ** -134, F16: 2.0 ** -25}          # ... and in the subnormal range
F32_ALLOW = 2.0 ** -14                               # the fp32 arithmetic: exp2 / __expf, the reciprocal, the accumulation order
MARGIN = 40                                          # max c_i . c_j of a planted code set
LOG2E = float(np.float32(1.4426950408889634))

FWD_LENGTHS = [1, 7, 16, 32, 33, 50, 64, 65, 77, 96, 97, 160, 161, 257, 288]
BWD_LENGTHS = [1, 5, 31, 32, 33, 63, 64, 65, 128, 129, 192, 193, 256, 257, 288, 289, 320]
POOL_LENGTHS = [1, 63, 64, 65, 128, 129, 192, 193, 256]
SHAPES = [(3, 3), (1, 12)]                           # (b, heads) the GPU file uses


def definition_of_d(L):
    """Which D the backward at this length forms: mha_bwd_wave (L <= 32) rowsum(P * dP), mha_bwd_tiled rowsum(dO * O_given)."""
    return "wave" if L <= 32 else "tiled"


# ---- layout: [b * L, heads * 64] rows <-> [b, heads, L, 64] ---------------------------------------------------------------------------
def split_heads(x, b, L, heads):
    return x.reshape(b, L, heads, 64).permute(0, 2, 1, 3)


def merge_heads(x):
    b, heads, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * L, heads * 64)


def pack_qkv(q, k, v):
    return torch.cat([merge_heads(q), merge_heads(k), merge_heads(v)], dim=1).contiguous()


def unpack_qkv(qkv, b, L, heads):
    w = heads * 64
    return tuple(split_heads(qkv[:, i * w:(i + 1) * w], b, L, heads) for i in range(3))


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def half_ulp16(ref64, dt):
    """Half a unit in the last place of the 16-bit type at |ref64| (tests/test_gpu_row_kernels.py::_half_ulp)."""
    mant, emin = (7, -126) if dt == BF16 else (10, -14)
    _, e = torch.frexp(ref64.abs().double())
    return torch.pow(2.0, (e.double() - 1).clamp_min(emin) - mant - 1)


def r16(x64, dt):
    """The error of one round-to-nearest of x to the 16-bit type, at most."""
    return (U[dt] * x64.abs()).clamp_min(TINY[dt])


def ratio(got, ref64, bound):
    got = got.double().cpu()
    assert got.shape == ref64.shape == bound.shape, (got.shape, ref64.shape, bound.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float(((got - ref64).abs() / bound.clamp_min(1e-300)).max()) if got.numel() else 0.0


def within(got, ref64, bound, what=""):
    """|got - ref64| <= bound element-wise; returns the worst ratio (and reports it when it fails)."""
    worst = ratio(got, ref64, bound)
    assert worst <= 1.0, (what, "error / bound = %.3g" % worst)
    return worst


# ---- planted inputs ------------------------------------------------------------------------------------------------------------------
def codes(L, seed):
    """c [L, 64] in {+-1}, max_{i != j} c_i . c_j <= MARGIN (asserted; a draw that misses it is replaced by the next seed's)."""
    worst = -64.0
    for attempt in range(16):
        u = synth.uniform(seed + 104729 * attempt, "attn.code", L * 64)
        c = np.where(u < 0.5, -1.0, 1.0).reshape(L, 64)
        g = c @ c.T
        np.fill_diagonal(g, -64.0)
        worst = float(g.max())
        if worst <= MARGIN:
            break
    assert worst <= MARGIN, (L, seed, worst)
    return torch.from_numpy(c), worst


def edge_keys(L):
    """Keys at which the kernels' bookkeeping changes: 0, 15/16, 31/32, 63/64, the last key of every 16-key accumulator tile, L - 1."""
    return sorted({e for e in [0, 15, 16, 31, 32, 63, 64, L - 1] + list(range(15, L, 16)) if 0 <= e < L})


def plant_pi(L, causal, bh):
    """The key every query attends to, for (batch, head) number bh: a pseudo-random remainder, every edge key from some other query,
    a many-to-one target, and last every edge key once more (on the diagonal under the causal mask: the last key the mask allows)."""
    i = np.arange(L)
    u = synth.uniform(1000 + bh, "attn.pi", L)
    pi = np.floor(u * (i + 1 if causal else L)).astype(np.int64)
    edges = edge_keys(L)
    for n, e in enumerate(edges):
        span = L - e if causal else L
        pi[(e if causal else 0) + (7 * n + 3 * bh + 1) % span] = e
    star = edges[bh % len(edges)]
    pi[(i % 7 == bh % 7) & ((i >= star) | (not causal))] = star
    for e in edges:
        pi[e if causal else (e + bh + 1) % L] = e
    assert pi.min() >= 0 and pi.max() < L and (not causal or bool((pi <= i).all()))
    return torch.from_numpy(pi)


def plant_v(b, L, heads, seed):
    """Integers in [-128, 128], float64 [b, heads, L, 64]; columns 0 .. 2 encode (key % 16, key // 16, b * heads + h): no two rows of
    the whole tensor are equal."""
    v = torch.from_numpy(synth.randint(seed, "attn.v", b * heads * L * 64, -128, 129).astype(np.float64)).view(b, heads, L, 64).clone()
    j = torch.arange(L, dtype=torch.float64)
    v[..., 0] = (j % 16) * 16 - 128
    v[..., 1] = torch.div(j, 16, rounding_mode="floor") - 64
    v[..., 2] = (torch.arange(b * heads, dtype=torch.float64).view(b, heads, 1) - 64).expand(b, heads, L)
    assert float(v.abs().max()) <= 128
    return v


def plant_dout(b, L, heads, seed):
    """Integers in [-8, 8], float64 [b, heads, L, 64]."""
    return torch.from_numpy(synth.randint(seed, "attn.do", b * heads * L * 64, -8, 9).astype(np.float64)).view(b, heads, L, 64)


def plant_onehot(b, L, heads, causal, dt, seed=0):
    """qkv [b * L, 3 W] of type dt whose softmax is exactly one-hot at pi; `out` = the expected forward output v[pi], `worst` = the
    largest off-target c_i . c_j over all (b, h)."""
    q, k, pis, worst = [], [], [], -64.0
    for bh in range(b * heads):
        c, w = codes(L, 7 * seed + 131 * L + bh)
        pi = plant_pi(L, causal, bh)
        k.append(8.0 * c)
        q.append(8.0 * c[pi])
        pis.append(pi)
        worst = max(worst, w)
    q, k = torch.stack(q).view(b, heads, L, 64), torch.stack(k).view(b, heads, L, 64)
    pi = torch.stack(pis).view(b, heads, L)
    v = plant_v(b, L, heads, seed + 1)
    want = torch.gather(v, 2, pi[..., None].expand(b, heads, L, 64))
    return dict(qkv=pack_qkv(q, k, v).to(dt), pi=pi, v=v, out=merge_heads(want).to(dt), worst=worst)


def onehot_backward(plant, b, L, heads, dt, seed=0):
    """dout (integers in [-8, 8]) and the expected dqkv for plant_onehot's input with O = v[pi]: dQ = dK = 0, dV[j] = the exact sum of
    dO[i] over pi(i) = j, rounded once."""
    do = plant_dout(b, L, heads, seed + 2)
    dv = torch.zeros(b, heads, L, 64, dtype=torch.float64)
    dv.scatter_add_(2, plant["pi"][..., None].expand(b, heads, L, 64), do)
    z = torch.zeros_like(dv)
    return merge_heads(do).to(dt), pack_qkv(z, z, dv).to(dt)


def plant_uniform(b, L, heads, causal, dt, seed=0):
    """qkv whose live scores are all -512; `ref` (float64 [b * L, W]) = the mean of the allowed V rows, `bound` = one rounding of the
    type plus one fp32 ulp (1 / n and its product with the exact integer sum)."""
    c = torch.stack([codes(1, 50021 * (seed + 1) + 131 * L + bh)[0][0] for bh in range(b * heads)]).view(b, heads, 1, 64)
    k = (8.0 * c).expand(b, heads, L, 64)
    v = plant_v(b, L, heads, seed + 3)
    n = torch.arange(1, L + 1, dtype=torch.float64).view(L, 1)
    mean = v.cumsum(2) / n if causal else (v.sum(2, keepdim=True) / L).expand(b, heads, L, 64)
    ref = merge_heads(mean)
    return dict(qkv=pack_qkv(-k, k, v).to(dt), ref=ref, bound=half_ulp16(ref, dt) + 2.0 ** -23 * ref.abs())


def plant_pool(b, L, heads, dt, uniform, seed=0):
    """hgr_attnpool_attend's operands (q fp32 [b, E], k, v 16-bit [b * L, E]) planted one-hot - the target key of (b, h) walks through
    0, 63, 64, L - 1 - or uniform; `ref` float64 [b, E] (exact for one-hot: bound 0) and `bound`."""
    v = plant_v(b, L, heads, seed + 4)
    q, k, want = [], [], []
    targets = [t for t in (0, 63, 64, L - 1) if t < L]
    for bh in range(b * heads):
        vb = v.view(b * heads, L, 64)[bh]
        if uniform:
            c = codes(1, 9973 * (seed + 1) + 131 * L + bh)[0]
            k.append((8.0 * c).expand(L, 64))
            q.append(-8.0 * c[0])
            want.append(vb.sum(0) / L)
        else:
            c = codes(L, 7 * seed + 131 * L + bh)[0]
            t = targets[bh % len(targets)]
            k.append(8.0 * c)
            q.append(8.0 * c[t])
            want.append(vb[t])
    q = torch.stack(q).view(b, heads * 64).float().contiguous()
    k = merge_heads(torch.stack(k).view(b, heads, L, 64)).to(dt)
    ref = torch.stack(want).view(b, heads * 64)
    bound = half_ulp16(ref, dt) + 2.0 ** -23 * ref.abs() if uniform else torch.zeros_like(ref)
    return dict(q=q, k=k, v=merge_heads(v).to(dt), ref=ref, bound=bound)


def rand_qkv(b, L, heads, scale, dt, seed):
    return torch.from_numpy((scale * synth.normal(seed, "attn.qkv", b * L * 3 * heads * 64)).astype(np.float32)).view(b * L, 3 * heads * 64).to(dt)


def rand_rows(b, L, heads, scale, dt, seed):
    return torch.from_numpy((scale * synth.normal(seed, "attn.do", b * L * heads * 64)).astype(np.float32)).view(b * L, heads * 64).to(dt)


# ---- float64 references from the input bits ---------------------------------------------------------------------------------------------
def _mask(L, causal):
    return torch.ones(L, L, dtype=torch.bool).triu_(1) if causal else torch.zeros(L, L, dtype=torch.bool)


def ref_forward(qkv, b, L, heads, causal):
    """softmax(q k^T / 8 [+ mask]) v in float64: out, p, the scaled scores' row maximum and 1 / sum exp(s - max), all [b, heads, L, ..]."""
    q, k, v = (t.double() for t in unpack_qkv(qkv, b, L, heads))
    s = (q @ k.transpose(-1, -2) / 8).masked_fill(_mask(L, causal), float("-inf"))
    mx = s.max(-1).values
    e = torch.exp(s - mx[..., None])
    den = e.sum(-1)
    p = e / den[..., None]
    return dict(q=q, k=k, v=v, p=p, out=p @ v, mx=mx, inv=1.0 / den,
                mx_bound=2.0 ** -20 * (q.abs() @ k.abs().transpose(-1, -2) / 8).masked_fill(_mask(L, causal), 0.0).max(-1).values)


def bound_forward(f, dt):
    return half_ulp16(f["out"], dt) + r16(f["p"], dt) @ f["v"].abs() + F32_ALLOW * (f["p"] @ f["v"].abs())


def ref_backward(qkv, o_given, dout, b, L, heads, causal, dt, definition=None):
    """dq, dk, dv in float64 [b, heads, L, 64] and their bounds, with the D of `definition` (default: the one the kernel for L uses)."""
    definition = definition or definition_of_d(L)
    f = ref_forward(qkv, b, L, heads, causal)
    q, k, v, p = f["q"], f["k"], f["v"], f["p"]
    do, og = split_heads(dout, b, L, heads).double(), split_heads(o_given, b, L, heads).double()
    dp = do @ v.transpose(-1, -2)
    d = (do * og).sum(-1) if definition == "tiled" else (p * dp).sum(-1)
    ds = p * (dp - d[..., None]) / 8
    a32 = p * (do.abs() @ v.abs().transpose(-1, -2) + (do.abs() * og.abs()).sum(-1)[..., None]) / 8
    t = lambda x: x.transpose(-1, -2)
    ref = dict(dq=ds @ k, dk=t(ds) @ q, dv=t(p) @ do)
    bound = dict(dq=half_ulp16(ref["dq"], dt) + r16(ds, dt) @ k.abs() + F32_ALLOW * (a32 @ k.abs()),
                 dk=half_ulp16(ref["dk"], dt) + t(r16(ds, dt)) @ q.abs() + F32_ALLOW * (t(a32) @ q.abs()),
                 dv=half_ulp16(ref["dv"], dt) + t(r16(p, dt)) @ do.abs() + F32_ALLOW * (t(p) @ do.abs()))
    return ref, bound


def ref_pool(q, k, v, b, L, heads, dt):
    """hgr_attnpool_attend in float64 [b, E] and its bound (P stays fp32 in the kernel: one rounding, the output's)."""
    qh = q.double().view(b, heads, 1, 64)
    kh, vh = split_heads(k, b, L, heads).double(), split_heads(v, b, L, heads).double()
    p = torch.softmax(qh @ kh.transpose(-1, -2) / 8, -1)
    ref = (p @ vh).reshape(b, heads * 64)
    return ref, half_ulp16(ref, dt) + F32_ALLOW * (p @ vh.abs()).reshape(b, heads * 64)


# ---- fp32 emulation of the kernels' arithmetic ---------------------------------------------------------------------------------------------
def emu_forward(qkv, b, L, heads, causal, dt, swap_v=None, drop_last=False, no_max=False):
    """mha_fwd: fp32 scores, exp2 of one FMA, the sum over the unrounded exponentials, P rounded to 16 bit, fp32 products, the output
    rounded once.  swap_v = (i, j): V rows i and j exchanged; drop_last: key L - 1 masked; no_max: no maximum subtracted - the three
    mistakes the tests below must catch.  Returns out [b * L, W] of type dt and stats [b, heads, L, 2]."""
    q, k, v = (t.float() for t in unpack_qkv(qkv, b, L, heads))
    if swap_v:
        v = v.clone()
        v[..., list(swap_v), :] = v[..., list(swap_v)[::-1], :]
    mask = _mask(L, causal)
    if drop_last:
        mask = mask.clone()
        mask[:, L - 1] = True
    s = ((q @ k.transpose(-1, -2)) * 0.125).masked_fill(mask, float("-inf"))
    mx = s.max(-1).values
    nmx = torch.zeros_like(mx) if no_max else -mx * LOG2E
    pe = torch.exp2((s.double() * LOG2E + nmx.double()[..., None]).float())        # one FMA: the product is exact in float64
    inv = 1.0 / pe.sum(-1)
    o = pe.to(dt).float() @ v
    out = (o.double() * inv.double()[..., None]).to(dt)                              # the product rounded ONCE (mul_pack16)
    return merge_heads(out), torch.stack([mx, inv], -1)


def emu_backward(qkv, o_given, dout, b, L, heads, causal, dt, definition):
    """mha_bwd_tiled / mha_bwd_wave: P = exp(s - max) / sum in fp32, D by `definition`, P and dS rounded to 16 bit, fp32 products,
    results rounded once.  Returns dqkv [b * L, 3 W] of type dt."""
    q, k, v = (t.float() for t in unpack_qkv(qkv, b, L, heads))
    do, og = split_heads(dout, b, L, heads).float(), split_heads(o_given, b, L, heads).float()
    s = ((q @ k.transpose(-1, -2)) * 0.125).masked_fill(_mask(L, causal), float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e * (1.0 / e.sum(-1, keepdim=True)) if definition == "tiled" else e / e.sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    d = (do * og).sum(-1) if definition == "tiled" else (p * dp).sum(-1)
    ds = p * (dp - d[..., None]) * 0.125
    p16, ds16 = p.to(dt).float(), ds.to(dt).float()
    t = lambda x: x.transpose(-1, -2)
    return pack_qkv((ds16 @ k).to(dt), (t(ds16) @ q).to(dt), (t(p16) @ do).to(dt))


def emu_pool(q, k, v, b, L, heads, dt):
    qh = q.float().view(b, heads, 1, 64)
    kh, vh = split_heads(k, b, L, heads).float(), split_heads(v, b, L, heads).float()
    s = (qh @ kh.transpose(-1, -2)) * 0.125
    pe = torch.exp(s - s.max(-1, keepdim=True).values)
    return ((pe @ vh) * (1.0 / pe.sum(-1, keepdim=True))).to(dt).reshape(b, heads * 64)


def same_values(a, b):
    """Equal as values (+0 == -0), no NaN on either side."""
    return a.shape == b.shape and bool((a.double() == b.double()).all())


def check_backward(got, ref, bound, b, L, heads, what):
    """got dqkv [b * L, 3 W] against ref_backward's result; returns the worst ratios (dq, dk, dv)."""
    return tuple(within(g, ref[n], bound[n], (what, n)) for n, g in zip(("dq", "dk", "dv"), unpack_qkv(got, b, L, heads)))


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
ALL_LENGTHS = sorted(set(FWD_LENGTHS + BWD_LENGTHS + POOL_LENGTHS))
EMU_LENGTHS = [33, 77, 257, 320]
_worst = {}


def _note(key, value):
    _worst[key] = max(_worst.get(key, 0.0), value)


@pytest.mark.parametrize("L", ALL_LENGTHS)
def test_planted_inputs_meet_their_margin(L):
    for b, heads in SHAPES:
        for causal in (False, True):
            pl = plant_onehot(b, L, heads, causal, BF16)
            assert pl["worst"] <= MARGIN
            q, k, v = (t.double() for t in unpack_qkv(pl["qkv"], b, L, heads))
            s = q @ k.transpose(-1, -2) / 8
            tgt = torch.gather(s, 3, pl["pi"][..., None])
            assert bool((tgt == 512).all())
            off = s.scatter(3, pl["pi"][..., None], float("-inf"))
            if L > 1:
                assert float(off.max()) <= 8 * MARGIN and (float(off.max()) - 512) * LOG2E <= -277
            i = torch.arange(L)
            assert not causal or bool((pl["pi"] <= i).all())
            for bh in range(b * heads):                                   # every edge key is some query's target in every (b, h)
                assert set(edge_keys(L)) <= set(pl["pi"].view(b * heads, L)[bh].tolist())
            if L > 2 * len(edge_keys(L)):                                 # many-to-one: in some (b, h) a key serves several queries
                assert any(len(p.unique()) < L for p in pl["pi"].view(b * heads, L))
            rows = torch.cat([v.reshape(-1, 64), torch.zeros(1, 64, dtype=torch.float64)])
            assert len(torch.unique(rows, dim=0)) == b * heads * L + 1    # pairwise distinct, none all zero
            for dt in DTS:                                                # every planted value is exact in both types
                assert torch.equal(pl["qkv"].double(), pl["qkv"].to(dt).double())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [1, 16, 33, 65, 257, 288])
def test_emulation_reproduces_planted_expectations(dt, causal, L):
    b, heads = 3, 3
    pl = plant_onehot(b, L, heads, causal, dt)
    out, stats = emu_forward(pl["qkv"], b, L, heads, causal, dt)
    assert torch.equal(out, pl["out"])
    assert bool((stats[..., 0] == 512).all()) and bool((stats[..., 1] == 1).all())
    do, want = onehot_backward(pl, b, L, heads, dt)
    for definition in ("tiled", "wave"):
        assert same_values(emu_backward(pl["qkv"], pl["out"], do, b, L, heads, causal, dt, definition), want), definition
    un = plant_uniform(b, L, heads, causal, dt)
    within(emu_forward(un["qkv"], b, L, heads, causal, dt)[0], un["ref"], un["bound"], "uniform")
    if L <= 256:
        for uniform in (False, True):
            pp = plant_pool(b, L, heads, dt, uniform)
            got = emu_pool(pp["q"], pp["k"], pp["v"], b, L, heads, dt).double()
            assert bool(((got - pp["ref"]).abs() <= pp["bound"]).all()), uniform


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("scale", [1.0, 3.0, 5.0])
@pytest.mark.parametrize("L", EMU_LENGTHS)
def test_emulation_stays_within_the_bound(dt, scale, L):
    b, heads = 2, 3
    tag = "bf16" if dt == BF16 else "f16"
    for causal in (False, True):
        qkv = rand_qkv(b, L, heads, scale, dt, 10 * L + int(scale))
        f = ref_forward(qkv, b, L, heads, causal)
        if L <= 288:
            out, stats = emu_forward(qkv, b, L, heads, causal, dt)
            _note(("fwd", tag), within(split_heads(out, b, L, heads), f["out"], bound_forward(f, dt), ("fwd", L, scale, causal)))
            assert bool(((stats[..., 0].double() - f["mx"]).abs() <= f["mx_bound"]).all())
            assert bool(((stats[..., 1].double() - f["inv"]).abs() <= F32_ALLOW * f["inv"]).all())
        o16 = merge_heads(f["out"]).to(dt)
        do = rand_rows(b, L, heads, 0.5 * scale, dt, 11 * L + int(scale))
        for definition in ("tiled", "wave"):
            ref, bound = ref_backward(qkv, o16, do, b, L, heads, causal, dt, definition)
            got = emu_backward(qkv, o16, do, b, L, heads, causal, dt, definition)
            for n, w in zip(("dq", "dk", "dv"), check_backward(got, ref, bound, b, L, heads, (definition, L, scale, causal))):
                _note((n, tag), w)
    if L <= 256:
        e = heads * 64
        q = torch.from_numpy((scale * synth.normal(12 * L, "attn.q", b * e)).astype(np.float32)).view(b, e)
        k, v = rand_rows(b, L, heads, scale, dt, 13 * L), rand_rows(b, L, heads, scale, dt, 14 * L)
        ref, bound = ref_pool(q, k, v, b, L, heads, dt)
        _note(("pool", tag), within(emu_pool(q, k, v, b, L, heads, dt), ref, bound, ("pool", L, scale)))
    print("worst error / bound so far:", {k: round(v, 3) for k, v in sorted(_worst.items())})


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("broken", [dict(swap_v=(255, 256)), dict(drop_last=True), dict(no_max=True)], ids=["v_rows_swapped", "last_key_dropped", "no_max_subtraction"])
def test_broken_emulation_is_caught(dt, broken):
    """Each mistake must fail the planted one-hot expectation at L = 257; the two that move keys must ALSO exceed the bound on N(0, 1)
    inputs.  (Without the max-subtraction N(0, 1) scores do not overflow: only the planted 512 does.)"""
    b, L, heads = 3, 257, 3
    for causal in (False, True):
        pl = plant_onehot(b, L, heads, causal, dt)
        assert torch.equal(emu_forward(pl["qkv"], b, L, heads, causal, dt)[0], pl["out"])
        out = emu_forward(pl["qkv"], b, L, heads, causal, dt, **broken)[0]
        assert not torch.equal(out, pl["out"])
        if "no_max" in broken:
            continue
        qkv = rand_qkv(b, L, heads, 1.0, dt, 99)
        f = ref_forward(qkv, b, L, heads, causal)
        bad = split_heads(emu_forward(qkv, b, L, heads, causal, dt, **broken)[0], b, L, heads).double()
        assert ratio(bad, f["out"], bound_forward(f, dt)) > 1.0


def test_mha_bwd_refuses_misaligned_operands_and_large_grids_before_any_launch():
    """The three backward entry points refuse what hgr_mha refuses - an operand that is not 16-byte aligned, B * heads >= 2^31 - with
    HGR_EINVAL and a message that names the entry point.  They return before any launch, so no device is needed."""
    import ctypes as C
    from hgr_net_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    p = p + (-p) % 16
    calls = {"hgr_mha_bwd": lambda a, b, heads: lib.hgr_mha_bwd(a[0], a[1], a[2], a[3], b, 16, heads, 0, 0, None),
             "hgr_mha_bwd_stats": lambda a, b, heads: lib.hgr_mha_bwd_stats(a[0], a[1], a[2], a[3], p, b, 16, heads, 0, 0, None),
             "hgr_mha_bwd_colsum": lambda a, b, heads: lib.hgr_mha_bwd_colsum(a[0], a[1], a[2], a[3], None, p, b, 16, heads, 0, 1, None)}
    for name, call in calls.items():
        for off in (2, 8):                                                # one element, half a vector
            for which in range(4):
                args = [p + off if i == which else p for i in range(4)]
                assert call(args, 1, 1) == -1 and name.encode() + b":" in lib.hgr_last_error() and b"aligned" in lib.hgr_last_error(), (name, which)
        assert call([p] * 4, 65536, 32768) == -1 and name.encode() + b": grid too large" in lib.hgr_last_error(), name
