"""GPU: the row kernels of the FREE baseline (hgr_free.hip) against float64 restatements and against their unfused twins.

Bounds, none of them fitted to the device's output:
  * nll_rows16 - loss within 4 ulp of max|logit| and probabilities within 2^-20 absolute of a float64 softmax (an fp32 sum over n
    terms in a tree of depth log2 n); dlogits = that probability minus the one-hot, rounded ONCE to 16 bits: half a 16-bit ulp of
    the value on top of the 2^-20.  Against `ce_rows` + `cast16` the sums run in another order (a workgroup per row instead of a
    wave), so dlogits may differ by one 16-bit ulp and the loss by the same 4 ulp.
  * adam_l2_cast16 - bit-equal to `adam_l2` fed alpha * (g0 + g1 + ...) summed in torch fp32 in that order, w16 to `cast16`.
  * the counter normal - the 32-bit draws equal the host twin's bit for bit; the normals are within 1e-5 absolute of the float64
    twin (|z| < 7, a few ulp of logf / cospif / sqrtf); 2^20 draws have |mean| < 5 / sqrt(n) and |var - 1| < 5 sqrt(2 / n).
  * bias_act_rows / free_fr_tail - fp32 outputs within 2e-6 absolute of float64 (values in (0, 1) behind one or two library
    expf, or |x| < 8 for the LeakyReLU: a few ulp); 16-bit outputs one more rounding: half an ulp, at most 2^-8 (bf16) / 2^-11 (f16) of the value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T16 = {"bf16": torch.bfloat16, "f16": torch.float16}
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}      # half an ulp over the value: 8 / 11 significant bits


def _mods():
    from hgr_net_amd import ops
    from hgr_net_amd.baseline import free
    return ops, free


def _rows(seed, name, rows, cols):
    from hgr_net_amd.baseline import free
    return free.synth_rows(seed, name, rows, cols)


def _ord16(t: torch.Tensor) -> torch.Tensor:
    """16-bit floats as integers in value order (adjacent values differ by one)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def _ulp_of_max(x: np.ndarray) -> float:
    return float(np.spacing(np.float32(np.abs(x).max())))


# ---- nll_rows16 -----------------------------------------------------------------------------------------------------------------------------
def _nll_cases():
    from hgr_net_amd import ops
    return [1, 7, 8, 63, 64, 65, 257, 2049, ops.NLL_RESIDENT_COLS, ops.NLL_RESIDENT_COLS + 8]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("n_i", range(10))
def test_nll_rows16_against_float64_and_unfused_twin(n_i, dt):
    ops, _ = _mods()
    n = _nll_cases()[n_i]
    ld = -(-n // 8) * 8
    for rows in (1, 3, 70):
        x = 4.0 * _rows(11, f"nll.{n}.{rows}", rows, n)
        lab = (np.arange(rows) * 7919) % n
        lab[0], lab[-1] = n - 1, 0                                  # the label in the last and in the first column
        if rows >= 3 and n >= 2:
            x[1, 0], x[1, n - 1] = 80.0, -80.0                      # logits of +-80
            x[2, :] = -80.0
            x[2, n // 2] = 80.0
        buf = torch.full((rows, ld), 5.0, dtype=torch.float32, device=DEV)
        buf[:, :n] = torch.from_numpy(x).to(DEV)
        labels = torch.from_numpy(lab.astype(np.int32)).to(DEV)
        loss = torch.empty(rows, dtype=torch.float32, device=DEV)
        d16 = torch.full((rows, ld + 8), 3.0, dtype=T16[dt], device=DEV)
        out = torch.full((rows, ld), 9.0, dtype=torch.float32, device=DEV)
        ops.nll_rows16(buf, labels, n=n, loss_rows=loss, dlogits=d16, logsm=out)
        x64 = x.astype(np.float64)
        mx = x64.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(x64 - mx).sum(1))
        p64 = np.exp(x64 - lse[:, None])
        ref_loss = lse - x64[np.arange(rows), lab]
        tol = 4 * _ulp_of_max(x)
        e_loss = np.abs(loss.cpu().numpy() - ref_loss).max()
        onehot = np.zeros_like(p64)
        onehot[np.arange(rows), lab] = 1.0
        d_ref = p64 - onehot
        d_got = d16[:, :n].float().cpu().numpy().astype(np.float64)
        e_d = (np.abs(d_got - d_ref) - HALF_ULP[T16[dt]] * np.abs(d_ref)).max()
        ls = out[:, :n].cpu().numpy()
        e_ls = np.abs(ls - (x64 - lse[:, None])).max()
        print(f"n={n} rows={rows} {dt}: loss err {e_loss:.3g} (tol {tol:.3g}), dlogits excess {e_d:.3g} (tol {2.0 ** -20:.3g}), logsm err {e_ls:.3g}")
        assert e_loss <= tol
        assert e_d <= 2.0 ** -20 + 2.0 ** -24                        # f16 subnormal spacing below 2^-14
        assert e_ls <= tol + _ulp_of_max(ls)
        assert (d16[:, n:ld] == 0).all(), "pad columns of dlogits are zeros"
        assert (d16[:, ld:] == 3.0).all() and (out[:, n:] == 9.0).all() and (buf[:, n:] == 5.0).all(), "nothing outside its columns"
        # in place: the log-softmax replaces the logits; the same bits as out of place
        inplace = buf.clone()
        ops.nll_rows16(inplace, None, n=n, logsm=inplace)
        assert torch.equal(inplace[:, :n], out[:, :n]) and (inplace[:, n:] == 5.0).all()
        # the unfused twin: ce_rows, then cast16
        l2 = torch.empty(rows, dtype=torch.float32, device=DEV)
        d32 = torch.zeros((rows, ld), dtype=torch.float32, device=DEV)
        ops.ce_rows(buf[:, :n], labels, l2, d32, gscale=1.0)
        t16 = torch.empty((rows, ld), dtype=T16[dt], device=DEV)
        ops.cast16(d32, t16)
        assert (_ord16(t16) - _ord16(d16[:, :ld].contiguous())).abs().max().item() <= 1, "dlogits within one 16-bit ulp of the twin"
        assert np.abs(l2.cpu().numpy() - ref_loss).max() <= tol
        e_twin = (l2 - loss).abs().max().item()
        print(f"n={n} rows={rows} {dt}: |loss - twin's loss| {e_twin:.3g}")
        assert e_twin <= tol, "the loss within the same 4 ulp of the unfused twin's"


def test_nll_rows16_rejects_a_label_outside_the_row_quietly_as_nan():
    ops, _ = _mods()
    x = torch.zeros((2, 8), dtype=torch.float32, device=DEV)
    loss = torch.zeros(2, dtype=torch.float32, device=DEV)
    ops.nll_rows16(x, torch.tensor([9, 3], dtype=torch.int32, device=DEV), n=7, loss_rows=loss)
    got = loss.cpu().numpy()
    assert np.isnan(got[0]) and abs(got[1] - np.log(7.0)) < 1e-6


# ---- adam_l2_cast16 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("n", [4, 1020, 65540])
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("alpha", [1.0, 1.0 / 1512])
def test_adam_l2_cast16_is_adam_l2_then_cast16(n, slices, alpha, dt):
    ops, _ = _mods()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p0 = dev(0.02 * _rows(3, f"adam.p.{n}", 1, n)[0])
    pa, pb = p0.clone(), p0.clone()
    ma, va, mb, vb = (torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(4))
    wa = torch.empty(n, dtype=T16[dt], device=DEV)
    wb = torch.empty(n, dtype=T16[dt], device=DEV)
    for step in (1, 2):
        g = dev(_rows(3, f"adam.g.{n}.{slices}.{step}", slices, n) / np.float32(alpha))
        ops.adam_l2_cast16(pa, g, ma, va, wa, 1e-3, step, slices=slices, alpha=alpha, betas=(0.5, 0.999), wd=0.01)
        gs = g[0].clone()
        for s in range(1, slices):
            gs = gs + g[s]
        gp = gs * torch.tensor(alpha, dtype=torch.float32, device=DEV)
        ops.adam_l2(pb, gp.contiguous(), mb, vb, 1e-3, step, betas=(0.5, 0.999), wd=0.01)
        ops.cast16(pb, wb)
        for name, a, b in (("p", pa, pb), ("m", ma, mb), ("v", va, vb), ("w16", wa, wb)):
            assert torch.equal(a, b), f"{name} differs at step {step}"
    assert not torch.equal(pa, p0)


# ---- the counter normal and gen_input -------------------------------------------------------------------------------------------------------
def test_normal_counter_bits_values_chunks_and_moments():
    ops, free = _mods()
    rows, cols = 37, 72
    for row0 in (0, 5, (1 << 32) + 3):
        z = torch.empty((rows, cols), dtype=torch.float32, device=DEV)
        bits = torch.empty((rows, cols, 2), dtype=torch.int32, device=DEV)
        ops.normal_counter(z, 12345, 1, row0, bits)
        a, b = free.normal_bits_host(12345, 1, row0, rows, cols)
        got = bits.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[..., 0], a) and np.array_equal(got[..., 1], b), "the integer hash equals the host twin"
        err = np.abs(z.cpu().numpy() - free.normal_host(12345, 1, row0, rows, cols)).max()
        print(f"row0={row0}: |z - host| = {err:.3g}")
        assert err < 1e-5
    # a strided destination, a negative seed, another stream: not the same numbers
    wide = torch.zeros((rows, cols + 8), dtype=torch.float32, device=DEV)
    ops.normal_counter(wide[:, :cols], -7, 0)
    assert np.abs(wide[:, :cols].cpu().numpy() - free.normal_host(-7, 0, 0, rows, cols)).max() < 1e-5 and (wide[:, cols:] == 0).all()
    n = 1 << 20
    big = torch.empty((1024, 1024), dtype=torch.float32, device=DEV)
    ops.normal_counter(big, 1, 0)
    v = big.double()
    mean, var = float(v.mean()), float(v.var(unbiased=False))
    print(f"moments of 2^20 draws: mean {mean:.3g}, var - 1 {var - 1:.3g}")
    assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1) < 5 * np.sqrt(2 / n)


@pytest.mark.parametrize("num,nz,a", [(1, 8, 8), (3, 64, 72), (100, 72, 64), (3, 8, 64)])
@pytest.mark.parametrize("dt", ["bf16", "f16", "fp32"])
def test_free_gen_input(num, nz, a, dt):
    ops, free = _mods()
    tdt = {**T16, "fp32": torch.float32}[dt]
    ncls, natt = 5, 9
    att = torch.from_numpy(_rows(4, f"gen.att.{a}", natt, a)).to(DEV)
    cls = np.array([3, 0, 8, 3, 5], dtype=np.int32)
    rows = ncls * num
    one = torch.zeros((rows, nz + a + 8), dtype=tdt, device=DEV)
    ops.free_gen_input(one[:, :nz + a], att, torch.from_numpy(cls).to(DEV), num, nz, seed=21, stream=0)
    assert (one[:, nz + a:] == 0).all()
    ref32 = torch.cat((torch.from_numpy(free.normal_host(21, 0, 0, rows, nz)).to(DEV), att[torch.from_numpy(np.repeat(cls, num)).long().to(DEV)].double()), 1)
    got = one[:, :nz + a].double()
    assert torch.equal(got[:, nz:], ref32[:, nz:].to(torch.float32).to(tdt).double()), "attribute columns: the table's rows, rounded once"
    err = (got[:, :nz] - ref32[:, :nz]).abs() - HALF_ULP[tdt] * ref32[:, :nz].abs()
    assert err.max().item() < 1e-5
    # three launches with row0 write the same table as one
    cuts = [0, rows // 3, rows // 3 + max(1, rows // 2), rows] if rows >= 3 else [0, 1, rows, rows]
    three = torch.zeros_like(one)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            ops.free_gen_input(three[lo:hi, :nz + a], att, torch.from_numpy(cls).to(DEV), num, nz, seed=21, stream=0, row0=lo)
    assert torch.equal(one, three)
    # explicit noise
    z = torch.from_numpy(_rows(4, f"gen.z.{rows}.{nz}", rows, nz)).to(DEV)
    ex = torch.zeros((rows, nz + a), dtype=tdt, device=DEV)
    ops.free_gen_input(ex, att, torch.from_numpy(cls).to(DEV), num, nz, z=z)
    assert torch.equal(ex[:, :nz], z.to(tdt)) and torch.equal(ex[:, nz:], one[:, nz:nz + a])


# ---- bias_act_rows and free_fr_tail ---------------------------------------------------------------------------------------------------------
def _close(got: torch.Tensor, ref: np.ndarray, tdt) -> float:
    excess = np.abs(got.double().cpu().numpy() - ref) - HALF_ULP[tdt] * np.abs(ref)
    return float(excess.max())


@pytest.mark.parametrize("c", [8, 64, 72])
@pytest.mark.parametrize("dt", ["bf16", "f16", "fp32"])
def test_bias_act_rows(c, dt):
    ops, _ = _mods()
    tdt = {**T16, "fp32": torch.float32}[dt]
    rows, col0 = 13, 16
    x = 2.0 * _rows(6, f"ba.x.{c}", rows, c)
    bias = _rows(6, f"ba.b.{c}", 1, c)[0]
    xd = torch.full((rows, c + 4), 7.0, dtype=torch.float32, device=DEV)
    xd[:, :c] = torch.from_numpy(x).to(DEV)
    u = x.astype(np.float64) + bias.astype(np.float64)
    for act, ref in ((ops.ACT_LRELU02, np.where(u > 0, u, 0.2 * u)), (ops.ACT_SIGMOID, 1.0 / (1.0 + np.exp(-u)))):
        y = torch.full((rows, col0 + c + 8), 3.0, dtype=tdt, device=DEV)
        ops.bias_act_rows(xd[:, :c], torch.from_numpy(bias).to(DEV), y, act, col0=col0)
        assert _close(y[:, col0:col0 + c], ref, tdt) < 2e-6
        assert (y[:, :col0] == 3.0).all() and (y[:, col0 + c:] == 3.0).all(), "the other columns stay untouched"


@pytest.mark.parametrize("a", [8, 64, 72])
@pytest.mark.parametrize("dt", ["bf16", "f16", "fp32"])
def test_free_fr_tail(a, dt):
    ops, free = _mods()
    tdt = {**T16, "fp32": torch.float32}[dt]
    rows, col0 = 11, 24
    lat = 2.0 * _rows(8, f"tail.l.{a}", rows, 2 * a)
    bias = _rows(8, f"tail.b.{a}", 1, 2 * a)[0]
    eps = _rows(8, f"tail.e.{a}", rows, a)
    ld = torch.from_numpy(lat).to(DEV)
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))

    def ref(noise, with_bias):
        l64 = lat.astype(np.float64) + (bias.astype(np.float64) if with_bias else 0.0)
        return sig(l64[:, :a] + noise * sig(l64[:, a:])), l64[:, :a]

    for with_bias in (True, False):
        b = torch.from_numpy(bias).to(DEV) if with_bias else None
        y = torch.full((rows, col0 + a + 8), 3.0, dtype=tdt, device=DEV)
        mus = torch.empty((rows, a), dtype=torch.float32, device=DEV)
        ops.free_fr_tail(ld, y, col0=col0, bias=b, eps=torch.from_numpy(eps).to(DEV), mus=mus)
        want, mu = ref(eps.astype(np.float64), with_bias)
        assert _close(y[:, col0:col0 + a], want, tdt) < 2e-6 and np.abs(mus.cpu().numpy() - mu).max() < 1e-6
        assert (y[:, :col0] == 3.0).all() and (y[:, col0 + a:] == 3.0).all()
        # counter noise: the numbers of normal_host at (seed, stream, row0 + r, c); 1e-5 of noise moves the output by less than 1e-5 / 4
        y2 = torch.full((rows, col0 + a + 8), 3.0, dtype=tdt, device=DEV)
        ops.free_fr_tail(ld, y2, col0=col0, bias=b, seed=5, stream=1, row0=1000)
        want2, _ = ref(free.normal_host(5, 1, 1000, rows, a), with_bias)
        assert _close(y2[:, col0:col0 + a], want2, tdt) < 2e-6 + 2.5e-6
