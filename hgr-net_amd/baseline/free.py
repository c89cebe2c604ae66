"""FREE baseline on MI355X, the validation route of baseline/FREE/validate.py: load a trained generator and FR module, synthesise
features for the test classes, fit the softmax classifier on cat(x, hidden, h) and run `test()`.  `train_free.py` (WGAN-GP: its
gradient penalties need second derivatives) is NOT part of this module.

`Encoder`, `Generator`, `Discriminator`, `FR` and `LinearLogSoftmaxClassifier` take the reference's constructor arguments (an
`opt`-like namespace, `make_opt`), carry its parameter names and load its checkpoints unchanged.  Reference quirks, kept:

  * config.py forces nz = latent_size = attSize; classifier.py hard-codes 2048 feature columns.
  * FR.forward draws its reparameterisation noise in eval mode too: the classifier's input is random at test time as well.
  * fit_zsl copies every batch into a fixed [1512, input_dim] buffer (512 real + 1000 synthetic rows) and SKIPS the last loader
    batch of every epoch; next_batch permutes the synthetic rows before its first call and again at every wrap.
  * test() is CNZSL's on LOG-probabilities: every off-level column reads -1, and a log-probability is at most 0, so a level pick
    can only match when the classifier puts more than e^-1 on one node of that level.

On the device the products are `hgr_gemm_nt` in bf16 / f16 with fp32 accumulation (`dtype="fp32"`: `hgr_matmul_f32` in slices of
K), everything between them one of the row kernels of hgr_free.hip.  Noise is counter-based (`normal_host` is its twin): a pure
function of (seed, stream, row, column), so a synthetic table does not depend on how its rows were chunked.  One classifier step
launches a row gather, the two FR products with `bias_act_rows` / `free_fr_tail` writing into the classifier input, the logits
product, `nll_rows16`, the split-K weight gradient, `adam_l2_cast16`, the bias's `colsum` + `adam_l2` and `dot_f32` for the mean
loss - no host read, no atomics, bit-equal when repeated from the same state.  HGR_FREE_NLL_FUSED=0 / HGR_FREE_ADAM_FUSED=0 select
the unfused twins (`ce_rows` + `cast16`; `colsum` + `adam_l2` + `cast16`).
"""
from __future__ import annotations

import math
import os
import types
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch
from torch import nn

from .. import ops, wgrad
from ._shared import K_SLICE, TOP, BufferPool, TreeScorer, fmix32, mean_rows, need_device, sliced_matmul_f32  # noqa: F401
from .cnzsl import synth_rows  # noqa: F401
from .dgp_eval import ListTree

RES = 2048                                   # classifier.py:63,108: `.view(-1, 2048)`
STREAM_Z, STREAM_EPS = 0, 1                  # counter streams: generator noise, FR reparameterisation noise
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}
NO_TRAIN = "{}: this build runs FREE's validation route only (eval mode); training the GAN is the reference's train_free.py"


def make_opt(attSize: int = 1024, resSize: int = RES, ngh: int = 4096, ndh: int = 1024, latensize: int = 2048, nclass_seen: int = 983,
             decoder_hidden: int = 4096, encoder_hidden: int = 4096) -> types.SimpleNamespace:
    """The fields of config.py's `opt` the modules read, with its forced equalities (nz = latent_size = attSize)."""
    return types.SimpleNamespace(attSize=attSize, nz=attSize, latent_size=attSize, resSize=resSize, ngh=ngh, ndh=ndh, latensize=latensize,
                                 nclass_seen=nclass_seen, encoder_layer_sizes=[resSize, encoder_hidden],
                                 decoder_layer_sizes=[decoder_hidden, resSize])


def weights_init(m) -> None:
    """model.py:8-15 / util.weights_init."""
    name = m.__class__.__name__
    if name.find("Linear") != -1 and hasattr(m, "weight"):
        m.weight.data.normal_(0.0, 0.02)
        m.bias.data.fill_(0)
    elif name.find("BatchNorm") != -1:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0)


def _tdt(dtype) -> torch.dtype:
    if dtype not in TORCH_DT:
        raise ValueError(f"dtype must be one of {sorted(TORCH_DT)}, got {dtype!r}")
    return TORCH_DT[dtype]


def _w16(layer: nn.Linear, tdt: torch.dtype, pad_to: int = 0) -> torch.Tensor:
    """The layer's weight in the MFMA type (rows padded with zeros up to `pad_to`), converted again when the weight has changed."""
    w = layer.weight.data
    key = (w._version, w.data_ptr(), tdt, pad_to)
    cache = layer.__dict__.setdefault("_hgr_w16", {})
    if cache.get("key") != key:
        n = max(pad_to, w.shape[0])
        w16 = torch.zeros((n, w.shape[1]), dtype=tdt, device=w.device)
        ops.cast16(w.contiguous(), w16[:w.shape[0]])
        cache["key"], cache["w16"] = key, w16
    return cache["w16"]


def product(x: torch.Tensor, layer: nn.Linear, dtype: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 x W^T (no bias) of one Linear: 16-bit MFMA with fp32 accumulation, or the fp32 product in slices of K_SLICE columns
    (one fp32 accumulator chain over thousands of terms drifts from a blocked sum, _shared.sliced_matmul_f32)."""
    n, k = layer.weight.shape
    if x.shape[1] != k:
        raise ValueError(f"input has {x.shape[1]} columns, the layer takes {k}")
    if out is None:
        out = torch.empty((x.shape[0], n), dtype=torch.float32, device=x.device)
    if dtype == "fp32":
        sliced_matmul_f32(x, layer.weight.data, out)
    else:
        if k % 64:
            raise ValueError(f"K={k} must be a multiple of 64 on the 16-bit route")
        ops.gemm_nt(x, _w16(layer, _tdt(dtype)), out)
    return out


class _Eval(nn.Module):
    dtype = "bf16"

    def _check_eval(self):
        if self.training:
            raise NotImplementedError(NO_TRAIN.format(type(self).__name__ + " in training mode"))


class Encoder(_Eval):
    """model.py:18-39 (parameters only: the encoder is used by train_free.py alone)."""

    def __init__(self, opt):
        super().__init__()
        sizes, latent = list(opt.encoder_layer_sizes), opt.latent_size
        self.fc1 = nn.Linear(sizes[0] + latent, sizes[-1])
        self.fc3 = nn.Linear(sizes[-1], latent * 2)
        self.linear_means = nn.Linear(latent * 2, latent)
        self.linear_log_var = nn.Linear(latent * 2, latent)
        self.apply(weights_init)

    def forward(self, x, c=None):
        raise NotImplementedError(NO_TRAIN.format("Encoder.forward"))


class Discriminator(_Eval):
    """model.py:66-78 (parameters only)."""

    def __init__(self, opt):
        super().__init__()
        self.fc1 = nn.Linear(opt.resSize + opt.attSize, opt.ndh)
        self.fc2 = nn.Linear(opt.ndh, 1)
        self.apply(weights_init)

    def forward(self, x, att):
        raise NotImplementedError(NO_TRAIN.format("Discriminator.forward"))


class Generator(_Eval):
    """model.py:42-62: x = sigmoid(fc3(lrelu_0.2(fc1(cat(z, c)))))."""

    def __init__(self, opt, dtype: str = "bf16"):
        super().__init__()
        sizes, latent = list(opt.decoder_layer_sizes), opt.latent_size
        self.latent_size, self.dtype = latent, dtype
        _tdt(dtype)
        self.fc1 = nn.Linear(latent * 2, sizes[0])
        self.fc3 = nn.Linear(sizes[0], sizes[1])
        self.apply(weights_init)
        self.out = None

    @torch.no_grad()
    def run(self, inp: torch.Tensor, out: Optional[torch.Tensor] = None, dtype: Optional[str] = None) -> torch.Tensor:
        """From the concatenated input [rows, nz + A] in the route's type; `out` [rows, resSize] receives the features."""
        self._check_eval()
        dtype = dtype or self.dtype
        tdt = _tdt(dtype)
        if inp.dtype != tdt:
            raise ValueError(f"input is {inp.dtype} on the {dtype} route")
        rows = inp.shape[0]
        x1 = torch.empty((rows, self.fc1.out_features), dtype=tdt, device=inp.device)
        ops.bias_act_rows(product(inp, self.fc1, dtype), self.fc1.bias.data, x1, ops.ACT_LRELU02)
        x = out if out is not None else torch.empty((rows, self.fc3.out_features), dtype=tdt, device=inp.device)
        ops.bias_act_rows(product(x1, self.fc3, dtype), self.fc3.bias.data, x, ops.ACT_SIGMOID)
        self.out = x1
        return x

    @torch.no_grad()
    def forward(self, z, c=None, dtype: Optional[str] = None):
        self._check_eval()
        need_device(z, "FREE", "z")
        need_device(c, "FREE", "c")
        dtype = dtype or self.dtype
        rows, nz = z.shape
        inp = torch.empty((rows, nz + c.shape[1]), dtype=_tdt(dtype), device=z.device)
        ident = torch.arange(rows, dtype=torch.int32, device=z.device)
        ops.free_gen_input(inp, c.float().contiguous(), ident, 1, nz, z=z.float().contiguous())
        return self.run(inp, dtype=dtype)


class FR(_Eval):
    """model.py:86-128.  `forward` returns the reference's six values; `hidden_h` is the part the classifier uses and writes
    straight into the concatenated input."""

    def __init__(self, opt, attSize: int, dtype: str = "bf16"):
        super().__init__()
        self.embedSz, self.hidden, self.lantent = 0, None, None
        self.latensize, self.attSize, self.dtype = opt.latensize, opt.attSize, dtype
        _tdt(dtype)
        if attSize != opt.attSize:
            raise ValueError(f"FR(opt, attSize={attSize}) with opt.attSize={opt.attSize}: forward splits lantent at opt.attSize")
        self.fc1 = nn.Linear(opt.resSize, opt.ngh)
        self.fc3 = nn.Linear(opt.ngh, attSize * 2)
        self.discriminator = nn.Linear(opt.attSize, 1)
        self.classifier = nn.Linear(opt.attSize, opt.nclass_seen)
        self.apply(weights_init)
        self.eps_rows = 0                       # rows of counter noise drawn so far: the row0 of the next call

    @torch.no_grad()
    def hidden_h(self, big: torch.Tensor, dtype: Optional[str] = None, eps: Optional[torch.Tensor] = None, seed: int = 0,
                 mus: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`big` [rows, resSize + ngh + A] in the route's type with the features in its first resSize columns: fills in
        hidden = lrelu(fc1(x)) and h = sigmoid(mu + eps sigmoid(sd)) - compute_fear_out's cat([x, hidden, h]) (classifier.py:316-341)."""
        self._check_eval()
        dtype = dtype or self.dtype
        res, ngh, a = self.fc1.in_features, self.fc1.out_features, self.attSize
        if big.dtype != _tdt(dtype) or big.shape[1] != res + ngh + a:
            raise ValueError(f"the classifier input must be {_tdt(dtype)} [rows, {res + ngh + a}], got {big.dtype} {tuple(big.shape)}")
        rows = big.shape[0]
        ops.bias_act_rows(product(big[:, :res], self.fc1, dtype), self.fc1.bias.data, big, ops.ACT_LRELU02, col0=res)
        self.hidden = big[:, res:res + ngh]
        self.lantent = product(self.hidden, self.fc3, dtype)
        ops.free_fr_tail(self.lantent, big, col0=res + ngh, bias=self.fc3.bias.data, eps=eps, seed=seed, stream=STREAM_EPS,
                         row0=self.eps_rows, mus=mus)
        if eps is None:
            self.eps_rows += rows
        return big

    @torch.no_grad()
    def forward(self, feat, train_G: bool = False, eps: Optional[torch.Tensor] = None, seed: int = 0, dtype: Optional[str] = None):
        self._check_eval()
        need_device(feat, "FREE", "feat")
        dtype = dtype or self.dtype
        res, ngh, a = self.fc1.in_features, self.fc1.out_features, self.attSize
        rows, dev = feat.shape[0], feat.device
        big = torch.empty((rows, res + ngh + a), dtype=_tdt(dtype), device=dev)
        big[:, :res].copy_(feat)
        if eps is None:                          # the same numbers the counter route of the tail would draw
            eps = ops.normal_counter(torch.empty((rows, a), dtype=torch.float32, device=dev), seed, STREAM_EPS, self.eps_rows)
            self.eps_rows += rows
        mus = torch.empty((rows, a), dtype=torch.float32, device=dev)
        self.hidden_h(big, dtype, eps.float().contiguous(), mus=mus)
        stds = torch.empty((rows, a), dtype=torch.float32, device=dev)
        ops.bias_act_rows(self.lantent[:, a:], self.fc3.bias.data[a:], stds, ops.ACT_SIGMOID)
        encoder_out = torch.addcmul(mus, eps.float(), stds)                       # reparameter(): randn * sigma + mu
        dis_in = mus if train_G else encoder_out
        dis_out = self.discriminator.bias.data.expand(rows, 1).contiguous()
        ops.matmul_f32(dis_in, self.discriminator.weight.data.t(), dis_out, accumulate=True)
        ns = self.classifier.out_features
        pred = torch.zeros((rows, -(-ns // 8) * 8), dtype=torch.float32, device=dev)[:, :ns]
        pred.copy_(self.classifier.bias.data.expand(rows, ns))
        ops.matmul_f32(mus, self.classifier.weight.data.t(), pred, accumulate=True)
        ops.nll_rows16(pred, None, logsm=pred)                                    # self.logic: LogSoftmax(dim=1), in place
        return mus, stds, dis_out, pred, encoder_out, big[:, res + ngh:]

    def getLayersOutDet(self):
        return self.hidden.detach()


class LinearLogSoftmaxClassifier(_Eval):
    """classifier.py:365-372: `fc` and a log-softmax.  The class dimension is padded to a multiple of 8 for the kernels (zero weight
    rows, zero bias); the padding never enters the softmax."""

    def __init__(self, input_dim: int, nclass: int, dtype: str = "bf16"):
        super().__init__()
        self.fc = nn.Linear(input_dim, nclass)
        self.dtype = dtype
        _tdt(dtype)

    @torch.no_grad()
    def logits(self, x: torch.Tensor, dtype: Optional[str] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fc(x) as fp32 [rows, Npad]; columns >= nclass are padding."""
        dtype = dtype or self.dtype
        n, k = self.fc.weight.shape
        npad = -(-n // 8) * 8
        if out is None:
            out = torch.empty((x.shape[0], npad), dtype=torch.float32, device=x.device)
        if dtype == "fp32":
            out.zero_()
            out[:, :n].copy_(self.fc.bias.data.expand(x.shape[0], n))
            sliced_matmul_f32(x, self.fc.weight.data, out, accumulate_first=True)
        else:
            if k % 64:
                raise ValueError(f"K={k} must be a multiple of 64 on the 16-bit route")
            bias = self.__dict__.setdefault("_hgr_bias", {})
            bkey = (self.fc.bias.data._version, self.fc.bias.data.data_ptr())
            if bias.get("key") != bkey:
                bp = torch.zeros(npad, dtype=torch.float32, device=x.device)
                bp[:n].copy_(self.fc.bias.data)
                bias["key"], bias["b"] = bkey, bp
            ops.gemm_nt(x, _w16(self.fc, _tdt(dtype), npad), out, bias=bias["b"], epilogue=ops.EPI_BIAS)
        return out

    @torch.no_grad()
    def forward(self, x, dtype: Optional[str] = None):
        self._check_eval()
        need_device(x, "FREE", "x")
        dtype = dtype or self.dtype
        n = self.fc.out_features
        lg = self.logits(x.to(_tdt(dtype)).contiguous(), dtype)
        ops.nll_rows16(lg, None, n=n, logsm=lg)
        return lg[:, :n]


# ---- synthesis (classifier.py:21-43) ---------------------------------------------------------------------------------------------------------
@torch.no_grad()
def synthesize(generator: Generator, classes, attribute: torch.Tensor, num: int = 100, seed: int = 0, dtype: Optional[str] = None,
               chunk_classes: int = 64) -> Tuple[torch.Tensor, torch.Tensor]:
    """generate_syn_feature: (features [len(classes) * num, resSize] on the device in the route's type, labels int64): `num` rows
    per class from z ~ N(0, 1) and the class's attribute row, labelled with the class's node index.  The noise of row i is the
    counter normal of (seed, STREAM_Z, i, column): the table does not depend on `chunk_classes`."""
    need_device(attribute, "FREE", "attribute")
    dtype = dtype or generator.dtype
    cls = np.asarray(classes.detach().cpu() if torch.is_tensor(classes) else classes, dtype=np.int64).reshape(-1)
    if cls.size < 1 or cls.min() < 0 or cls.max() >= attribute.shape[0] or num < 1 or chunk_classes < 1:
        raise ValueError(f"classes must be node indices below {attribute.shape[0]}, num and chunk_classes positive")
    dev, nz = attribute.device, generator.latent_size
    att = attribute.float().contiguous()
    if att.shape[1] != nz:
        raise ValueError(f"attribute has {att.shape[1]} columns, the generator takes {nz}")
    cls_dev = torch.from_numpy(cls.astype(np.int32)).to(dev)
    out = torch.empty((cls.size * num, generator.fc3.out_features), dtype=_tdt(dtype), device=dev)
    for c0 in range(0, cls.size, chunk_classes):
        r0, r1 = c0 * num, min(cls.size, c0 + chunk_classes) * num
        inp = torch.empty((r1 - r0, 2 * nz), dtype=_tdt(dtype), device=dev)
        ops.free_gen_input(inp, att, cls_dev, num, nz, seed=seed, stream=STREAM_Z, row0=r0)
        generator.run(inp, out=out[r0:r1], dtype=dtype)
    return out, torch.from_numpy(cls).to(dev).repeat_interleave(num)


class SynBatcher:
    """next_batch's index arithmetic (classifier.py:124-158) on the host: which rows of the ORIGINAL synthetic table a call takes.
    The reference permutes the table itself, so its permutations compose; `perm` supplies them (default: torch.randperm on a host
    generator)."""

    def __init__(self, ntrain: int, seed: int = 0, perm: Optional[Callable[[int], torch.Tensor]] = None):
        self.ntrain, self.index_in_epoch, self.epochs_completed = int(ntrain), 0, 0
        self.gen = torch.Generator().manual_seed(int(seed))
        self.perm = perm if perm is not None else (lambda n: torch.randperm(n, generator=self.gen))
        self.order = torch.arange(self.ntrain)

    def _shuffle(self) -> None:
        p = torch.as_tensor(self.perm(self.ntrain)).long()
        if p.numel() != self.ntrain:
            raise ValueError("a permutation of all synthetic rows is needed")
        self.order = self.order[p]

    def next(self, syn_batch_size: int = 1000) -> torch.Tensor:
        if syn_batch_size > self.ntrain:
            raise ValueError(f"{syn_batch_size} synthetic rows per batch out of {self.ntrain}")
        start = self.index_in_epoch
        if self.epochs_completed == 0 and start == 0:
            self._shuffle()
        if start + syn_batch_size > self.ntrain:
            self.epochs_completed += 1
            rest = self.order[start:self.ntrain]
            self._shuffle()
            self.index_in_epoch = syn_batch_size - rest.numel()
            return torch.cat((rest, self.order[:self.index_in_epoch]))
        self.index_in_epoch += syn_batch_size
        return self.order[start:self.index_in_epoch]


def _switch(name: str) -> bool:
    return os.environ.get(name, "1") != "0"


class FREEClassifier(TreeScorer):
    """classifier.py:45-341 `CLASSIFIER` on cached features.  `tree`: a dgp_eval.ListTree, or (c2p, d2n, ordered_nodes) as gen_tree
    returns them.  `attribute` [N, A] on the device; `test_index` the candidate node indices (the synthetic classes).  test() counts
    through _shared.TreeScorer (`add`, `add_rows`, `counters`, `result`; an `eps` behind the targets goes to `log_probs`)."""

    def __init__(self, netG: Generator, netFR: FR, tree, test_index, attribute: torch.Tensor, nclass: int, lr: float = 0.001,
                 beta1: float = 0.5, nepoch: int = 20, batch_size: int = 1512, syn_num: int = 100, syn_batch_size: int = 1000,
                 dtype: str = "bf16", seed: int = 0, syn: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                 perm: Optional[Callable[[int], torch.Tensor]] = None):
        need_device(attribute, "FREE", "attribute")
        self.dev, self.dtype, self.tdt = attribute.device, dtype, _tdt(dtype)
        self.netG, self.netFR = netG.to(self.dev).eval(), netFR.to(self.dev).eval()
        if not isinstance(tree, ListTree):
            c2p, d2n, nodes = tree
            depth = np.array([len(c) for c in c2p], dtype=np.int32)
            tree = ListTree(list(nodes), [list(c) for c in c2p], depth, {int(k): list(v) for k, v in dict(d2n).items()}, int(depth.max()) + 1)
        super().__init__(tree, test_index, self.dev)
        n, te = self.n, self.test_index
        if attribute.shape[0] != n or nclass < n:
            raise ValueError(f"{attribute.shape[0]} attribute rows and {nclass} classes for {n} nodes")
        self.attribute, self.nclass = attribute, int(nclass)
        self.lr, self.betas, self.nepoch, self.batch_size, self.syn_batch_size, self.seed = lr, (beta1, 0.999), nepoch, int(batch_size), int(syn_batch_size), seed
        res, ngh, a = netFR.fc1.in_features, netFR.fc1.out_features, netFR.attSize
        self.res, self.input_dim = res, res + ngh + a
        if self.input_dim % 64:
            raise ValueError(f"K = {res} + {ngh} + {a} = {self.input_dim} must be a multiple of 64")
        if not 0 < self.syn_batch_size < self.batch_size:
            raise ValueError("batch_size = real rows + syn_batch_size")
        self.nll_fused, self.adam_fused = _switch("HGR_FREE_NLL_FUSED"), _switch("HGR_FREE_ADAM_FUSED")
        # the model: master weights padded to a multiple of 8 classes; the module's parameters are views of the first nclass rows
        self.model = LinearLogSoftmaxClassifier(self.input_dim, self.nclass, dtype)
        self.model.apply(weights_init)
        self.model.to(self.dev).eval()
        self.npad = -(-self.nclass // 8) * 8
        self.wp = torch.zeros((self.npad, self.input_dim), dtype=torch.float32, device=self.dev)
        self.bp = torch.zeros(self.npad, dtype=torch.float32, device=self.dev)
        self.load_model(self.model.state_dict())
        self.mw, self.vw, self.mb, self.vb = (torch.zeros_like(t) for t in (self.wp, self.wp, self.bp, self.bp))
        self.t = 0
        self.syn_feature, self.syn_label = syn if syn is not None else synthesize(self.netG, te, attribute, syn_num, seed, dtype)
        self.ntrain = self.syn_feature.shape[0]
        self.batcher = SynBatcher(self.ntrain, seed, perm)
        self._pool = BufferPool(self.dev)
        self._buf, self._bufs = self._pool.pool, self._pool.bufs

    # -- the model's state -------------------------------------------------------------------------------------------------------------------
    def load_model(self, sd: dict) -> None:
        """`fc.weight` / `fc.bias` (the saved `cls_{attSize}` file) into the padded master copy; refreshes the 16-bit operand."""
        w, b = torch.as_tensor(sd["fc.weight"]), torch.as_tensor(sd["fc.bias"])
        if tuple(w.shape) != (self.nclass, self.input_dim) or b.numel() != self.nclass:
            raise ValueError(f"fc.weight {tuple(w.shape)} / fc.bias {tuple(b.shape)} for [{self.nclass}, {self.input_dim}]")
        self.wp[:self.nclass].copy_(w)
        self.bp[:self.nclass].copy_(b)
        self.model.fc.weight.data = self.wp[:self.nclass]
        self.model.fc.bias.data = self.bp[:self.nclass]
        if self.dtype != "fp32":
            self.w16 = torch.empty((self.npad, self.input_dim), dtype=self.tdt, device=self.dev)
            ops.cast16(self.wp, self.w16)

    # -- inputs ------------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def features(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """compute_fear_out: cat([x, hidden, h]) [rows, input_dim] in the route's type."""
        need_device(x, "FREE", "x")
        if x.dim() != 2 or x.shape[1] != self.res:
            raise ValueError(f"features must be [rows, {self.res}], got {tuple(x.shape)}")
        big = out if out is not None else torch.empty((x.shape[0], self.input_dim), dtype=self.tdt, device=self.dev)
        big[:, :self.res].copy_(x)
        return self.netFR.hidden_h(big, self.dtype, eps, self.seed)

    @torch.no_grad()
    def next_batch(self, train_feature: torch.Tensor, train_label: torch.Tensor, syn_batch_size: Optional[int] = None,
                   eps: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        """(cat(real, synthetic) through compute_fear_out, the labels): the reference's call; the synthetic rows follow its wrap rule."""
        idx = self.batcher.next(self.syn_batch_size if syn_batch_size is None else syn_batch_size).to(self.dev)
        self.last_index = idx
        rows = train_feature.shape[0] + idx.numel()
        big = out if out is not None else torch.empty((rows, self.input_dim), dtype=self.tdt, device=self.dev)
        nr = train_feature.shape[0]
        big[:nr, :self.res].copy_(train_feature)
        big[nr:, :self.res].copy_(self.syn_feature.index_select(0, idx))
        self.netFR.hidden_h(big, self.dtype, eps, self.seed)
        return big, torch.cat((train_label.reshape(-1).long(), self.syn_label.index_select(0, idx)))

    # -- training ----------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step_on(self, big: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """One optimiser step on a prepared input [B, input_dim]; returns the mean loss as a 0-dim device tensor."""
        if self.dtype == "fp32":
            raise NotImplementedError('the fit runs on the 16-bit routes (dtype="bf16" / "f16"); dtype="fp32" serves the forward passes and test()')
        b, k, n, npad = big.shape[0], self.input_dim, self.nclass, self.npad
        lab = labels.reshape(-1).to(torch.int32)
        logits = self.model_logits(big, self._buf("logits", (b, npad)))
        loss_rows, loss = self._buf("loss_rows", (b,)), self._buf("loss", (1,))
        self.t += 1
        d16 = self._buf("d16", (b, npad), self.tdt)
        if self.nll_fused:
            ops.nll_rows16(logits, lab, n=n, loss_rows=loss_rows, dlogits=d16)
        else:
            d32 = self._buf("d32", (b, npad), zero=True)   # ce_rows writes n columns: the padding columns stay zero
            ops.ce_rows(logits[:, :n], lab, loss_rows, d32, gscale=1.0)
            ops.cast16(d32, d16)
        _, s, kc, _ = wgrad.plan(npad, k, b)
        part = self._buf("part", (s, npad, k))
        ops.gemm_tn_splitk(d16, big, part, kc)
        gb = self._buf("gb", (npad,))
        if self.adam_fused:
            ops.adam_l2_cast16(self.wp, part, self.mw, self.vw, self.w16, self.lr, self.t, slices=s, alpha=1.0 / b, betas=self.betas)
        else:
            gw = self._buf("gw", (npad, k))
            ops.colsum(part.view(s, npad * k), gw.view(-1), self._buf("csw", (npad * k,)), accumulate=False, alpha=1.0 / b)
            ops.adam_l2(self.wp, gw, self.mw, self.vw, self.lr, self.t, self.betas)
            ops.cast16(self.wp, self.w16)
        ops.colsum(d16, gb, self._buf("cs", ((b + 511) // 512 * npad,)), accumulate=False, alpha=1.0 / b)
        ops.adam_l2(self.bp, gb, self.mb, self.vb, self.lr, self.t, self.betas)
        return mean_rows(self._pool, loss_rows, loss).clone().reshape(())

    def model_logits(self, big: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """fc(big) [rows, Npad] fp32 from the master weights (their 16-bit copy on the 16-bit routes)."""
        if self.dtype == "fp32":
            return self.model.logits(big, "fp32", out)
        return ops.gemm_nt(big, self.w16, out, bias=self.bp, epilogue=ops.EPI_BIAS)

    @torch.no_grad()
    def step(self, real_feats: torch.Tensor, real_labels: torch.Tensor, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One iteration of fit_zsl's loop body: the batch is exactly `batch_size` rows (classifier.py:111 copies into a fixed buffer)."""
        need_device(real_feats, "FREE", "real_feats")
        need_device(real_labels, "FREE", "real_labels")
        if real_feats.shape[0] + self.syn_batch_size != self.batch_size:
            raise ValueError(f"{real_feats.shape[0]} real + {self.syn_batch_size} synthetic rows do not fill the [{self.batch_size}, {self.input_dim}] buffer")
        big, lab = self.next_batch(real_feats, real_labels, eps=eps, out=self._buf("big", (self.batch_size, self.input_dim), self.tdt))
        return self.step_on(big, lab)

    def fit_zsl(self, loader, nepoch: Optional[int] = None, log: Optional[Callable[[str], None]] = print) -> list:
        """`loader`: a sized iterable of (features [b, resSize], labels [b]) device batches.  The LAST batch of every epoch is skipped
        (classifier.py:105).  Returns the loss tensors of the steps taken."""
        losses, n = [], len(loader)
        for epoch in range(self.nepoch if nepoch is None else nepoch):
            if log is not None:
                log(str(epoch))
            for i, (feats, labels) in enumerate(loader):
                if i < n - 1:
                    losses.append(self.step(feats, labels))
        return losses

    # -- scoring -----------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def log_probs(self, feats: torch.Tensor, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`self.model(cat([feats, hidden, h]))`: log-softmax [rows, Npad] fp32 (columns >= nclass are padding)."""
        big = self.features(feats, eps)
        lg = self.model_logits(big, torch.empty((big.shape[0], self.npad), dtype=torch.float32, device=self.dev))
        ops.nll_rows16(lg, None, n=self.nclass, logsm=lg)
        return lg

    scores = log_probs

    def test(self, loader) -> str:
        """`loader`: (features [b, resSize], the batch's one target) pairs; returns the metric string."""
        for feats, target in loader:
            self.add(feats, target)
        return self.result()


# ---- host twins: plain torch / numpy ------------------------------------------------------------------------------------------------------
def normal_bits_host(seed: int, stream: int, row0: int, rows: int, cols: int) -> Tuple[np.ndarray, np.ndarray]:
    """The two 32-bit draws (a, b), uint32 [rows, cols], of hgr_normal_counter (include/hgr.h)."""
    m = 0xFFFFFFFF
    key = fmix32(np.array(((seed & m) + 0x9E3779B9 * ((stream & m) + 1)) & m, dtype=np.uint64))
    key = fmix32(key ^ 0xC2B2AE35)
    r = np.arange(row0, row0 + rows, dtype=np.uint64)
    rk = fmix32(key ^ (r & m))
    rk = fmix32((rk + 0x9E3779B9 * ((r >> 32) + 1)) & m)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    return fmix32(rk ^ ((2 * c) & m)).astype(np.uint32), fmix32(rk ^ ((2 * c + 1) & m)).astype(np.uint32)


def normal_host(seed: int, stream: int, row0: int, rows: int, cols: int) -> np.ndarray:
    """float64 [rows, cols]: the counter normals of rows [row0, row0 + rows) - Box-Muller on the two draws, evaluated in float64."""
    a, b = normal_bits_host(seed, stream, row0, rows, cols)
    u1 = ((a >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.pi * ((b >> 8).astype(np.float64) * 2.0 ** -23))


def _sd(sd: dict, dtype) -> Dict[str, torch.Tensor]:
    return {k: (v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype) for k, v in sd.items()}


def generator_host(sd: dict, z, c, dtype=torch.float32, tap: Optional[dict] = None) -> torch.Tensor:
    """Generator.forward from a state dict, on the CPU in `dtype`."""
    w = _sd(sd, dtype)
    x1 = torch.nn.functional.leaky_relu(torch.cat((torch.as_tensor(z).to(dtype), torch.as_tensor(c).to(dtype)), -1) @ w["fc1.weight"].t() + w["fc1.bias"], 0.2)
    if tap is not None:
        tap["x1"] = x1
    return torch.sigmoid(x1 @ w["fc3.weight"].t() + w["fc3.bias"])


def fr_host(sd: dict, x, eps, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """FR.forward's values that the classifier uses, from a state dict: mus, stds, encoder_out, hidden, h."""
    w = _sd(sd, dtype)
    a = w["fc3.weight"].shape[0] // 2
    hidden = torch.nn.functional.leaky_relu(torch.as_tensor(x).to(dtype) @ w["fc1.weight"].t() + w["fc1.bias"], 0.2)
    lat = hidden @ w["fc3.weight"].t() + w["fc3.bias"]
    mus, stds = lat[:, :a], torch.sigmoid(lat[:, a:])
    enc = torch.as_tensor(eps).to(dtype) * stds + mus
    return {"mus": mus, "stds": stds, "encoder_out": enc, "hidden": hidden, "h": torch.sigmoid(enc)}


def features_host(sd_fr: dict, x, eps, dtype=torch.float32) -> torch.Tensor:
    """compute_fear_out: cat([x, hidden, h])."""
    f = fr_host(sd_fr, x, eps, dtype)
    return torch.cat((torch.as_tensor(x).to(dtype), f["hidden"], f["h"]), 1)


def fit_state_host(sd: dict, dtype=torch.float32) -> dict:
    w = _sd(sd, dtype)
    return {"sd": {k: w[k].clone() for k in ("fc.weight", "fc.bias")}, "m": {k: torch.zeros_like(w[k]) for k in ("fc.weight", "fc.bias")},
            "v": {k: torch.zeros_like(w[k]) for k in ("fc.weight", "fc.bias")}, "t": 0}


def fit_step_host(state: dict, big, labels, lr: float = 0.001, betas=(0.5, 0.999), eps: float = 1e-8, update: bool = True):
    """One fit_zsl step on a prepared input, in the state's dtype: NLLLoss(LogSoftmax(fc(big))), autograd, torch.optim.Adam's
    arithmetic.  Returns (loss, {'fc.weight', 'fc.bias'} gradients, log-probabilities)."""
    sd = state["sd"]
    dtype = sd["fc.weight"].dtype
    leaf = {k: sd[k].clone().requires_grad_(True) for k in sd}
    logp = torch.log_softmax(torch.as_tensor(big).to(dtype) @ leaf["fc.weight"].t() + leaf["fc.bias"], 1)
    loss = torch.nn.functional.nll_loss(logp, torch.as_tensor(labels).long().reshape(-1))
    gw, gb = torch.autograd.grad(loss, [leaf["fc.weight"], leaf["fc.bias"]])
    grads = {"fc.weight": gw, "fc.bias": gb}
    if update:
        state["t"] += 1
        t = state["t"]
        with torch.no_grad():
            for k, g in grads.items():
                state["m"][k] = betas[0] * state["m"][k] + (1 - betas[0]) * g
                state["v"][k] = betas[1] * state["v"][k] + (1 - betas[1]) * g * g
                denom = state["v"][k].sqrt() / math.sqrt(1 - betas[1] ** t) + eps
                sd[k] = sd[k] - (lr / (1 - betas[0] ** t)) * state["m"][k] / denom
    return loss.detach(), grads, logp.detach()


# ---- synthetic material (hgr_net_amd.synth: a pure function of the seed) -----------------------------------------------------------------
def synth_state(seed: int, opt, which: str, att_gain: float = 1.0) -> Dict[str, np.ndarray]:
    """A state dict of fp32 arrays for `which` = 'netG' or 'netFR': fan-in scaled normal weights (the outputs spread over (0, 1)
    instead of sitting at sigmoid(0)), small normal biases.  `att_gain` multiplies the generator's weights on the attribute half of
    its input: the attribute rows have norm 1 beside noise of norm sqrt(nz), so at gain 1 the synthetic classes hardly differ."""
    if which == "netG":
        shapes = {"fc1": (opt.decoder_layer_sizes[0], 2 * opt.latent_size), "fc3": (opt.decoder_layer_sizes[1], opt.decoder_layer_sizes[0])}
    elif which == "netFR":
        shapes = {"fc1": (opt.ngh, opt.resSize), "fc3": (2 * opt.attSize, opt.ngh), "discriminator": (1, opt.attSize),
                  "classifier": (opt.nclass_seen, opt.attSize)}
    else:
        raise ValueError("which: 'netG' or 'netFR'")
    sd = {}
    for name, (o, i) in shapes.items():
        sd[name + ".weight"] = synth_rows(seed, f"free.{which}.{name}.w", o, i) * np.float32(1.0 / math.sqrt(i))
        sd[name + ".bias"] = 0.1 * synth_rows(seed, f"free.{which}.{name}.b", 1, o).reshape(o)
    if which == "netG" and att_gain != 1.0:
        sd["fc1.weight"][:, opt.latent_size:] *= np.float32(att_gain)
    return sd
