#!/usr/bin/env python3
"""Generates tests/golden/dgp_train_small.npz by RUNNING the reference's DGP training arithmetic on the CPU (`.cuda()`
patched to identity, like tools/make_golden_dgp.py): baseline/DGP/models/gcn_dense_att.py::GCN_Dense_Att in training mode,
baseline/DGP/utils.py::l2_loss on 60 selected rows and torch.optim.Adam(lr=1e-3, weight_decay=5e-4) for 3 epochs
(train_gcn_dense_att.py:80-102), on the graph and word vectors of tests/golden/dgp_small.npz.  hidden_layers = "40": no
dropout, the only configuration whose arithmetic another implementation can reproduce.  The fixture holds inputs (rows,
targets, initial parameters) and outputs (the six gradients of epoch 1, the three training losses, the parameters after
epoch 3, and per element the smallest |coupled gradient| / max |coupled gradient| over the epochs) only."""
import sys
from pathlib import Path

sys.dont_write_bytecode = True
sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden_dgp import GOLD, REF                                  # noqa: E402  (also puts the repository on sys.path)

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402

from hgr_net_amd import synth                                          # noqa: E402
from oracle import dgp_ref                                             # noqa: E402

# upper bounds of the thresholds tests/test_gpu_dgp_train.py uses (100 x its gradient tolerances): attention logits, other tensors
THETA_ATT, THETA = 1e-3, 4e-4
EPOCHS, N_ROWS, HIDDEN = 3, 60, 40


def main():
    z = np.load(GOLD / "dgp_small.npz")
    groups, p = [], 0
    for s in z["edges_set_sizes"]:
        groups.append([tuple(e) for e in z["edges_set_flat"][p:p + s].tolist()])
        p += s
    edges_set = [[list(e) for e in g] for g in dgp_ref.fold_groups(groups, int(z["lim"]))]
    n, x = len(z["wnids"]), torch.from_numpy(z["x"])
    dim_out = z["out"].shape[1]

    sys.path.insert(0, str(REF))
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from models.gcn_dense_att import GCN_Dense_Att
    from utils import l2_loss
    torch.manual_seed(7)
    gcn = GCN_Dense_Att(n, edges_set, x.shape[1], dim_out, str(HIDDEN))
    with torch.no_grad():
        gcn.a_att.copy_(torch.tensor([0.3, -0.2, 0.5, 0.1, -0.4]))
        gcn.r_att.copy_(torch.tensor([-0.1, 0.4, 0.0, 0.25, 0.6]))
        for conv in gcn.layers:
            conv.b.copy_(torch.from_numpy(synth.normal(8, f"dgp.train.b{conv.b.numel()}", conv.b.numel()).astype(np.float32) * 0.1))
    rows = np.random.default_rng(5).permutation(n)[:N_ROWS].astype(np.int64)
    targets = torch.nn.functional.normalize(torch.from_numpy(synth.normal(9, "dgp.train.fc", N_ROWS * dim_out).reshape(N_ROWS, dim_out).astype(np.float32)))
    sd0 = {k: v.detach().numpy().copy() for k, v in gcn.state_dict().items()}
    opt = torch.optim.Adam(gcn.parameters(), lr=1e-3, weight_decay=5e-4)          # train_gcn_dense_att.py:80
    names = {id(p): k for k, p in gcn.named_parameters()}
    losses, grads1, gmin = [], {}, {}
    for epoch in range(1, EPOCHS + 1):                                             # train_gcn_dense_att.py:96-102
        gcn.train()
        out = gcn(x)
        loss = l2_loss(out[rows], targets)       # mask_l2_loss with one index list: a[mask], b[mask] of equal row order
        opt.zero_grad()
        loss.backward()
        for prm in gcn.parameters():
            k = names[id(prm)]
            if epoch == 1:
                grads1[k] = prm.grad.numpy().copy()
            g = (prm.grad + 5e-4 * prm.detach()).abs().numpy()                     # what Adam's moments see
            ratio = g / g.max()
            gmin[k] = ratio if k not in gmin else np.minimum(gmin[k], ratio)
        opt.step()
        losses.append(float(loss.detach()))
    sd3 = {k: v.detach().numpy().copy() for k, v in gcn.state_dict().items()}
    for k, r in gmin.items():
        theta = THETA_ATT if k.endswith("_att") else THETA
        small = float((r < theta).mean())
        print(f"{k:14s} elements below {theta:g} x max|g| in some epoch: {100 * small:.2f} %")
        assert small <= 0.01, (k, small)
    print("losses", losses)
    assert losses[2] < losses[0]
    dst = GOLD / "dgp_train_small.npz"
    np.savez_compressed(dst, rows=rows.astype(np.int32), targets=targets.numpy(), hidden=np.int32(HIDDEN), lr=np.float32(1e-3),
                        weight_decay=np.float32(5e-4), losses=np.array(losses, np.float64),
                        **{"sd0_" + k: v for k, v in sd0.items()}, **{"grad1_" + k: v for k, v in grads1.items()},
                        **{"sd3_" + k: v for k, v in sd3.items()}, **{"gmin_" + k: v.astype(np.float32) for k, v in gmin.items()})
    print("wrote", dst, dst.stat().st_size)


if __name__ == "__main__":
    main()
