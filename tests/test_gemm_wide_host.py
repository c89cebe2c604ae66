"""CPU: the shape contract of the 320 x 256 tile residual producer (hgr_gemm_nt_res_stats_wide_ok, host code) and the argument
validation of its entry point.  Everything runs in a child process with the device hidden, as the plan replay does: the contract is
then the 256-compute-unit one on any machine, and a rejected call launches nothing."""
import json
import os
import subprocess
import sys

import torch

_CHILD = r'''
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
_p, _i, _l, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
lib.hgr_gemm_nt_res_stats_wide_ok.argtypes = [_l, _l, _l, _l, _l, _l, _i]
lib.hgr_gemm_nt_res_stats_wide.argtypes = [_p, _l, _p, _l, _p, _p, _l, _p, _p, _f, _p, _i, _i, _i, _i, _p]
lib.hgr_last_error.restype = C.c_char_p
job = json.loads(sys.argv[2])
ok = [lib.hgr_gemm_nt_res_stats_wide_ok(*c) for c in job["ok"]]
ptr = lambda i, off=0: 0x100000000000 * (i + 1) + off          # distinct, aligned, never dereferenced
calls = []
for c in job["calls"]:
    m, n, k, lda, ldw, ldx, dt = c["shape"]
    ops = [ptr(i, c.get("off", {}).get(str(i), 0)) for i in range(7)]
    for i in c.get("null", []):
        ops[i] = None
    rc = lib.hgr_gemm_nt_res_stats_wide(ops[0], lda, ops[1], ldw, ops[2], ops[3], ldx, ops[4], ops[5], c.get("guard", 1e6), ops[6], m, n, k, dt, None)
    calls.append([rc, lib.hgr_last_error().decode()])
print(json.dumps({"ok": ok, "calls": calls}))
'''

BF16, F16 = 0, 1


def _limit(rows):
    """The smallest leading dimension with rows * ld * 2 >= 2^32, % 8 == 0."""
    return -(-(1 << 32) // (2 * rows * 8)) * 8


def test_wide_contract_and_entry_validation():
    from hgr_net_amd import _lib, ops
    la, lw = _limit(3200), _limit(2560)
    assert 3200 * (la - 8) * 2 < 1 << 32 <= 3200 * la * 2 and la < 1 << 21 and lw < 1 << 21
    cases = [  # (M, N, K, lda, ldw, ldx, dtype) -> covered
        ((319, 256, 256, 256, 256, 256, F16), 0), ((320, 256, 256, 256, 256, 256, F16), 1), ((640, 256, 256, 256, 256, 256, BF16), 1),
        ((0, 256, 256, 256, 256, 256, F16), 0),
        ((320, 128, 256, 256, 256, 128, F16), 0), ((320, 384, 256, 256, 256, 384, F16), 0), ((320, 0, 256, 256, 256, 256, F16), 0),
        ((320, 256, 128, 128, 128, 256, F16), 0), ((320, 256, 320, 320, 320, 256, F16), 0), ((320, 256, 384, 384, 384, 256, F16), 1),
        ((320, 256, 192, 192, 192, 256, F16), 0),
        # tiles against the 256 compute units: exactly as many, one more; ViT-B/32's c_proj at batch 512 (240) and 258 tiles of its width
        ((320 * 256, 256, 256, 256, 256, 256, F16), 1), ((320 * 257, 256, 256, 256, 256, 256, F16), 0),
        ((25600, 768, 3072, 3072, 3072, 768, F16), 1), ((320 * 86, 768, 3072, 3072, 3072, 768, F16), 0), ((25600, 768, 768, 768, 768, 768, BF16), 1),
        # strides: too short, misaligned, aligned and wider
        ((320, 256, 256, 248, 256, 256, F16), 0), ((320, 256, 256, 260, 256, 256, F16), 0), ((320, 256, 256, 264, 256, 256, F16), 1),
        ((320, 256, 256, 256, 260, 256, F16), 0), ((320, 256, 256, 256, 264, 256, F16), 1),
        ((320, 256, 256, 256, 256, 248, F16), 0), ((320, 256, 256, 256, 256, 260, F16), 0), ((320, 256, 256, 256, 256, 264, F16), 1),
        ((320, 256, 256, 1 << 21, 256, 256, F16), 0), ((320, 256, 256, (1 << 21) - 8, 256, 256, F16), 1),
        ((320, 256, 256, 256, 256, 1 << 23, F16), 0),
        # every operand below 4 GB: one step below the edge and at it, for A, W and the pair
        ((3200, 256, 256, la - 8, 256, 256, F16), 1), ((3200, 256, 256, la, 256, 256, F16), 0),
        ((320, 2560, 256, 256, lw - 8, 2560, F16), 1), ((320, 2560, 256, 256, lw, 2560, F16), 0),
        ((3200, 256, 256, 256, 256, la - 8, F16), 1), ((3200, 256, 256, 256, 256, la, F16), 0),
        ((320, 256, 256, 256, 256, 256, 2), 0), ((320, 256, 256, 256, 256, 256, -1), 0),
    ]
    good = (320, 256, 256, 256, 256, 256, F16)
    calls = [  # rejected before anything is launched: the stream is null and no operand exists
        {"shape": (319, 256, 256, 256, 256, 256, F16)},
        {"shape": (320, 256, 320, 320, 320, 256, F16)},
        {"shape": (320 * 257, 256, 256, 256, 256, 256, F16)},
        {"shape": (3200, 256, 256, la, 256, 256, F16)},
        {"shape": (320, 256, 256, 256, 256, 260, F16)},
        {"shape": (320, 256, 256, 256, 256, 256, 2)},
        {"shape": good, "null": [2]}, {"shape": good, "null": [4]},
        {"shape": good, "off": {"0": 8}}, {"shape": good, "off": {"3": 8}}, {"shape": good, "off": {"6": 2}},
        {"shape": good, "guard": 0.0},
    ]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HGR_")}
    child = subprocess.run([sys.executable, "-c", _CHILD, str(_lib.LIB_PATH), json.dumps({"ok": [c for c, _ in cases], "calls": calls})],
                           capture_output=True, text=True, timeout=120, env=dict(clean, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    assert child.returncode == 0, child.stderr[-2000:]
    got = json.loads(child.stdout)
    for (case, want), ok in zip(cases, got["ok"]):
        assert ok == want, (case, ok)
    for call, (rc, msg) in zip(calls, got["calls"]):
        assert rc != 0 and msg.startswith("hgr_gemm_nt_res_stats_wide:"), (call, rc, msg)
    assert "operands beyond 4 GB" in got["calls"][3][1] and "bad dtype" in got["calls"][5][1] and "null operand" in got["calls"][6][1]

    # the tensor-level wrapper asks the same function (dtype by torch type or by code; an unknown type is not covered)
    assert ops.gemm_nt_res_stats_wide_ok(320, 256, 256, 256, 256, 256, torch.float16) and ops.gemm_nt_res_stats_wide_ok(320, 256, 256, 256, 256, 256, BF16)
    assert not ops.gemm_nt_res_stats_wide_ok(319, 256, 256, 256, 256, 256, torch.bfloat16)
    assert not ops.gemm_nt_res_stats_wide_ok(320, 256, 256, 256, 256, 256, torch.float32)


def test_proj_wide_switch_is_read_once_with_by_shape_default():
    """HGR_PROJ_WIDE: 0 never, 1 (default, and anything unknown) by shape, 2 wherever the library covers the shape."""
    code = "from hgr_net_amd.clip import model; print(model.PROJ_WIDE)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k != "HGR_PROJ_WIDE"}
    for value, want in ((None, "1"), ("0", "0"), ("2", "2"), ("7", "1")):
        env = dict(base) if value is None else dict(base, HGR_PROJ_WIDE=value)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, env=env, timeout=300)
        assert out.stdout.strip() == want, (value, out.stdout, out.stderr[-500:])
