"""Replays rows of tests/golden/gemm_plans.json through hgr_gemm_plan_capture (tests/test_abi_and_host.py::test_gemm_plans_match_golden).

A row is {"entry", "args", "knobs", "env", "launches"}: one call of an NT-family entry point with fake, aligned, non-null operand
addresses (host only: nothing is dereferenced and nothing is launched), the knob setters in force, the environment of the process,
and the launches the call makes.  The library reads its environment once, so the rows of one "env" share a fresh process:

    python gemm_plan_replay.py libhgr.so rows.json      (the environment of the rows set by the parent)  ->  one JSON list of launch lists

The table holds the plans of 256 CUs (an MI355X, and what the library assumes without a device) and of no other HGR_* variable than
the row's; the test starts the process accordingly.

The child loads the library with bare ctypes (no torch: it starts in a tenth of a second), hence the prototypes below; the test
checks them against hgr_net_amd._lib.SIGNATURES.
"""
import ctypes as C
import json
import sys
from pathlib import Path

FIELDS = ("kernel", "variant", "epilogue", "out_f32", "act", "grid_x", "grid_y", "tiles_m", "tiles_n", "total",
          "nbig", "big_panels", "tiles_m_half", "group", "m_fastest", "vec_ok", "row0", "rows")
F16 = 1
EPI_HAS_BIAS = (1, 2, 3, 4, 5)          # every epilogue but NONE, ACCUM, QGELU_GRAD16
EPI_HAS_SECOND = (3, 5, 7)              # BIAS_RESIDUAL, BIAS_ADD16_RELU, QGELU_GRAD16

_p, _i, _l, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
ARGTYPES = {
    "hgr_gemm_nt": [_p, _l, _p, _l, _p, _l, _p, _p, _l, _i, _i, _i, _i, _i, _i, _p],
    "hgr_gemm_nt_splitk": [_p, _l, _p, _l, _p, _l, _i, _i, _i, _i, _i, _p],
    "hgr_conv3x3_nhwc": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "hgr_conv3x3_nhwc_plain": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p],
    "hgr_gemm_nt_res_stats": [_p, _l, _p, _l, _p, _p, _l, _p, _p, _i, _i, _i, _i, _p],
    "hgr_gemm_nt_res_stats_guard": [_p, _l, _p, _l, _p, _p, _l, _p, _p, _f, _p, _i, _i, _i, _i, _p],
    "hgr_gemm_nt_ln": [_p, _l, _p, _l, _p, _l, _p, _p, _p, _f, _i, _i, _i, _i, _i, _p],
    "hgr_gemm_nt_bias_gelu_dual": [_p, _l, _p, _l, _p, _l, _p, _l, _p, _i, _i, _i, _i, _p],
    "hgr_gemm_nt_qgelu_grad_colsum": [_p, _l, _p, _l, _p, _l, _p, _l, _p, _i, _i, _i, _i, _p],
    "hgr_gemm_plan_capture": [_p, _i],
    "hgr_gemm_set_tile": [_i], "hgr_gemm_set_tail": [_i, _i], "hgr_gemm_set_persist": [_i], "hgr_gemm_set_p8": [_i],
}


def _ptr(i, off=0):
    """Operand i of a call: distinct, 4 KiB-aligned, never dereferenced."""
    return C.c_void_p(0x100000000000 * (i + 1) + off)


def call(lib, entry, a):
    """The one library call a row describes; returns its status."""
    dt = a.get("dtype", F16)
    if entry == "gemm_nt":
        m, n, k, epi = a["M"], a["N"], a["K"], a["epilogue"]
        second = epi in EPI_HAS_SECOND
        return lib.hgr_gemm_nt(_ptr(0), a.get("lda", k), _ptr(1), a.get("ldw", k), _ptr(2, a.get("c_off", 0)), a.get("ldc", n),
                               _ptr(3, a.get("bias_off", 0)) if epi in EPI_HAS_BIAS else None, _ptr(4, a.get("res_off", 0)) if second else None,
                               a.get("ldr", n if second else 0), m, n, k, dt, epi, a["out_f32"], None)
    if entry == "gemm_nt_splitk":
        return lib.hgr_gemm_nt_splitk(_ptr(0), a["K"], _ptr(1), a["K"], _ptr(2), a.get("ldc", a["N"]), a["M"], a["N"], a["K"], a["kc"], dt, None)
    if entry == "conv3x3_nhwc":
        return lib.hgr_conv3x3_nhwc(_ptr(0), _ptr(1), _ptr(2), _ptr(3, a.get("out_off", 0)), a["B"], a["H"], a["W"], a["C"], a["Cout"], a["stride"], a["Kp"], dt, None)
    if entry == "conv3x3_nhwc_plain":
        return lib.hgr_conv3x3_nhwc_plain(_ptr(0), _ptr(1), _ptr(3, a.get("out_off", 0)), a["B"], a["H"], a["W"], a["C"], a["Cout"], a["Kp"], dt, None)
    m, n, k = a["M"], a["N"], a["K"]
    if entry == "gemm_nt_res_stats":
        return lib.hgr_gemm_nt_res_stats(_ptr(0), k, _ptr(1), k, _ptr(2), _ptr(3), n, _ptr(4), _ptr(5), m, n, k, dt, None)
    if entry == "gemm_nt_res_stats_guard":
        return lib.hgr_gemm_nt_res_stats_guard(_ptr(0), k, _ptr(1), k, _ptr(2), _ptr(3), n, _ptr(4), _ptr(5), 1e6, _ptr(6), m, n, k, dt, None)
    if entry == "gemm_nt_ln":
        return lib.hgr_gemm_nt_ln(_ptr(0), k, _ptr(1), k, _ptr(2), n, _ptr(3), _ptr(4), _ptr(5), 1e-5, m, n, k, dt, a["act"], None)
    if entry == "gemm_nt_bias_gelu_dual":
        return lib.hgr_gemm_nt_bias_gelu_dual(_ptr(0), k, _ptr(1), k, _ptr(2), n, _ptr(3), n, _ptr(4), m, n, k, dt, None)
    if entry == "gemm_nt_qgelu_grad_colsum":
        return lib.hgr_gemm_nt_qgelu_grad_colsum(_ptr(0), k, _ptr(1), k, _ptr(2), n, _ptr(3), n, _ptr(4), m, n, k, dt, None)
    raise ValueError(entry)


def set_knobs(lib, knobs):
    """Applies {"tile", "tail": [enabled, full_panels], "persist", "p8"} through the setters; returns what restores them (the
    setters return the previous value; hgr_gemm_set_tail that of `enabled` only, so full_panels goes back to -1 = choose, which is
    what a process that forced no panel count has)."""
    prev = {}
    for name, value in knobs.items():
        fn = getattr(lib, "hgr_gemm_set_" + name)
        old = fn(*value) if name == "tail" else fn(value)
        assert old >= 0, (name, value, lib.hgr_last_error())
        prev[name] = [1 if old else 0, -1] if name == "tail" else old
    return prev


def replay(lib, rows):
    """The launches every row plans, as lists of dicts with FIELDS; the knobs are back where they were afterwards."""
    out = []
    for row in rows:
        buf = (C.c_int32 * (len(FIELDS) * 4))()
        prev = set_knobs(lib, row.get("knobs", {}))
        try:
            assert lib.hgr_gemm_plan_capture(buf, 4) == 0
            rc = call(lib, row["entry"], row["args"])
            assert rc == 0, (row, rc, lib.hgr_last_error())
        finally:
            set_knobs(lib, prev)
        recs = [dict(zip(FIELDS, buf[i * len(FIELDS):(i + 1) * len(FIELDS)])) for i in range(4)]
        out.append(recs[:next(i for i, r in enumerate(recs + [{"kernel": 0}]) if r["kernel"] == 0)])
    return out


if __name__ == "__main__":
    lib = C.CDLL(sys.argv[1])
    for name, argtypes in ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes
    lib.hgr_last_error.restype = C.c_char_p
    print(json.dumps(replay(lib, json.loads(Path(sys.argv[2]).read_text()))))
