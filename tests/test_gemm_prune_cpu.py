"""Forward-GEMM dispatch after the schedule tables were pruned to the schedules that run (host arithmetic through
mtts_conv_gemm_plan / mtts_conv_gemm_workspace_size, no device).

Step plans pinned: every launch of the bf16-parity train step (profiles/r05/gemm_log_parity.jsonl: 161 records with
their full arguments) must plan the schedule, split count, workgroups, resident workgroups, rounds, fill and
workspace that the library planned at 173ec10, the last commit with the full tables.  The expectation is a recorded
list, tests/golden/gemm_step_plans.json, written by this file's __main__ from a build of 173ec10:

    MTTS_LIB=<173ec10 build>/lib/libmtts_hip.so python tests/test_gemm_prune_cpu.py

Removed ids rejected: the schedule ids that left the tables, and the kept ones in a precision they are not built
for, fail with MTTS_ERR_INVALID_ARG from the plan and answer 0 to the workspace query; the kept ids answer."""
import ctypes
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LOG = ROOT / "profiles" / "r05" / "gemm_log_parity.jsonl"
PINNED = Path(__file__).resolve().parent / "golden" / "gemm_step_plans.json"

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5  # include/mtts.h
REG_BF16, REG_F32 = (7, 12), (3, 7, 11, 18)
GLDS = (41, 42, 44, 45, 46, 47)
WREG = 96
REMOVED = [0, 1, 2, 4, 5, 6, 8, 9, 10, 13, 14, 15, 16, 17] + list(range(32, 41)) + [43]


def _records():
    return [json.loads(line) for line in LOG.read_text().splitlines() if line.strip()]


def _args(r):
    """The launch's mtts_conv_gemm_args from its log record; pointers are 16-byte aligned placeholders (the plan
    dereferences nothing), null where the launch passed none."""
    from matcha.models.components import _ops as O

    a = O.ConvGemmArgs()
    a.A, a.W, a.C = 4096, 8192, 12288
    a.a_scale = 16384 if r["asc"] else None
    a.bias = 20480 if r["bias"] else None
    a.residual = 24576 if r["res"] else None
    a.c_scale = 28672 if r["cs"] else None
    a.C_pre = 32768 if r["pre"] else None
    a.aux = 36864 if r["aux"] else None
    a.seed = 40960 if r["drop"] else None
    a.dropout_p = 0.1 if r["drop"] else 0.0
    a.lda, a.Ti, a.To, a.nb, a.in_stride = r["lda"], r["Ti"], r["To"], r["nb"], r["in_stride"]
    a.ntaps, a.cin = r["ntaps"], r["cin"]
    for j, o in enumerate(r["offs"]):
        a.off[j] = o
    a.N, a.K, a.Kp, a.act = r["N"], r["K"], r["Kp"], r["act"]
    a.ldr, a.ldc, a.ldaux = r["ldr"], r["ldc"], (r["ldc"] if r["aux"] else 0)
    a.To_full, a.out_stride, a.out_off = r["To_full"], r["out_stride"], r["out_off"]
    a.flags = r["flags"]
    return a


def _plan(a, prec, cfg=-1, splits=0):
    """(status, out[0:6]) of mtts_conv_gemm_plan."""
    from matcha import _native as N

    out = (ctypes.c_int32 * 6)()
    rc = N.lib().mtts_conv_gemm_plan(ctypes.byref(a), prec, cfg, splits, ctypes.byref(out))
    return rc, list(out)


def _ws(a, prec, cfg=-1, splits=0):
    from matcha import _native as N

    return int(N.lib().mtts_conv_gemm_workspace_size(ctypes.byref(a), prec, cfg, splits))


def _step_plans():
    plans = []
    for r in _records():
        a = _args(r)
        rc, out = _plan(a, r["prec"], r["cfg"], r["splits"])
        assert rc == 0, (rc, r)
        plans.append({"plan": out, "ws": _ws(a, r["prec"], r["cfg"], r["splits"])})
    return plans


def test_step_plans_pinned_to_the_full_tables():
    want = json.loads(PINNED.read_text())
    recs = _records()
    assert len(recs) == len(want) == 161
    got = _step_plans()
    for i, (r, g, w) in enumerate(zip(recs, got, want)):
        assert g == w, (i, {k: r[k] for k in ("M", "N", "K", "ntaps", "flags", "act", "prec")}, g, w)
    # the record covers every family of schedule the dispatch keeps
    ids = {w["plan"][0] for w in want}
    assert ids & set(REG_F32) and ids & set(REG_BF16) and ids & set(GLDS) and WREG in ids, sorted(ids)
    assert not ids & set(REMOVED), sorted(ids)


def _small(flags=0):
    """B = 2, T = 33, 64 -> 64 channels, one tap: valid for every schedule family (cin >= 64, K = 64 not among the
    weight-stationary kernel's K values)."""
    return _args(dict(asc=False, bias=False, res=False, cs=False, pre=False, aux=False, drop=False, lda=64, Ti=33, To=33,
                      nb=2, in_stride=1, ntaps=1, cin=64, offs=[0], N=64, K=64, Kp=64, act=0, ldr=0, ldc=64, To_full=33,
                      out_stride=1, out_off=0, flags=flags))


@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg", REMOVED)
def test_removed_ids_are_rejected(cfg, prec):
    a = _small()
    rc, _ = _plan(a, prec, cfg)
    assert rc == ERR_INVALID_ARG, (cfg, prec, rc)
    assert _ws(a, prec, cfg) == 0
    assert _ws(a, prec, cfg, 4) == 0


def test_kept_ids_answer_in_the_precisions_they_are_built_for():
    from matcha.models.components import _ops as O

    a = _small()
    for cfg in REG_BF16 + GLDS:
        rc, out = _plan(a, O.PREC_BF16, cfg)
        assert rc == 0 and out[0] == cfg and out[1] == 1, (cfg, rc, out)
    for cfg in REG_F32:
        rc, out = _plan(a, O.PREC_FP32, cfg)
        assert rc == 0 and out[0] == cfg, (cfg, rc, out)
    for prec in (O.PREC_FP32, O.PREC_BF16):
        rc, out = _plan(a, prec)
        assert rc == 0 and out[0] in ((3,) if prec == O.PREC_FP32 else REG_BF16), (prec, rc, out)
    # the register schedules that are built for one precision only
    for cfg, prec in [(12, O.PREC_FP32), (3, O.PREC_BF16), (11, O.PREC_BF16), (18, O.PREC_BF16)]:
        rc, _ = _plan(a, prec, cfg)
        assert rc == ERR_INVALID_ARG, (cfg, prec, rc)
        assert _ws(a, prec, cfg, 4) == 0
    # an LDS-DMA schedule at fp32 is refused as the launch refuses it: the kernels are bf16
    rc, _ = _plan(a, O.PREC_FP32, 41)
    assert rc == ERR_UNSUPPORTED, rc
    assert _ws(a, O.PREC_FP32, 41, 4) == 0
    # explicit split K on a kept fp32 schedule still sizes its slabs
    k = _args(dict(asc=False, bias=False, res=False, cs=False, pre=False, aux=False, drop=False, lda=64, Ti=33, To=33,
                   nb=2, in_stride=1, ntaps=3, cin=64, offs=[-1, 0, 1], N=64, K=192, Kp=192, act=0, ldr=0, ldc=64,
                   To_full=33, out_stride=1, out_off=0, flags=0))
    for cfg in REG_F32:
        assert _ws(k, O.PREC_FP32, cfg, 2) == 2 * 66 * 64 * 4, cfg


if __name__ == "__main__":
    import sys

    sys.path[:0] = [str(ROOT / "matcha-tts-etu-upmc-ensam_amd"), str(ROOT)]
    PINNED.write_text(json.dumps(_step_plans(), separators=(",", ":")).replace("},{", "},\n{") + "\n")
    print("wrote", PINNED)
