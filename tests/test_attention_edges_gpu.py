"""The attention kernels' block prologue and epilogue (csrc/attention.hip) at their edges.

Bitwise pin: tests/golden/attention_r9_hashes.json holds SHA-256 of o, lse and d(q|k|v) written by
tools/r9/attention_hashes.py on the build of 8b22a1e, before the row-fragment loads became unconditional loads from
clamped addresses and the bf16 stores 16 bytes wide.  Neither changes a value, a rounding or a summation order, so
the hashes must not move.

Bounds: the same call on compact tensors and on views cut from the middle of larger NaN-filled buffers (rows
before and after, a row pitch wider than H*D) gives bitwise the same results and leaves the surround untouched --
a clamped load that strays reads NaN, a wide store that strays overwrites one."""
from __future__ import annotations

import importlib.util
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = Path(__file__).resolve().parent.parent

_spec = importlib.util.spec_from_file_location("attention_hashes", ROOT / "tools" / "r9" / "attention_hashes.py")
AH = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(AH)
GOLDEN = json.loads((ROOT / "tests" / "golden" / "attention_r9_hashes.json").read_text())


def test_golden_covers_the_cases():
    assert sorted(GOLDEN) == sorted(AH.case_id(c) for c in AH.CASES)


@pytest.mark.parametrize("case", AH.CASES, ids=AH.case_id)
def test_attention_bitwise_equals_parent(case):
    want = GOLDEN[AH.case_id(case)]
    for _ in range(2):  # repeatable
        got = AH.hashes(case, DEV)
        assert got == want


def _nan_like(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _embed(t, pitch, rows_before, rows_after=3):
    """t [B, T, W] as a view of a NaN-filled [rows_before + B*T + rows_after, pitch] buffer -> (buffer, view)."""
    B, T, W = t.shape
    buf = _nan_like((rows_before + B * T + rows_after, pitch), t.dtype)
    view = buf[rows_before:rows_before + B * T, :W].view(B, T, W)
    view.copy_(t)
    return buf, view


def _surround_untouched(buf, view_filled_from, rows_before, W):
    """Everything of `buf` outside rows [rows_before, rows_before + n) x columns [0, W) is still NaN, bit for bit."""
    n = view_filled_from
    ref = _nan_like(buf.shape, buf.dtype)
    a = buf.clone()
    a[rows_before:rows_before + n, :W] = 0
    ref[rows_before:rows_before + n, :W] = 0
    ai = a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32)
    ri = ref.view(torch.int16) if ref.dtype == torch.bfloat16 else ref.view(torch.int32)
    return torch.equal(ai, ri)


def _run_strided(case, qkv, bias, dout, o, dqkv):
    """attention forward + backward through the C entry points on caller-made (possibly strided) tensors."""
    import ctypes
    import os

    from matcha import _native as N
    from matcha.models.components import _ops as O

    B, T, H, D, st, pr, p, short = case
    C = H * D
    prec = O.PREC_BF16 if pr == "bf16" else O.PREC_FP32
    seed = torch.tensor([1234, 99], dtype=torch.int32, device=DEV) if p > 0 else None
    lse = torch.empty(B, H, T, device=DEV)
    es = qkv.element_size()
    a = O.AttnArgs()
    a.q, a.k, a.v, a.ldq = qkv.data_ptr(), qkv.data_ptr() + C * es, qkv.data_ptr() + 2 * C * es, qkv.stride(1)
    a.key_bias, a.o, a.ldo, a.lse = bias.data_ptr(), o.data_ptr(), o.stride(1), lse.data_ptr()
    a.B, a.T, a.H, a.D, a.scale = B, T, H, D, 1.0 / (D ** 0.5)
    a.dropout_p, a.seed = float(p), N.ptr(seed)
    if st == "bf16":
        a.flags = O.ATTN_F_IO_BF16
    g = O.AttnGrads()
    g.dout, g.lddo = dout.data_ptr(), dout.stride(1)
    g.dq, g.dk, g.dv, g.ldd = dqkv.data_ptr(), dqkv.data_ptr() + C * es, dqkv.data_ptr() + 2 * C * es, dqkv.stride(1)
    lib = N.lib()
    ws = torch.empty(int(lib.mtts_attention_bwd_workspace_size(B, T, H)), dtype=torch.uint8, device=DEV)
    old = os.environ.get("MTTS_ATTN_SHORT")
    if short is not None:
        os.environ["MTTS_ATTN_SHORT"] = short
    try:
        N.check(lib.mtts_attention_fwd(ctypes.byref(a), prec, O._stream(qkv)), "mtts_attention_fwd")
        N.check(lib.mtts_attention_bwd(ctypes.byref(a), ctypes.byref(g), prec, ws.data_ptr(), ws.numel(),
                                       O._stream(qkv)), "mtts_attention_bwd")
        torch.cuda.synchronize()
    finally:
        if short is not None:
            if old is None:
                del os.environ["MTTS_ATTN_SHORT"]
            else:
                os.environ["MTTS_ATTN_SHORT"] = old
    return lse


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# extra elements per row: 8 keeps a bf16 row pitch 16-byte aligned (the 16-byte store path), 4 leaves it 8-byte
# aligned (the 8-byte stores); fp32 rows are 16-byte aligned with either
@pytest.mark.parametrize("extra", [8, 4])
@pytest.mark.parametrize("case", AH.CASES, ids=AH.case_id)
def test_attention_stays_inside_its_rows_and_columns(case, extra):
    B, T, H, D, st, pr, p, short = case
    C = H * D
    qkv, bias, dout = AH.make_inputs(case, DEV)
    o_c = torch.empty(B, T, C, device=DEV, dtype=qkv.dtype)
    d_c = torch.empty(B, T, 3 * C, device=DEV, dtype=qkv.dtype)
    lse_c = _run_strided(case, qkv, bias, dout, o_c, d_c)

    rb = 4  # rows before: keeps the views' bases 16-byte aligned for both pitches (4 * pitch * 2 bytes)
    qbuf, qv = _embed(qkv, 3 * C + extra, rows_before=rb)
    gbuf, gv = _embed(dout, C + extra, rows_before=rb)
    obuf, ov = _embed(torch.zeros_like(o_c), C + extra, rows_before=rb)
    dbuf, dv = _embed(torch.zeros_like(d_c), 3 * C + extra, rows_before=rb)
    # the outputs' own cells start as NaN too: every one of them must be written
    ov.fill_(float("nan"))
    dv.fill_(float("nan"))
    lse_v = _run_strided(case, qv, bias, gv, ov, dv)

    assert torch.equal(_bits(ov), _bits(o_c))
    assert torch.equal(_bits(dv), _bits(d_c))
    assert torch.equal(lse_v.view(torch.int32), lse_c.view(torch.int32))
    assert _surround_untouched(obuf, B * T, rb, C)
    assert _surround_untouched(dbuf, B * T, rb, 3 * C)
    assert _surround_untouched(qbuf, B * T, rb, 3 * C) and torch.equal(_bits(qv), _bits(qkv))
    assert _surround_untouched(gbuf, B * T, rb, C) and torch.equal(_bits(gv), _bits(dout))
