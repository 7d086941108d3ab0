"""mtts_conv_gemm_plan (host arithmetic, no device): the schedule pick by rounds on the train step's decoder GEMMs.

The benched step (B = 32, 600 mel frames, channels (256, 256); matcha/models/components/decoder.py) runs its N = 256
convs and linears on 19200 rows (full resolution) and 9600 rows (half resolution and the mid blocks):
  K = 768   k = 3 convs over 256 channels (ResnetBlock1D block2 / block1, the level's last conv, final_block)
  K = 1024  the FeedForward down-projection (one tap over 1024 channels)
  K = 1536  block1 of the up path's ResnetBlock1D over the 512-channel skip concat (k = 3)
  K = 512   its 1x1 res_conv (one tap over 512 channels), and on 9600 rows the two 2-tap phases of the
            ConvTranspose1d(4, 2, 1) upsample over 256 channels
each with the operand kinds the bf16-parity policy produces (profiles/r06/final/launches.txt: fp32 or bf16 A with
split weight planes in the forward, one plane in the backward).  Pinned per case: the schedule id and split count;
checked: tiles, rounds and fill against the arithmetic, the plan of the picked id given explicitly, and the
workspace-size query against the plan's splits."""
import ctypes

import pytest

from matcha import _native as N

ROWS = {9600: (32, 300), 19200: (32, 600)}
KS = {768: (256, 3), 1024: (1024, 1), 1536: (512, 3), 512: (512, 1), (512, 2): (256, 2)}
KIND_NAMES = ["fp32 A", "bf16 A", "fp32 A, split W", "bf16 A, split W"]
# schedule -> (rows, cols) of its tile; (schedule, kind) -> resident workgroups per CU = min(160 KiB / (stages x
# stage bytes), 2048 threads / workgroup), stage bytes = rows x 64 x (2 | 4) + planes x cols x 128
TILE = {41: (64, 256), 42: (64, 256), 45: (64, 64), 46: (160, 64), 47: (160, 128)}
RESIDENT = {(45, 0): 3, (46, 0): 1, (46, 1): 2, (46, 2): 1, (46, 3): 2, (47, 1): 1, (47, 3): 1, (42, 0): 1}


def _expected(rows, k, kind):
    """The pinned pick: 160 x 128 (47) for a bf16 A on 19200 rows -- 240 workgroups, one round of the 256 one-resident
    slots; 160 x 64 (46) on 9600 rows -- 240 workgroups -- and for an fp32 A with split weights on 19200 -- 480,
    two rounds at 94 %; fp32 A with one plane: 64 x 64 two-stage (45) past one round of 64 x 256 tiles (the measured
    exception), and the register schedule 12 below K = 768 (outside the LDS-DMA pick)."""
    K = k if isinstance(k, int) else k[0]
    if kind == 0:
        if K < 768:
            return 12
        return 45 if rows == 19200 else 46
    if kind in (1, 3):
        return 47 if rows == 19200 else 46
    return 46


def _args(B, T, cin, taps, Nn, kind):
    from matcha.models.components import _ops as O

    a = O.ConvGemmArgs()
    a.A, a.W, a.C = 4096, 8192, 12288  # 16-byte aligned placeholders: the plan dereferences nothing
    a.lda, a.Ti, a.To, a.nb, a.in_stride, a.ntaps, a.cin = cin, T, T, B, 1, taps, cin
    for j in range(taps):
        a.off[j] = j - (taps - 1) // 2
    a.N, a.K, a.Kp = Nn, cin * taps, cin * taps
    a.ldc, a.To_full, a.out_stride = Nn, T, 1
    a.flags = (O.GEMM_F_A_BF16 if kind & 1 else 0) | (O.GEMM_F_W_SPLIT if kind & 2 else 0)
    return a


def _plan(a, cfg=-1, splits=0):
    from matcha.models.components import _ops as O

    out = (ctypes.c_int32 * 6)()
    N.check(N.lib().mtts_conv_gemm_plan(ctypes.byref(a), O.PREC_BF16, cfg, splits, ctypes.byref(out)), "plan")
    return list(out)


def _ceil(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=KIND_NAMES)
@pytest.mark.parametrize("k", list(KS), ids=[str(k) for k in KS])
@pytest.mark.parametrize("rows", [9600, 19200])
def test_step_decoder_gemm_plans(rows, k, kind):
    from matcha.models.components import _ops as O

    B, T = ROWS[rows]
    cin, taps = KS[k]
    a = _args(B, T, cin, taps, 256, kind)
    sched, splits, tiles, resident, nrounds, fill = _plan(a)
    assert sched == _expected(rows, k, kind), (sched, rows, k, KIND_NAMES[kind])
    assert splits == 1
    if sched >= O.GEMM_GLDS:
        bm, bn = TILE[sched]
        assert tiles == _ceil(rows, bm) * _ceil(256, bn)
        assert resident == RESIDENT[(sched, kind)]
        assert nrounds == _ceil(tiles, 256 * resident)
        assert fill == 1000 * tiles // (nrounds * 256 * resident)
    else:
        assert (tiles, resident, nrounds, fill) == (0, 0, 0, 0)
    assert _plan(a, cfg=sched) == [sched, splits, tiles, resident, nrounds, fill]
    ws = N.lib().mtts_conv_gemm_workspace_size(ctypes.byref(a), O.PREC_BF16, -1, 0)
    assert ws == 0  # unsplit


def test_fills_of_the_160_row_tiles():
    """The figures the schedules were built for: 240 workgroups on 256 slots, 480 on 512 (94 %), against 59 % for
    the 64-row tiles they replace (300 of 512, 600 of 1024, 150 of 256)."""
    a = _args(32, 600, 256, 3, 256, 3)
    assert _plan(a)[2:] == [240, 1, 1, 937]
    assert _plan(a, cfg=41)[2:] == [300, 1, 2, 585]
    a = _args(32, 300, 256, 3, 256, 3)
    assert _plan(a)[2:] == [240, 2, 1, 468]  # one round of the two-resident schedule: one workgroup per CU
    assert _plan(a, cfg=44)[2:] == [600, 2, 2, 585]
    a = _args(32, 300, 256, 3, 256, 2)
    assert _plan(a)[2:] == [240, 1, 1, 937]
    assert _plan(a, cfg=41)[2:] == [150, 1, 1, 585]


def test_long_form_rows_use_the_same_function():
    """B = 8, 512 x 4096: 32768 and 16384 rows are 205 and 103 row tiles of 160 (the last one partial); the pick is
    the same modelled-time minimum, and whatever it picks its figures are the arithmetic of that schedule."""
    from matcha.models.components import _ops as O

    for rows, (B, T) in {32768: (8, 4096), 16384: (8, 2048)}.items():
        for kind in (1, 2, 3):
            a = _args(B, T, 256, 3, 256, kind)
            sched, splits, tiles, resident, nrounds, fill = _plan(a)
            assert sched in TILE and splits == 1
            bm, bn = TILE[sched]
            assert tiles == _ceil(rows, bm) * _ceil(256, bn)
            assert nrounds == _ceil(tiles, 256 * resident) and fill == 1000 * tiles // (nrounds * 256 * resident)
            assert _plan(a, cfg=sched) == [sched, splits, tiles, resident, nrounds, fill]


def test_split_k_plan_agrees_with_the_workspace_query():
    """The split-K rule (schedule 42 only) stays: the text encoder's 3840 x 192 x 2304 conv splits K four ways, the
    plan counts tiles x splits workgroups, and the size query asks for exactly the plan's slabs."""
    from matcha.models.components import _ops as O

    a = _args(32, 120, 768, 3, 192, 0)
    sched, splits, tiles, resident, nrounds, fill = _plan(a)
    assert (sched, splits) == (42, 4)
    assert tiles == _ceil(3840, 64) * 1 * 4 and resident == 1 and nrounds == 1 and fill == 1000 * 240 // 256
    ws = N.lib().mtts_conv_gemm_workspace_size(ctypes.byref(a), O.PREC_BF16, -1, 0)
    assert ws == splits * 3840 * 192 * 4
    assert _plan(a, cfg=sched) == [sched, splits, tiles, resident, nrounds, fill]
    assert _plan(a, splits=1)[:2] == [42, 1]
    assert N.lib().mtts_conv_gemm_workspace_size(ctypes.byref(a), O.PREC_BF16, -1, 1) == 0
