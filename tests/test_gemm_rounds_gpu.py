"""160-row LDS-DMA schedules (csrc/conv_gemm_glds.hip: 46 = 160 x 64 two-stage, ten waves; 47 = 160 x 128 three-stage):
the same v_mfma_f32_32x32x16_bf16 products in the same K order as the 64-row schedules, so every output is compared
BITWISE with the current schedule of the same operand kind -- 44 (bf16 A) / 45 (fp32 A) for the 64-wide tile, 41 for
the 128-wide one -- on the smallest shapes at which a 160-row tile can go wrong: a 20-row partial tile with the batch
edge (and the 3-tap halo) inside a tile, a tile that is mostly padding, fewer K steps than stages, a K step count that
is no multiple of the stage count, a tap change on every K step, the register-addressed loop (cin % 64 != 0), partial
N tiles, a 0/1 row mask with zero rows at the tile edges, one and two weight planes, every epilogue term through the
16-byte and the generic epilogue, and split K.  Plus the schedule table's resident-workgroups figure of every
instantiation against the runtime's occupancy answer."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# (schedule, bf16 A, split weights) with an instantiation of its own, and the current schedule it must equal
COMBOS = [(46, False, False), (46, False, True), (46, True, False), (46, True, True), (47, True, False), (47, True, True)]


def _old(sched, a16):
    return 41 if sched == 47 else (44 if a16 else 45)


_CACHE = {}


def _operands(B, T, cin, taps, N, a16, split):
    """Inputs of one case, built once and shared (never modified): A, packed W, Kp."""
    from matcha.models.components import _ops as O

    key = (B, T, cin, taps, N, a16, split)
    if key not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(B * 1000 + T + cin + taps + N)
        K = cin * taps
        x = torch.randn(B, T, cin, generator=g).to(DEV)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
        if split:
            hi = w.bfloat16()
            Wp = torch.cat([hi, (w - hi.float()).bfloat16()]).contiguous()
            Wp._mtts_w_split = True
            Kp = K
        else:
            Wp, Kp = O.pack_weight(w, O.PREC_BF16)
        _CACHE[key] = (x.bfloat16() if a16 else x, Wp, Kp)
    return _CACHE[key]


def _edge_mask(B, T):
    """0/1 row mask with zero rows on both sides of every 160-row tile edge and at the batch edge."""
    m = torch.ones(B * T)
    for r in range(0, B * T, 160):
        m[max(r - 2, 0):r + 2] = 0
    for r in range(T, B * T, T):
        m[r - 1:r + 1] = 0
    m[-3:] = 0
    return m.to(DEV)


def _run(cfg, B, T, cin, taps, N, a16, split, masked=False, splits=0, **epi):
    from matcha.models.components import _ops as O

    A, Wp, Kp = _operands(B, T, cin, taps, N, a16, split)
    stride2 = epi.pop("stride2", False)
    c16 = epi.pop("c16", False)
    To_full = 2 * T if stride2 else T
    C = torch.full((B, To_full, N), 7.0, device=DEV, dtype=torch.bfloat16 if c16 else torch.float32)
    kw = dict(epi)
    if masked:
        kw["a_scale"] = _edge_mask(B, T)
    if stride2:
        kw.update(out_stride=2, out_off=1)
    offs = [j - (taps - 1) // 2 for j in range(taps)]
    O._gemm(A, T, T, B, 1, offs, cin, Wp, Kp, N, C, To_full, prec=O.PREC_BF16, tile_cfg=cfg, splits=splits, **kw)
    torch.cuda.synchronize()
    return C


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N", [64, 96])  # whole tiles / a partial N tile (W rows past N: w_nok)
@pytest.mark.parametrize("cin,taps", [(64, 1), (64, 3), (320, 1), (96, 3)])  # nk = 1, 3 (a tap per step), 5; register-addressed loop
@pytest.mark.parametrize("B,T", [(2, 170), (1, 33)])  # M = 340: 2 tiles + 20 rows, batch edge inside tile 2; one tile, mostly padding
@pytest.mark.parametrize("sched,a16,split", COMBOS)
def test_160_row_schedules_bitwise(sched, a16, split, B, T, cin, taps, N, masked):
    got = _run(sched, B, T, cin, taps, N, a16, split, masked)
    want = _run(_old(sched, a16), B, T, cin, taps, N, a16, split, masked)
    assert torch.isfinite(got).all() and not (got == 7.0).all()
    assert torch.equal(got, want)


def _epilogue(kind, B, T, N):
    g = torch.Generator(device="cpu").manual_seed(11)
    if kind == "bias":
        return dict(bias=torch.randn(N, generator=g).to(DEV))
    if kind == "residual":
        return dict(residual=torch.randn(B, T, N, generator=g).to(DEV))
    if kind == "c16":
        return dict(c16=True)
    if kind == "stride2":
        return dict(stride2=True, bias=torch.randn(N, generator=g).to(DEV))
    return dict(dropout_p=0.1, seed=torch.tensor([1234, 567], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("N", [96, 62])  # N % 4 == 0: the 16-byte epilogue; N % 4 != 0: the generic one
@pytest.mark.parametrize("kind", ["bias", "residual", "c16", "stride2", "dropout"])
@pytest.mark.parametrize("sched,a16,split", COMBOS)
def test_160_row_epilogues_bitwise(sched, a16, split, kind, N):
    B, T, cin, taps = 2, 170, 64, 3
    got = _run(sched, B, T, cin, taps, N, a16, split, True, **_epilogue(kind, B, T, N))
    want = _run(_old(sched, a16), B, T, cin, taps, N, a16, split, True, **_epilogue(kind, B, T, N))
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)  # the rows a stride-2 phase leaves alone keep their fill in both
    if kind == "stride2":
        assert (got[:, 0::2] == 7.0).all() and not (got[:, 1::2] == 7.0).all()


@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("sched,a16,split", COMBOS)
def test_160_row_split_k_bitwise(sched, a16, split, splits):
    """Split K runs on the new schedules as on the old: the same split count sums the same partials in the same
    order."""
    B, T, cin, taps, N = 2, 170, 128, 3, 96  # 6 K steps
    bias = torch.arange(N, dtype=torch.float32, device=DEV) / N
    got = _run(sched, B, T, cin, taps, N, a16, split, True, splits=splits, bias=bias)
    want = _run(_old(sched, a16), B, T, cin, taps, N, a16, split, True, splits=splits, bias=bias)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_table_resident_workgroups_vs_runtime_occupancy():
    """The table's resident workgroups per CU (LDS and threads) of every LDS-DMA instantiation against
    hipOccupancyMaxActiveBlocksPerMultiprocessor: never above the runtime's answer, at most one below it (the API can
    answer one too high)."""
    from matcha import _native as N

    lib = N.lib()
    seen = set()
    for sched in range(32, 96):
        for kind in range(5):
            for lean in (0, 1):
                out = (ctypes.c_int32 * 2)()
                if lib.mtts_conv_gemm_glds_occupancy(sched, kind, lean, ctypes.byref(out)) != 0:
                    continue  # no instantiation of its own for this kind
                seen.add((sched, kind))
                table, api = out[0], out[1]
                print(sched, kind, lean, "table", table, "runtime", api)
                assert table >= 1 and api - 1 <= table <= api, (sched, kind, lean, table, api)
    for want in [(41, 0), (41, 1), (41, 2), (41, 3), (44, 3), (44, 4), (45, 2), (46, 0), (46, 1), (46, 2), (46, 3),
                 (47, 1), (47, 3)]:
        assert want in seen, want
