"""Each fused decoder operator (HIP, token-major) against a plain PyTorch fp32 reference of the same
op, forward and backward.  Tolerances (relative L2): fp32 MFMA mode 2e-5 fwd / 1e-4 grads; bf16 MFMA
mode 1.5e-2 (bf16 operand rounding, fp32 accumulation)."""
from __future__ import annotations

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {"fp32": (2e-5, 1e-4), "bf16": (1.5e-2, 1.5e-2)}


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _ctx(prec):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=(prec == "bf16"))


def _mask(B, T, lengths):
    m = torch.zeros(B, T, device=DEV)
    for b, L in enumerate(lengths):
        m[b, :L] = 1
    return m


def _run(fn, ref, inputs, prec):
    """fn/ref take the same leaf tensors; compares outputs and all input grads."""
    torch.manual_seed(0)
    xs = [t.detach().clone().requires_grad_(t.requires_grad) for t in inputs]
    rs = [t.detach().clone().requires_grad_(t.requires_grad) for t in inputs]
    with _ctx(prec):
        y = fn(*xs)
    yr = ref(*rs)
    g = torch.randn_like(yr)
    (y * g).sum().backward()
    (yr * g).sum().backward()
    ftol, gtol = TOL[prec]
    assert rel(y, yr) < ftol, rel(y, yr)
    for a, b in zip(xs, rs):
        if b.grad is not None:
            assert a.grad is not None
            assert rel(a.grad, b.grad) < gtol, (tuple(b.shape), rel(a.grad, b.grad))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,Cin,Cout,k,stride,pad,masked", [
    (2, 37, 32, 64, 3, 1, 1, True), (3, 64, 160, 256, 3, 1, 1, True), (2, 40, 64, 48, 1, 1, 0, True),
    (2, 41, 32, 32, 3, 2, 1, True), (2, 64, 256, 256, 3, 2, 1, True), (1, 300, 512, 256, 3, 1, 1, False),
    (2, 33, 256, 80, 1, 1, 0, True)])
def test_conv_tm(prec, B, T, Cin, Cout, k, stride, pad, masked):
    from matcha.models.components._ops import conv_tm

    x = torch.randn(B, T, Cin, device=DEV, requires_grad=True)
    w = (torch.randn(Cout, Cin, k, device=DEV) / math.sqrt(Cin * k)).requires_grad_(True)
    b = torch.randn(Cout, device=DEV, requires_grad=True)
    m = _mask(B, T, [T - 5 * i for i in range(B)]) if masked else None

    def ref(x, w, b):
        xx = x * m.unsqueeze(-1) if m is not None else x
        return F.conv1d(xx.transpose(1, 2), w, b, stride=stride, padding=pad).transpose(1, 2)

    _run(lambda x, w, b: conv_tm(x, w, b, m, stride=stride, padding=pad), ref, [x, w, b], prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_tm_out_scale(prec):
    from matcha.models.components._ops import conv_tm

    B, T = 2, 50
    x = torch.randn(B, T, 256, device=DEV, requires_grad=True)
    w = (torch.randn(80, 256, 1, device=DEV) / 16).requires_grad_(True)
    b = torch.randn(80, device=DEV, requires_grad=True)
    m = _mask(B, T, [50, 31])
    ref = lambda x, w, b: (F.conv1d((x * m[..., None]).transpose(1, 2), w, b).transpose(1, 2) * m[..., None])
    _run(lambda x, w, b: conv_tm(x, w, b, m, padding=0, out_scale=m), ref, [x, w, b], prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C", [(2, 19, 32), (3, 150, 256)])
def test_conv_transpose_tm(prec, B, T, C):
    from matcha.models.components._ops import conv_transpose_tm

    x = torch.randn(B, T, C, device=DEV, requires_grad=True)
    w = (torch.randn(C, C, 4, device=DEV) / math.sqrt(C * 2)).requires_grad_(True)
    b = torch.randn(C, device=DEV, requires_grad=True)
    m = _mask(B, T, [T - 3 * i for i in range(B)])
    ref = lambda x, w, b: F.conv_transpose1d((x * m[..., None]).transpose(1, 2), w, b, 2, 1).transpose(1, 2)
    _run(lambda x, w, b: conv_transpose_tm(x, w, b, m), ref, [x, w, b], prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("M,K,Nn,res", [(300, 256, 768, False), (4800, 256, 256, True), (77, 32, 96, True)])
def test_linear_tm(prec, M, K, Nn, res):
    from matcha.models.components._ops import linear_tm

    x = torch.randn(2, M // 2 if M % 2 == 0 else M, K, device=DEV, requires_grad=True)
    w = (torch.randn(Nn, K, device=DEV) / math.sqrt(K)).requires_grad_(True)
    b = torch.randn(Nn, device=DEV, requires_grad=True)
    r = torch.randn(*x.shape[:-1], Nn, device=DEV, requires_grad=True)
    if res:
        _run(lambda x, w, b, r: linear_tm(x, w, b, residual=r), lambda x, w, b, r: F.linear(x, w, b) + r,
             [x, w, b, r], prec)
    else:
        _run(lambda x, w, b: linear_tm(x, w, b), lambda x, w, b: F.linear(x, w, b), [x, w, b], prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("M,C", [(600, 256), (130, 32)])
def test_ff_tm(prec, M, C):
    from matcha.models.components._ops import ff_tm

    x = torch.randn(M, C, device=DEV, requires_grad=True)
    w1 = (torch.randn(4 * C, C, device=DEV) / math.sqrt(C)).requires_grad_(True)
    b1 = torch.randn(4 * C, device=DEV, requires_grad=True)
    w2 = (torch.randn(C, 4 * C, device=DEV) / math.sqrt(4 * C)).requires_grad_(True)
    b2 = torch.randn(C, device=DEV, requires_grad=True)
    r = torch.randn(M, C, device=DEV, requires_grad=True)
    ref = lambda x, w1, b1, w2, b2, r: F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2) + r
    _run(lambda x, w1, b1, w2, b2, r: ff_tm(x, w1, b1, w2, b2, residual=r), ref, [x, w1, b1, w2, b2, r], prec)


def test_dropout_epilogues_consistent(monkeypatch):
    """Train-mode dropout: about p of the outputs dropped, survivors scaled 1/(1-p), and the backward
    regenerates the same mask (checked against an explicit-mask torch computation; for the FeedForward, whose
    mask is hidden behind the second Linear, the mask recomputed on the host from the recorded seed)."""
    import dropout_ref as DR
    import numpy as np

    from matcha.models.components import _ops as O
    from matcha.models.components._ops import ff_tm, linear_tm

    seeds, new_seed = [], O._new_seed
    monkeypatch.setattr(O, "_new_seed", lambda device: seeds.append(new_seed(device)) or seeds[-1])
    torch.manual_seed(1)
    M, K, Nn, p = 2048, 256, 256, 0.25
    x = torch.randn(M, K, device=DEV, requires_grad=True)
    w = (torch.randn(Nn, K, device=DEV) / 16).requires_grad_(True)
    y = linear_tm(x, w, None, dropout_p=p)
    full = F.linear(x.detach(), w.detach())
    keep = y.detach() != 0
    frac = 1 - keep.float().mean().item()
    assert abs(frac - p) < 0.01, frac
    torch.testing.assert_close(y.detach()[keep], full[keep] / (1 - p), rtol=1e-5, atol=1e-5)
    g = torch.randn_like(y)
    (y * g).sum().backward()
    exp_dx = (g * keep / (1 - p)) @ w.detach()
    assert rel(x.grad, exp_dx) < 1e-5
    # FF: dropout between GELU and the second Linear
    w1 = (torch.randn(4 * K, K, device=DEV) / 16).requires_grad_(True)
    w2 = (torch.randn(K, 4 * K, device=DEV) / 32).requires_grad_(True)
    xx = torch.randn(M, K, device=DEV, requires_grad=True)
    y2 = ff_tm(xx, w1, None, w2, None, dropout_p=p)
    (y2 * g).sum().backward()
    assert len(seeds) == 2  # linear_tm's, then ff_tm's
    drop = torch.from_numpy(DR.keep_mask(seeds[1], np.arange(M), np.arange(4 * K), p)).to(DEV).double()
    drop = drop * float(np.float32(DR.keep_scale(p)))
    xr, w1r, w2r = (t.detach().double().requires_grad_(True) for t in (xx, w1, w2))
    y2r = F.linear(F.gelu(F.linear(xr, w1r)) * drop, w2r)
    (y2r * g.double()).sum().backward()
    ftol, gtol = TOL["fp32"]
    assert rel(y2, y2r) < ftol, rel(y2, y2r)
    for got, want in ((xx.grad, xr.grad), (w1.grad, w1r.grad), (w2.grad, w2r.grad)):
        assert rel(got, want) < gtol, (tuple(want.shape), rel(got, want))


@pytest.mark.parametrize("B,T,C,G,masked,add", [(2, 37, 32, 8, True, True), (3, 600, 256, 8, True, True),
                                                 (2, 300, 256, 8, False, False), (1, 5, 64, 8, True, False)])
def test_group_norm_mish_tm(B, T, C, G, masked, add):
    from matcha.models.components._ops import group_norm_mish_tm

    h = (torch.randn(B, T, C, device=DEV) * 3 + 1).requires_grad_(True)
    gam = (1 + 0.1 * torch.randn(C, device=DEV)).requires_grad_(True)
    bet = (0.1 * torch.randn(C, device=DEV)).requires_grad_(True)
    m = _mask(B, T, [T - 2 * i for i in range(B)]) if masked else None
    a = torch.randn(B, C, device=DEV, requires_grad=True)

    def ref(h, gam, bet, a):
        y = F.mish(F.group_norm(h.transpose(1, 2), G, gam, bet, 1e-5)).transpose(1, 2)
        if m is not None:
            y = y * m[..., None]
        return y + a[:, None, :] if add else y

    _run(lambda h, gam, bet, a: group_norm_mish_tm(h, gam, bet, G, m, a if add else None), ref, [h, gam, bet, a],
         "fp32")


@pytest.mark.parametrize("M,C", [(19200, 256), (77, 32), (5, 1024)])
def test_layer_norm_tm(M, C):
    from matcha.models.components._ops import layer_norm_tm

    x = (torch.randn(M, C, device=DEV) * 2 + 0.5).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(C, device=DEV)).requires_grad_(True)
    b = (0.1 * torch.randn(C, device=DEV)).requires_grad_(True)
    _run(lambda x, w, b: layer_norm_tm(x, w, b), lambda x, w, b: F.layer_norm(x, (C,), w, b, 1e-5), [x, w, b],
         "fp32")


def test_ops_refuse_cpu_and_never_fall_back():
    from matcha import _native as N
    from matcha.models.components._ops import conv_tm

    with pytest.raises(N.NativeError):
        conv_tm(torch.randn(1, 4, 8), torch.randn(8, 8, 3), None)


# Strict bf16 checks at the train step's full size (many workgroups per CU).  Operands are rounded to
# bf16 up front, so the bf16 MFMA products are exact and only fp32 accumulation order separates the
# kernels from a float64 reference: every entry must agree to 1e-5 of the output's scale, and repeated
# calls must be bitwise identical.  The loose 1.5e-2 relative tolerance above let through a
# packed-fp32 miscompute in the wgrad staging (wrong low halves in lanes 16-31/48-63 under CU
# co-residency, relative error 3e-3..1e-2); these catch that class of error.
BIG = [(32, 600, 256, 768, 1), (32, 600, 512, 256, 3), (32, 120, 192, 768, 3)]
# T < rows_per_step: the generic row walk (wgrad INC=false), the instantiation whose packed-fp32 build
# faulted
GENERIC = [(1200, 16, 256, 768, 1), (800, 24, 512, 256, 3)]


@pytest.mark.parametrize("B,T,Cin,Cout,k", BIG + GENERIC)
@pytest.mark.parametrize("rows_per_step,target_blocks,depth", [(-1, -1, -1), (32, -1, 1), (32, 1024, 1),
                                                               (64, 1024, 1), (32, 512, 2)])
def test_wgrad_bf16_exact_and_deterministic(B, T, Cin, Cout, k, rows_per_step, target_blocks, depth):
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(B * T + Cin + Cout + k)
    x = torch.randn(B, T, Cin, generator=g).bfloat16().float().to(DEV)
    dy = torch.randn(B, T, Cout, generator=g).bfloat16().float().to(DEV)
    pad = k // 2
    ref = torch.nn.grad.conv1d_weight(x.double().transpose(1, 2), (Cout, Cin, k), dy.double().transpose(1, 2),
                                      padding=pad)
    refb = dy.double().sum((0, 1))
    outs = []
    for _ in range(3):
        dw = torch.full((Cout, Cin, k), float("nan"), device=DEV)
        db = torch.full((Cout,), float("nan"), device=DEV)
        O._wgrad(dy, T, 1, 0, x, T, T, B, 1, [j - pad for j in range(k)], Cin, Cout, dw, (Cin * k, k, 1),
                 prec=O.PREC_BF16, db=db, rows_per_step=rows_per_step, target_blocks=target_blocks, depth=depth)
        outs.append((dw, db))
    torch.cuda.synchronize()
    dw, db = outs[0]
    assert (dw.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (db.double() - refb).abs().max().item() <= 1e-5 * refb.abs().max().item()
    for dw2, db2 in outs[1:]:
        assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("B,T,Cin,Cout,k,stride", [(8, 300, 256, 256, 3, 1), (8, 301, 256, 256, 3, 2), (6, 77, 192, 768, 5, 1),
                                                  (4, 64, 512, 160, 1, 1), (32, 40, 96, 200, 3, 1)])
def test_wgrad_masked_strided(B, T, Cin, Cout, k, stride):
    """The default bf16 wgrad schedule with a 0/1 row mask, ragged lengths, stride 2, 1..5 taps and N / K not
    multiples of the 128 tile: against float64 on bf16-exact operands (1e-5 of the output scale), bitwise
    repeatable, and equal in value to the explicit 32-row one-step schedule."""
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(B * T + Cin + k + stride)
    x = torch.randn(B, T, Cin, generator=g).bfloat16().float().to(DEV)
    lengths = torch.randint(T // 3, T + 1, (B,), generator=g)
    lengths[0] = T
    m = (torch.arange(T)[None] < lengths[:, None]).float().to(DEV)
    pad = k // 2
    To = (T + 2 * pad - k) // stride + 1
    dy = torch.randn(B, To, Cout, generator=g).bfloat16().float().to(DEV)
    xm = (x * m.unsqueeze(-1)).double()
    ref = torch.nn.grad.conv1d_weight(xm.transpose(1, 2), (Cout, Cin, k), dy.double().transpose(1, 2), stride=stride,
                                      padding=pad)
    refb = dy.double().sum((0, 1))
    outs = []
    for sched in [(-1, -1, -1)] * 2 + [(32, -1, 1)]:
        dw = torch.full((Cout, Cin, k), float("nan"), device=DEV)
        db = torch.full((Cout,), float("nan"), device=DEV)
        O._wgrad(dy, To, 1, 0, x, T, To, B, stride, [j - pad for j in range(k)], Cin, Cout, dw, (Cin * k, k, 1),
                 prec=O.PREC_BF16, a_scale=m, db=db, rows_per_step=sched[0], target_blocks=sched[1], depth=sched[2])
        outs.append((dw, db))
    torch.cuda.synchronize()
    dw, db = outs[0]
    assert (dw.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (db.double() - refb).abs().max().item() <= 1e-5 * refb.abs().max().item()
    assert torch.equal(dw, outs[1][0]) and torch.equal(db, outs[1][1])
    torch.testing.assert_close(dw, outs[2][0], rtol=1e-5, atol=1e-5 * ref.abs().max().item())


@pytest.mark.parametrize("B,T,Cin,Cout,k", BIG)
@pytest.mark.parametrize("cfg", [-1, 7, 12, 41, 42, 44])
def test_gemm_bf16_exact_and_deterministic(B, T, Cin, Cout, k, cfg):
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(B * T + Cin + Cout + k + 1)
    x = torch.randn(B, T, Cin, generator=g).bfloat16().float().to(DEV)
    w = (torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)).bfloat16().float().to(DEV)
    pad = k // 2
    ref = F.conv1d(x.double().transpose(1, 2), w.double(), padding=pad).transpose(1, 2)
    Wp, Kp = O.pack_weight(w.permute(0, 2, 1).reshape(Cout, k * Cin), O.PREC_BF16)
    outs = []
    for _ in range(3):
        y = torch.full((B, T, Cout), float("nan"), device=DEV)
        O._gemm(x, T, T, B, 1, [j - pad for j in range(k)], Cin, Wp, Kp, Cout, y, T, prec=O.PREC_BF16, tile_cfg=cfg)
        outs.append(y)
    torch.cuda.synchronize()
    assert (outs[0].double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    for y2 in outs[1:]:
        assert torch.equal(outs[0], y2)


@pytest.mark.parametrize("cfg,splits", [(41, 1), (42, 3), (44, 1), (44, 4), (-1, 0)])
@pytest.mark.parametrize("act,pre", [(0, False), (1, True)])
def test_gemm_lds_dma_split_k_epilogue(cfg, splits, act, pre):
    """LDS-DMA schedules (incl. split-K + combine pass) against the register-staged config 7 on the
    whole epilogue: ragged 0/1 row mask (masked rows DMA'd from the zero chunk), bias, GELU with the
    pre-activation store, dropout, residual, output row scale and a stride-2 output phase."""
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(7 + splits + act)
    B, T, Cin, Cout = 5, 77, 256, 320
    x = torch.randn(B, T, Cin, generator=g).to(DEV)
    msk = (torch.rand(B * T, generator=g) > 0.2).float().to(DEV)
    w = (torch.randn(Cout, Cin * 3, generator=g) / math.sqrt(Cin * 3)).to(DEV)
    Wp, Kp = O.pack_weight(w, O.PREC_BF16)
    bias = torch.randn(Cout, generator=g).to(DEV)
    res = torch.randn(B, 2 * T, Cout, generator=g).to(DEV)
    cs = torch.rand(B * 2 * T, generator=g).to(DEV)
    seed = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)
    outs = []
    for c, sp in [(7, 1), (cfg, splits)]:
        y = torch.zeros(B, 2 * T, Cout, device=DEV)
        yp = torch.zeros(B, 2 * T, Cout, device=DEV) if pre else None
        O._gemm(x, T, T, B, 1, [-1, 0, 1], Cin, Wp, Kp, Cout, y, 2 * T, 2, 1, prec=O.PREC_BF16, a_scale=msk,
                bias=bias, act=act, residual=res, c_scale=cs, C_pre=yp, dropout_p=0.1, seed=seed, tile_cfg=c,
                splits=sp)
        outs.append((y, yp))
    torch.cuda.synchronize()
    (y0, p0), (y1, p1) = outs
    assert (y1[:, 0::2] == 0).all()  # the other output phase is untouched
    assert rel(y1, y0) < 1e-5, rel(y1, y0)
    if pre:
        assert rel(p1, p0) < 1e-5, rel(p1, p0)


@pytest.mark.parametrize("B,T,Cin,Cout,k,cfg", [(32, 600, 1024, 256, 1, -1), (32, 300, 256, 256, 3, -1),
                                                 (5, 77, 256, 320, 3, 44), (4, 120, 192, 768, 3, 42),
                                                 (2, 33, 96, 64, 3, 41), (2, 33, 96, 64, 3, 42), (2, 33, 96, 64, 3, 44)])
def test_bf16_operand_storage_bitwise(B, T, Cin, Cout, k, cfg):
    """bf16-stored A (MTTS_GEMM_F_A_BF16) and bf16 C (MTTS_GEMM_F_C_BF16): the GEMM and the wgrad on a
    bf16 A are bitwise equal to the fp32-A path on the same (bf16-representable) values, and a bf16 C
    is the fp32 C rounded once.  (The 96-channel cases: K steps that cross taps, the register-addressed loop of
    the 64-row LDS-DMA schedules for both A storages.)"""
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(B + T + Cin + Cout)
    x = torch.randn(B, T, Cin, generator=g).bfloat16().to(DEV)
    m = (torch.rand(B * T, generator=g) > 0.2).float().to(DEV)
    w = (torch.randn(Cout, Cin * k, generator=g) / math.sqrt(Cin * k)).to(DEV)
    Wp, Kp = O.pack_weight(w, O.PREC_BF16)
    offs = [j - k // 2 for j in range(k)]
    c_cfg = cfg if cfg >= 0 else 41
    y32 = torch.empty(B, T, Cout, device=DEV)
    O._gemm(x.float(), T, T, B, 1, offs, Cin, Wp, Kp, Cout, y32, T, prec=O.PREC_BF16, a_scale=m, tile_cfg=c_cfg)
    y16a = torch.empty(B, T, Cout, device=DEV)
    O._gemm(x, T, T, B, 1, offs, Cin, Wp, Kp, Cout, y16a, T, prec=O.PREC_BF16, a_scale=m, tile_cfg=cfg)
    yc = torch.empty(B, T, Cout, device=DEV, dtype=torch.bfloat16)
    O._gemm(x.float(), T, T, B, 1, offs, Cin, Wp, Kp, Cout, yc, T, prec=O.PREC_BF16, a_scale=m, tile_cfg=c_cfg)
    torch.cuda.synchronize()
    if cfg >= 0:
        assert torch.equal(y16a, y32)
    else:
        assert rel(y16a, y32) < 1e-6  # the heuristic may pick another schedule for the bf16 A
    assert torch.equal(yc, y32.bfloat16())
    dy = torch.randn(B, T, Cout, generator=g).to(DEV)
    outs = []
    for xa in (x.float(), x):
        dw = torch.empty(Cout, Cin, k, device=DEV)
        db = torch.empty(Cout, device=DEV)
        O._wgrad(dy, T, 1, 0, xa, T, T, B, 1, offs, Cin, Cout, dw, (Cin * k, k, 1), prec=O.PREC_BF16, a_scale=m, db=db)
        outs.append((dw, db))
    torch.cuda.synchronize()
    # fp32 A runs the LDS-DMA wgrad, bf16 A the register-staged one: the same bf16 products, summed over
    # other row splits (128-row rounds) and the bias column sums in another fixed order -- equal to fp32
    # reordering (~1e-6 of the scale for sums of up to 19200 terms)
    for a, b in zip(outs[0], outs[1]):
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()


def test_reduce_partials_jobs():
    """csrc/reduce.hip against torch sums: plain and weight-layout jobs, float4 and scalar paths (n % 4),
    long narrow jobs (16 slices), accumulate, several jobs in one batched launch."""
    from matcha import _native as N
    from matcha._abi import ReduceJob as Job

    g = torch.Generator(device=DEV).manual_seed(5)
    cases = []  # (part [S, stride], out tensor, expected, job)
    # plain, vector path, accumulate
    p0 = torch.randn(7, 1024, device=DEV, generator=g)
    o0 = torch.randn(1024, device=DEV, generator=g)
    cases.append((p0, o0, o0 + p0.sum(0), dict(stride=1024, n=1024, splits=7, accumulate=1)))
    # plain, scalar path (n % 4 != 0, stride > n), long narrow (16 slices)
    p1 = torch.randn(300, 258, device=DEV, generator=g)
    o1 = torch.zeros(255, device=DEV)
    cases.append((p1, o1, p1[:, :255].sum(0), dict(stride=258, n=255, splits=300, accumulate=0)))
    # weight layout: slab [N][K], K = taps*cin -> out[n, c, j] of a [N][cin][taps] conv weight
    Nn, cin, taps, S = 24, 16, 3, 5
    p2 = torch.randn(S, Nn * cin * taps, device=DEV, generator=g)
    o2 = torch.zeros(Nn, cin, taps, device=DEV)
    e2 = p2.sum(0).view(Nn, taps, cin).permute(0, 2, 1)
    cases.append((p2, o2, e2, dict(stride=Nn * cin * taps, n=Nn * cin * taps, splits=S, accumulate=0,
                                   cols=cin * taps, cin=cin, sr=cin * taps, sc=taps, sj=1)))
    jobs = (Job * len(cases))()
    for i, (p, o, _, kw) in enumerate(cases):
        jobs[i] = Job(part=p.data_ptr(), out=o.data_ptr(), **kw)
    N.check(N.lib().mtts_reduce_partials(jobs, len(cases), torch.cuda.current_stream().cuda_stream),
            "mtts_reduce_partials")
    torch.cuda.synchronize()
    for p, o, e, _ in cases:
        torch.testing.assert_close(o, e, rtol=1e-5, atol=1e-4)


def _preln_inputs(B, T, C, heads, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV).requires_grad_(True)
    h = r(B, T, C)
    ln_w, ln_b = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True), r(C, sc=0.1)
    wq, wk, wv = (r(C, C, sc=C ** -0.5) for _ in range(3))
    wo, bo = r(C, C, sc=C ** -0.5), r(C, sc=0.1)
    w1, b1 = r(4 * C, C, sc=C ** -0.5), r(4 * C, sc=0.1)
    w2, b2 = r(C, 4 * C, sc=(4 * C) ** -0.5), r(C, sc=0.1)
    key_bias = torch.zeros(B, T, device=DEV)
    for b in range(B):
        key_bias[b, : T - 7 * b] = 1  # the reference's float 0/1 mask, added to the scores
    return h, ln_w, ln_b, wq, wk, wv, wo, bo, w1, b1, w2, b2, key_bias


def _preln_ref(h, ln_w, ln_b, wq, wk, wv, wo, bo, w1, b1, w2, b2, key_bias, heads):
    """BasicTransformerBlock (transformer.py:297-370) in plain torch fp32."""
    B, T, C = h.shape
    n = F.layer_norm(h, (C,), ln_w, ln_b, 1e-5)
    sp = lambda t: t.view(B, T, heads, C // heads).transpose(1, 2)
    o = F.scaled_dot_product_attention(sp(n @ wq.T), sp(n @ wk.T), sp(n @ wv.T), attn_mask=key_bias[:, None, None, :])
    h = h + F.linear(o.transpose(1, 2).reshape(B, T, C), wo, bo)
    n = F.layer_norm(h, (C,), ln_w, ln_b, 1e-5)
    return h + F.linear(F.gelu(F.linear(n, w1, b1)), w2, b2)


def _preln_fused(h, ln_w, ln_b, wq, wk, wv, wo, bo, w1, b1, w2, b2, key_bias, heads):
    from matcha.models.components import _ops as O

    h = O.preln_attention_tm(h, ln_w, ln_b, 1e-5, key_bias, heads, wq, wk, wv, wo, bo)
    return O.preln_ff_tm(h, ln_w, ln_b, 1e-5, w1, b1, w2, b2)


def _preln_unfused(h, ln_w, ln_b, wq, wk, wv, wo, bo, w1, b1, w2, b2, key_bias, heads):
    from matcha.models.components import _ops as O

    n = O.layer_norm_tm(h, ln_w, ln_b, 1e-5)
    qkv = O.linear_tm(n, (wq, wk, wv), None)
    h = O.linear_tm(O.attention_tm(qkv, key_bias, heads), wo, bo, residual=h)
    n = O.layer_norm_tm(h, ln_w, ln_b, 1e-5)
    return O.ff_tm(n, w1, b1, w2, b2, residual=h)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C,heads", [(2, 150, 256, 4), (3, 37, 64, 2)])
def test_preln_blocks_vs_torch(prec, B, T, C, heads):
    """The fused pre-LN sub-blocks (LN output bf16 in bf16-mixed, residual gradient added in the LN
    backward) against plain torch fp32."""
    *ins, kb = _preln_inputs(B, T, C, heads)
    _run(lambda *a: _preln_fused(*a, kb, heads), lambda *a: _preln_ref(*a, kb, heads), ins, prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_preln_blocks_match_unfused_ops(prec):
    """Fusing changes where values live, not the arithmetic: bitwise equal to the op-by-op composition in
    fp32 mode.  In bf16-mixed mode the fused block also STORES q|k|v, o, dO and dq|dk|dv as bf16 (the
    op-by-op path keeps them fp32 and rounds them to bf16 MFMA operands inside the kernels): the q
    prescale then rounds twice and o is rounded once more before the output projection, so forward and
    gradients agree to bf16 rounding (~1e-3)."""
    B, T, C, heads = 2, 150, 256, 4
    *ins, kb = _preln_inputs(B, T, C, heads)
    outs = []
    for fn in (_preln_fused, _preln_unfused):
        xs = [t.detach().clone().requires_grad_(True) for t in ins]
        with _ctx(prec):
            y = fn(*xs, kb, heads)
        torch.manual_seed(1)
        y.backward(torch.randn_like(y))
        outs.append((y.detach(), [x.grad for x in xs]))
    (y0, g0), (y1, g1) = outs
    if prec == "fp32":
        assert torch.equal(y0, y1)
    else:
        assert rel(y0, y1) < 5e-3, rel(y0, y1)
    for i, (a, b) in enumerate(zip(g0, g1)):
        if prec == "fp32":
            assert torch.equal(a, b), i
        else:
            assert rel(a, b) < 1e-2, (i, rel(a, b))


@pytest.mark.parametrize("B,T,C,G,dy16", [(4, 600, 256, 8, False), (3, 300, 256, 8, True), (2, 2000, 256, 8, True)])
def test_group_norm_mish_bf16_storage(B, T, C, G, dy16):
    """bf16-stored GroupNorm input / output / gradient (MTTS_NORM_F_X/Y/DY_BF16): the same fp32 arithmetic
    on the exactly widened values, outputs rounded once -- equal to the fp32-storage kernel's result
    rounded to bf16 (the register-resident and the streaming kernels)."""
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(B * T + G)
    h = (torch.randn(B, T, C, generator=g) * 2 + 0.5).bfloat16().to(DEV)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    m = _mask(B, T, [T - 9 * i for i in range(B)])
    add = torch.randn(B, C, generator=g).to(DEV)
    # dy16: a bf16 output, whose incoming gradient autograd hands over as bf16 (the Block1D feeding a
    # conv); else an fp32 output from a bf16 input with an fp32 gradient (the block feeding the residual)
    dy = torch.randn(B, T, C, generator=g).to(DEV)
    if dy16:
        dy = dy.bfloat16().float()
    outs = []
    for x, o16 in ((h.float(), False), (h, dy16)):
        xx = x.clone().requires_grad_(True)
        with _ctx("bf16"):
            y = O.group_norm_mish_tm(xx, gamma, beta, G, m, add, out_bf16=o16)
        y.backward(dy.to(y.dtype))
        outs.append((y.detach(), xx.grad))
    (y32, g32), (y16, g16) = outs
    assert y16.dtype == (torch.bfloat16 if dy16 else torch.float32) and g16.dtype == torch.bfloat16
    torch.testing.assert_close(y16.float(), y32.to(y16.dtype).float(), rtol=0, atol=0)
    torch.testing.assert_close(g16.float(), g32.bfloat16().float(), rtol=0, atol=0)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_bf16_storage_chain(stride):
    """conv (bf16 out) -> GroupNorm+Mish (bf16 out) -> conv: the bf16-mixed storage path against the same
    ops with fp32 storage (bf16 rounding of the stored activations and gradients only)."""
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(11 + stride)
    B, T, C = 4, 300, 256
    x = torch.randn(B, T, C, generator=g).to(DEV)
    w1 = (torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C)).to(DEV)
    w2 = (torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C)).to(DEV)
    b1, b2 = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    gam, bet = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    m = _mask(B, T, [T - 13 * i for i in range(B)])
    res = []
    for bf in (False, True):
        ins = [t.clone().requires_grad_(True) for t in (x, w1, w2, b1, b2, gam, bet)]
        xx, ww1, ww2, bb1, bb2, gg, be = ins
        with _ctx("bf16"):
            h = O.conv_tm(xx, ww1, bb1, m, out_bf16=bf)
            a = O.group_norm_mish_tm(h, gg, be, 8, m, out_bf16=bf)
            y = O.conv_tm(a, ww2, bb2, m, stride=stride)
        assert (h.dtype == torch.bfloat16) == bf and (a.dtype == torch.bfloat16) == bf and y.dtype == torch.float32
        torch.manual_seed(3)
        y.backward(torch.randn_like(y))
        res.append((y.detach(), [t.grad for t in ins]))
    (y0, g0), (y1, g1) = res
    assert rel(y1, y0) < 1e-2, rel(y1, y0)
    for i, (a, b) in enumerate(zip(g1, g0)):
        assert rel(a, b) < 2e-2, (i, rel(a, b))


@pytest.mark.parametrize("a16,y16", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("B,T,Cin,Cout,k", [(8, 300, 256, 256, 3), (5, 77, 192, 768, 5), (32, 40, 256, 128, 1)])
def test_wgrad_linear_walk_storage(a16, y16, B, T, Cin, Cout, k):
    """The register wgrad's linear row walk (stride 1, equal lengths: every product conv / linear) with
    each operand storage, a ragged 0/1 row mask and the bias sums: against float64 (1e-5 of the scale)
    and bitwise repeatable; with and without the bias gradient (the raw-bf16 dY staging)."""
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(B * T + Cin + k + 2 * a16 + y16)
    x = torch.randn(B, T, Cin, generator=g).bfloat16().float().to(DEV)
    lengths = torch.randint(T // 3, T + 1, (B,), generator=g)
    lengths[0] = T
    m = (torch.arange(T)[None] < lengths[:, None]).float().to(DEV)
    pad = k // 2
    dy = torch.randn(B, T, Cout, generator=g).bfloat16().float().to(DEV)
    ref = torch.nn.grad.conv1d_weight((x * m.unsqueeze(-1)).double().transpose(1, 2), (Cout, Cin, k),
                                      dy.double().transpose(1, 2), padding=pad)
    refb = dy.double().sum((0, 1))
    xa = x.bfloat16() if a16 else x
    dya = dy.bfloat16() if y16 else dy
    outs = []
    for with_db in (True, True, False):
        dw = torch.full((Cout, Cin, k), float("nan"), device=DEV)
        db = torch.full((Cout,), float("nan"), device=DEV) if with_db else None
        O._wgrad(dya, T, 1, 0, xa, T, T, B, 1, [j - pad for j in range(k)], Cin, Cout, dw, (Cin * k, k, 1),
                 prec=O.PREC_BF16, a_scale=m, db=db)
        outs.append((dw, db))
    torch.cuda.synchronize()
    dw, db = outs[0]
    assert (dw.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (db.double() - refb).abs().max().item() <= 1e-5 * refb.abs().max().item()
    assert torch.equal(dw, outs[1][0]) and torch.equal(db, outs[1][1])
    assert torch.equal(dw, outs[2][0])  # the bias-free path stages the same values



@pytest.mark.parametrize("stride", [1, 2])
def test_grad_link_two_consumers(stride):
    """GradLink: a later consumer of x hands its input gradient to an earlier conv's dgrad epilogue
    (Resnet1D's res_conv -> block1 conv; the up path's concat slice -> the down conv).  The sum equals
    autograd's: fp32 mode, against the same ops without the link; the concat case reads a row-strided
    slice in place."""
    from matcha.models.components import _ops as O

    B, T, C = 3, 37, 64
    m = _mask(B, T, [37, 20, 29])
    x0 = torch.randn(B, T, C, device=DEV)
    w1, b1 = torch.randn(C, C, 3, device=DEV) * 0.1, torch.randn(C, device=DEV)
    w2, b2 = torch.randn(C, C, 1, device=DEV) * 0.1, torch.randn(C, device=DEV)
    other = torch.randn(B, T, C, device=DEV)

    def run(linked, concat):
        x = x0.clone().requires_grad_(True)
        link = O.GradLink() if linked else None
        y1 = O.conv_tm(x, w1, b1, m, stride=stride, padding=1, dx_link=link, dx_link_role="take" if linked else None)
        if concat:  # x also enters [other | x]; the first channels' gradient is dropped
            y2 = O.cat_skip_tm(other, x, link)[..., C:] * m.unsqueeze(-1)
        else:
            y2 = O.conv_tm(x, w2, b2, m, padding=0, dx_link=link, dx_link_role="give" if linked else None)
        return x, y1, y2

    for concat in (False, True):
        if stride == 2 and not concat:
            continue  # Resnet1D's convs are stride 1; a stride-2 taker only meets the concat
        torch.manual_seed(5)
        g1 = torch.randn(B, (T + 2 - 3) // stride + 1, C, device=DEV)
        g2 = torch.randn(B, T, C, device=DEV)
        grads = []
        for linked in (False, True):
            x, y1, y2 = run(linked, concat)
            ((y1 * g1).sum() + (y2 * g2).sum()).backward()
            grads.append(x.grad.clone())
        assert rel(grads[1], grads[0]) < 1e-6, (concat, rel(grads[1], grads[0]))


def test_decoder_grad_links_match_autograd_sums():
    """The decoder with its GradLinks (Resnet1D inputs, skip / concat) vs the same decoder with autograd
    summing the input gradients (the module attribute decoder._DX_LINK = False): same loss, same parameter
    gradients (fp32 mode; the fused sums differ from autograd's only in the sign of masked zeros)."""
    from matcha.models.components import decoder as D

    torch.manual_seed(11)
    dec = D.Decoder(in_channels=160, out_channels=80, channels=(256, 256), dropout=0.0, attention_head_dim=64,
                    n_blocks=1, num_mid_blocks=2, num_heads=2).to(DEV).eval()
    B, T = 4, 61
    m = _mask(B, T, [61, 40, 17, 55])
    x, mu = torch.randn(B, T, 80, device=DEV), torch.randn(B, T, 80, device=DEV)
    t = torch.rand(B, device=DEV)
    res = []
    saved = D._DX_LINK
    try:
        for on in (False, True):
            D._DX_LINK = on
            dec.zero_grad(set_to_none=True)
            xr = x.clone().requires_grad_(True)
            out = dec.forward_tm(xr, m, mu, t)
            (out * torch.linspace(-1, 1, 80, device=DEV)).sum().backward()
            res.append((out.detach(), xr.grad.clone(), [p.grad.clone() for p in dec.parameters() if p.grad is not None]))
    finally:
        D._DX_LINK = saved
    (o0, gx0, gp0), (o1, gx1, gp1) = res
    assert torch.equal(o0, o1)
    assert rel(gx1, gx0) < 1e-6
    assert len(gp0) == len(gp1)
    worst = max(rel(a, b) for a, b in zip(gp1, gp0))
    assert worst < 1e-5, worst


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_transpose_tm_row_strided_grad(prec):
    """The transposed conv's backward reads a channel slice of a concat gradient in place (row-strided
    dgrad / wgrad operand, decoder up path) -- same gradients as the torch reference."""
    from matcha.models.components._ops import conv_transpose_tm

    B, T, C = 3, 45, 64
    x = torch.randn(B, T, C, device=DEV, requires_grad=True)
    w = (torch.randn(C, C, 4, device=DEV) / math.sqrt(C * 2)).requires_grad_(True)
    b = torch.randn(C, device=DEV, requires_grad=True)
    m = _mask(B, T, [T, T - 7, T - 20])
    other = torch.randn(B, 2 * T, 32, device=DEV)
    ref = lambda x, w, b: torch.cat(  # noqa: E731
        [F.conv_transpose1d((x * m[..., None]).transpose(1, 2), w, b, 2, 1).transpose(1, 2), other], -1)
    _run(lambda x, w, b: torch.cat([conv_transpose_tm(x, w, b, m), other], -1), ref, [x, w, b], prec)


@pytest.mark.parametrize("p", [0.1, 0.05, 0.3])
def test_dropout_keep_rate_unbiased_and_pairs_independent(p):
    """the counter-based mask (mtts_common.h dropout_keep: one hash per column pair, 16-bit uniforms) keeps
    an element with probability (65536 - ceil(p * 65536)) / 65536 and dropout_scale rescales by exactly its inverse,
    so the mean of dropout(ones) is 1 up to sampling noise (no 2^-16 grid bias); the even / odd columns of a pair
    (the two halves of one hash) and adjacent rows are uncorrelated."""
    from matcha import _native as N
    from matcha.models.components import _ops as O

    rows, cols = 4096, 4096
    x = torch.ones(rows, cols, device=DEV)
    y = torch.empty_like(x)
    seed = torch.tensor([987654321, 12345], dtype=torch.int32, device=DEV)
    N.check(N.lib().mtts_dropout_apply(x.data_ptr(), y.data_ptr(), rows, cols, cols, float(p), seed.data_ptr(),
                                       O._stream(y)), "mtts_dropout_apply")
    torch.cuda.synchronize()
    keep = (y != 0).double()
    n = keep.numel()
    want_keep = (65536 - math.ceil(p * 65536)) / 65536
    sd = math.sqrt(want_keep * (1 - want_keep) / n)
    assert abs(keep.mean().item() - want_keep) < 5 * sd
    scale = y[y != 0].unique()
    assert scale.numel() == 1 and scale.item() == pytest.approx(1.0 / want_keep, rel=1e-7)
    assert abs(y.double().mean().item() - 1.0) < 5 * sd / want_keep  # unbiased
    k = keep - keep.mean()

    def corr(a, b):
        return ((a * b).mean() / (a.std() * b.std())).item()

    lim = 5.0 / math.sqrt(n / 2)
    assert abs(corr(k[:, 0::2], k[:, 1::2])) < lim  # the two halves of one hash
    assert abs(corr(k[:, 1:-1:2], k[:, 2::2])) < lim  # across adjacent pairs
    assert abs(corr(k[:-1], k[1:])) < lim  # adjacent rows
