"""Every dropout path of the HIP kernels against a float64 torch reference that applies the EXACT mask.

The mask is a pure function of (seed words, row key, column key, p) -- csrc/mtts_common.h dropout_keep, restated
on the host in tests/dropout_ref.py -- so each site is checked element by element: which (row, col) key it
hashes, the scale it applies, and where in the epilogue order (bias -> pre-activation store -> act -> dropout ->
residual -> c_scale) the drop happens.  Wherever the mask is visible in an output its zero pattern is compared
exactly; values are compared with float64 torch at the tolerances the same ops meet without dropout
(test_decoder_ops_gpu.TOL, test_attention_fwd_bwd's bounds): dropout multiplies by a constant and zeroes
entries, which leaves relative error as it was.

Seeds: the low-level entry points take a seed tensor; the autograd-level ops draw theirs from _ops._new_seed,
which the tests wrap to record every tensor it hands out, in order."""
from __future__ import annotations

import math

import dropout_ref as DR
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from test_decoder_ops_gpu import TOL, rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ helpers
def _keep(seed, rows, cols, p) -> torch.Tensor:
    """bool [len(rows), len(cols)] on the device, from the host restatement of the hash."""
    return torch.from_numpy(DR.keep_mask(seed, np.asarray(rows), np.asarray(cols), p)).to(DEV)


def _keep_rc(seed, nrows, ncols, p) -> torch.Tensor:
    return _keep(seed, np.arange(nrows), np.arange(ncols), p)


def _scale(p) -> float:
    return float(np.float32(DR.keep_scale(p)))  # the kernels' fp32 factor


def _drop64(seed, nrows, ncols, p) -> torch.Tensor:
    """keep * scale as a float64 constant [nrows, ncols]."""
    return _keep_rc(seed, nrows, ncols, p).double() * _scale(p)


def _seed(lo, hi) -> torch.Tensor:
    return torch.tensor([lo, hi], dtype=torch.int32, device=DEV)


def _ctx(prec):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=(prec == "bf16"))


def _ragged(B, T, step=5):
    m = torch.zeros(B, T, device=DEV)
    for b in range(B):
        m[b, : max(1, T - step * b)] = 1
    return m


def _conv64(x, w, b, pad):
    """Conv1d, token-major, float64: x [B, T, Cin], w [Cout, Cin, k] -> [B, T + 2 pad - k + 1, Cout]."""
    k = w.shape[-1]
    To = x.shape[1] + 2 * pad - k + 1
    xp = F.pad(x, (0, 0, pad, pad))
    y = sum(xp[:, j:j + To] @ w[:, :, j].transpose(0, 1) for j in range(k))
    return y if b is None else y + b


def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def _dgelu64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _record_seeds(monkeypatch):
    """Wraps _ops._new_seed: the returned list receives every seed tensor an op draws, in order."""
    from matcha.models.components import _ops as O

    seeds, orig = [], O._new_seed

    def wrapper(device):
        s = orig(device)
        seeds.append(s)
        return s

    monkeypatch.setattr(O, "_new_seed", wrapper)
    return seeds


def _run_op(monkeypatch, fn, ref, inputs, prec, nseeds, gseed=0):
    """fn(*leaves) under `prec` with the seeds recorded; ref(seeds, *float64 leaves); compares the output and
    every input gradient in relative L2 at TOL[prec].  Returns (y, y_ref, seeds)."""
    seeds = _record_seeds(monkeypatch)
    xs = [t.detach().clone().requires_grad_(True) for t in inputs]
    with _ctx(prec):
        y = fn(*xs)
    assert len(seeds) == nseeds, len(seeds)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed)).to(DEV)
    (y * g).sum().backward()
    rs = [t.detach().double().requires_grad_(True) for t in inputs]
    yr = ref(seeds, *rs)
    (yr * g.double()).sum().backward()
    ftol, gtol = TOL[prec]
    errs = [rel(y, yr)] + [rel(a.grad, b.grad) for a, b in zip(xs, rs)]
    print("rel errors (output, then each input gradient):", ["%.3g" % e for e in errs])
    assert errs[0] < ftol, errs[0]
    for i, (a, b) in enumerate(zip(xs, rs)):
        assert a.grad is not None and errs[1 + i] < gtol, (i, tuple(b.shape), errs[1 + i])
    return y.detach(), yr.detach(), seeds


# ------------------------------------------------------------------------------------------ a. the port, bitwise
SEEDS = [(0, 0), (2 ** 31 - 2, 2 ** 31 - 2), (-1234567, -2 ** 31)]  # the last: high bits set (negative int32)


@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 1), (3, 7, 7), (257, 130, 136), (70000, 2, 2)])
def test_dropout_apply_matches_host_mask_bitwise(rows, cols, ld):
    """mtts_dropout_apply on ones: the zero pattern IS dropout_ref.keep_mask and every survivor is
    float32(keep_scale(p)).  (3, 7): a half column pair at the row end; ld 136: padded rows, the padding
    untouched; 70000 rows: row keys past 65535, where row * 0x9E3779B1 wraps."""
    from matcha import _native as N
    from matcha.models.components import _ops as O

    x = torch.ones(rows, ld, device=DEV)
    for p in (0.05, 0.1, 0.19, 0.3):
        for lo, hi in SEEDS:
            seed = _seed(lo, hi)
            y = torch.full((rows, ld), -7.0, device=DEV)
            N.check(N.lib().mtts_dropout_apply(x.data_ptr(), y.data_ptr(), rows, cols, ld, float(p), seed.data_ptr(),
                                               O._stream(y)), "mtts_dropout_apply")
            torch.cuda.synchronize()
            keep = _keep_rc(seed, rows, cols, p)
            assert torch.equal(y[:, :cols] != 0, keep), (p, lo, hi)
            want = torch.where(keep, torch.tensor(np.float32(DR.keep_scale(p)), device=DEV), torch.zeros((), device=DEV))
            assert torch.equal(y[:, :cols], want), (p, lo, hi)
            assert (y[:, cols:] == -7.0).all()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_act_dropout_bwd_bitwise(p):
    """mtts_act_dropout_bwd (ACT_NONE; ACT_RELU gated by a y with zeros and negatives) and
    mtts_act_dropout_bwd_scaled (0/1 row scale) on random dy: bitwise float32(dy) [* row_scale] * gate * keep *
    float32(scale), computed in numpy float32 in the kernel's operation order."""
    from matcha import _native as N
    from matcha.models.components import _ops as O

    rows, cols = 131, 70
    g = torch.Generator().manual_seed(11)
    dy = torch.randn(rows, cols, generator=g)
    yv = torch.randn(rows, cols, generator=g)
    yv[torch.rand(rows, cols, generator=g) < 0.3] = 0.0  # zeros (dropped or cut) beside the negatives
    rs = (torch.rand(rows, generator=g) > 0.3).float()
    seed = _seed(-77, 2 ** 31 - 2)
    keep = DR.keep_mask(seed, np.arange(rows), np.arange(cols), p)
    sc = np.float32(DR.keep_scale(p))
    zero = np.float32(0.0)
    dyn, yn, rsn = dy.numpy(), yv.numpy(), rs.numpy()
    dyd, yd, rsd = dy.to(DEV), yv.to(DEV), rs.to(DEV)
    lib, st = N.lib(), O._stream(dyd)

    def check(out, want, what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(torch.from_numpy(want.astype(np.float32)).to(DEV))), what

    out = torch.full_like(dyd, float("nan"))
    N.check(lib.mtts_act_dropout_bwd(dyd.data_ptr(), None, out.data_ptr(), rows, cols, cols, O.ACT_NONE, float(p),
                                     seed.data_ptr(), st), "mtts_act_dropout_bwd")
    check(out, np.where(keep, dyn * sc, zero), "ACT_NONE")
    out = torch.full_like(dyd, float("nan"))
    N.check(lib.mtts_act_dropout_bwd(dyd.data_ptr(), yd.data_ptr(), out.data_ptr(), rows, cols, cols, O.ACT_RELU,
                                     float(p), seed.data_ptr(), st), "mtts_act_dropout_bwd")
    check(out, np.where(keep, np.where(yn > 0, dyn, zero) * sc, zero), "ACT_RELU")
    out = torch.full_like(dyd, float("nan"))
    N.check(lib.mtts_act_dropout_bwd_scaled(dyd.data_ptr(), None, rsd.data_ptr(), out.data_ptr(), rows, cols, cols,
                                            O.ACT_NONE, float(p), seed.data_ptr(), st), "mtts_act_dropout_bwd_scaled")
    check(out, np.where(keep, (dyn * rsn[:, None]) * sc, zero), "row scale")


# ------------------------------------------------------------------------------------------ b. GEMM epilogues
def _gemm_epilogue_case(prec, B, T, Cin, Cout, k, cfg, splits, gelu):
    """One O._gemm launch pair on a stride-2 output phase (output row b * 2T + 2u + 1: the dropout row key is the
    row of C, not the GEMM row): bias + [GELU with the pre-activation store] + dropout, zero pattern exact and
    values against float64; then with a residual and an output row scale, values only (dropout before the
    residual, the row scale last)."""
    from matcha.models.components import _ops as O

    p = 0.1
    P = O.PREC_BF16 if prec == "bf16" else O.PREC_FP32
    g = torch.Generator().manual_seed(1000 * B + T + Cin + Cout + k + (7 if gelu else 0))
    K = Cin * k
    x = torch.randn(B, T, Cin, generator=g).to(DEV)
    msk = (torch.rand(B * T, generator=g) > 0.2).float().to(DEV)
    # pre-activations of std ~0.6: no GELU output rounds to zero (erf saturates in fp32 below about -5.4)
    w = (torch.randn(Cout, K, generator=g) / math.sqrt(K) * 0.5).to(DEV)
    bias = (torch.randn(Cout, generator=g) * 0.3).to(DEV)
    res = torch.randn(B, 2 * T, Cout, generator=g).to(DEV)
    cs = (torch.rand(B * 2 * T, generator=g) + 0.5).to(DEV)
    Wp, Kp = O.pack_weight(w, P)
    offs = [j - k // 2 for j in range(k)]
    seed = _seed(12345, -678)
    # float64 reference of the phase rows
    xm = (x * msk.view(B, T, 1)).double()
    pre = _conv64(xm, w.double().view(Cout, k, Cin).permute(0, 2, 1), bias.double(), k // 2)
    assert pre.abs().max().item() < 5.0  # the test's own precondition (see above)
    a = _gelu64(pre) if gelu else pre
    keep = _keep_rc(seed, B * 2 * T, Cout, p).view(B, 2 * T, Cout)[:, 1::2]
    ftol = TOL[prec][0]
    act = O.ACT_GELU if gelu else O.ACT_NONE
    for full in (False, True):
        y = torch.full((B, 2 * T, Cout), 7.0, device=DEV)
        yp = torch.full((B, 2 * T, Cout), 7.0, device=DEV) if gelu else None
        O._gemm(x, T, T, B, 1, offs, Cin, Wp, Kp, Cout, y, 2 * T, 2, 1, prec=P, a_scale=msk, bias=bias, act=act,
                residual=res if full else None, c_scale=cs if full else None, C_pre=yp, dropout_p=p, seed=seed,
                tile_cfg=cfg, splits=splits)
        torch.cuda.synchronize()
        assert (y[:, 0::2] == 7.0).all()  # the other output phase is untouched
        got = y[:, 1::2]
        want = a * keep * _scale(p)
        if full:
            want = (want + res[:, 1::2].double()) * cs.view(B, 2 * T, 1)[:, 1::2].double()
        else:
            assert torch.equal(got != 0, keep)
        print("full" if full else "plain", "rel error %.3g" % rel(got, want))
        assert rel(got, want) < ftol, (full, rel(got, want))
        if gelu:  # the pre-activation is stored before the activation and the drop: never dropped
            assert (yp[:, 0::2] == 7.0).all() and (yp[:, 1::2] != 0).all()
            assert rel(yp[:, 1::2], pre) < ftol, rel(yp[:, 1::2], pre)
    if not gelu:
        # the scale, exactly: a zero A and a bias of ones make every pre-dropout value 1.0f, so each survivor is
        # float32(keep_scale(p)) to the bit (1 / (1 - p) differs from it by 7e-6, below any tolerance above)
        y = torch.full((B, 2 * T, Cout), 7.0, device=DEV)
        O._gemm(torch.zeros_like(x), T, T, B, 1, offs, Cin, Wp, Kp, Cout, y, 2 * T, 2, 1, prec=P, a_scale=msk,
                bias=torch.ones_like(bias), dropout_p=p, seed=seed, tile_cfg=cfg, splits=splits)
        torch.cuda.synchronize()
        assert torch.equal(y[:, 1::2], keep.float() * np.float32(DR.keep_scale(p)))


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("cfg,splits", [(7, 1), (41, 1), (42, 3), (44, 1), (44, 4), (-1, 0)])
def test_gemm_epilogue_dropout_bf16(cfg, splits, gelu):
    """Register-staged config 7 (generic epilogue), the LDS-DMA schedules (16-byte epilogue), split-K + combine
    pass, and the heuristic's choice."""
    _gemm_epilogue_case("bf16", 5, 77, 256, 320, 3, cfg, splits, gelu)


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("prec,B,T,Cin,Cout,k", [("fp32", 2, 37, 32, 64, 3), ("fp32", 2, 37, 32, 80, 3),
                                                 ("fp32", 2, 29, 256, 1, 1), ("bf16", 2, 29, 256, 1, 1)])
def test_gemm_epilogue_dropout_default_cfg(prec, B, T, Cin, Cout, k, gelu):
    """The exact-fp32 kernels at a whole and a partial (N = 80) column tile, and the duration predictor's
    1-channel projection (N = 1: the scalar epilogue, a lone half column pair)."""
    _gemm_epilogue_case(prec, B, T, Cin, Cout, k, -1, 0, gelu)


def test_gemm_epilogue_dropout_ff_storage_variants():
    """The FeedForward block's bf16-mixed launches, built the way _PreLNFeedForwardTM builds them: bf16 A, bf16
    C and C_pre with GELU + dropout in the forward; ACT_DGELU on a bf16 aux with a bf16 C + dropout in the
    backward -- the only place the FeedForward backward's mask is directly visible (dz's zero pattern)."""
    from matcha.models.components import _ops as O

    p = 0.1
    M, C = 300, 256
    H = 4 * C
    g = torch.Generator().manual_seed(5)
    n = torch.randn(M, C, generator=g).to(DEV).bfloat16()
    w1 = (torch.randn(H, C, generator=g) / math.sqrt(C) * 0.5).to(DEV)
    b1 = (torch.randn(H, generator=g) * 0.3).to(DEV)
    w2 = (torch.randn(C, H, generator=g) / math.sqrt(H)).to(DEV)
    seed = _seed(2 ** 31 - 2, 17)
    keep = _keep_rc(seed, M, H, p)
    ftol = TOL["bf16"][0]
    # forward: hid = dropout(gelu(n W1^T + b1)) (bf16), z = the pre-activation (bf16)
    W1p, K1p = O.packed(O.spec_linear((w1,), one_plane=not O._FF1_SPLIT), O.PREC_BF16)
    z = torch.empty(M, H, device=DEV, dtype=torch.bfloat16)
    hid = torch.empty(M, H, device=DEV, dtype=torch.bfloat16)
    O._gemm(n, M, M, 1, 1, [0], C, W1p, K1p, H, hid, M, prec=O.PREC_BF16, bias=b1, act=O.ACT_GELU, C_pre=z,
            dropout_p=p, seed=seed)
    torch.cuda.synchronize()
    pre = n.double() @ w1.double().T + b1.double()
    assert pre.abs().max().item() < 5.0
    assert torch.equal(hid != 0, keep)
    assert rel(hid, _gelu64(pre) * keep * _scale(p)) < ftol
    assert (z != 0).all() and rel(z, pre) < ftol
    # backward: dz = (dy W2) * gelu'(z) * keep * scale (bf16), z read as the bf16 aux
    dy = torch.randn(M, C, generator=g).to(DEV)
    W2t, K2p = O.packed(O.spec_linear((w2,), dgrad=True), O.PREC_BF16)
    dz = torch.empty(M, H, device=DEV, dtype=torch.bfloat16)
    O._gemm(dy, M, M, 1, 1, [0], C, W2t, K2p, H, dz, M, prec=O.PREC_BF16, act=O.ACT_DGELU, aux=z, dropout_p=p,
            seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(dz != 0, keep)
    want = (dy.double() @ w2.double()) * _dgelu64(z.double()) * keep * _scale(p)
    assert rel(dz, want) < ftol, rel(dz, want)


# ------------------------------------------------------------------------------------------ c. the ops
def _relu_inputs(prec, Cout, fan, g):
    """Conv weight scale and bias ahead of a ReLU.  fp32: generic values (the kernel and the float64 reference
    agree on the sign of every pre-activation to ~1e-6 of its scale).  bf16: the pre-activation carries
    ~4e-3 of rounding, so about 0.15 % of generic pre-activations would land on the other side of the kink than
    in float64 and their whole gradient would count as error (~5 % in relative L2, unrelated to dropout); there
    the bias is +-3 with |w.x| << 3, as in test_conv_relu_dropout_grad: each gate is decided by its channel."""
    if prec == "fp32":
        return 1.0 / math.sqrt(fan), torch.randn(Cout, generator=g) * 0.5
    return 0.2 / math.sqrt(fan), torch.where(torch.arange(Cout) % 2 == 0, 3.0, -3.0)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,K,Nn", [(2, 33, 64, 48), (2, 77, 256, 256)])
def test_linear_tm_dropout_vs_float64(monkeypatch, prec, B, T, K, Nn):
    """(residual + dropout((x * m) W^T + b)) * m; row key = the flat output row.  (2, 77, 256, 256) reaches the
    LDS-DMA schedules in bf16."""
    from matcha.models.components import _ops as O

    g = torch.Generator().manual_seed(B * T + K)
    x = torch.randn(B, T, K, generator=g).to(DEV)
    w = (torch.randn(Nn, K, 1, generator=g) / math.sqrt(K)).to(DEV)
    b = torch.randn(Nn, generator=g).to(DEV)
    r = torch.randn(B, T, Nn, generator=g).to(DEV)
    m = _ragged(B, T)
    md = m.double().unsqueeze(-1)

    def ref(seeds, x, w, b, r):
        d = _drop64(seeds[0], B * T, Nn, 0.1).view(B, T, Nn)
        return (r + ((x * md) @ w[:, :, 0].T + b) * d) * md

    _run_op(monkeypatch, lambda x, w, b, r: O.linear_tm(x, w, b, residual=r, dropout_p=0.1, in_scale=m, out_scale=m),
            ref, [x, w, b, r], prec, 1)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [3, 5])
def test_conv_tm_relu_dropout_vs_float64(monkeypatch, prec, k):
    """dropout(relu(conv(x * m) + b)): a dropped element is exactly zero, a kept one with a clearly positive
    pre-activation is not; values and gradients against float64."""
    from matcha.models.components import _ops as O

    B, T, Cin, Cout = 3, 50, 64, 96
    g = torch.Generator().manual_seed(k)
    ws, b = _relu_inputs(prec, Cout, Cin * k, g)
    x = torch.randn(B, T, Cin, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, k, generator=g) * ws).to(DEV)
    b = b.to(DEV)
    m = _ragged(B, T)
    md = m.double().unsqueeze(-1)
    pre = {}

    def ref(seeds, x, w, b):
        pre["v"] = _conv64(x * md, w, b, k // 2)
        return torch.relu(pre["v"]) * _drop64(seeds[0], B * T, Cout, 0.1).view(B, T, Cout)

    y, _, seeds = _run_op(monkeypatch, lambda x, w, b: O.conv_tm(x, w, b, mask=m, relu=True, dropout_p=0.1), ref,
                          [x, w, b], prec, 1)
    keep = _keep_rc(seeds[0], B * T, Cout, 0.1).view(B, T, Cout)
    assert (y[~keep] == 0).all()
    sure = keep & (pre["v"].detach() > 0.05)
    assert sure.any() and (y[sure] > 0).all()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_ffn_tm_dropout_vs_float64(monkeypatch, prec):
    """(x + dropout_out(conv2(dropout_in(relu(conv1(x * m)))))) * m: two seeds, p_in drawn first; conv2 reads the
    UNMASKED h (the rows next to the padding see the padded rows' relu(bias))."""
    from matcha.models.components import _ops as O

    B, T, C, F_ = 3, 45, 64, 128
    g = torch.Generator().manual_seed(2)
    ws, b1 = _relu_inputs(prec, F_, 3 * C, g)
    x = torch.randn(B, T, C, generator=g).to(DEV)
    w1 = (torch.randn(F_, C, 3, generator=g) * ws).to(DEV)
    b1 = b1.to(DEV)
    w2 = (torch.randn(C, F_, 3, generator=g) / math.sqrt(3 * F_)).to(DEV)
    b2 = (torch.randn(C, generator=g) * 0.1).to(DEV)
    m = _ragged(B, T)
    md = m.double().unsqueeze(-1)

    def ref(seeds, x, w1, b1, w2, b2):
        h = torch.relu(_conv64(x * md, w1, b1, 1)) * _drop64(seeds[0], B * T, F_, 0.1).view(B, T, F_)
        f = _conv64(h, w2, b2, 1) * _drop64(seeds[1], B * T, C, 0.19).view(B, T, C)
        return (x + f) * md

    _run_op(monkeypatch, lambda x, a, bb, c, d: O.conv_ffn_tm(x, a, bb, c, d, m, residual=x, p_in=0.1, p_out=0.19), ref,
            [x, w1, b1, w2, b2], prec, 2)


def _ff_inputs(M, C, g):
    x = torch.randn(M, C, generator=g).to(DEV)
    w1 = (torch.randn(4 * C, C, generator=g) / math.sqrt(C)).to(DEV)
    b1 = torch.randn(4 * C, generator=g).to(DEV)
    w2 = (torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C)).to(DEV)
    b2 = torch.randn(C, generator=g).to(DEV)
    return x, w1, b1, w2, b2


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("M,C", [(130, 32), (600, 256)])
def test_ff_tm_dropout_vs_float64(monkeypatch, prec, M, C):
    """dropout(gelu(x W1^T + b1)) W2^T + b2 + r: the mask sits between the GELU and the second Linear."""
    from matcha.models.components import _ops as O

    g = torch.Generator().manual_seed(M + C)
    x, w1, b1, w2, b2 = _ff_inputs(M, C, g)
    r = torch.randn(M, C, generator=g).to(DEV)

    def ref(seeds, x, w1, b1, w2, b2, r):
        return (_gelu64(x @ w1.T + b1) * _drop64(seeds[0], M, 4 * C, 0.25)) @ w2.T + b2 + r

    _run_op(monkeypatch, lambda x, w1, b1, w2, b2, r: O.ff_tm(x, w1, b1, w2, b2, residual=r, dropout_p=0.25), ref,
            [x, w1, b1, w2, b2, r], prec, 1)


def _ln_inputs(C, g):
    return (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C,heads", [(2, 150, 256, 4), (3, 37, 64, 2)])
def test_preln_ff_tm_dropout_vs_float64(monkeypatch, prec, B, T, C, heads):
    """h + W2 dropout(gelu(W1 LN(h) + b1)) + b2 (bf16-mixed: bf16 LN output, hidden, pre-activation and dz)."""
    from matcha.models.components import _ops as O

    g = torch.Generator().manual_seed(B * T + C)
    h = torch.randn(B, T, C, generator=g).to(DEV)
    lw, lb = _ln_inputs(C, g)
    _, w1, b1, w2, b2 = _ff_inputs(1, C, g)
    b1, b2 = b1 * 0.1, b2 * 0.1

    def ref(seeds, h, lw, lb, w1, b1, w2, b2):
        n = F.layer_norm(h, (C,), lw, lb, 1e-5)
        d = _drop64(seeds[0], B * T, 4 * C, 0.1).view(B, T, 4 * C)
        return h + (_gelu64(n @ w1.T + b1) * d) @ w2.T + b2

    _run_op(monkeypatch, lambda h, lw, lb, w1, b1, w2, b2: O.preln_ff_tm(h, lw, lb, 1e-5, w1, b1, w2, b2, dropout_p=0.1),
            ref, [h, lw, lb, w1, b1, w2, b2], prec, 1)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C,heads", [(2, 150, 256, 4), (3, 37, 64, 2)])
def test_preln_attention_tm_dropout_vs_float64(monkeypatch, prec, B, T, C, heads):
    """h + dropout(to_out(SDPA(LN(h) [Wq; Wk; Wv]^T, additive 0/1 key mask)) + b_out), ragged key mask."""
    from matcha.models.components import _ops as O

    g = torch.Generator().manual_seed(B * T + C + 1)
    h = torch.randn(B, T, C, generator=g).to(DEV)
    lw, lb = _ln_inputs(C, g)
    wq, wk, wv, wo = ((torch.randn(C, C, generator=g) * C ** -0.5).to(DEV) for _ in range(4))
    bo = (torch.randn(C, generator=g) * 0.1).to(DEV)
    kb = _ragged(B, T, 7)
    d_ = C // heads

    def ref(seeds, h, lw, lb, wq, wk, wv, wo, bo):
        n = F.layer_norm(h, (C,), lw, lb, 1e-5)
        sp = lambda t: t.view(B, T, heads, d_).transpose(1, 2)
        s = sp(n @ wq.T) @ sp(n @ wk.T).transpose(-1, -2) / math.sqrt(d_) + kb.double()[:, None, None, :]
        o = (s.softmax(-1) @ sp(n @ wv.T)).transpose(1, 2).reshape(B, T, C)
        return h + (o @ wo.T + bo) * _drop64(seeds[0], B * T, C, 0.1).view(B, T, C)

    _run_op(monkeypatch,
            lambda h, lw, lb, wq, wk, wv, wo, bo: O.preln_attention_tm(h, lw, lb, 1e-5, kb, heads, wq, wk, wv, wo, bo,
                                                                       dropout_p=0.1),
            ref, [h, lw, lb, wq, wk, wv, wo, bo], prec, 1)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", [(300, 192), (5, 1024)])
def test_layer_norm_tm_dropout_vs_float64(monkeypatch, relu, M, C):
    """LayerNorm -> [ReLU] -> dropout, fp32 (the op has no bf16 mode): the ReLU comes BEFORE the drop; without
    it the zero pattern of the output is the mask."""
    from matcha.models.components import _ops as O

    g = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).to(DEV)
    w = ((torch.rand(C, generator=g) * 0.9 + 0.1) * torch.sign(torch.randn(C, generator=g))).to(DEV)
    b = (torch.randn(C, generator=g) * 0.5).to(DEV)
    pre = {}

    def ref(seeds, x, w, b):
        pre["v"] = F.layer_norm(x, (C,), w, b, 1e-5)
        return (torch.relu(pre["v"]) if relu else pre["v"]) * _drop64(seeds[0], M, C, 0.1)

    y, _, seeds = _run_op(monkeypatch, lambda x, w, b: O.layer_norm_tm(x, w, b, 1e-5, relu=relu, dropout_p=0.1), ref,
                          [x, w, b], "fp32", 1)
    keep = _keep_rc(seeds[0], M, C, 0.1)
    if relu:
        assert (y[~keep] == 0).all()
        sure = keep & (pre["v"].detach() > 1e-3)
        assert sure.any() and (y[sure] > 0).all()
    else:
        assert torch.equal(y != 0, keep)


@pytest.mark.parametrize("M,C", [(7, 192), (5, 1024)])
def test_layer_norm_tail_scale_exact(monkeypatch, M, C):
    """w = 0, b = 1: the LayerNorm output is 1.0f exactly, so the tail's survivors are float32(keep_scale(p)) to
    the bit."""
    from matcha.models.components import _ops as O

    seeds = _record_seeds(monkeypatch)
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(C)).to(DEV)
    for p in (0.1, 0.19):
        y = O.layer_norm_tm(x, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), 1e-5, relu=True, dropout_p=p)
        assert torch.equal(y, _keep_rc(seeds[-1], M, C, p).float() * np.float32(DR.keep_scale(p))), p


# ------------------------------------------------------------------------------------------ d. attention
def _attn_modes():
    from matcha.models.components import _ops as O

    return {"fp32": (O.PREC_FP32, torch.float32), "bf16": (O.PREC_BF16, torch.float32),
            "bf16-io16": (O.PREC_BF16, torch.bfloat16)}


PATTERN_SHAPES = [(2, 33, 2, 96, "1"), (2, 128, 2, 96, "1"),  # the short kernels and their edge
                  (2, 129, 1, 64, "1"), (1, 300, 4, 32, "1"), (3, 200, 2, 96, "1"),  # long: key tail, several tiles
                  (2, 33, 2, 96, "0"), (2, 128, 2, 96, "0")]  # the short shapes down the long kernels


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16-io16"])
@pytest.mark.parametrize("B,T,H,D,short", PATTERN_SHAPES)
def test_attention_dropout_pattern_is_host_mask(monkeypatch, B, T, H, D, short, mode):
    """The dropped probability matrix, exposed exactly: with v zero but a one-hot window v[key w0 + j] = e_j,
    o[b, q, h*D + j] is the dropped probability of key w0 + j; the windows are swept over all T keys.  Its zero
    pattern must be the host mask with row key (b*H + h)*T + q and column key = the GLOBAL key index, for every
    (b, h) -- a mask shared between heads or batch entries, or keyed on a tile-local key, fails here -- and the
    kept entries must be the float64 softmax times the scale.  0/1 additive key bias and q, k ~ 0.5 N(0, 1):
    every probability is positive and far from rounding to zero."""
    from matcha.models.components import _ops as O

    monkeypatch.setenv("MTTS_ATTN_SHORT", short)
    prec, dt = _attn_modes()[mode]
    p, C = 0.1, H * D
    g = torch.Generator().manual_seed(B * T + H * D)
    qk = (torch.randn(B, T, 2 * C, generator=g) * 0.5).to(DEV)
    kb = _ragged(B, T, 7)
    seed = _seed(-1234567, 99)
    P = torch.zeros(B, H, T, T, device=DEV)
    for w0 in range(0, T, D):
        n = min(D, T - w0)
        v = torch.zeros(B, T, H, D, device=DEV)
        v[:, w0:w0 + n, :, :n] = torch.eye(n, device=DEV)[None, :, None, :]
        qkv = torch.cat([qk, v.view(B, T, C)], -1).to(dt).contiguous()
        o = torch.full((B, T, C), float("nan"), device=DEV, dtype=dt)
        lse = torch.empty(B, H, T, device=DEV)
        O._attn_fwd(qkv, kb, o, lse, H, prec, dropout_p=p, seed=seed)
        torch.cuda.synchronize()
        o4 = o.float().view(B, T, H, D)
        assert (o4[..., n:] == 0).all()  # no key behind the zero columns of v
        P[:, :, :, w0:w0 + n] = o4[..., :n].permute(0, 2, 1, 3)
    keep = _keep_rc(seed, B * H * T, T, p).view(B, H, T, T)
    for b in range(B):
        for h in range(H):
            assert torch.equal(P[b, h] != 0, keep[b, h]), (b, h)
    q, k = (t.double().view(B, T, H, D).transpose(1, 2) for t in qk.split(C, dim=-1))
    want = (q @ k.transpose(-1, -2) / math.sqrt(D) + kb.double()[:, None, None, :]).softmax(-1) * keep * _scale(p)
    if mode == "fp32":
        torch.testing.assert_close(P.double(), want, rtol=1e-4, atol=2e-5)
    else:
        assert rel(P, want) < 1.5e-2, rel(P, want)


@pytest.mark.parametrize("T", [128, 256])  # the short and the long forward kernel
def test_attention_dropout_scale_exact(T):
    """q = k = 0 and no key bias: every score is 0, every probability 1 / T -- exact in fp32 for a power-of-two
    T, in whichever order the kernel normalises and rescales -- so with a one-hot v window each surviving output
    is float32(keep_scale(p)) / T to the bit, and the pattern is again the host mask."""
    from matcha.models.components import _ops as O

    B, H, D, p = 1, 2, 32, 0.1
    C = H * D
    seed = _seed(31337, -9)
    kb = torch.zeros(B, T, device=DEV)
    want = _keep_rc(seed, B * H * T, T, p).view(B, H, T, T).float() * (np.float32(DR.keep_scale(p)) / np.float32(T))
    for w0 in range(0, T, D):
        v = torch.zeros(B, T, H, D, device=DEV)
        v[:, w0:w0 + D] = torch.eye(D, device=DEV)[None, :, None, :]
        qkv = torch.cat([torch.zeros(B, T, 2 * C, device=DEV), v.view(B, T, C)], -1).contiguous()
        o = torch.full((B, T, C), float("nan"), device=DEV)
        lse = torch.empty(B, H, T, device=DEV)
        O._attn_fwd(qkv, kb, o, lse, H, O.PREC_FP32, dropout_p=p, seed=seed)
        torch.cuda.synchronize()
        assert torch.equal(o.view(B, T, H, D).permute(0, 2, 1, 3), want[..., w0:w0 + D]), w0


VALUE_CASES = [(2, 70, 2, 96, "enc", "1"), (2, 130, 2, 64, "dec", "1"), (1, 300, 4, 32, "dec", "1"),
               (2, 130, 2, 64, "dec", "0"), (1, 300, 4, 32, "dec", "0")]  # "0": the two-launch backward


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,H,D,bias_kind,merged", VALUE_CASES)
def test_attention_dropout_values_vs_float64(monkeypatch, B, T, H, D, bias_kind, merged, precision):
    """_attn_fwd + _attn_bwd with dropout and an explicit seed on random q, k, v, dO against float64 autograd of
    softmax(s) * keep * scale @ v: the forward, dQ and dK/dV kernels (merged and two-launch) must all regenerate
    the same mask.  Encoder key bias (m - 1) * 1e4 or the decoder's additive 0/1 mask; bounds of
    test_attention_fwd_bwd."""
    from matcha.models.components import _ops as O

    monkeypatch.setenv("MTTS_ATTN_BWD_MERGED", merged)
    prec = O.PREC_FP32 if precision == "fp32" else O.PREC_BF16
    p, C = 0.1, H * D
    g = torch.Generator().manual_seed(B * 1000 + T)
    qkv = (torch.randn(B, T, 3 * C, generator=g) * 1.5).to(DEV)
    do = torch.randn(B, T, C, generator=g).to(DEV)
    m = _ragged(B, T, 9)
    kb = (m - 1) * 1e4 if bias_kind == "enc" else m
    seed = _seed(424242, -5)
    o = torch.empty(B, T, C, device=DEV)
    lse = torch.empty(B, H, T, device=DEV)
    O._attn_fwd(qkv, kb, o, lse, H, prec, dropout_p=p, seed=seed)
    dqkv = O._attn_bwd(do, qkv, kb, o, lse, H, prec, dropout_p=p, seed=seed)
    torch.cuda.synchronize()
    xr = qkv.double().requires_grad_(True)
    q, k, v = (t.view(B, T, H, D).transpose(1, 2) for t in xr.split(C, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(D) + kb.double()[:, None, None, :]
    drop = _drop64(seed, B * H * T, T, p).view(B, H, T, T)
    orf = ((s.softmax(-1) * drop) @ v).transpose(1, 2).reshape(B, T, C)
    orf.backward(do.double())
    print("rel errors: o %.3g, dqkv %.3g" % (rel(o, orf), rel(dqkv, xr.grad)))
    if precision == "fp32":
        torch.testing.assert_close(o.double(), orf.detach(), rtol=1e-4, atol=2e-5)
        torch.testing.assert_close(dqkv.double(), xr.grad, rtol=1e-4, atol=5e-5)
    else:
        assert rel(o, orf) < 1.5e-2
        gn = xr.grad.norm().item()
        for i, name in enumerate("qkv"):
            err = (dqkv[..., i * C:(i + 1) * C].double() - xr.grad[..., i * C:(i + 1) * C]).norm().item()
            assert err < 3e-2 * gn, (name, err / gn)

