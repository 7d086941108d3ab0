"""tests/norm_ref.py on the CPU: the float64 references equal torch's own float64 ops (outputs and every
gradient to 1e-12), and the case tables of tests/test_norms_float64_gpu.py reach the kernel variants and the
boundaries they claim, by the launchers' rules as norm_ref restates them."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
import test_norms_float64_gpu as G

RTOL = 1e-12


def _r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _same(a, b, what):
    a, b = a.detach(), b.detach()
    err = float((a - b).abs().max() / b.abs().max())
    assert err <= RTOL, (what, err)


def _grads(y, dy, leaves):
    return torch.autograd.grad(y, leaves, dy)


@pytest.mark.parametrize("B,T,C,G_,masked,add", [(2, 7, 24, 2, True, True), (3, 5, 32, 8, True, False),
                                                 (1, 1, 16, 4, False, True), (2, 33, 40, 2, False, False)])
def test_gn_mish_ref_equals_torch(B, T, C, G_, masked, add):
    h = (_r(B, T, C, seed=T) * 3 + 1).requires_grad_(True)
    gamma = (1 + 0.1 * _r(C, seed=T + 1)).requires_grad_(True)
    beta = (0.1 * _r(C, seed=T + 2)).requires_grad_(True)
    a = _r(B, C, seed=T + 3).requires_grad_(True) if add else None
    m = G._ragged_mask(B, T).double() if masked else None
    dy = _r(B, T, C, seed=T + 4)
    want = F.mish(F.group_norm(h.transpose(1, 2), G_, gamma, beta, 1e-5)).transpose(1, 2)
    if m is not None:
        want = want * m[..., None]
    if a is not None:
        want = want + a[:, None, :]
    got = R.gn_mish_ref(h, gamma, beta, G_, m, a, 1e-5)
    _same(got, want, "y")
    leaves = [h, gamma, beta] + ([a] if add else [])
    for i, (p, q) in enumerate(zip(_grads(got, dy, leaves), _grads(want, dy, leaves))):
        _same(p, q, f"grad {i}")
    u = R.gn_u_ref(h, gamma, beta, G_)
    _same(u * torch.tanh(F.softplus(u, threshold=1e9)), F.mish(F.group_norm(h.transpose(1, 2), G_, gamma, beta,
                                                                            1e-5)).transpose(1, 2), "u")


@pytest.mark.parametrize("M,C", [(5, 4), (9, 36), (3, 260)])
def test_layer_norm_ref_equals_torch(M, C):
    x = (_r(M, C, seed=C) * 3 + 1).requires_grad_(True)
    w = (1 + 0.1 * _r(C, seed=C + 1)).requires_grad_(True)
    b = (0.1 * _r(C, seed=C + 2)).requires_grad_(True)
    dy = _r(M, C, seed=C + 3)
    got, want = R.layer_norm_ref(x, w, b, 1e-5), F.layer_norm(x, (C,), w, b, 1e-5)
    _same(got, want, "y")
    for i, (p, q) in enumerate(zip(_grads(got, dy, [x, w, b]), _grads(want, dy, [x, w, b]))):
        _same(p, q, f"grad {i}")


@pytest.mark.parametrize("sigma", [2.0 ** -13, 1e-4])
@pytest.mark.parametrize("B,C,T", [(1, 1, 1), (2, 7, 9), (3, 5, 66)])
def test_losses_ref_equals_torch_expression(B, C, T, sigma):
    """The expression of tests/test_cfm_prep_gpu.py (flow_matching.py:141-149, matcha_tts.py:319-323) in
    float64.  1 - 2^-13 is exact in fp32, so there the plain `1 - sigma` applies; at 1e-4 the constant is the
    fp32 one the kernel multiplies by."""
    v = {k: t.double() for k, t in G._loss_inputs(B, C, T).items()}
    u_pred, mu_y = v["u_pred"].requires_grad_(True), v["mu_y"].requires_grad_(True)
    x1, z, mask = v["x1"], v["z"], v["mask"]
    c = 1 - sigma if sigma == 2.0 ** -13 else float(np.float32(1 - sigma))
    u = x1 - c * z
    m3 = mask[:, None, :]
    diff_w = torch.sum((u_pred.transpose(1, 2) - u) ** 2) / (torch.sum(m3) * C)
    prior_w = torch.sum(0.5 * ((x1 - mu_y) ** 2 + math.log(2 * math.pi)) * m3) / (torch.sum(m3) * C)
    diff, prior = R.losses_ref(u_pred, mu_y, x1, z, mask, sigma)
    _same(diff, diff_w, "diff")
    _same(prior, prior_w, "prior")
    one = torch.ones((), dtype=torch.float64)
    for got, want, leaf in ((diff, diff_w, u_pred), (prior, prior_w, mu_y)):
        _same(_grads(got, one, [leaf])[0], _grads(want, one, [leaf])[0], "grad")
    d0, p0 = R.losses_ref(None, mu_y, x1, z, mask, sigma)
    assert float(d0) == 0.0 and float(p0) == float(prior)


def test_fp32_restatement_separates_one_pass_variance():
    """The conditioning input (mean 30, std 0.5): in plain fp32 a one-pass variance E[x^2] - E[x]^2 errs far
    more than the two-pass form the references (and the kernels) use, so a bound of 4 x the two-pass error
    tells the recipes apart."""
    x = G._gn_inputs(2, 600, 256, 8, scale=0.5, shift=30.0)["h"]
    xg = x.reshape(2, 600, 8, 32)
    ref = R.gn_u_ref(x.double(), torch.ones(256).double(), torch.zeros(256).double(), 8)
    two = R.gn_u_ref(x, torch.ones(256), torch.zeros(256), 8)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var1 = (xg * xg).mean(dim=(1, 3), keepdim=True) - mean * mean
    one = ((xg - mean) / torch.sqrt(var1 + 1e-5)).reshape(2, 600, 256)
    e2, e1 = float((two.double() - ref).abs().max()), float((one.double() - ref).abs().max())
    assert e1 > 20 * G.COND_FACTOR * e2, (e1, e2)


# ------------------------------------------------------------------------------------------ case tables
def test_gn_cases_cover_every_variant_and_boundary():
    passes = lambda c: R.gn_passes(c[1], c[2], c[3])[2]  # noqa: E731
    variants = {R.gn_variant(T, C, G_) for _, T, C, G_, _, _ in G.GN_CASES}
    assert {v[0] for v in variants} == {"reg4", "reg8", "stream"}
    assert {v[1] for v in variants} == {"reg4", "reg6", "stream"}
    # both sides of every switch, in the model's geometry (cpg 32) and at cols 64
    for C, G_ in ((256, 8), (512, 2)):
        assert {4, 5, 6, 7, 8, 9} <= {passes(c) for c in G.GN_CASES if (c[2], c[3]) == (C, G_)}
    # exactly on a boundary: T = P * rpp and T = P * rpp + 1 (a dropped or doubled row at t = P * rpp)
    for P in (4, 6, 8):
        for C, G_ in ((256, 8), (512, 2)):
            rpp = R.gn_passes(1, C, G_)[1]
            ts = {c[1] for c in G.GN_CASES if (c[2], c[3]) == (C, G_)}
            assert {P * rpp, P * rpp + 1} <= ts
    idle = {R.gn_passes(c[1], c[2], c[3])[0] for c in G.GN_CASES if 1024 % R.gn_passes(c[1], c[2], c[3])[0]}
    assert {3, 5, 59} <= idle  # cols that do not divide 1024: idle threads, odd-cols column sums
    for cols in (3, 59):  # each of them in a register-resident and past the first switch
        ps = {passes(c) for c in G.GN_CASES if R.gn_passes(c[1], c[2], c[3])[0] == cols}
        assert min(ps) <= 4 < max(ps)
    assert any(not c[4] and not c[5] for c in G.GN_CASES) and any(c[0] == 1 for c in G.GN_CASES)
    assert any(c[1] == 1 for c in G.GN_CASES)
    # the backward takes cpg <= 256
    assert all(c[2] // c[3] <= 256 and (c[2] // c[3]) % 4 == 0 for c in G.GN_CASES)
    for B, T, C, G_ in G.GN_BF16_CASES:
        assert (B, T, C, G_, True, True) in G.GN_CASES or (T, C, G_) == (300, 24, 2)
    assert {R.gn_variant(T, C, G_) for _, T, C, G_ in G.GN_BF16_CASES} == {
        ("reg4", "reg4"), ("reg8", "reg6"), ("reg8", "stream"), ("stream", "stream")}


def test_ln_cases_cover_every_variant_and_tail():
    fwd = {(M, C): R.ln_fwd_variant(M, C) for M, C in G.LN_CASES}
    assert any(v == (1, 4) and M % 16 != 0 for (M, C), v in fwd.items())  # four rows per wave, row tail
    assert any(v == (1, 4) and M % 16 != 0 and C < 256 for (M, C), v in fwd.items())
    assert any(v == (1, 1) and M == 8191 for (M, C), v in fwd.items())  # just below the switch
    assert any(v == (4, 1) and C % 256 != 0 for (M, C), v in fwd.items())  # a partly filled chunk
    assert {(C - 1) // 256 + 1 for (M, C), v in fwd.items() if v[0] == 4} == {2, 4}
    assert set(fwd.values()) == {(1, 1), (1, 4), (4, 1)}
    rows = {R.ln_bwd_rows_per_block(M, C) for M, C in G.LN_CASES}
    assert {4, 16, 32, 128} <= rows
    assert any(R.ln_bwd_rows_per_block(M, C) == 128 and M > 128 * 768 for M, C in G.LN_CASES)  # the cap bites
    # a last block of one row (rend), for both row groupings
    assert any(M % R.ln_bwd_rows_per_block(M, C) == 1 and C <= 256 for M, C in G.LN_CASES)
    assert any(M % R.ln_bwd_rows_per_block(M, C) == 1 and C > 256 for M, C in G.LN_CASES)
    assert {R.ln_fwd_variant(M, C) for M, C in G.LN_RES_CASES} == {(1, 4), (4, 1)}
    assert R.ln_fwd_variant(*G.LN_RELU_CASE) == (1, 4)


def test_ln_rules_at_the_documented_points():
    assert R.ln_fwd_variant(8192, 256) == (1, 4) and R.ln_fwd_variant(8191, 256) == (1, 1)
    assert R.ln_fwd_variant(100000, 260) == (4, 1)
    assert [R.ln_bwd_rows_per_block(M, 256) for M in (1, 12288, 12289, 98304, 98305, 10 ** 6)] == [
        16, 16, 32, 128, 128, 128]
    assert [R.ln_bwd_rows_per_block(M, 1024) for M in (1, 3072, 3073)] == [4, 4, 8]
    assert R.gn_passes(600, 256, 8) == (8, 128, 5) and R.gn_variant(600, 256, 8) == ("reg8", "reg6")
    assert R.gn_passes(140, 472, 2) == (59, 17, 9)


def test_loss_cases_cover_the_tile_edges():
    ts = {T for _, _, T in G.LOSS_CASES}
    assert {1, 63, 64, 65, 128, 129} <= ts  # T = 1, below / on / past one and two 64-frame tiles
    cs = {C for _, C, _ in G.LOSS_CASES}
    assert 1 in cs and 128 in cs and any(C % 4 for C in cs)
    for B, C, T in G.LOSS_CASES:
        m = G._loss_inputs(B, C, T)["mask"]
        assert float(m[0].sum()) == T and (B == 1 or float(m[1].sum()) == 1)
