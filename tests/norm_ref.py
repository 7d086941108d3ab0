"""Plain-torch restatements of csrc/norms.hip and csrc/losses.hip, written from the formulas -- test
infrastructure only.  Run them on float64 tensors for the reference, on float32 ones for the "plain fp32
restatement" the conditioning tests compare a kernel's error with; gradients come from autograd.
gn_variant / ln_fwd_variant / ln_bwd_rows_per_block restate the launchers' shape rules, so the case tables
of tests/test_norms_float64_gpu.py can be checked on the CPU for the kernels they claim to reach."""
from __future__ import annotations

import math

import numpy as np
import torch

GN_THREADS = 1024  # norms.hip: kGnThreads


def gn_mish_ref(h, gamma, beta, G, mask=None, add=None, eps=1e-5):
    """mish(GroupNorm(h)) * mask[b, t] + add[b, c] of a token-major h [B, T, C].  The statistics run over the
    whole padded T of each (b, group) (two-pass, biased variance, eps inside the sqrt); mish(u) =
    u * tanh(log(1 + exp(u))) with no softplus threshold."""
    B, T, C = h.shape
    x = h.reshape(B, T, G, C // G)
    mean = x.mean(dim=(1, 3), keepdim=True)
    d = x - mean
    var = (d * d).mean(dim=(1, 3), keepdim=True)
    xhat = (d / torch.sqrt(var + eps)).reshape(B, T, C)
    u = xhat * gamma + beta
    y = u * torch.tanh(torch.logaddexp(u, torch.zeros_like(u)))
    if mask is not None:
        y = y * mask[:, :, None]
    if add is not None:
        y = y + add[:, None, :]
    return y


def gn_u_ref(h, gamma, beta, G, eps=1e-5):
    """The Mish argument u = xhat * gamma + beta of gn_mish_ref (to band elements by |u|)."""
    B, T, C = h.shape
    x = h.reshape(B, T, G, C // G)
    d = x - x.mean(dim=(1, 3), keepdim=True)
    var = (d * d).mean(dim=(1, 3), keepdim=True)
    return (d / torch.sqrt(var + eps)).reshape(B, T, C) * gamma + beta


def layer_norm_ref(x, w, b, eps=1e-5):
    """LayerNorm over the last dim: two-pass, biased variance, eps inside the sqrt."""
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + eps) * w + b


def losses_ref(u_pred, mu_y, x1, z, mask, sigma_min):
    """(diff_loss, prior_loss) per the header of losses.hip.  u_pred [B, T, C] or None, mu_y [B, C, T] or
    None, x1 (= y) and z [B, C, T], mask [B, T].  The diff loss is unmasked (padded frames contribute), the
    prior loss is masked, both are divided by sum(mask) * C.  u = x1 - float32(1 - sigma_min) * z: the kernel
    multiplies by that fp32 constant, here widened."""
    C = x1.shape[1]
    denom = mask.sum() * C
    zero = torch.zeros((), dtype=x1.dtype)
    diff = prior = zero
    if u_pred is not None:
        one_minus_sigma = float(np.float32(1.0 - float(sigma_min)))
        u = x1 - one_minus_sigma * z
        diff = ((u_pred.transpose(1, 2) - u) ** 2).sum() / denom
    if mu_y is not None:
        prior = (0.5 * ((x1 - mu_y) ** 2 + math.log(2 * math.pi)) * mask[:, None, :]).sum() / denom
    return diff, prior


def gn_passes(T, C, G):
    """(cols, rows per pass, passes) of a GroupNorm+Mish launch -- norms.hip:199 (cols = cg / 4, rpp =
    kGnThreads / cols) and the `passes` of gn_fwd_launch / gn_bwd_launch (norms.hip:643, :691)."""
    cols = C // G // 4
    rpp = GN_THREADS // cols
    return cols, rpp, (T + rpp - 1) // rpp


def gn_variant(T, C, G):
    """(forward, backward) kernel a shape runs.  Restates gn_fwd_launch (norms.hip:643-652: passes <= 4 ->
    reg<4>, <= 8 -> reg<8>, else streaming) and gn_bwd_launch (norms.hip:691-700: <= 4 -> reg<4>, <= 6 ->
    reg<6>, else streaming)."""
    p = gn_passes(T, C, G)[2]
    fwd = "reg4" if p <= 4 else "reg8" if p <= 8 else "stream"
    bwd = "reg4" if p <= 4 else "reg6" if p <= 6 else "stream"
    return fwd, bwd


def ln_fwd_variant(M, C):
    """(NI, R): float4 chunks per lane and rows per wave of the LayerNorm forward.  Restates
    mtts_layernorm_fwd (norms.hip:761: R = 4 when C <= 256 and M >= 4 * 4 * 512, and :766-775: NI = 4 with
    R = 1 when C > 256)."""
    if C > 256:
        return 4, 1
    return 1, (4 if M >= 4 * 4 * 512 else 1)


def ln_bwd_rows_per_block(M, C):
    """Rows per block of the LayerNorm backward.  Restates ln_bwd_rows_in_flight / ln_rows_per_block
    (norms.hip:507-513): ceil(M / 768) rounded up to a multiple of q = 16 (C <= 256) or 4, within [q, 128]."""
    q = 4 * (4 if C <= 256 else 1)
    r = (M + 767) // 768
    r = (r + q - 1) // q * q
    return q if r < q else min(r, 128)
