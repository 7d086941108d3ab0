"""The vocoder entry points of include/mtts_vocoder.h on torch tensors (inference only, device tensors only).

Activations are token-major [B*L, C] fp32; weights come packed (``pack_conv`` / ``pack_upsample`` / ``pack_post``,
plain torch, once per load -- not on the hot path)."""
from __future__ import annotations

import ctypes

import torch

from matcha import _native as N
from matcha._abi import (MTTS_ERR_INVALID_ARG as ERR_INVALID_ARG, MTTS_ERR_SHAPE as ERR_SHAPE,  # noqa: F401
                         MTTS_VOC_ACC_ADD as ACC_ADD, MTTS_VOC_ACC_INIT as ACC_INIT, MTTS_VOC_ACC_MEAN as ACC_MEAN,
                         MTTS_VOC_ACC_NONE as ACC_NONE, MTTS_VOC_MAX_TAPS as MAX_TAPS, VocConvArgs)


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight [N, cin, k] -> [N, k*cin] (tap-major, channel-minor)."""
    return w.detach().float().permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def pack_post(w: torch.Tensor) -> torch.Tensor:
    """conv_post weight [1, C, 7] -> [7*C]."""
    return pack_conv(w).reshape(-1)


def pack_upsample(w: torch.Tensor, u: int) -> torch.Tensor:
    """ConvTranspose1d weight [cin, cout, 2u] -> the phase-packed [u*cout, 2*cin] of mtts_voc_upsample: output
    sample t*u + p is w[:, :, q+u] . x[t-1] + w[:, :, q] . x[t] for p < u/2 and w[:, :, q] . x[t] + w[:, :, q-u] . x[t+1]
    otherwise, q = p + u/2."""
    w = w.detach().float()
    rows = []
    for p in range(u):
        q = p + u // 2
        first, second = (w[:, :, q + u], w[:, :, q]) if p < u // 2 else (w[:, :, q], w[:, :, q - u])
        rows.append(torch.cat([first.t(), second.t()], dim=1))
    return torch.cat(rows, dim=0).contiguous()


def conv_raw(a: torch.Tensor, wp: torch.Tensor, bias, B: int, L: int, k: int, d: int, *, leaky=False, slope=0.1,
             residual=None, out=None, acc=None, acc_mode=ACC_NONE, acc_div=1.0) -> int:
    """mtts_voc_conv; returns the status (0 or a negative mtts_status)."""
    N.require_device(a, wp, bias, residual, out, acc)
    args = VocConvArgs(N.ptr(a), N.ptr(wp), N.ptr(bias), N.ptr(residual), N.ptr(out), N.ptr(acc), B, L,
                       a.shape[-1], wp.shape[0], k, d, int(bool(leaky)), float(slope), acc_mode, float(acc_div))
    return N.lib().mtts_voc_conv(ctypes.byref(args), N.stream_handle(a.device))


def conv(a, wp, bias, B, L, k, d, *, leaky=False, slope=0.1, residual=None, out=None, acc=None, acc_mode=ACC_NONE,
         acc_div=1.0, want_out=True):
    """Dilated "same" Conv1d on token-major ``a`` [B*L, cin] with the packed weight ``wp`` [N, k*cin].  Returns the
    output [B*L, N] (``out`` if given; None with ``want_out=False``, when only ``acc`` is wanted).  ``out`` may be
    ``residual``; neither ``out`` nor ``acc`` may be ``a``."""
    if out is None and want_out:
        out = torch.empty(B * L, wp.shape[0], device=a.device, dtype=torch.float32)
    N.check(conv_raw(a, wp, bias, B, L, k, d, leaky=leaky, slope=slope, residual=residual, out=out, acc=acc,
                     acc_mode=acc_mode, acc_div=acc_div), "mtts_voc_conv")
    return out


def upsample_raw(a, wp, bias, out, B, L, cin, cout, k, u, slope=0.1) -> int:
    N.require_device(a, wp, bias, out)
    return N.lib().mtts_voc_upsample(N.ptr(a), N.ptr(wp), N.ptr(bias), N.ptr(out), B, L, cin, cout, k, u, float(slope),
                                     N.stream_handle(a.device))


def upsample(a, wp, bias, B, L, k, u, slope=0.1):
    """leaky_relu + ConvTranspose1d(k = 2u, stride u): token-major [B*L, cin] -> [B*L*u, cout]."""
    cin, cout = a.shape[-1], wp.shape[0] // max(u, 1)
    out = torch.empty(B * L * u, cout, device=a.device, dtype=torch.float32)
    N.check(upsample_raw(a, wp, bias, out, B, L, cin, cout, k, u, slope), "mtts_voc_upsample")
    return out


def pre(mel, wp, bias):
    """conv_pre on the channel-major mel [B, n_mels, T] -> token-major [B*T, N]."""
    N.require_device(mel, wp, bias)
    B, cin, T = mel.shape
    lib = N.lib()
    nbytes = lib.mtts_voc_pre_workspace_size(B, T, cin)
    ws = torch.empty(max(nbytes // 4, 1), device=mel.device, dtype=torch.float32)
    out = torch.empty(B * T, wp.shape[0], device=mel.device, dtype=torch.float32)
    N.check(lib.mtts_voc_pre(N.ptr(mel), N.ptr(wp), N.ptr(bias), N.ptr(out), B, T, cin, wp.shape[0], N.ptr(ws),
                             ws.numel() * 4, N.stream_handle(mel.device)), "mtts_voc_pre")
    return out


def post(a, w, bias, B, L, slope=0.01):
    """leaky_relu(slope) + Conv1d(C, 1, 7) + tanh: token-major [B*L, C] -> [B, 1, L]."""
    N.require_device(a, w, bias)
    out = torch.empty(B, 1, L, device=a.device, dtype=torch.float32)
    N.check(N.lib().mtts_voc_post(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(out), B, L, a.shape[-1], float(slope),
                                  N.stream_handle(a.device)), "mtts_voc_post")
    return out
