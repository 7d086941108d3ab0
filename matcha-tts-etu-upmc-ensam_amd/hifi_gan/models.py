"""HiFi-GAN ``Generator`` (reference hifi_gan/models.py:11-125), inference on the HIP kernels of
include/mtts_vocoder.h.

The parameters live in ``weight_norm``-wrapped Conv1d / ConvTranspose1d modules with the reference's names, so
``load_state_dict(torch.load(path)["generator"])`` takes a published checkpoint; the modules' own forwards are
never called.  ``forward`` folds the weight norm (w = g v / ||v||, dim 0), packs the weights for the kernels once
(again whenever a parameter changes) and runs token-major [B*L, C] fp32 from conv_pre to conv_post: one launch
per resblock conv, two per transposed conv and for conv_pre, one for conv_post and nothing else -- the leaky ReLUs,
the residual adds, the sum over a stage's resblocks and its division ride in the conv kernel's operand load and
epilogue."""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.nn.utils import remove_weight_norm, weight_norm

from matcha import _graphs as G
from matcha import _native as N

from . import ops as V

LRELU_SLOPE = 0.1  # models.py:8
# models.py:112 calls F.leaky_relu(x) before conv_post WITHOUT a slope: torch's default 0.01, not LRELU_SLOPE.
# Published checkpoints were trained with it, so it is kept.
POST_SLOPE = 0.01
N_MELS = 80  # models.py:81


def _padding(k: int, d: int = 1) -> int:
    return (k * d - d) // 2


def _wn_conv(cin, cout, k, d):
    return weight_norm(nn.Conv1d(cin, cout, k, 1, dilation=d, padding=_padding(k, d)))


class ResBlock1(nn.Module):
    """models.py:11-48: three (dilated conv, conv) pairs, each with a residual."""

    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        self.convs1 = nn.ModuleList([_wn_conv(channels, channels, kernel_size, d) for d in dilation])
        self.convs2 = nn.ModuleList([_wn_conv(channels, channels, kernel_size, 1) for _ in dilation])

    def pairs(self):
        return [(c1, c2) for c1, c2 in zip(self.convs1, self.convs2)]


class ResBlock2(nn.Module):
    """models.py:51-72: dilated convs, each with a residual."""

    def __init__(self, channels, kernel_size=3, dilation=(1, 3)):
        super().__init__()
        self.convs = nn.ModuleList([_wn_conv(channels, channels, kernel_size, d) for d in dilation])

    def pairs(self):
        return [(c,) for c in self.convs]


def _validate(h):
    rates, ks = list(h.upsample_rates), list(h.upsample_kernel_sizes)
    if len(rates) != len(ks) or not rates:
        raise ValueError("upsample_rates and upsample_kernel_sizes must be non-empty lists of one length")
    if len(h.resblock_kernel_sizes) != len(h.resblock_dilation_sizes) or not len(h.resblock_kernel_sizes):
        raise ValueError("resblock_kernel_sizes and resblock_dilation_sizes must be non-empty lists of one length")
    for u, k in zip(rates, ks):
        if k != 2 * u or u % 2 or u < 2:
            raise ValueError(f"upsample kernel {k} / rate {u}: the HIP transposed conv needs k == 2 * rate, rate even")
    for k in h.resblock_kernel_sizes:
        if k % 2 == 0 or k > V.MAX_TAPS or k < 1:
            raise ValueError(f"resblock kernel size {k}: the HIP conv takes odd sizes up to {V.MAX_TAPS}")
    for ds in h.resblock_dilation_sizes:
        if any(d < 1 for d in ds):
            raise ValueError(f"resblock dilations {ds}: must be >= 1")
    c0 = h.upsample_initial_channel
    for i in range(len(rates) + 1):
        if c0 % (2 ** i) or (c0 // 2 ** i) % 8:
            raise ValueError(f"upsample_initial_channel {c0} / 2^{i} is not a multiple of 8 channels")


class Generator(nn.Module):
    """``Generator(h)(mel [B, 80, T]) -> wav [B, 1, T * prod(h.upsample_rates)]``, inference only.

    An unsupported config (an even or > 11 resblock kernel, an upsample kernel != 2 * rate, a channel count that
    is no multiple of 8) raises ValueError here, not at the first launch."""

    # the whole forward of one (B, T) is captured once into a HIP graph and replayed; bounded cache
    # (matcha/_graphs.py), a fresh one whenever the weights are repacked
    graph: bool = True
    _GRAPH_CACHE_MAX = 8

    def __init__(self, h):
        super().__init__()
        _validate(h)
        self.h = h
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        c0 = h.upsample_initial_channel
        self.conv_pre = weight_norm(nn.Conv1d(N_MELS, c0, 7, 1, padding=3))
        block = ResBlock1 if h.resblock == "1" else ResBlock2
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            self.ups.append(weight_norm(nn.ConvTranspose1d(c0 // 2 ** i, c0 // 2 ** (i + 1), k, u,
                                                           padding=(k - u) // 2)))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            ch = c0 // 2 ** (i + 1)
            for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
                self.resblocks.append(block(ch, k, tuple(d)))
        self.conv_post = weight_norm(nn.Conv1d(ch, 1, 7, 1, padding=3))
        for m in list(self.ups) + [self.conv_post]:  # models.py:97-98 (init_weights)
            m.weight_v.data.normal_(0.0, 0.01)
        self.hop = math.prod(h.upsample_rates)  # samples per mel frame

    # ---- parameters -----------------------------------------------------------------------------------------
    def _conv_modules(self):
        mods = [("conv_pre", self.conv_pre)]
        mods += [(f"ups.{i}", m) for i, m in enumerate(self.ups)]
        for i, rb in enumerate(self.resblocks):
            for name, lst in rb.named_children():
                mods += [(f"resblocks.{i}.{name}.{j}", m) for j, m in enumerate(lst)]
        return mods + [("conv_post", self.conv_post)]

    def remove_weight_norm(self):
        """models.py:118-125: replaces every (weight_g, weight_v) by the folded weight."""
        for _, m in self._conv_modules():
            if hasattr(m, "weight_g"):
                remove_weight_norm(m)
        return self

    @staticmethod
    def _folded(m) -> torch.Tensor:
        if hasattr(m, "weight_g"):  # what remove_weight_norm computes: g * v / ||v|| over dim 0's slices
            return torch._weight_norm(m.weight_v.detach(), m.weight_g.detach(), 0)
        return m.weight.detach()

    def folded_weights(self) -> dict:
        """name -> folded weight of every conv (``remove_weight_norm`` need not have been called)."""
        return {name + ".weight": self._folded(m) for name, m in self._conv_modules()}

    def load_state_dict(self, state_dict, *args, **kwargs):
        """Also takes a checkpoint saved after ``remove_weight_norm`` (plain ``*.weight`` keys)."""
        if "conv_pre.weight" in state_dict and "conv_pre.weight_g" not in state_dict:
            self.remove_weight_norm()
        return super().load_state_dict(state_dict, *args, **kwargs)

    # ---- packed weights -------------------------------------------------------------------------------------
    def _packed(self):
        stamp = tuple((p.data_ptr(), p._version) for p in self.parameters())
        pk = self.__dict__.get("_pack")
        if pk is not None and pk["stamp"] == stamp:
            return pk
        f32 = lambda t: None if t is None else t.detach().float().contiguous()  # noqa: E731
        pk = {"stamp": stamp}
        pk["pre"] = (V.pack_conv(self._folded(self.conv_pre)), f32(self.conv_pre.bias))
        pk["ups"] = [(V.pack_upsample(self._folded(m), m.stride[0]), f32(m.bias), m.kernel_size[0], m.stride[0])
                     for m in self.ups]
        pk["res"] = [[[(V.pack_conv(self._folded(c)), f32(c.bias), c.kernel_size[0], c.dilation[0]) for c in pair]
                      for pair in rb.pairs()] for rb in self.resblocks]
        pk["post"] = (V.pack_post(self._folded(self.conv_post)), f32(self.conv_post.bias))
        self.__dict__["_pack"] = pk
        self.__dict__["_graphs"] = G.GraphCache(self._GRAPH_CACHE_MAX)  # captured graphs hold the old buffers
        return pk

    # ---- forward --------------------------------------------------------------------------------------------
    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        N.require_device(mel, self.conv_pre.bias)
        if torch.is_grad_enabled() and mel.requires_grad:
            raise RuntimeError("hifi_gan.Generator is inference only: the mel requires a gradient "
                               "(call it under torch.no_grad() / on a detached mel)")
        if mel.dim() != 3 or mel.shape[1] != N_MELS:
            raise ValueError(f"mel must be [B, {N_MELS}, T], got {tuple(mel.shape)}")
        with torch.no_grad():
            mel = mel.detach().float().contiguous()
            pk = self._packed()
            if self.graph and not torch.cuda.is_current_stream_capturing():
                return self._forward_graph(mel, pk)
            return self._forward_eager(mel, pk)

    def _forward_graph(self, mel, pk):
        def build():
            with torch.inference_mode(False):  # a later call outside inference mode still copies into it
                smel = torch.empty(mel.shape, device=mel.device, dtype=torch.float32)
            smel.copy_(mel)
            return smel, *G.capture(lambda: self._forward_eager(smel, pk), mel.device)

        smel, g, out = self._graphs.lookup((tuple(mel.shape), mel.device), build)
        smel.copy_(mel)
        g.replay()
        return out.clone()

    def _forward_eager(self, mel, pk):
        B, _, L = mel.shape
        if B == 0 or L == 0:
            return torch.zeros(B, 1, L * self.hop, device=mel.device, dtype=torch.float32)
        x = V.pre(mel, *pk["pre"])  # models.py:101
        nk = self.num_kernels
        for i, (wp, bias, k, u) in enumerate(pk["ups"]):
            x = V.upsample(x, wp, bias, B, L, k, u, LRELU_SLOPE)  # models.py:103-104
            L *= u
            acc = torch.empty_like(x)
            tmp, h0, h1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            for j in range(nk):  # models.py:105-111: xs = sum of the resblocks, then / num_kernels
                pairs = pk["res"][i * nk + j]
                mode = V.ACC_INIT if j == 0 else V.ACC_MEAN if j == nk - 1 else V.ACC_ADD
                if nk == 1:
                    mode = V.ACC_INIT  # xs / 1
                h, spare = x, h0  # x itself is shared by the stage's resblocks and never written
                for m, pair in enumerate(pairs):
                    last = m == len(pairs) - 1
                    a = h
                    if len(pair) == 2:  # ResBlock1 (models.py:36-41): xt = c1(lrelu(x)); xt = c2(lrelu(xt)); x = xt + x
                        w1, b1, k1, d1 = pair[0]
                        a = V.conv(h, w1, b1, B, L, k1, d1, leaky=True, slope=LRELU_SLOPE, out=tmp)
                    w2, b2, k2, d2 = pair[-1]  # ResBlock2 (models.py:64-67): x = c(lrelu(x)) + x
                    # the output may be the residual's own buffer, never the conv's input
                    dst = spare if (h is x or a is h) else h
                    V.conv(a, w2, b2, B, L, k2, d2, leaky=True, slope=LRELU_SLOPE, residual=h,
                           out=None if last else dst, want_out=not last,
                           acc=acc if last else None, acc_mode=mode if last else V.ACC_NONE, acc_div=float(nk))
                    if a is h and not last:  # ResBlock2 ping-pongs between the two spare buffers
                        spare = h1 if dst is h0 else h0
                    h = dst
            x = acc
        return V.post(x, *pk["post"], B, L, POST_SLOPE)  # models.py:112-114
