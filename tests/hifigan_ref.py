"""A plain-torch restatement of the reference HiFi-GAN generator (hifi_gan/models.py:11-125), written for the
tests: the float64 / fp32 CPU reference of the whole generator and, on the GPU, the torch conv1d /
conv_transpose1d composition tools/vocoder_bench.py times against.  Same module tree and parameter names as the
reference (weight_norm'd convs), so the name-keyed weight recipe and a published state dict apply unchanged.
Test infrastructure only; the product is hifi_gan/models.py on the HIP kernels."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import weight_norm

LRELU_SLOPE = 0.1  # models.py:8


def _conv(ch, k, d):  # models.py:16-17 with get_padding (utils.py:34-35)
    return weight_norm(nn.Conv1d(ch, ch, k, 1, dilation=d, padding=(k * d - d) // 2))


class RefResBlock1(nn.Module):  # models.py:11-42
    def __init__(self, ch, k, dilation):
        super().__init__()
        self.convs1 = nn.ModuleList([_conv(ch, k, d) for d in dilation])
        self.convs2 = nn.ModuleList([_conv(ch, k, 1) for _ in dilation])

    def forward(self, x):
        for c1, c2 in zip(self.convs1, self.convs2):
            xt = c2(F.leaky_relu(c1(F.leaky_relu(x, LRELU_SLOPE)), LRELU_SLOPE))
            x = xt + x
        return x


class RefResBlock2(nn.Module):  # models.py:51-68
    def __init__(self, ch, k, dilation):
        super().__init__()
        self.convs = nn.ModuleList([_conv(ch, k, d) for d in dilation])

    def forward(self, x):
        for c in self.convs:
            x = c(F.leaky_relu(x, LRELU_SLOPE)) + x
        return x


class RefGenerator(nn.Module):  # models.py:75-116
    def __init__(self, h):
        super().__init__()
        self.num_kernels, c0 = len(h.resblock_kernel_sizes), h.upsample_initial_channel
        self.conv_pre = weight_norm(nn.Conv1d(80, c0, 7, 1, padding=3))
        block = RefResBlock1 if h.resblock == "1" else RefResBlock2
        self.ups = nn.ModuleList(
            weight_norm(nn.ConvTranspose1d(c0 // 2 ** i, c0 // 2 ** (i + 1), k, u, padding=(k - u) // 2))
            for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            ch = c0 // 2 ** (i + 1)
            for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
                self.resblocks.append(block(ch, k, d))
        self.conv_post = weight_norm(nn.Conv1d(ch, 1, 7, 1, padding=3))

    def forward(self, x):
        x = self.conv_pre(x)
        for i, up in enumerate(self.ups):
            x = up(F.leaky_relu(x, LRELU_SLOPE))
            xs = None
            for j in range(self.num_kernels):  # models.py:105-111: in-place sum, then a division
                r = self.resblocks[i * self.num_kernels + j](x)
                xs = r if xs is None else xs.add_(r)
            x = xs / self.num_kernels
        return torch.tanh(self.conv_post(F.leaky_relu(x)))  # models.py:112: torch's default slope 0.01


CONFIGS = {  # the fixture's two cases (tests/golden/_hifigan_golden.py)
    "v1_small": dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4],
                     upsample_initial_channel=128, resblock_kernel_sizes=[3, 7, 11],
                     resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]]),
    "v3_small": dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8],
                     upsample_initial_channel=64, resblock_kernel_sizes=[3, 5, 7],
                     resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]]),
}
V1 = dict(CONFIGS["v1_small"], upsample_initial_channel=512)  # the published V1 size (tools/vocoder_bench.py)
