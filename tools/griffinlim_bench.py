"""Times mel -> waveform by Griffin-Lim on the MI355X: the graph replay of GriffinLimVocoder (HIP kernels of
include/mtts_griffinlim.h) beside the same algorithm from torch's own device ops (torch.stft / torch.istft), in
one process on one machine.

    python tools/griffinlim_bench.py [--iters 32] [--frames 600] [--batches 1 8] [--reps 30] [--rounds 7]

Per batch size: both paths are warmed up, then timed in alternating rounds of `reps` calls each (host clock around
work that ends in a device synchronise); the median over rounds and the min .. max spread are reported in
milliseconds per call, with the ratio of the medians, the largest waveform difference between the two paths on the
same initial phase, and the HIP path's launches per call.  Prints one JSON line per batch size."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matcha-tts-etu-upmc-ensam_amd"))

import torch  # noqa: E402

from matcha.utils.audio_process import GriffinLimVocoder, slaney_mel_basis  # noqa: E402


class TorchOpsGriffinLim:
    """exp, pinv product, relu and the Griffin-Lim loop on torch.stft / torch.istft, all on the device."""

    def __init__(self, device, n_iter, momentum=0.99):
        basis = slaney_mel_basis(22050, 1024, 80, 0.0, 8000.0).double()
        self.pinv = torch.linalg.pinv(basis).float().to(device)
        self.window = torch.hann_window(1024, device=device)
        self.n_iter, self.m = n_iter, momentum / (1 + momentum)

    def _istft(self, X):
        return torch.istft(X, 1024, hop_length=256, win_length=1024, window=self.window, center=True)

    def _stft(self, x):
        return torch.stft(x, 1024, hop_length=256, win_length=1024, window=self.window, center=True,
                          pad_mode="reflect", return_complex=True)

    @torch.no_grad()
    def __call__(self, log_mel, angles):
        lin = torch.relu(self.pinv @ torch.exp(log_mel))
        ang, tprev = angles, torch.zeros_like(angles)
        for _ in range(self.n_iter):
            reb = self._stft(self._istft(lin * ang))
            ang = reb - tprev * self.m
            ang = ang / (ang.abs() + 1e-16)
            tprev = reb
        return self._istft(lin * ang)


def _time(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("griffinlim_bench needs the GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        T = args.frames
        # a speech-like log-mel: a slowly moving harmonic comb over a decaying spectral envelope
        t = torch.arange(T)[None, None] / 40.0
        k = torch.arange(80)[None, :, None]
        log_mel = (-2.0 - 0.05 * k + 2.0 * torch.sin(0.6 * k + t + torch.rand(B, 1, 1, generator=g) * 6.28)
                   + 0.3 * torch.randn(B, 80, T, generator=g)).clamp(min=math.log(1e-5)).to(dev)
        angles = torch.view_as_complex(torch.rand(B, 513, T, 2, generator=g)).to(dev)
        hip = GriffinLimVocoder(n_iter=args.iters)
        ops = TorchOpsGriffinLim(dev, args.iters)
        run_hip = lambda: hip(log_mel, angles=angles)  # noqa: E731
        run_ops = lambda: ops(log_mel, angles)  # noqa: E731
        a, b = run_hip()[:, 0, :(T - 1) * 256], run_ops()
        diff = float((a - b).abs().max() / b.abs().max())
        for fn in (run_hip, run_ops):
            _time(fn, 5)
        th, to = [], []
        for _ in range(args.rounds):
            th.append(_time(run_hip, args.reps))
            to.append(_time(run_ops, args.reps))
        med_h, med_o = statistics.median(th), statistics.median(to)
        print(json.dumps({
            "B": B, "T": T, "n_iter": args.iters,
            "hip_graph_ms": round(med_h, 4), "hip_graph_ms_min_max": [round(min(th), 4), round(max(th), 4)],
            "torch_ops_ms": round(med_o, 4), "torch_ops_ms_min_max": [round(min(to), 4), round(max(to), 4)],
            "torch_ops_over_hip": round(med_o / med_h, 2),
            "hip_launches_per_call": 2 * args.iters + 3,
            "max_rel_diff_between_paths": diff,
            "reps_per_round": args.reps, "rounds": args.rounds,
        }), flush=True)


if __name__ == "__main__":
    main()
