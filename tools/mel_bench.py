"""Times waveform batch -> padded log-mel batch on the MI355X: MelSpectrogram.batch (one launch of mtts_mel_from_wav
on the int16 batch) beside the two ways the rocFFT path (MelSpectrogram.__call__) gets the same tensors, in one process
on one machine:

    loop   one __call__ per utterance on its own waveform, copied into a zeroed [B, 80, F] batch: correct, many launches
    dense  one __call__ on the padded batch: the fewest launches, but wrong in every shorter utterance's last frames
           and non-zero after them

    python tools/mel_bench.py [--batches 1 32] [--seconds 7.0] [--reps 500] [--rounds 7]
    python tools/mel_bench.py --only fused|loop|dense --batches 32 --calls 20     (for a kernel trace: no timing)

Both rocFFT paths are handed fp32 waveforms already on the device (the int16 -> fp32 conversion they need is not
charged to them).  Utterance lengths are ragged: uniform in [0.5, 1] of `seconds`, the longest exactly `seconds`.  Per
batch size the three paths are warmed up, then timed in alternating rounds of `reps` calls each (host clock around
work that ends in a device synchronise); the median over rounds and the min .. max spread are reported in
milliseconds per call, with the ratios of the medians and the largest log-mel difference between `batch` and `loop`
on the valid frames (and between `dense` and `loop`, which shows what `dense` gets wrong).  One JSON line per batch size."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matcha-tts-etu-upmc-ensam_amd"))

import torch  # noqa: E402

from matcha.utils.audio_process import MelSpectrogram  # noqa: E402

CFG = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000)


def _time(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _case(B, seconds, dev):
    g = torch.Generator().manual_seed(B)
    longest = int(seconds * 22050)
    L = -(-longest // 256) * 256
    lengths = (longest * (0.5 + 0.5 * torch.rand(B, generator=g))).long()
    lengths[0] = longest
    # speech-like level: a few decaying harmonics plus noise, zero past each utterance's end
    t = torch.arange(L)[None] / 22050.0
    f0 = 90.0 + 120.0 * torch.rand(B, 1, generator=g)
    x = sum(0.25 / h * torch.sin(2 * torch.pi * h * f0 * t) for h in range(1, 6)) + 0.02 * torch.randn(B, L, generator=g)
    x = x * (torch.arange(L)[None] < lengths[:, None])
    pcm = (x.clamp(-1, 1) * 32767).round().to(torch.int16)
    return pcm.to(dev), lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--seconds", type=float, default=7.0)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["fused", "loop", "dense"], default=None)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mel_bench needs the GPU: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    mel = MelSpectrogram(**CFG)
    for B in args.batches:
        pcm, lengths = _case(B, args.seconds, dev)
        lens = lengths.tolist()
        lengths_dev = lengths.to(dev, torch.int32)
        y32 = pcm.to(torch.float32) / 32768.0
        F = pcm.shape[1] // 256

        def fused():
            return mel.batch(pcm, lengths_dev)

        def loop():
            out = torch.zeros(B, 80, F, dtype=torch.float32, device=dev)
            for b, n in enumerate(lens):
                out[b, :, :n // 256] = mel(y32[b:b + 1, :n])[0]
            return out

        def dense():
            return mel(y32)

        paths = {"fused": fused, "loop": loop, "dense": dense}
        if args.only:
            for _ in range(args.calls):
                paths[args.only]()
            torch.cuda.synchronize()
            print(json.dumps({"B": B, "only": args.only, "calls": args.calls}), flush=True)
            continue
        a, a_len = fused()
        ref, wrong = loop(), dense()
        valid = torch.arange(F, device=dev)[None, None] < a_len[:, None, None]
        assert a_len.tolist() == [n // 256 for n in lens]
        diff = float(((a - ref).abs() * valid).max())
        diff_dense = float(((wrong[:, :, :F] - ref).abs() * valid).max())
        for fn in paths.values():
            _time(fn, 3)
        times = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                times[k].append(_time(fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({
            "B": B, "L": pcm.shape[1], "frames": F, "valid_frames": int(a_len.sum()),
            **{f"{k}_ms": round(med[k], 4) for k in paths},
            **{f"{k}_ms_min_max": [round(min(times[k]), 4), round(max(times[k]), 4)] for k in paths},
            "loop_over_fused": round(med["loop"] / med["fused"], 2),
            "dense_over_fused": round(med["dense"] / med["fused"], 2),
            "max_abs_diff_fused_vs_loop_valid": diff,
            "max_abs_diff_dense_vs_loop_valid": diff_dense,
            "padding_all_zero_fused": bool(((a * ~valid) == 0).all()),
            "reps_per_round": args.reps, "rounds": args.rounds,
        }), flush=True)


if __name__ == "__main__":
    main()
