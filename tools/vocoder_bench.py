"""Times the HiFi-GAN generator (hifi_gan.Generator on the HIP kernels) at the published V1 size against the same
module run through torch's own conv1d / conv_transpose1d on the GPU (tests/hifigan_ref.py, weight norm folded).

    python tools/vocoder_bench.py [--batches 1 8] [--frames 600] [--rounds 5] [--per-round 10] [--out FILE]

Per batch size: HIP events around single calls after a warm-up, the two implementations alternating in rounds in
one process, the median over rounds x per-round calls (50 by default).  Ours is a HIP-graph replay (what a user's
call does); torch runs eagerly, launch by launch, which is how that module runs for a user.  Reported: ms per call,
the real-time factor at 22,050 Hz (compute time / audio time; smaller is faster), and the share of the 157.3 TF
fp32-MFMA peak the whole call achieves from an algorithmic FLOP count (a whole-program rate, not a kernel's).
Needs the GPU: there is no fallback.  One JSON line per batch size."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "matcha-tts-etu-upmc-ensam_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

PEAK_F32_MFMA = 157.3e12
SR = 22050


def flops(cfg, B, T):
    """Multiply-adds x 2 of every conv of the generator (models.py:100-116), from the layer shapes."""
    c = cfg["upsample_initial_channel"]
    L = T
    total = 2 * B * L * 80 * c * 7
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        total += 2 * B * (L * u) * c * (c // 2) * (k // u)  # k / u taps reach each output sample
        L, c = L * u, c // 2
        per_block = 2 if cfg["resblock"] == "1" else 1
        for rk, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            total += 2 * B * L * c * c * rk * len(ds) * per_block
    return total + 2 * B * L * c * 7


def time_calls(fn, n):
    import torch

    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=10)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import torch

    from golden.weights_recipe import apply_recipe
    from hifi_gan import AttrDict, Generator
    from hifigan_ref import V1, RefGenerator

    if not torch.cuda.is_available():
        raise SystemExit("vocoder_bench needs the MI355X")
    dev = torch.device("cuda:0")
    ours = Generator(AttrDict(V1))
    apply_recipe(ours, 1)
    ours = ours.to(dev).eval()
    ref = None
    if not args.skip_torch:
        ref = RefGenerator(AttrDict(V1))
        apply_recipe(ref, 1)
        for m in ref.modules():
            if hasattr(m, "weight_g"):
                torch.nn.utils.remove_weight_norm(m)
        ref = ref.to(dev).eval()
    sink = open(args.out, "a") if args.out else None
    with torch.no_grad():
        for B in args.batches:
            mel = torch.randn(B, 80, args.frames, device=dev, generator=torch.Generator(dev).manual_seed(5)) * 1.5 - 5.5
            y = ours(mel)  # captures the graph
            for _ in range(3):
                ours(mel)
            res = {"B": B, "frames": args.frames, "samples": y.shape[-1], "gflop": flops(V1, B, args.frames) / 1e9}
            if ref is not None:
                for _ in range(3):
                    yr = ref(mel)
                res["max_abs_vs_torch"] = float((y - yr).abs().max())
            torch.cuda.synchronize()
            t_ours, t_ref = [], []
            for _ in range(args.rounds):
                t_ours += time_calls(lambda: ours(mel), args.per_round)
                if ref is not None:
                    t_ref += time_calls(lambda: ref(mel), args.per_round)
            audio_s = B * y.shape[-1] / SR
            for name, ts in (("hip", t_ours), ("torch", t_ref)):
                if ts:
                    ms = statistics.median(ts)
                    res[name + "_ms"] = round(ms, 3)
                    res[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
                    res[name + "_rtf"] = round(ms / 1e3 / audio_s, 5)
                    res[name + "_share_of_f32_mfma_peak"] = round(res["gflop"] * 1e9 / (ms / 1e3) / PEAK_F32_MFMA, 4)
            line = json.dumps(res)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()


if __name__ == "__main__":
    main()
