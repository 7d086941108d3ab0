"""Times the Trainer's step on random mel segments (TrainConfig.out_size) at the long-form shape, three ways:
whole utterances (out_size=None, captured), the device crop (out_size=S, captured) and the reference's host-side
crop (out_size=S with MTTS_SEGMENT_HOST=1, eager: its device->host copy cannot be captured).

Each variant is warmed at its shape, then the variants alternate in blocks of --block steps inside one process
until each has --steps samples; every step is bracketed by HIP events and each block ends on a device sync.
Prints one JSON line per repeat with the medians (ms) and quartiles; run it with --repeats 2 for the spread.
Needs the GPU.  Usage: python tools/segment_step.py [--batch 8 --tx 512 --ty 4096 --out-size 512]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "matcha-tts-etu-upmc-ensam_amd"), str(ROOT)]
from matcha.models.matcha_tts import MatchaTTS  # noqa: E402
from matcha.training import TrainConfig, Trainer, synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--tx", type=int, default=512)
ap.add_argument("--ty", type=int, default=4096)
ap.add_argument("--out-size", type=int, default=512)
ap.add_argument("--precision", default="bf16-parity")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--block", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=2)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("segment_step.py needs the GPU")
dev = torch.device("cuda:0")
batch = synthetic_batch(args.batch, args.tx, args.ty, device=dev)


def make(out_size, graph):
    torch.manual_seed(0)
    model = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(dev)
    return Trainer(model, TrainConfig(precision=args.precision, graph=graph, out_size=out_size))


# name -> (trainer, MTTS_SEGMENT_HOST)
variants = {"whole_graph": (make(None, True), None), "segment_device_graph": (make(args.out_size, True), None),
            "segment_host_eager": (make(args.out_size, False), "1")}


def run(name, n, times=None):
    tr, host = variants[name]
    if host is not None:
        os.environ["MTTS_SEGMENT_HOST"] = host
    try:
        evs = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.step([batch])
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
    finally:
        os.environ.pop("MTTS_SEGMENT_HOST", None)
    if times is not None:
        times.extend(a.elapsed_time(b) for a, b in evs)


for name in variants:
    run(name, args.warmup)
for rep in range(args.repeats):
    times = {name: [] for name in variants}
    while len(times["whole_graph"]) < args.steps:
        for name in variants:
            run(name, args.block, times[name])
    out = {"repeat": rep, "shape": f"{args.batch}x{args.tx}x{args.ty}", "out_size": args.out_size,
           "precision": args.precision, "steps": len(times["whole_graph"])}
    for name, t in times.items():
        q = statistics.quantiles(t, n=4)
        out[name] = {"median_ms": round(statistics.median(t), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3)}
    print(json.dumps(out), flush=True)
