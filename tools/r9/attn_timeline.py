"""Per-wave phase timeline of the attention kernels (diagnostic build -DMTTS_ATTN_TIMELINE=1, see g_atl in
csrc/attention.hip):

    MTTS_BUILD_VARIANT=atl MTTS_EXTRA_HIPCC_FLAGS=-DMTTS_ATTN_TIMELINE=1 python build_native.py
    python tools/r9/attn_timeline.py [--out OUT.json]         (MTTS_LIB names another timeline build)

Runs one forward and one backward call at each attention shape of the flagship step (B = 32; decoder H = 2, D = 64,
T = 600 and 300 on bf16 storage; encoder H = 2, D = 96, T = 120 in fp32) and reads the 100 MHz stamps lane 0 of
every wave wrote: entry, fragment loads issued, first barrier passed, tile loop done, last store issued.  Prints,
per kernel role, the prologue (entry -> first barrier), loop and epilogue shares of the waves' lifetime."""
import argparse
import ctypes
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
os.environ.setdefault("MTTS_LIB", str(ROOT / "matcha-tts-etu-upmc-ensam_amd" / "lib" / "libmtts_hip_atl.so"))
sys.path[:0] = [str(ROOT / "matcha-tts-etu-upmc-ensam_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from matcha import _native as N  # noqa: E402
from matcha.models.components import _ops as O  # noqa: E402

SLOTS, WAVES = 8, 16384
KINDS = {1: "fwd", 2: "bwd dQ role", 3: "bwd dK/dV role", 4: "fwd short", 5: "bwd dQ short", 6: "bwd dK/dV short"}
SHAPES = [(32, 600, 2, 64, "bf16"), (32, 300, 2, 64, "bf16"), (32, 120, 2, 96, "fp32")]
TICK = 0.01  # us per 100 MHz tick


def read(fn):
    buf = np.zeros(WAVES * SLOTS, dtype=np.int64)
    assert fn(buf.ctypes.data) == buf.nbytes
    t = buf.reshape(WAVES, SLOTS)
    return t[t[:, 1] > 0]


def summarise(t):
    out = {}
    for kind, name in KINDS.items():
        w = t[t[:, 0] == kind]
        if not len(w):
            continue
        entry, frag, bar, loop, end = (w[:, i].astype(np.float64) for i in range(1, 6))
        life = (end - entry).sum()
        out[name] = {
            "waves": int(len(w)),
            "span_us": round(float((end.max() - entry.min()) * TICK), 2),
            "wave_life_us_mean": round(float((end - entry).mean() * TICK), 2),
            "fragment_issue_us_mean": round(float((frag - entry).mean() * TICK), 2),
            "prologue_us_mean": round(float((bar - entry).mean() * TICK), 2),
            "loop_us_mean": round(float((loop - bar).mean() * TICK), 2),
            "epilogue_us_mean": round(float((end - loop).mean() * TICK), 2),
            "prologue_share": round(float((bar - entry).sum() / life), 4),
            "loop_share": round(float((loop - bar).sum() / life), 4),
            "epilogue_share": round(float((end - loop).sum() / life), 4),
        }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fn = N.lib().mtts_attn_timeline_read
    fn.restype, fn.argtypes = ctypes.c_longlong, [ctypes.c_void_p]
    dev = torch.device("cuda:0")
    res = {"lib": Path(os.environ["MTTS_LIB"]).name}
    for B, T, H, D, mode in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(T + D)
        dt = torch.bfloat16 if mode == "bf16" else torch.float32
        prec = O.PREC_BF16 if mode == "bf16" else O.PREC_FP32
        C = H * D
        qkv = torch.randn(B, T, 3 * C, generator=g).to(dev).to(dt)
        do = torch.randn(B, T, C, generator=g).to(dev).to(dt)
        kb = torch.zeros(B, T, device=dev)
        for b in range(B):
            kb[b, : max(1, T - (T // 64) * b)] = 1
        o = torch.empty(B, T, C, device=dev, dtype=dt)
        lse = torch.empty(B, H, T, device=dev)
        for _ in range(3):
            O._attn_fwd(qkv, kb, o, lse, H, prec)
            O._attn_bwd(do, qkv, kb, o, lse, H, prec)
        torch.cuda.synchronize()
        key = f"B{B} T{T} H{H} D{D} {mode}"
        res[key] = {}
        for leg in ("fwd", "bwd"):
            assert fn(None) > 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if leg == "fwd":
                O._attn_fwd(qkv, kb, o, lse, H, prec)
            else:
                O._attn_bwd(do, qkv, kb, o, lse, H, prec)
            e1.record()
            torch.cuda.synchronize()
            s = summarise(read(fn))
            s["event_us"] = round(e0.elapsed_time(e1) * 1e3, 1)
            res[key][leg] = s
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
