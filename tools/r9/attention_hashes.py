"""SHA-256 of the raw bytes of o, lse and d(q|k|v) of the attention kernels at the shapes that reach each edge of
csrc/attention.hip (a block of one row, dh < D, T = 1, both storages, dropout, the short path and its threshold).

    python tools/r9/attention_hashes.py [--out tests/golden/attention_r9_hashes.json]

tests/golden/attention_r9_hashes.json was written by this script on the build of 8b22a1e, the parent of the
round-9 prologue / epilogue change; tests/test_attention_edges_gpu.py recomputes the hashes and compares, so the
kernels stay bitwise what they were.  Inputs come from a seeded CPU generator and a 0/1 key mask like
tests/test_attention_gpu.py's _case."""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(ROOT / "matcha-tts-etu-upmc-ensam_amd")]

import torch  # noqa: E402

# (B, T, H, D, storage, precision, dropout, MTTS_ATTN_SHORT)
CASES = [
    # long path
    (2, 129, 2, 64, "bf16", "bf16", 0.0, None),  # the second block holds one row
    (2, 300, 2, 64, "bf16", "bf16", 0.0, None),
    (1, 130, 1, 40, "fp32", "bf16", 0.0, None),  # dh < D, partial chunk
    (2, 77, 2, 16, "fp32", "fp32", 0.0, "0"),
    (1, 200, 2, 96, "fp32", "fp32", 0.1, None),
    # short path
    (3, 33, 2, 96, "fp32", "fp32", 0.1, None),
    (2, 120, 2, 96, "fp32", "fp32", 0.0, None),
    (2, 128, 2, 96, "fp32", "bf16", 0.0, None),
    (1, 1, 1, 64, "fp32", "fp32", 0.0, None),
    (2, 96, 1, 64, "bf16", "bf16", 0.0, None),
]


def case_id(c):
    B, T, H, D, st, pr, p, short = c
    return f"B{B}-T{T}-H{H}-D{D}-{st}-{pr}-p{p}" + ("" if short is None else f"-short{short}")


def make_inputs(c, dev):
    """q|k|v [B, T, 3 H D], the 0/1 key mask [B, T] (batch 0 full) and dO [B, T, H D] in the case's storage."""
    B, T, H, D, st, _, _, _ = c
    g = torch.Generator(device="cpu").manual_seed(9000 + 131 * B + 7 * T + D)
    qkv = torch.randn(B, T, 3 * H * D, generator=g) * 1.5
    lengths = torch.randint(max(1, T // 2), T + 1, (B,), generator=g)
    lengths[0] = T
    bias = (torch.arange(T)[None, :] < lengths[:, None]).float()
    dout = torch.randn(B, T, H * D, generator=g)
    dt = torch.bfloat16 if st == "bf16" else torch.float32
    return qkv.to(dt).to(dev), bias.to(dev), dout.to(dt).to(dev)


def run_case(c, qkv, bias, dout, o=None, dqkv_like=None):
    """One forward and backward call -> (o, lse, dqkv).  `o`: the output tensor to fill (a view is allowed)."""
    from matcha.models.components import _ops as O

    B, T, H, D, st, pr, p, short = c
    prec = O.PREC_BF16 if pr == "bf16" else O.PREC_FP32
    seed = torch.tensor([1234, 99], dtype=torch.int32, device=qkv.device) if p > 0 else None
    old = os.environ.get("MTTS_ATTN_SHORT")
    if short is not None:
        os.environ["MTTS_ATTN_SHORT"] = short
    try:
        if o is None:
            o = torch.empty(B, T, H * D, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, H, T, device=qkv.device)
        O._attn_fwd(qkv, bias, o, lse, H, prec, dropout_p=p, seed=seed)
        dqkv = O._attn_bwd(dout, qkv, bias, o, lse, H, prec, dropout_p=p, seed=seed)
        torch.cuda.synchronize()
    finally:
        if short is not None:
            if old is None:
                del os.environ["MTTS_ATTN_SHORT"]
            else:
                os.environ["MTTS_ATTN_SHORT"] = old
    return o, lse, dqkv


def sha(t):
    t = t.contiguous().cpu()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def hashes(c, dev):
    o, lse, dqkv = run_case(c, *make_inputs(c, dev))
    return {"o": sha(o), "lse": sha(lse), "dqkv": sha(dqkv)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {case_id(c): hashes(c, dev) for c in CASES}
    text = json.dumps(res, indent=1, sort_keys=True) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
