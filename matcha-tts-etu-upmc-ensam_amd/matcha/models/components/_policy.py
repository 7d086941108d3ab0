"""The forward-precision policy: which arithmetic a forward GEMM (and the attention / LayerNorm beside it) runs
inside a bf16 autocast region.  Everything that decides it lives here; _ops reads it through ForwardPolicy's named
predicates only.

THE POLICY IS READ IN THE FORWARD ONLY.  An op captures `prec` at its forward, its dgrad operands are never split
(operand_kind returns `prec` for them) and the weight gradients take no policy, so backward() computes the same
wherever it is called -- inside a context, after it, or on autograd's device thread, where a context variable
holds its default.

  set_weight_split(True)  process-wide (bench.py and the tests call it outside any context): every bf16 forward
                          operand as two planes, hi = bf16(w) and lo = bf16(w - hi).  PackSpec.one_plane is NOT
                          honoured: the mode's error numbers mean "every weight split" 
  parity_policy()         the Trainer's "bf16-parity": split planes except where a spec says one_plane, and the
                          ambient text-encoder precision PARITY_ENCODER
  precise_forward(kind)   "bf16x3" (split W and split fp32 A, three MFMAs per product), "bf16x6" (three exact planes
                          per operand, six MFMAs) or "fp32" (fp32 packed weights on the exact-fp32 MFMA: 32-true's
                          forward, its outputs 32-true's); attention forward exact fp32, LayerNorm outputs fp32.
                          The text encoder runs under one of these (ENCODER_FORWARD): its activations' bf16
                          rounding decides the alignment's near-ties, and bf16x3 still flipped one (round 4)
"""
from __future__ import annotations

import contextlib
import contextvars
import dataclasses
import os

import torch

from matcha._abi import MTTS_PREC_BF16 as PREC_BF16, MTTS_PREC_FP32 as PREC_FP32

PACK_BF16_SPLIT = 2  # pack-cache kind: the bf16 hi + lo planes of a forward operand
PACK_BF16_SPLIT3 = 3  # pack-cache kind: hi + mid + lo bf16 planes (== w exactly) of a bf16x6 forward operand

# The parity policy's two constants, read once.
# MTTS_PARITY_FF1_SPLIT=1: the decoder FeedForward's GELU up-projection takes split planes too.  It keeps ONE plane by
# default: its share of the diffusion loss's weight-rounding error is ~3.5 % (tools/r3/weight_sensitivity.py) and its
# split planes cost the most of any GEMM (the GELU epilogue pins it to the register schedule).  Measured
# (profiles/r04/ff1_one_plane/): step 7.99 / 8.01 -> 7.85 / 7.86 ms; parity errors (prior, diff) B=4 vs the reference
# fixture 0 / 1.2e-5, B=32 0 / 3.4e-7, 512 x 4096 1.9e-7 / 3.3e-5, alignment exact in all three.  The down-projection
# (~3 % share) is always split under the policy (A/B last runnable at 3dd8270).
FF1_SPLIT = os.environ.get("MTTS_PARITY_FF1_SPLIT", "0") != "0"
# MTTS_PARITY_ENCODER: the policy's text-encoder forward, "fp32fwd" or "bf16x6".  bf16x6 measured 8.16 vs 8.05 ms per
# step and 1-3x the fp32 kernel's error, enough to move 2 of 437 durations at B=4 (profiles/r04/x6)
PARITY_ENCODER = os.environ.get("MTTS_PARITY_ENCODER", "fp32fwd")

_KIND_OF = {"fp32": PREC_FP32, "bf16x6": PACK_BF16_SPLIT3, "bf16x3": PACK_BF16_SPLIT}  # precise_forward's kinds
_process_split = False  # process-wide, not a context variable: visible from every thread


def set_weight_split(on: bool) -> bool:
    """Selects one (False) or two (True) bf16 weight planes for the bf16-mixed forward GEMMs from the next
    forward on; returns the previous setting.  (Captured graphs keep the packing they were captured with.)"""
    global _process_split
    old, _process_split = _process_split, bool(on)
    return old


@dataclasses.dataclass(frozen=True)
class ForwardPolicy:
    parity: bool = False  # the parity policy is active: split planes, and PackSpec.one_plane is honoured
    precise: str | None = None  # None, "bf16x3", "bf16x6" or "fp32" (precise_forward)
    encoder: str = "bf16"  # the ambient text-encoder precision, for a model that sets none (ENCODER_FORWARD)

    @property
    def weight_split(self) -> bool:
        return self.parity or _process_split

    def operand_kind(self, spec, prec: int) -> int:
        """The pack kind of `spec` in a `prec` region: `prec` itself outside bf16 and for a dgrad operand; for a
        bf16 forward operand precise_forward's kind, else one plane for a one_plane spec under the parity policy,
        else the split planes where selected."""
        if prec != PREC_BF16 or spec.dgrad:
            return prec
        if self.precise is not None:
            return _KIND_OF[self.precise]
        if spec.one_plane and self.parity:
            return PREC_BF16
        return PACK_BF16_SPLIT if self.weight_split else PREC_BF16

    def split_a(self, w_split: bool, a_dtype: torch.dtype) -> bool:
        """bf16x3: a GEMM on split weight planes also splits its fp32 A operand."""
        return bool(w_split) and self.precise is not None and a_dtype == torch.float32

    def attention_prec(self, prec: int) -> int:
        """The attention forward: exact fp32 (on fp32 q|k|v) under precise_forward, else the region's."""
        return PREC_FP32 if self.precise is not None else prec

    def ln_out_bf16(self, prec: int) -> bool:
        """A LayerNorm output that is only a GEMM's A operand may be stored bf16 -- not under precise_forward,
        whose GEMMs read the fp32 A's low bits."""
        return prec == PREC_BF16 and self.precise is None


_POLICY: contextvars.ContextVar = contextvars.ContextVar("mtts_forward_policy", default=ForwardPolicy())
policy = _POLICY.get


@contextlib.contextmanager
def _use(**changes):
    tok = _POLICY.set(dataclasses.replace(_POLICY.get(), **changes))
    try:
        yield
    finally:
        _POLICY.reset(tok)


def precise_forward(on: bool | str = True):
    """on: True / "bf16x3", "bf16x6" or "fp32" (module docstring); False: off.  The backward of the same ops stays
    bf16 one-plane either way."""
    return _use(precise=("bf16x3" if on is True else on) if on else None)


def parity_policy(on: bool = True):
    """bf16-parity inside a bf16 autocast region (module docstring).  on=False: no policy -- the process-wide
    split stays in force and the ambient text encoder is "bf16"."""
    return _use(parity=bool(on), encoder=PARITY_ENCODER if on else "bf16")


# text-encoder precision name (MatchaTTS.encoder_precision, ForwardPolicy.encoder) -> its precise_forward kind;
# "fp32" is no forward policy: autocast off around the encoder, forward AND backward exact fp32
ENCODER_FORWARD = {"bf16": None, "bf16x3": "bf16x3", "bf16x6": "bf16x6", "fp32fwd": "fp32"}


def encoder_context(name: str, device_type: str):
    if name == "fp32":
        return torch.autocast(device_type=device_type, enabled=False)
    kind = ENCODER_FORWARD[name]  # an unknown name is an error, not a bf16 encoder
    return precise_forward(kind) if kind else contextlib.nullcontext()


# Trainer precision name -> (bf16 autocast, parity policy): the one copy in the product
TRAINER_PRECISIONS = {"32-true": (False, False), "bf16-mixed": (True, False), "bf16-parity": (True, True)}


@contextlib.contextmanager
def trainer_precision(name: str):
    """The contexts of one Trainer precision on the device."""
    amp, parity = TRAINER_PRECISIONS[name]
    with contextlib.ExitStack() as st:
        if amp:
            st.enter_context(torch.autocast("cuda", dtype=torch.bfloat16))
        if parity:
            st.enter_context(parity_policy())
        yield
