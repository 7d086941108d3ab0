"""Parameter-gradient sums deferred to batched launches (csrc/reduce.hip, csrc/conv_gemm.hip).

Inside deferred_grad_sums() the weight-gradient GEMMs and the norm backwards only QUEUE the fixed-order sums
of their partial slabs; the context exit runs the queue as one launch instead of ~120 small ones.  The
weight-gradient GEMMs themselves are queued too and a flush launches them batched -- up to 12 layers per
launch, each job keeping its own row split, so a job's slabs are bitwise those of its own launch with the
same plan -- before their sums.  The plan itself differs by default (mtts_wgrad_plan_mode(0)): a queued job
takes the batched split plan (fewer, longer splits), an immediate one the per-launch plan, so the two round
differently (both deterministic); mtts_wgrad_plan_mode(1) gives every job the batched plan (the tests that
compare them bitwise set it).  The workspaces holding the partials (and the queued GEMMs' inputs) are kept
alive until the flush.  Valid only while nothing reads a parameter gradient before the exit: fresh gradients
(AccumulateGrad steals them, no copy kernel) of LEAF weights -- a Function whose weights are not all leaves
(ctx.leaf False) sums at once.

Side stream: at the decoder -> encoder seam of the backward (flow_matching._CfmPack) the decoder's queued
weight gradients + sums are launched on a side stream, forked there and joined at the deferral's exit, so
their chip-filling batched launches overlap the text encoder's latency-bound backward.  Past the seam the
encoder's own gradients follow them there in chunks of enc_side_jobs sums.
"""
from __future__ import annotations

import contextlib
import functools

import torch

from matcha import _native as N


class _Deferral:
    def __init__(self):
        self.on = False          # inside deferred_grad_sums()
        self.seam = False        # the backward is past the decoder -> encoder seam (a side flush has run)
        self.keep = []           # tensors the next main-stream flush reads
        self.side_keep = []      # tensors the side stream's work reads, until it is joined
        self.side = {}           # device index -> side stream
        self.side_used = False   # the side stream has work that the exit must join
        # past the seam, side-flush again whenever this many sums are queued -- the text encoder's own weight
        # gradients then queue behind the decoder's batch on the side stream instead of all running on the main
        # one after the encoder's backward (same box: 0 -> 7.20 ms, 8 7.47, 16 7.22, 24 7.12, 32 7.10,
        # 40 7.14, 48 7.11, 64 7.11)
        self.enc_side_jobs = 32

    def _fork(self):
        """This device's side stream, ordered after the current stream's work so far."""
        dev = torch.cuda.current_device()
        side = self.side.get(dev)
        if side is None:
            side = self.side[dev] = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        self.side_used = True
        return side

    def _join_side(self):
        """The current stream waits for the side stream's work; what it read may then be freed."""
        if self.side_used:
            main = torch.cuda.current_stream()
            for side in self.side.values():
                main.wait_stream(side)
            self.side_used = False
        self.side_keep.clear()

    @contextlib.contextmanager
    def deferred_grad_sums(self, enabled: bool = True):
        if not enabled or self.on:
            yield
            return
        lib = N.lib()
        lib.mtts_defer_reductions(1)
        self.on = True
        self.seam = False
        ok = False
        try:
            yield
            ok = True
        finally:
            lib.mtts_defer_reductions(0)
            self.on = False
            try:
                if ok:
                    N.check(lib.mtts_flush_reductions(torch.cuda.current_stream().cuda_stream), "mtts_flush_reductions")
                else:
                    lib.mtts_discard_reductions()
            finally:
                self._join_side()
                self.keep.clear()  # stream-ordered frees, after the flush launch

    def keep_partials(self, *ts):
        if self.on:
            self.keep.extend(t for t in ts if t is not None)

    def keep_for_side(self, *ts) -> None:
        self.side_keep.extend(t for t in ts if t is not None)

    def flush_deferred_side(self) -> None:
        """Inside deferred_grad_sums() (no-op outside): everything queued so far -- the weight-gradient GEMMs,
        batched, then the sums -- runs on a side stream forked from the current one here, while the backward
        continues on it; the deferral's exit (or the next main-stream flush) joins it.  Inputs and slabs stay
        alive until then (side_keep); the outputs are fresh parameter gradients that nothing reads before the
        join."""
        if not self.on:
            return
        lib = N.lib()
        if lib.mtts_pending_reductions() == 0:
            return
        N.check(lib.mtts_flush_reductions(self._fork().cuda_stream), "mtts_flush_reductions")
        self.side_keep.extend(self.keep)
        self.keep.clear()
        self.seam = True

    def _side_flush_encoder_chunk(self):
        """Past the seam: once enc_side_jobs sums are queued they go to the side stream, behind the decoder's
        batch there, instead of all at the end on the main one."""
        if self.seam and N.lib().mtts_pending_reductions() >= self.enc_side_jobs:
            self.flush_deferred_side()

    def param_grad_side_stream(self):
        """Inside deferred_grad_sums(): the deferral's side stream, already ordered after the current stream,
        for backward work whose only outputs are fresh parameter gradients (joined at the deferral's exit like
        the side flush); None otherwise.  The caller allocates on the current stream and hands every tensor
        the side work reads to keep_for_side()."""
        return self._fork() if self.on else None

    def side_fork_available(self) -> bool:
        """Whether side_fork() would return a stream (without forking): lets a caller finish the main-stream
        work the side work reads before the fork orders the side stream after it."""
        return self.on

    def flush_for_bucket(self):
        """Inside deferred_grad_sums(), before a data-parallel bucket is packed: every queued weight gradient
        and sum runs now on the deferral's side stream (the main stream goes on with the backward; the seam
        overlap of the N=1 step is kept).  Returns the side stream whose work so far the packer must wait for
        (None: nothing was launched there)."""
        if not self.on:
            return None
        self.flush_deferred_side()
        return self.side.get(torch.cuda.current_device()) if self.side_used else None

    def flush_deferred_grad_sums(self) -> None:
        """Runs the queued parameter-gradient sums now, on the current stream (inside deferred_grad_sums();
        no-op outside), after joining the side stream."""
        if not self.on:
            return
        self._join_side()
        N.check(N.lib().mtts_flush_reductions(torch.cuda.current_stream().cuda_stream), "mtts_flush_reductions")
        self.keep.clear()  # stream-ordered frees, after the flush launch

    def grad_sums(self, backward):
        """Backward decorator: a Function with non-leaf weights sums its partials at once."""
        @functools.wraps(backward)
        def run(ctx, *grads):
            if not self.on:
                return backward(ctx, *grads)
            if getattr(ctx, "leaf", True):
                out = backward(ctx, *grads)
                self._side_flush_encoder_chunk()
                return out
            lib = N.lib()
            lib.mtts_defer_reductions(0)
            try:
                return backward(ctx, *grads)
            finally:
                lib.mtts_defer_reductions(1)
        return run


DEFER = _Deferral()
deferred_grad_sums = DEFER.deferred_grad_sums
flush_deferred_side = DEFER.flush_deferred_side
param_grad_side_stream = DEFER.param_grad_side_stream
side_fork = DEFER.param_grad_side_stream  # the same fork, for forward work that runs ahead (prefetch)
side_fork_available = DEFER.side_fork_available
keep_for_side = DEFER.keep_for_side
flush_for_bucket = DEFER.flush_for_bucket
flush_deferred_grad_sums = DEFER.flush_deferred_grad_sums
_grad_sums = DEFER.grad_sums
_keep_partials = DEFER.keep_partials
