"""Train-step driver: the semantics of the reference's Lightning loop (train.py:81-102,
baselightningmodule.py:115-162) on one process per GPU.

  - fp32 master weights, AdamW(1e-4, (0.9, 0.999), eps 1e-8, wd 1e-6) + per-epoch cosine
    (configure_optimizers)
  - gradient clipping by global norm 1.0 (gradient_clip_val=1.0)
  - gradient accumulation (accumulate_grad_batches; the reference uses 2 x 16 = 32 per step)
  - the step's 4 logged losses reduced in ONE collective (the reference issues one sync_dist
    all-reduce per self.log call)

Two execution modes:
  graph=True (default on GPU): the whole step is captured once per input shape into a HIP graph and
    replayed (shape-keyed LRU cache, TrainConfig.graph_cache) -- about a thousand kernel launches per
    step become one graph launch.  Gradients are NOT pre-allocated: param.grad is None when backward
    starts, so autograd hands each parameter its freshly computed gradient tensor (no per-parameter
    accumulate kernel).  N=1: clip + AdamW (csrc/optim.hip, over one flat parameter array) run in a
    second graph on those tensors.  N>1 (matcha/dp.py): post-accumulate-grad hooks pack the gradients
    bucket by bucket into a flat fp32 buffer and fork each bucket's RCCL all-reduce (libmtts_hip's own
    communicator, capturable) onto a side stream while backward continues; the join, clip and AdamW on
    views of the reduced buffer are in the SAME graph.  With torch.distributed as the transport (gloo,
    the shared-GPU rehearsal) the graph only packs, the host reduces the flat buffer, and a second
    graph steps.  Dropout masks (torch's and the HIP epilogues') come from device-side RNG state, so
    every replay draws new masks.  Inputs are copied into static buffers before each replay.
  graph=False (eager): torch DDP over RCCL (bucketed all-reduce overlapped with backward, no_sync for
    non-final accumulation micro-batches), or the same bucket reducer (dp="buckets").

N>1 graph step: every replay issues the same collective sequence (the buckets of one fixed layout -- rank
0's recorded backward order, broadcast once -- in bucket order), whatever shape a rank's batch has; a
capture's warm-up passes never communicate (the reducer packs only), and the communicator's connections
are set up once by an eager all-reduce per bucket on every rank when the reducer is built.  By default
(TrainConfig.agree_shapes=True) every rank pads to the MAX padded Tx / Ty over ranks -- one host-side gloo
all-reduce per step, no GPU sync -- so all ranks capture and replay the same graph together; the extra padding
changes the padded-length dependent parts of the arithmetic (GroupNorm statistics, conv bias leaking into padded
frames).  agree_shapes=False lets each rank pad to its own length, as the reference's DDP would, and capture new
shapes on its own (tested over gloo; not yet run with the in-graph RCCL transport on a multi-GPU box).

Around the step, the rest of the reference's loop (Trainer.fit): validation_step / validate (eval(), no_grad(),
captured per shape like the step), save_checkpoint / load_checkpoint (matcha/checkpoint.py: Lightning's file layout,
the optimizer state in torch.optim.AdamW's form in both modes; a graph-mode load writes into the flat arrays in place,
so captured steps stay valid), and per-epoch last / top-k checkpoints and resume.  None of it touches the step.

Synthetic LJSpeech-shaped batches: token ids ~ U{1..149}, lengths ~ U[0.7 max, max]
with element 0 = max, mels ~ N(0, 1) zeroed past the length.  A batch dict may carry "t" [B, 1, 1] and
"z" [B, n_feats, Ty]: the CFM randomness injected for parity tests (MatchaTTS.forward's keywords); with
TrainConfig.out_size = S, "z" is [B, n_feats, S] and "out_offset" [B] injects the segment windows.
"durations" ([B, Tx] or [B, 1, Tx], any real dtype; e.g. MatchaTTS.align's) goes to a
MatchaTTS(use_precomputed_durations=True) as forward's ``durations``: the captured step then holds one
duration_path launch in place of the MAS kernels, and a replay reads the batch's durations from its static buffer.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass

import torch
import torch.distributed as dist

from matcha import _graphs as G
from matcha import _native as N
from matcha._abi import AdamWChunk as _AdamWChunk
from matcha.models.components import _ops as OPS
from matcha.models.components._defer import deferred_grad_sums
from matcha.models.components._policy import trainer_precision
from matcha.models.matcha_tts import MatchaTTS


def synthetic_batch(B: int, Tx: int, Ty: int, n_feats: int = 80, seed: int = 0, device="cuda",
                    n_vocab: int = 150) -> dict:
    g = torch.Generator().manual_seed(seed)
    x_lengths = (Tx * (0.7 + 0.3 * torch.rand(B, generator=g))).long().clamp(1, Tx)
    y_lengths = (Ty * (0.7 + 0.3 * torch.rand(B, generator=g))).long().clamp(1, Ty)
    x_lengths[0], y_lengths[0] = Tx, Ty
    y_lengths = torch.maximum(y_lengths, x_lengths)
    x = torch.randint(1, n_vocab, (B, Tx), generator=g)
    y = torch.randn(B, n_feats, Ty, generator=g)
    pos_x = torch.arange(Tx)[None, :]
    pos_y = torch.arange(Ty)[None, None, :]
    x = x * (pos_x < x_lengths[:, None])
    y = y * (pos_y < y_lengths[:, None, None])
    return {k: v.to(device) for k, v in dict(x=x, x_lengths=x_lengths, y=y, y_lengths=y_lengths).items()}


def _total_and_logged(dur, prior, diff, segments: int = 1):
    """(total = dur + prior + diff, the logged [dur, prior, diff, total] as detached fp32) in one launch on the
    device; the CPU data-parallel tests drive the loop with a CPU stand-in model.  segments > 1 (merged
    micro-batches, [segments] tensors): the mean over micro-batches of each one's total / logged vector."""
    if segments > 1:
        parts = [OPS.loss_sum(dur[j], prior[j] if torch.is_tensor(prior) else 0, diff[j]) for j in range(segments)]
        return sum(tp[0] for tp in parts) / segments, sum(tp[1] for tp in parts) / segments
    if dur.device.type == "cuda":
        return OPS.loss_sum(dur, prior, diff)
    total = dur + prior + diff
    return total, torch.stack([dur, torch.as_tensor(prior), diff, total]).detach().float()


# how Trainer._armed arms the data-parallel reducer for a backward
ARM_OVERLAP = "overlap"  # pack, each bucket's all-reduce forked off as the backward completes it
ARM_REDUCE_AFTER = "reduce-after"  # pack; the caller reduces after the backward (torch.distributed transport)
ARM_PACK_ONLY = "pack-only"  # pack, never communicate (a capture's warm-up passes)


class _FlatClipAdamW:
    """clip_grad_norm_(max_norm) + AdamW(lr, (0.9, 0.999), eps 1e-8, wd 1e-6) -- the reference step's
    optimizer (baselightningmodule.py:59-65, train.py gradient_clip_val) -- as mtts_clip_adamw over a
    flat parameter array.  lr is a float64 device scalar (the cosine schedule writes it); the step count lives
    on the device; the gradient table is rebuilt whenever the gradient tensors change (eager calls)
    and frozen by bind_grads() for graph capture."""

    CHUNK = 32768

    def __init__(self, params, lr: torch.Tensor, max_norm: float, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6):
        if lr.dtype != torch.float64:
            raise TypeError("lr must be a float64 device scalar (torch derives AdamW's scalars in double)")
        self.params = list(params)
        dev = self.params[0].device
        offs, off = [], 0
        for p in self.params:
            offs.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.flat = torch.zeros(off, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                self.flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.flat[o:o + p.numel()].view_as(p)
        self.offsets = offs
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.step_t = torch.zeros(1, device=dev, dtype=torch.float32)
        self.lr, self.max_norm = lr, float(max_norm or 0.0)
        self.betas, self.eps, self.wd = betas, eps, weight_decay
        # gradients are SUMS over grad_scale^-1 data-parallel ranks (RcclComm: ncclSum); the mean is taken here
        self.grad_scale = 1.0
        self._table = None
        self._key = None
        self._ws = None
        self.state = {}  # (torch.optim API surface used by callers)

    def _build(self):
        key = tuple((p.grad.data_ptr() if p.grad is not None else 0) for p in self.params)
        if key == self._key:
            return
        rows = []
        for p, o in zip(self.params, self.offsets):
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise RuntimeError("fused AdamW expects contiguous fp32 gradients")
            n = g.numel()
            for s in range(0, n, self.CHUNK):
                rows.append((g.data_ptr() + 4 * s, o + s, min(self.CHUNK, n - s)))
        arr = (_AdamWChunk * max(len(rows), 1))()
        for i, (gp, o, n) in enumerate(rows):
            arr[i].grad, arr[i].offset, arr[i].n = gp, o, n
        host = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
        self._table = host.to(self.flat.device)
        self._n = len(rows)
        nws = int(N.lib().mtts_clip_adamw_workspace_size(self._n))
        self._ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=self.flat.device)
        self._key = key

    def bind_grads(self):
        self._key = None
        self._build()

    def step(self):
        if torch.cuda.is_current_stream_capturing():
            if self._table is None:
                raise RuntimeError("bind_grads() before capturing the optimizer step")
        else:
            self._build()
        b1, b2 = self.betas
        N.check(N.lib().mtts_clip_adamw_scaled(N.ptr(self._table), self._n, N.ptr(self.flat), N.ptr(self.exp_avg),
                                               N.ptr(self.exp_avg_sq), N.ptr(self.lr), N.ptr(self.step_t),
                                               self.max_norm, b1, b2, self.eps, self.wd, self.grad_scale,
                                               N.ptr(self._ws), self._ws.numel(),
                                               torch.cuda.current_stream(self.flat.device).cuda_stream),
                "mtts_clip_adamw_scaled")

    def state_snapshot(self):
        return [t.clone() for t in (self.exp_avg, self.exp_avg_sq, self.step_t)]

    def state_restore(self, snap):
        for t, s_ in zip((self.exp_avg, self.exp_avg_sq, self.step_t), snap):
            t.copy_(s_)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            p.grad = None


@dataclass
class TrainConfig:
    accumulate_grad_batches: int = 1
    gradient_clip_val: float = 1.0
    bucket_mb: float = 25.0  # DDP buckets (eager) and the graph step's all-reduce buckets
    # graph step: one bucket boundary at the decoder / encoder seam of the backward (the decoder's gradients are
    # issued together where the N=1 step side-flushes them), buckets up to seam_bucket_mb inside each part.
    # Round 4, forced-DP step on one GPU: 25 MB buckets flushed the queued weight gradients mid-decoder-backward
    # (+0.39 ms over the plain step); False: plain bucket_mb buckets
    bucket_seams: bool = True
    seam_bucket_mb: float = 64.0
    # "32-true" (reference), "bf16-mixed" (autocast), or "bf16-parity": bf16-mixed with split bf16 weight
    # planes (every forward GEMM but the decoder FF's GELU up-projection) and the text encoder's forward on the
    # exact-fp32 MFMA -- alignment exact, losses within 1e-4 of 32-true
    # (tests/test_headline_gpu.py; components/_policy.py)
    precision: str = "32-true"
    graph: bool = False
    lr: float = 1e-4
    eta_min: float = 1e-6
    t_max_epochs: int = 1000
    # captured steps kept per input-shape key (LRU); collate(x_quantum=16, y_quantum=64) on bucketed batches
    # keeps real data to ~20 padded shapes (tests/test_data_path.py) -- size the cache to cover them.  Each
    # cached graph keeps its own memory pool holding the whole step's activations and gradients (~2-3 GB at
    # B=32 x 600 frames bf16-mixed, ~6 GB at B=8 x 4096): 20 shapes fit the MI355X's 288 GB many times
    graph_cache: int = 4
    dp: str = "auto"  # N>1 exchange: "ddp" (eager only), "buckets" (GradBucketReducer), "auto"
    comm: str = "auto"  # bucket reducer transport: "rccl" (capturable, libmtts_hip), "torch", "auto"
    # N>1 graph step: pad every rank's batch to the MAX padded shape over ranks (see the module docstring), so
    # every rank captures and replays the same graph and issues the same in-graph RCCL collectives.  ON by default
    # (ADVICE r4): rank-local captures beside peers that replay in-graph RCCL all-reduces have never run on a
    # multi-GPU box; False keeps each rank's own padding (as DDP in the reference's setup) -- exercised over gloo
    # by tests/test_dp_multirank_gpu.py
    agree_shapes: bool = True
    # run the data-parallel exchange even at world size 1 (a world-size-1 process group must exist): the
    # bucketed RCCL path's cost on one GPU (bench.py extra_configs.dp_forced_n1); MTTS_FORCE_DP=1 does the same
    force_dp: bool = False
    # accumulate_grad_batches > 1 with micro-batches of one padded shape: ONE forward / backward of the stacked
    # micro-batches, each loss normalised per micro-batch (MatchaTTS.forward(segments=n)) -- the gradient of
    # (1/n) sum_i L_i that accumulation computes; every op but the losses is per utterance (GroupNorm / LayerNorm
    # statistics per utterance and padded length), so only the weight-gradient reductions' rounding differs.
    # Micro-batches of different padded shapes take the stashed fresh-gradient path (_fwd_bwd_stash)
    merge_micro_batches: bool = True
    # train on a random window of out_size mel frames per utterance (MatchaTTS.forward(out_size=...), the
    # reference's matcha_tts.py:290-312): the decoder and the CFM / prior losses see the window, the alignment
    # and the duration loss the whole utterance.  The windows are drawn on the device inside the step, so a
    # captured step replays with fresh ones; a batch's "out_offset" (int [B]) injects them, "z" is then
    # [B, n_feats, out_size].  None: whole utterances
    out_size: int | None = None


class Trainer:
    # MTTS_FORCE_DP=1: run the data-parallel exchange even at world size 1 (rehearses the bucketed
    # RCCL path on a one-GPU box; the all-reduce of one rank is a copy)
    force_dp = os.environ.get("MTTS_FORCE_DP", "0") == "1"

    def __init__(self, model: MatchaTTS, cfg: TrainConfig = TrainConfig()):
        self.cfg = cfg
        self.model = model
        self.world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        self.dev = next(model.parameters()).device
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.global_step = 0
        self.epoch = 0
        self.last_losses = None
        self.dp = self.world > 1 or ((self.force_dp or cfg.force_dp) and dist.is_available() and dist.is_initialized())
        mode = cfg.dp if cfg.dp != "auto" else ("buckets" if cfg.graph else "ddp")
        if cfg.graph and mode == "ddp":
            raise ValueError("the graph step exchanges gradients with the bucket reducer (dp='buckets')")
        self.dp_mode = mode if self.dp else None
        self.reducer = None
        self._recorder = None
        self._arm = None  # an ARM_* mode inside _armed(): the next backward arms the reducer
        self._graphs = G.GraphCache(cfg.graph_cache)  # captured steps per input-shape key, LRU
        self._val_graphs = G.GraphCache(cfg.graph_cache)  # validation_step's: it never evicts a train step
        self._best_k = {}  # fit's best checkpoints: file name -> loss/val (saved with every checkpoint)
        # bench.py's N>1 path (matcha/watchdog.py): a host watchdog told of every step / graph key / bucket issue,
        # and device progress markers captured into the step (one after each bucket's all-reduce, one at its end)
        self.watchdog = None
        self.progress = None
        # a gloo group for the host-side agreements (padded shapes, bucket layout): never syncs the GPU
        self._host_group = None
        if self.dp and self.world > 1:
            if dist.get_backend() == "gloo":
                self._host_group = dist.group.WORLD
            else:
                from matcha.dp import stdout_to_stderr

                with stdout_to_stderr():  # gloo's connect message stays off the bench's JSON stdout
                    self._host_group = dist.new_group(backend="gloo")
        if self.dp and self.world > 1:  # identical initial weights on every rank (what DDP's broadcast does)
            for p in model.state_dict().values():
                dist.broadcast(p, 0)
        if cfg.graph:
            for p in self.params:
                p.grad = None
            self.lr = torch.tensor(cfg.lr, device=self.dev, dtype=torch.float64)  # torch keeps lr a double
            # clip + AdamW as two HIP launches (csrc/optim.hip) over one flat fp32 parameter array:
            # the parameters become views into it (names / state_dict unchanged), each region
            # 16-byte aligned; the moments are flat arrays of the same layout
            self.optimizer = _FlatClipAdamW(self.params, self.lr, cfg.gradient_clip_val)
            self.scheduler = None
            self.wrapped = model
        else:
            if self.dp_mode == "ddp":
                self.wrapped = torch.nn.parallel.DistributedDataParallel(
                    model, device_ids=[self.dev.index] if self.dev.type == "cuda" else None,
                    bucket_cap_mb=cfg.bucket_mb, gradient_as_bucket_view=True, broadcast_buffers=False)
            else:
                self.wrapped = model
            opt = model.configure_optimizers()
            self.optimizer = opt["optimizer"]
            self.scheduler = opt["lr_scheduler"]["scheduler"]

    # ------------------------------------------------------------------------------------ common
    def _autocast(self):
        return trainer_precision(self.cfg.precision) if self.dev.type == "cuda" else contextlib.nullcontext()

    def _losses(self, net, batch, out_size):
        """(dur, prior, diff) of `net` (self.wrapped to train, self.model to validate) on one batch under the
        trainer's precision context, the batch's "t" / "z" / "out_offset" (the parity tests' CFM randomness and
        segment windows) and "durations" (a use_precomputed_durations model's) injected."""
        inject = {k: batch[k] for k in ("t", "z", "out_offset", "durations") if k in batch}
        if out_size is not None:
            inject["out_size"] = out_size
        if batch.get("_segments", 1) > 1:  # merged micro-batches: per-micro-batch losses ([seg] tensors)
            inject["segments"] = batch["_segments"]
        with self._autocast():
            dur, prior, diff, *_ = net(x=batch["x"], x_lengths=batch["x_lengths"], y=batch["y"],
                                       y_lengths=batch["y_lengths"], **inject)
        return dur, prior, diff

    @contextlib.contextmanager
    def _armed(self, mode):
        """The last micro-batch's backward of the enclosed _fwd_bwd arms the reducer in `mode` (ARM_*): it packs
        the accumulated gradients (and the logged means) bucket by bucket as the backward produces them."""
        self._arm = mode
        try:
            yield
        except BaseException:
            # an aborted forward / backward leaves the reducer disarmed: its hooks issue nothing in a later
            # backward and a later finish() returns at once (it would otherwise issue the remaining buckets)
            if self.reducer is not None:
                self.reducer.disarm()
            raise
        finally:
            self._arm = None
            OPS.set_grad_slots(None)  # an aborted backward leaves no slots armed

    def _fwd_bwd(self, batches, sync_ctx=None):
        n = len(batches)
        if n > 1 and self._merge_ok(batches):
            batches = [self._merge(batches)]
            n = 1
        elif n > 1 and self._stash_ok():
            return self._fwd_bwd_stash(batches)
        # the parameter-gradient partial sums of the whole backward in batched launches
        # (components/_defer.py deferred_grad_sums): needs fresh gradients, which autograd steals (one
        # micro-batch, gradients set to None first), and no DDP hook reading them during the backward
        # (the bucket reducer flushes the queue per bucket)
        fresh = (self.dev.type == "cuda" and all(p.grad is None for p in self.params)
                 and (self.cfg.graph or self.dp_mode != "ddp"))
        # several micro-batches (accumulate_grad_batches): the FIRST one's gradients are fresh too -- its
        # backward runs deferred (batched weight gradients, flushed when it ends, before the next micro-batch
        # accumulates into them); the later ones accumulate and run per layer
        with deferred_grad_sums(fresh and n == 1):
            return self._fwd_bwd_body(batches, sync_ctx, defer_first=fresh and n > 1)

    def _merge_ok(self, batches) -> bool:
        """TrainConfig.merge_micro_batches and every micro-batch the same padded shapes (CUDA MatchaTTS)."""
        if not self.cfg.merge_micro_batches or self.dev.type != "cuda" or not isinstance(self.model, MatchaTTS):
            return False
        keys = set(batches[0])
        return all(set(b) == keys and all(b[k].shape == batches[0][k].shape and b[k].dtype == batches[0][k].dtype
                                          for k in keys) for b in batches[1:]) and "_segments" not in keys

    @staticmethod
    def _merge(batches):
        out = {k: torch.cat([b[k] for b in batches], 0) for k in batches[0]}
        out["_segments"] = len(batches)
        return out

    def _stash_ok(self) -> bool:
        """accumulate_grad_batches > 1 without data parallelism: every micro-batch can take the fresh-gradient
        path (batched, deferred weight gradients and sums, side-stream seam flushes) -- its gradients are
        stashed and summed at the end instead of accumulated per layer.  The DP reducer packs the last
        micro-batch's gradients as backward produces them, so it keeps the accumulating path."""
        return self.dev.type == "cuda" and not self.dp and all(p.grad is None for p in self.params)

    def _fwd_bwd_stash(self, batches):
        """Micro-batch i: forward + (total / n).backward() on fresh gradients under the gradient deferral (the
        N=1 step's fast path), its gradients stashed; the end sums them with multi-tensor adds in micro-batch
        order, ((g_1 + g_2) + g_3) ..., the fp32 adds autograd's AccumulateGrad does -- so the result equals
        the accumulating path's (tests/test_training_gpu.py::test_accumulate_grad_batches_2_vs_torch)."""
        n = len(batches)
        logged = None
        stash = []
        for i, batch in enumerate(batches):
            with deferred_grad_sums(True):
                vals = self._fwd_bwd_body([batch], div=n)
            logged = vals if logged is None else logged + vals
            stash.append([p.grad for p in self.params])
            for p in self.params:
                p.grad = None
        acc = list(stash[0])
        for g in stash[1:]:
            a_, b_ = [], []
            for k, gk in enumerate(g):
                if gk is None:
                    continue
                if acc[k] is None:
                    acc[k] = gk
                else:
                    a_.append(acc[k])
                    b_.append(gk)
            if a_:
                torch._foreach_add_(a_, b_)  # in place into micro-batch 1's (fresh, unaliased) gradients
        for p, gk in zip(self.params, acc):
            p.grad = gk
        return logged / n

    def _fwd_bwd_body(self, batches, sync_ctx=None, div=None, defer_first=False):
        n = len(batches)
        logged = None
        for i, batch in enumerate(batches):
            ctx = sync_ctx(i) if sync_ctx else contextlib.nullcontext()
            first = deferred_grad_sums(True) if (i == 0 and defer_first) else contextlib.nullcontext()
            with ctx, first:
                losses = self._losses(self.wrapped, batch, self.cfg.out_size)
                total, vals = _total_and_logged(*losses, segments=batch.get("_segments", 1))
                logged = vals if logged is None else logged + vals
                if i == n - 1 and self._arm is not None:
                    self.reducer.arm(logged / n, overlap=self._arm == ARM_OVERLAP, comm=self._arm != ARM_PACK_ONLY)
                d = div if div is not None else n
                (total / d if d > 1 else total).backward()
        return logged / n if n > 1 else logged

    def _clip_and_update(self):
        if isinstance(self.optimizer, _FlatClipAdamW):  # graph mode: clipping is inside the fused step
            self.optimizer.step()
            return
        if self.cfg.gradient_clip_val:
            torch.nn.utils.clip_grad_norm_(self.params, self.cfg.gradient_clip_val, foreach=True)
        self.optimizer.step()

    def _group_stacked(self, order):
        """The recorded backward order with the weights that one stacked GEMM produces (q|k|v of the decoder's
        attention and of the text encoder's) placed back to back in stacking order, so that their flat-buffer
        views form one region the stacked weight-gradient GEMM writes in place (_ops._grad_buf_stacked)."""
        groups = []
        for m in self.model.modules():
            for names in (("to_q", "to_k", "to_v"), ("query_conv", "key_conv", "value_conv")):
                if all(isinstance(getattr(m, n, None), torch.nn.Module) for n in names):
                    groups.append([getattr(m, n).weight for n in names])
        member = {id(p): g for g in groups for p in g}
        present = {id(p) for p in order}
        out, done = [], set()
        for p in order:
            g = member.get(id(p))
            if g is not None and all(id(q) in present for q in g):
                if id(p) not in done:
                    out.extend(g)
                    done.update(id(q) for q in g)
            else:
                out.append(p)
        return out

    def _ensure_reducer(self, batches, run_step):
        """First DP step: one pass with an arrival recorder fixes the bucket layout (backward order)."""
        if self.reducer is not None:
            return None
        from matcha import dp as DP

        rec = DP.ArrivalRecorder(self.params)
        try:
            logged = run_step()
        finally:
            rec.remove()
        order = self._group_stacked(rec.order)
        if self.world > 1:  # one bucket layout on every rank: rank 0's recorded backward order
            index = {id(p): i for i, p in enumerate(self.params)}
            box = [[index[id(p)] for p in order]]
            dist.broadcast_object_list(box, src=0, group=self._host_group)
            if sorted(box[0]) != sorted(index[id(p)] for p in order):
                raise RuntimeError("data parallel: the ranks differentiate different parameter sets")
            order = [self.params[i] for i in box[0]]
        comm = DP.make_comm(self.dev, self.cfg.comm)
        seams, mb = (), self.cfg.bucket_mb
        enc = getattr(self.model, "encoder", None)
        if self.cfg.bucket_seams and self.cfg.graph and isinstance(enc, torch.nn.Module):
            enc_ids = {id(p) for p in enc.parameters()}
            first_enc = next((p for p in order if id(p) in enc_ids), None)
            if first_enc is not None:
                seams, mb = (first_enc,), max(mb, self.cfg.seam_bucket_mb)
        reducer = DP.GradBucketReducer(order, comm, mb, self.dev, seams=seams)
        # the device's bucket mark holds the bucket tag in 8 bits (matcha/watchdog.py): refused here, not in a
        # hook in the middle of a backward
        limit = getattr(self.progress, "MAX_BUCKETS", None)
        if limit is not None and len(reducer.buckets) > limit:
            reducer.remove()
            if hasattr(comm, "close"):
                comm.close()
            raise ValueError(f"data parallel: the bucket layout has {len(reducer.buckets)} buckets, the device "
                             f"progress markers encode at most {limit} (raise bucket_mb)")
        self.reducer = reducer
        self.reducer.watchdog, self.reducer.progress = self.watchdog, self.progress
        if isinstance(self.optimizer, _FlatClipAdamW):  # the mean over ranks rides in the fused optimizer step
            self.optimizer.grad_scale = comm.post_scale
            self.reducer.grad_scale_applied = True
        if comm.capturable:
            self.reducer.warm()  # every rank, now: later captures run without any collective
        return logged

    # ------------------------------------------------------------------------------------ eager
    def _eager_step(self, batches):
        n = len(batches)
        ddp = self.dp_mode == "ddp"

        def sync_ctx(i):
            return self.wrapped.no_sync() if (ddp and i < n - 1) else contextlib.nullcontext()

        if self.dp_mode == "buckets" and self.reducer is None:
            logged = self._ensure_reducer(batches, lambda: self._fwd_bwd(batches))
            # this first step: pack what backward produced and reduce it in one call
            for i, p in enumerate(self.reducer.params):
                self.reducer.views[i].copy_(p.grad)
            self.reducer.flat[self.reducer.n_grad:].copy_(logged)
            self.reducer.reduce_now()
            self.reducer.attach_views()
            logged = self.reducer.scalars().clone()
        elif self.dp_mode == "buckets":
            with self._armed(ARM_OVERLAP):
                self._fwd_bwd(batches)
            self.reducer.finish()
            logged = self.reducer.scalars().clone()
        else:
            logged = self._fwd_bwd(batches, sync_ctx)
            if ddp:  # the step's logged scalars in one collective (sync_dist=True)
                dist.all_reduce(logged)
                logged = logged / self.world
        self._clip_and_update()
        if self.progress is not None and self.dev.type == "cuda":
            self.progress.mark_step(torch.cuda.current_stream(self.dev))
        self.optimizer.zero_grad(set_to_none=True)
        return logged

    # ------------------------------------------------------------------------------------ graph
    def _graph_capture(self, batches):
        """Captures the step for this input-shape key.  N=1: graph 1 = fwd+bwd (fresh gradients),
        graph 2 = clip + AdamW on them.  DP with a capturable communicator: ONE graph -- fwd, bwd with
        each bucket's RCCL all-reduce forked off as backward completes it, join, clip + AdamW on the
        reduced flat buffer.  DP with torch.distributed: graph 1 packs the buckets, the host reduces
        the flat buffer, graph 2 steps."""
        e = {"static": [{k: v.clone() for k, v in b.items()} for b in batches]}
        static = e["static"]
        # warm-up (allocator pools, lazy library loads, optimizer state) must not leave updates behind
        saved = [p.detach().clone() for p in self.params]
        saved_state = self.optimizer.state_snapshot()
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            # warm-up passes are rank-local (no collective): a rank may capture a new shape while its peers
            # replay; only the first step of all (the reducer's construction) communicates, on every rank
            for it in range(2):
                for p in self.params:
                    p.grad = None
                if self.dp and self.reducer is None:
                    self._ensure_reducer(batches, lambda: self._fwd_bwd(static))
                    for i, p in enumerate(self.reducer.params):
                        self.reducer.views[i].copy_(p.grad)
                    self.reducer.attach_views()
                elif self.dp:
                    with self._armed(ARM_PACK_ONLY):
                        self._fwd_bwd(static)
                    self.reducer.finish()
                else:
                    self._fwd_bwd(static)
                self._clip_and_update()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        gparams = [p for p in self.params if p.grad is not None]  # parameters the step differentiates
        with torch.no_grad():
            for p, s_ in zip(self.params, saved):
                p.copy_(s_)
            self.optimizer.state_restore(saved_state)  # moments / step back to their pre-warm-up values

        overlap = self.dp and self.reducer.comm.capturable
        if self.dp:
            self.reducer.attach_views()
            self.optimizer.bind_grads()  # the table points at the flat buffer's views (fixed addresses)

        def fwd_bwd():
            for p in self.params:
                p.grad = None  # autograd hands over each fresh gradient: no accumulate kernels
            if not self.dp:
                return self._fwd_bwd(static)
            with self._armed(ARM_OVERLAP if overlap else ARM_REDUCE_AFTER):
                logged = self._fwd_bwd(static)
            self.reducer.finish()  # joins the forked all-reduces; .grad -> flat views
            if overlap:
                self._clip_and_update()
                if self.progress is not None:  # the device's "step done" marker, a node of the graph
                    self.progress.mark_step(torch.cuda.current_stream(self.dev))
            return logged

        # (the warm-up above is the step's own: passes=0)
        e["g_fb"], e["logged"] = G.capture(fwd_bwd, self.dev, passes=0)
        e["fb_grads"] = [p.grad for p in gparams]  # graph-pool outputs, kept alive with the graph
        e["g_opt"] = None
        if not overlap:
            if not self.dp:  # the optimizer graph's table points at the (fixed) graph-pool gradients
                self.optimizer.bind_grads()
            e["g_opt"], _ = G.capture(self._clip_and_update, self.dev, passes=0, pool=e["g_fb"].pool())
        e["opt_keep"] = (self.optimizer._table, self.optimizer._ws)  # the captured kernels read these
        e["overlap"] = overlap
        return e

    def _agree_shapes(self, batches):
        """TrainConfig.agree_shapes (N>1 graph step, ON by default): MAX over ranks of each micro-batch's padded Tx /
        Ty (and one batch size), then zero padding up to it, so every rank looks up the same key.  The padded
        frames are masked, but the decoder's arithmetic depends on the padded length (GroupNorm statistics
        over the whole padded length, conv bias leaking into padded frames -- SURVEY 0.6), so with the default a
        rank's losses depend on its peers' padded lengths (tests/test_distributed_cpu.py measures the difference
        against per-rank padding); agree_shapes=False keeps each rank's own padding, as the reference's DDP
        would."""
        if not (self.cfg.agree_shapes and self.dp and self.world > 1 and self.cfg.graph):
            return batches
        dims = torch.tensor([[b["x"].shape[1], b["y"].shape[2], b["x"].shape[0], -b["x"].shape[0]] for b in batches],
                            dtype=torch.int64)
        dist.all_reduce(dims, op=dist.ReduceOp.MAX, group=self._host_group)
        out = []
        for b, (tx, ty, bmax, nbmin) in zip(batches, dims.tolist()):
            if bmax != -nbmin:
                raise ValueError(f"data parallel graph step: per-rank batch sizes differ ({-nbmin}..{bmax})")
            b = dict(b)
            if b["x"].shape[1] < tx:
                if "durations" in b:  # [B,Tx] or [B,1,Tx]: along Tx, like x (rows past x_lengths count for nothing)
                    b["durations"] = torch.nn.functional.pad(b["durations"], (0, tx - b["durations"].shape[-1]))
                b["x"] = torch.nn.functional.pad(b["x"], (0, tx - b["x"].shape[1]))
            if b["y"].shape[2] < ty:
                b["y"] = torch.nn.functional.pad(b["y"], (0, ty - b["y"].shape[2]))
                if "z" in b and self.cfg.out_size is None:  # with out_size, z is [B, n_feats, out_size]
                    b["z"] = torch.nn.functional.pad(b["z"], (0, ty - b["z"].shape[2]))
            out.append(b)
        return out

    def _graph_step(self, batches):
        batches = self._agree_shapes(batches)
        key = tuple(tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(b.items())) for b in batches)
        if self.watchdog is not None:
            self.watchdog.note(graph_key="|".join(f"B{b['x'].shape[0]}xTx{b['x'].shape[1]}xTy{b['y'].shape[-1]}"
                                                  for b in batches), graph_cached=key in self._graphs)
        e = self._graphs.lookup(key, lambda: self._graph_capture(batches))
        for b, s in zip(batches, e["static"]):
            for k, v in s.items():
                if b[k] is not v:
                    v.copy_(b[k], non_blocking=True)
        e["g_fb"].replay()
        if not self.dp:
            e["g_opt"].replay()
            return e["logged"]
        if not e["overlap"]:  # torch.distributed transport: one eager all-reduce of the packed buffer
            self.reducer.reduce_now()
            e["g_opt"].replay()
            if self.progress is not None:
                self.progress.mark_step(torch.cuda.current_stream(self.dev))
        return self.reducer.scalars().clone()  # the flat buffer is overwritten by the next replay

    def measure_dp_tail(self, batches) -> dict | None:
        """The data-parallel step's exposed tail: ONE extra eager forward + backward with the
        reducer armed exactly as in the graph step (every rank calls it together; no optimizer update, results
        discarded), with HIP events on the main stream at the end of the backward and on the reducer stream
        around the last bucket's pack + all-reduce.  Returns the all-reduce's own time and the part of it the
        main stream waits for (exposed = end of the last all-reduce - end of the backward, >= 0).  None unless a
        capturable (RCCL) reducer runs on a GPU."""
        r = self.reducer
        if r is None or not self.dp or self.dev.type != "cuda" or not r.comm.capturable:
            return None
        ev = {k: torch.cuda.Event(enable_timing=True) for k in ("start", "end", "bwd_end")}
        for p in self.params:
            p.grad = None
        r.tail_events = ev
        try:
            with self._armed(ARM_OVERLAP):  # (a forward / backward that raises leaves the reducer disarmed)
                self._fwd_bwd(self._agree_shapes(batches))
            r.finish()  # records "bwd_end": while tail_events is still set
        finally:
            r.tail_events = None
        torch.cuda.synchronize(self.dev)
        ar = ev["start"].elapsed_time(ev["end"])
        exposed = max(0.0, ev["bwd_end"].elapsed_time(ev["end"]))
        return {"tail_bucket": len(r.buckets) - 1, "tail_bucket_mb": round((r.spans[-1][1] - r.spans[-1][0]) * 4 / 2 ** 20, 3),
                "tail_pack_allreduce_us": round(ar * 1e3, 1), "tail_exposed_us": round(exposed * 1e3, 1),
                "note": "one eager fwd+bwd after the timed region, reducer armed as in the graph step: HIP events "
                        "around the last bucket's pack + all-reduce (reducer stream) and at the backward's end "
                        "(main stream); exposed = all-reduce end - backward end"}

    # ------------------------------------------------------------------------------------ api
    def step(self, batches: list[dict]) -> torch.Tensor:
        """One optimizer step over len(batches) == accumulate_grad_batches micro-batches.  Returns the
        device tensor [dur, prior, diff, total] (mean over micro-batches and ranks); nothing here
        synchronises with the host."""
        assert len(batches) == self.cfg.accumulate_grad_batches
        if self.watchdog is not None:
            self.watchdog.beat(step_enqueueing=self.global_step)
        logged = self._graph_step(batches) if self.cfg.graph else self._eager_step(batches)
        self.global_step += 1
        self.last_losses = logged
        if self.watchdog is not None:
            self.watchdog.beat(last_step_enqueued=self.global_step - 1)
        return logged

    def on_epoch_end(self):
        """CosineAnnealingLR(T_max=1000 epochs, eta_min=1e-6) stepped per epoch."""
        self.epoch += 1
        if self.scheduler is not None:
            self.scheduler.step()
        else:
            self.lr.fill_(self.cosine_lr(self.epoch))

    def cosine_lr(self, epoch: int) -> float:
        """The schedule's closed form after `epoch` epochs (graph mode's lr; load_checkpoint restores lr with it)."""
        c = self.cfg
        return c.eta_min + (c.lr - c.eta_min) * (1 + math.cos(math.pi * epoch / c.t_max_epochs)) / 2

    # ------------------------------------------------------------------------------------ validation
    VAL_NAMES = ("sub_loss/val_dur_loss", "sub_loss/val_prior_loss", "sub_loss/val_diff_loss", "loss/val")
    TRAIN_NAMES = ("sub_loss/train_dur_loss", "sub_loss/train_prior_loss", "sub_loss/train_diff_loss", "loss/train")

    def _val_losses(self, batch):
        """[dur, prior, diff, total] of one batch: the model's forward as the train step calls it (the batch's
        "t" / "z" / "out_offset" / "durations" injected) under the trainer's precision context.  out_size as
        get_losses applies it: TrainConfig.out_size, else the model's own."""
        out_size = self.cfg.out_size if self.cfg.out_size is not None else getattr(self.model, "out_size", None)
        return _total_and_logged(*self._losses(self.model, batch, out_size))[1]

    def _val_graph_step(self, batch):
        """validation_step on the GPU in graph mode: the forward captured once per input-shape key (an LRU of its
        own, TrainConfig.graph_cache entries: the train steps' captures are never evicted for it) and replayed
        from static input buffers.  No gradient deferral is open here, so MatchaTTS.forward takes no prefetch
        fork: the capture has one stream."""
        key = tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(batch.items()))

        def build():
            static = {k: v.clone() for k, v in batch.items()}
            return static, *G.capture(lambda: self._val_losses(static), self.dev, passes=2)

        static, g, out = self._val_graphs.lookup(key, build)
        for k, v in static.items():
            if batch[k] is not v:
                v.copy_(batch[k], non_blocking=True)
        g.replay()
        return out.clone()  # the next replay overwrites the graph's own output

    def validation_step(self, batch: dict) -> torch.Tensor:
        """The reference's validation_step (baselightningmodule.py:164-202) on one batch: the device tensor
        [dur, prior, diff, total], computed under no_grad() with the model in eval() (dropout off, as
        Lightning's validation loop sets it; every module's ``training`` flag is put back afterwards).  Touches
        no parameter, gradient, optimizer state or global_step, and does not synchronise with the host."""
        mods = list(self.model.modules())
        flags = [m.training for m in mods]
        # (a forward records how many dropout seeds it drew, to size the next one's pool: the train step's stays)
        seeds = [(m, m.__dict__["_mtts_seed_count"]) for m in mods if "_mtts_seed_count" in m.__dict__]
        self.model.eval()
        try:
            with torch.no_grad():
                if self.cfg.graph and self.dev.type == "cuda":
                    return self._val_graph_step(batch)
                return self._val_losses(batch)
        finally:
            for m, f in zip(mods, flags):
                m.training = f
            for m, n in seeds:
                m.__dict__["_mtts_seed_count"] = n

    def validate(self, batches) -> dict:
        """The mean of validation_step over `batches` (and over ranks: the per-batch vectors are summed on the
        device, the sum reduced ONCE over ranks -- the reference's sync_dist=True in one collective --, one host
        sync at the end) under the reference's names: sub_loss/val_{dur,prior,diff}_loss and loss/val."""
        acc = torch.zeros(5, dtype=torch.float32, device=self.dev)  # four sums and the batch count
        for batch in batches:
            acc[:4] += self.validation_step(batch)
            acc[4] += 1
        if self.world > 1:
            dist.all_reduce(acc)
        *sums, n = acc.tolist()
        if n == 0:
            raise ValueError("validate: no batches")
        return {name: s / n for name, s in zip(self.VAL_NAMES, sums)}

    # ------------------------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path) -> None:
        """One file in Lightning's layout (matcha/checkpoint.py): model, optimizer state in torch.optim.AdamW's
        form (either mode), epoch, global_step, schedule, RNG states."""
        from matcha import checkpoint as CK

        CK.save(self, path)

    def load_checkpoint(self, path) -> dict:
        """Restores what save_checkpoint wrote, in place: in graph mode every address stays (flat parameter and
        moment arrays, step counter, lr scalar -- lr recomputed from the epoch by on_epoch_end's formula), so
        steps captured before the call stay valid; in eager mode the optimizer's and the scheduler's state_dict."""
        from matcha import checkpoint as CK

        ck = CK.load(self, path)
        best = ck.get("callbacks", {}).get("best_k_models")
        if best is not None:
            self._best_k = {str(k): float(v) for k, v in best.items()}
        return ck

    # ------------------------------------------------------------------------------------ fit
    def fit(self, train_batches, val_batches=None, *, max_epochs: int, ckpt_dir=None, save_top_k: int = 3,
            save_last: bool = True, resume=None, log_every_n_steps: int = 10) -> list[dict]:
        """The reference's loop (train.py:81-109 through Lightning's fit).  Per epoch: one step() per
        cfg.accumulate_grad_batches micro-batches of train_batches (a trailing incomplete group is dropped),
        then validate(val_batches), then on_epoch_end(), then the checkpoints in ckpt_dir:
        ``last-epoch=EE-step=S.ckpt`` (replacing the previous last) and ``best-epoch=EE-loss_val=0.123.ckpt``,
        of which the save_top_k with the lowest loss/val are kept (ModelCheckpoint(monitor="loss/val",
        save_top_k=3) + save_last=True).  EE is the epoch that just ended, counted from 0.

        train_batches / val_batches: a callable epoch -> iterable of batch dicts (a sampler's set_epoch goes
        there), or a re-iterable.  resume: a checkpoint path, or True for find_latest_checkpoint(ckpt_dir);
        training continues at the checkpoint's epoch.  The host waits for the device once every
        log_every_n_steps steps (the four train losses) and once per
        validation, never otherwise.  Every logged row is appended to the returned history and, with ckpt_dir,
        written to ckpt_dir/metrics.csv (by rank 0)."""
        import csv

        from matcha.checkpoint import find_latest_checkpoint

        rank0 = self.world == 1 or dist.get_rank() == 0
        if ckpt_dir is not None:
            ckpt_dir = os.fspath(ckpt_dir)
            os.makedirs(ckpt_dir, exist_ok=True)
        self._best_k = {}
        if resume:
            if resume is True and ckpt_dir is None:
                raise ValueError("fit(resume=True) looks for the latest checkpoint in ckpt_dir")
            path = find_latest_checkpoint(ckpt_dir) if resume is True else find_latest_checkpoint(checkpoint_path=resume)
            if path is not None:
                self.load_checkpoint(path)
        if ckpt_dir is not None:  # best files that are gone (or another directory's) no longer count
            self._best_k = {k: v for k, v in self._best_k.items() if os.path.exists(os.path.join(ckpt_dir, k))}
        history: list[dict] = []
        csv_path = os.path.join(ckpt_dir, "metrics.csv") if (ckpt_dir is not None and rank0) else None
        rows, fields = [], []
        if csv_path is not None and resume and os.path.exists(csv_path):
            with open(csv_path, newline="") as f:
                rd = csv.DictReader(f)
                rows, fields = list(rd), list(rd.fieldnames or [])

        def log(row):
            history.append(row)
            if csv_path is None:
                return
            rows.append(row)
            new = [k for k in row if k not in fields]
            if new or len(rows) == 1:  # a wider table: written again from the start
                fields.extend(new)
                with open(csv_path, "w", newline="") as f:
                    w = csv.DictWriter(f, fieldnames=fields)
                    w.writeheader()
                    w.writerows(rows)
            else:
                with open(csv_path, "a", newline="") as f:
                    csv.DictWriter(f, fieldnames=fields).writerow(row)

        def batches_of(src, epoch):
            return src(epoch) if callable(src) else src

        last = None
        if ckpt_dir is not None:
            olds = sorted(f for f in os.listdir(ckpt_dir) if f.startswith("last-") and f.endswith(".ckpt"))
            last = os.path.join(ckpt_dir, olds[-1]) if olds else None
        n_acc = self.cfg.accumulate_grad_batches
        while self.epoch < max_epochs:
            epoch = self.epoch
            micro = []
            for batch in batches_of(train_batches, epoch):
                micro.append(batch)
                if len(micro) < n_acc:
                    continue
                logged = self.step(micro)
                micro = []
                if log_every_n_steps and self.global_step % log_every_n_steps == 0:
                    row = {"epoch": epoch, "step": self.global_step, **dict(zip(self.TRAIN_NAMES, logged.tolist()))}
                    log(row)
            val = None
            if val_batches is not None:
                val = self.validate(batches_of(val_batches, epoch))
                log({"epoch": epoch, "step": self.global_step, **val})
            self.on_epoch_end()
            if ckpt_dir is None:
                continue
            if val is not None and save_top_k:
                name = f"best-epoch={epoch:02d}-loss_val={val['loss/val']:.3f}.ckpt"
                ranked = sorted(list(self._best_k.items()) + [(name, val["loss/val"])], key=lambda kv: kv[1])
                keep = dict(ranked[:save_top_k] if save_top_k > 0 else ranked)
                dropped = [k for k in self._best_k if k not in keep]
                self._best_k = keep
                if name in keep:
                    self.save_checkpoint(os.path.join(ckpt_dir, name))
                if rank0:
                    for k in dropped:
                        with contextlib.suppress(FileNotFoundError):
                            os.remove(os.path.join(ckpt_dir, k))
            if save_last:
                path = os.path.join(ckpt_dir, f"last-epoch={epoch:02d}-step={self.global_step}.ckpt")
                self.save_checkpoint(path)
                if rank0 and last is not None and last != path:
                    with contextlib.suppress(FileNotFoundError):
                        os.remove(last)
                last = path
        return history
