"""Monotonic Alignment Search on the GPU (drop-in for matcha/utils/monotonic_align/__init__.py).

Reference: /root/reference/matcha/utils/monotonic_align/__init__.py:40-55 copies the lattice to the
host, runs the Cython Viterbi (core.pyx:16-128) on CPU threads and copies the path back -- a
device->host->device round trip and a stream synchronisation in the middle of every forward pass.
Here the whole thing stays on the stream: ``mtts_maximum_path_f32`` (csrc/mas.hip) reads the fp32
lattice and mask in HBM and writes the dense path; nothing synchronises with the host.

Parity: bit-identical paths to the compiled Cython for 1 <= t_x <= t_y (the reference's pure-Python
fallback, __init__.py:8-37, uses the opposite tie rule and is NOT the parity target).
"""
from __future__ import annotations

import math

import torch

from matcha import _native as N


def _check_tx(Tx: int, limit: int | None = None) -> None:
    """The DP keeps one utterance's text rows in one workgroup's registers (8 waves x 16 rows per lane at
    most, csrc/mas.hip mas_dp_mw_kernel): t_x <= 8192 (round 6; 4096 before), and 4096 for the row-major
    lattice compute_batch_alignments mutates.  The reference Cython (core.pyx:14-96) has no cap; LJSpeech tops
    out near 190 tokens and BASELINE config 5 uses 512, so the limit is a documented shape error, not a silent
    truncation."""
    limit = N.MTTS_MAS_MAX_TX if limit is None else limit
    if Tx > limit:
        raise ValueError(f"maximum_path: text length {Tx} exceeds the GPU kernel's limit of "
                         f"{limit} rows (MTTS_MAS_MAX_TX{'' if limit == N.MTTS_MAS_MAX_TX else '_ROW_MAJOR'}, "
                         f"include/mtts.h)")


def _workspace(B: int, Tx: int, Ty: int, device) -> torch.Tensor:
    nbytes = int(N.lib().mtts_maximum_path_workspace_size(B, Tx, Ty))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def maximum_path(value: torch.Tensor, mask: torch.Tensor, *, return_row_start: bool = False):
    """value, mask: [b, t_x, t_y]  ->  path [b, t_x, t_y] in value's dtype, on value's device.

    Same contract as the reference (__init__.py:40-55): the DP runs on value*mask in fp32,
    t_x = mask.sum(1)[:, 0], t_y = mask.sum(2)[:, 0]; the caller's tensors are not modified.
    With ``return_row_start`` also returns int32 [b, t_x] first-column-per-row (-1 = no path) and
    int32 [b, 2] lengths, which consumers (durations, mu_y gather) use instead of the dense path.
    """
    N.require_device(value, mask)
    if value.dim() != 3 or mask.shape != value.shape:
        raise ValueError(f"maximum_path expects value and mask of the same [b, t_x, t_y] shape, "
                         f"got {tuple(value.shape)} and {tuple(mask.shape)}")
    out_dtype = value.dtype
    flags = 0
    if value.dtype != torch.float32:
        # reference: value*mask in torch's promoted dtype, then .astype(np.float32) (__init__.py:45,48)
        value = (value * mask).to(torch.float32)
        flags |= N.MTTS_MAS_VALUE_PREMASKED
    if mask.dtype != torch.float32:
        mask = mask.to(torch.float32)
    value = value.contiguous()
    mask = mask.contiguous()
    B, Tx, Ty = value.shape
    _check_tx(Tx)
    dev = value.device
    path = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev)
    row_start = torch.empty((B, Tx), dtype=torch.int32, device=dev) if return_row_start else None
    lengths = torch.empty((B, 2), dtype=torch.int32, device=dev) if return_row_start else None
    ws = _workspace(B, Tx, Ty, dev)
    with torch.cuda.device(dev):
        rc = N.lib().mtts_maximum_path_f32(
            N.ptr(value), N.ptr(mask), N.ptr(path), B, Tx, Ty, flags, N.ptr(lengths),
            N.ptr(row_start), N.ptr(ws), ws.numel(), N.stream_handle(dev))
    N.check(rc, "mtts_maximum_path_f32")
    if out_dtype != torch.float32:
        path = path.to(out_dtype)
    if return_row_start:
        return path, row_start, lengths
    return path


def maximum_path_c(paths: torch.Tensor, values: torch.Tensor, t_xs: torch.Tensor,
                   t_ys: torch.Tensor, max_neg_val: float = -1e9) -> None:
    """Device twin of core.compute_batch_alignments (core.pyx:101-128), bound as maximum_path_c.

    paths int32 [b,t_x,t_y] (ones are set on the path, other entries untouched), values float32
    [b,t_x,t_y] (mutated in place to the DP lattice exactly like the Cython), t_xs/t_ys int32 [b].
    """
    N.require_device(paths, values, t_xs, t_ys)
    if paths.dtype != torch.int32 or values.dtype != torch.float32:
        raise TypeError("maximum_path_c expects int32 paths and float32 values (as the Cython)")
    if not (paths.is_contiguous() and values.is_contiguous()):
        raise ValueError("maximum_path_c mutates its arguments in place: they must be C-contiguous")
    B, Tx, Ty = values.shape
    _check_tx(Tx, N.MTTS_MAS_MAX_TX_ROW_MAJOR)
    t_xs = t_xs.to(torch.int32).contiguous()
    t_ys = t_ys.to(torch.int32).contiguous()
    dev = values.device
    ws = _workspace(B, Tx, Ty, dev)
    with torch.cuda.device(dev):
        rc = N.lib().mtts_compute_batch_alignments(
            N.ptr(paths), N.ptr(values), N.ptr(t_xs), N.ptr(t_ys), B, Tx, Ty, float(max_neg_val),
            N.ptr(ws), ws.numel(), N.stream_handle(dev))
    N.check(rc, "mtts_compute_batch_alignments")


# the reference binds the compiled core as maximum_path_c (__init__.py:4-5)
compute_batch_alignments = maximum_path_c


def prior_maximum_path(mu_x: torch.Tensor, y: torch.Tensor, x_lengths: torch.Tensor, y_lengths: torch.Tensor, *,
                       return_lattice: bool = False, dense: bool = True):
    """The training forward's alignment step fused (matcha_tts.py:276-288, MatchaTTS.forward):
    log-prior lattice from mu_x [B,C,Tx] and y [B,C,Ty] (fp32), masked by the length masks, Viterbi
    max path, and the duration target -- one lattice write to HBM instead of two bmm's, their
    elementwise tail, the [B,Tx,Ty] attention mask and a reduction over the dense path
    (csrc/mas.hip: log_prior_kernel -> mas_dp_kernel -> mas_expand_kernel / mas_runs_kernel).

    Returns (attn [B,Tx,Ty] fp32, dur [B,Tx] fp32 = attn.sum(-1), col_row [B,Ty] int32 = text row of
    each frame (-1 past t_y), row_start [B,Tx] int32, lengths [B,2] int32) and, with
    ``return_lattice``, the masked fp32 lattice [B,Tx,Ty] the DP ran on.  No gradient.
    ``dense=False`` skips the dense path (attn is None: the C entry's optional ``path``, one launch and a
    [B,Tx,Ty] write less) for consumers that read the runs only (segment_crop); nothing else changes."""
    N.require_device(mu_x, y, x_lengths, y_lengths)
    if mu_x.dim() != 3 or y.dim() != 3 or mu_x.shape[:2] != y.shape[:2]:
        raise ValueError(f"prior_maximum_path expects mu_x [B,C,Tx] and y [B,C,Ty], got {tuple(mu_x.shape)}, "
                         f"{tuple(y.shape)}")
    mu_x = mu_x.detach().to(torch.float32).contiguous()
    y = y.detach().to(torch.float32).contiguous()
    xl = x_lengths.detach().to(torch.int64).contiguous()
    yl = y_lengths.detach().to(torch.int64).contiguous()
    B, C, Tx = mu_x.shape
    _check_tx(Tx)
    Ty = y.shape[2]
    dev = mu_x.device
    attn = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if dense else None
    dur = torch.empty((B, Tx), dtype=torch.float32, device=dev)
    col_row = torch.empty((B, Ty), dtype=torch.int32, device=dev)
    row_start = torch.empty((B, Tx), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, 2), dtype=torch.int32, device=dev)
    lattice = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if return_lattice else None
    ws = torch.empty(max(int(N.lib().mtts_prior_maximum_path_workspace_size(B, Tx, Ty)), 1), dtype=torch.uint8,
                     device=dev)
    with torch.cuda.device(dev):
        rc = N.lib().mtts_prior_maximum_path(
            N.ptr(mu_x), N.ptr(y), N.ptr(xl), N.ptr(yl), B, C, Tx, Ty, N.ptr(attn), N.ptr(lengths), N.ptr(row_start),
            N.ptr(dur), N.ptr(col_row), N.ptr(lattice), N.ptr(ws), ws.numel(), N.stream_handle(dev))
    N.check(rc, "mtts_prior_maximum_path")
    out = (attn, dur, col_row, row_start, lengths)
    return out + (lattice,) if return_lattice else out


def duration_runs_host(d, t_x: int, t_y: int):
    """The device's duration rule restated in Python numbers (include/mtts.h, mtts_duration_path): for one
    utterance's durations ``d`` (a sequence of Tx numbers), t_x <= Tx text rows and t_y frames, returns
    (row_start [Tx], dur [Tx], col_row [t_y], t_cov).  Row x < t_x covers the frames [e_x, e_{x+1}) with
    e_x = min(ceil(c_x), t_y) and c the float64 running sum of max(d, 0) (NaN counts as 0); -1 / 0 past t_x;
    col_row is -1 from t_cov = e_{t_x} on.  It is generate_path(d, x_mask * y_mask) (utils/model.py) on runs."""
    Tx = len(d)
    t_x, t_y = min(max(int(t_x), 0), Tx), max(int(t_y), 0)
    c, e = 0.0, [0]
    for x in range(t_x):
        v = float(d[x])
        c += v if v > 0 else 0.0
        e.append(int(math.ceil(min(c, float(t_y)))))  # = min(ceil(c), t_y): t_y is an integer
    row_start = e[:t_x] + [-1] * (Tx - t_x)
    dur = [e[x + 1] - e[x] for x in range(t_x)] + [0] * (Tx - t_x)
    col_row = [-1] * t_y
    for x in range(t_x):
        col_row[e[x]:e[x + 1]] = [x] * (e[x + 1] - e[x])
    return row_start, dur, col_row, e[t_x]


def duration_path(durations: torch.Tensor, x_lengths: torch.Tensor, y_lengths: torch.Tensor, Ty: int, *,
                  dense: bool = True):
    """The alignment of precomputed durations (matcha_tts.py:273-274, use_precomputed_durations=True) as runs:
    generate_path(durations, x_mask * y_mask) and its sum(-1) without the cumsum, the [B*Tx, Ty] mask and the
    elementwise passes over [B,Tx,Ty] (csrc/mas.hip: duration_path_kernel -> mas_expand_kernel); the rule is
    duration_runs_host's.

    durations [B,Tx] or [B,1,Tx], any real or integer dtype (converted to fp32); x_lengths, y_lengths [B]; ``Ty``
    the padded mel length.  Returns (attn [B,Tx,Ty] fp32, dur [B,Tx] fp32 = attn.sum(-1), col_row [B,Ty] int32,
    row_start [B,Tx] int32, lengths [B,2] int32 = (t_x, t_y), run_lengths [B,2] int32 = (t_x, t_cov)): the
    durations need not cover t_y frames, so the last row's run ends at t_cov.  expand_rows and the backward of
    segment_crop take run_lengths; segment_crop's forward windows on lengths.  ``dense=False``: attn is None and
    the [B,Tx,Ty] write is skipped.  No gradient, no host sync."""
    N.require_device(durations, x_lengths, y_lengths)
    if durations.dim() == 3 and durations.shape[1] == 1:
        durations = durations[:, 0]
    if durations.dim() != 2 or durations.is_complex() or durations.dtype == torch.bool:
        raise ValueError(f"duration_path expects real durations [B,Tx] or [B,1,Tx], got {tuple(durations.shape)} "
                         f"{durations.dtype}")
    B, Tx = durations.shape
    Ty = int(Ty)
    if tuple(x_lengths.shape) != (B,) or tuple(y_lengths.shape) != (B,):
        raise ValueError(f"duration_path: x_lengths / y_lengths must be [B] = [{B}], got {tuple(x_lengths.shape)}, "
                         f"{tuple(y_lengths.shape)}")
    if Tx < 1 or Ty < 1:
        raise ValueError(f"duration_path: empty shape Tx={Tx}, Ty={Ty}")
    _check_tx(Tx)
    d = durations.detach().to(torch.float32).contiguous()
    xl = x_lengths.detach().to(torch.int64).contiguous()
    yl = y_lengths.detach().to(torch.int64).contiguous()
    dev = d.device
    attn = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if dense else None
    dur = torch.empty((B, Tx), dtype=torch.float32, device=dev)
    col_row = torch.empty((B, Ty), dtype=torch.int32, device=dev)
    row_start = torch.empty((B, Tx), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, 2), dtype=torch.int32, device=dev)
    run_lengths = torch.empty((B, 2), dtype=torch.int32, device=dev)
    if B == 0:
        return attn, dur, col_row, row_start, lengths, run_lengths
    with torch.cuda.device(dev):
        rc = N.lib().mtts_duration_path(N.ptr(d), N.ptr(xl), N.ptr(yl), B, Tx, Ty, N.ptr(attn), N.ptr(lengths),
                                        N.ptr(run_lengths), N.ptr(row_start), N.ptr(dur), N.ptr(col_row),
                                        N.stream_handle(dev))
    N.check(rc, "mtts_duration_path")
    return attn, dur, col_row, row_start, lengths, run_lengths


class _ExpandRows(torch.autograd.Function):
    """mu_y = attn^T @ mu_x for a hard alignment (matcha_tts.py:314-315) as a gather of mu_x columns;
    backward sums each text row's run of frames (deterministic segment sums, no atomics)."""

    @staticmethod
    def forward(ctx, mu_x, col_row, row_start, lengths):
        mu_x = mu_x.to(torch.float32).contiguous()
        B, C, Tx = mu_x.shape
        Ty = col_row.shape[1]
        out = torch.empty((B, C, Ty), dtype=torch.float32, device=mu_x.device)
        N.check(N.lib().mtts_expand_rows_fwd(N.ptr(mu_x), N.ptr(col_row), B, C, Tx, Ty, N.ptr(out),
                                             N.stream_handle(mu_x.device)), "mtts_expand_rows_fwd")
        ctx.save_for_backward(row_start, lengths)
        ctx.shape = (B, C, Tx, Ty)
        return out

    @staticmethod
    def backward(ctx, dy):
        row_start, lengths = ctx.saved_tensors
        B, C, Tx, Ty = ctx.shape
        dy = dy.to(torch.float32).contiguous()
        dx = torch.empty((B, C, Tx), dtype=torch.float32, device=dy.device)
        N.check(N.lib().mtts_expand_rows_bwd(N.ptr(dy), N.ptr(row_start), N.ptr(lengths), B, C, Tx, Ty, N.ptr(dx),
                                             N.stream_handle(dy.device)), "mtts_expand_rows_bwd")
        return dx, None, None, None


def expand_rows(mu_x: torch.Tensor, col_row: torch.Tensor, row_start: torch.Tensor, lengths: torch.Tensor):
    """[B,C,Tx] -> [B,C,Ty]: attn^T @ mu_x for the alignment prior_maximum_path returned (bitwise
    equal to the bmm on the one-hot attn: every other term is 0 * finite)."""
    N.require_device(mu_x, col_row, row_start, lengths)
    return _ExpandRows.apply(mu_x, col_row, row_start, lengths)


def segment_offset_host(word: int, t_y: int, out_size: int) -> tuple[int, int]:
    """The device's window rule restated in Python integers (include/mtts.h, mtts_segment_crop_fwd): for a
    31-bit random word, (offset, cut_len) of an utterance of t_y frames cropped to out_size.  The offset is
    uniform on [0, max_off) with max_off = max(t_y - out_size, 0): max_off itself is never drawn and
    max_off <= 1 gives 0, as the reference's random.choice(range(0, max_offset)) (matcha_tts.py:292-295)."""
    max_off = max(int(t_y) - int(out_size), 0)
    return ((int(word) & 0x7FFFFFFF) * max_off) >> 31, min(max(int(t_y), 0), int(out_size))


class _SegmentCrop(torch.autograd.Function):
    """mtts_segment_crop_fwd / _bwd: the window of y, of mu_y = attn^T @ mu_x and of attn in one launch; the
    backward sums each text row's frames inside the window in expand_rows' order (bitwise equal to its backward
    on the zero-padded full-length gradient)."""

    @staticmethod
    def forward(ctx, mu_x, y, col_row, row_start, lengths, out_size, offsets, words, want_attn, run_lengths):
        ctx.in_dtype = mu_x.dtype
        mu_x = mu_x.to(torch.float32).contiguous()
        B, C, Tx = mu_x.shape
        Ty, S, dev = y.shape[2], int(out_size), mu_x.device
        y_cut = torch.empty((B, C, S), dtype=torch.float32, device=dev)
        mu_y_cut = torch.empty((B, C, S), dtype=torch.float32, device=dev)
        attn_cut = torch.empty((B, Tx, S), dtype=torch.float32, device=dev) if want_attn else None
        mask = torch.empty((B, 1, S), dtype=torch.float32, device=dev)
        seg = torch.empty((B, 2), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            N.check(N.lib().mtts_segment_crop_fwd(
                N.ptr(y), N.ptr(mu_x), N.ptr(col_row), N.ptr(lengths), N.ptr(words), N.ptr(offsets), B, C, Tx, Ty, S,
                N.ptr(y_cut), N.ptr(mu_y_cut), N.ptr(attn_cut), N.ptr(mask), N.ptr(seg), N.stream_handle(dev)),
                "mtts_segment_crop_fwd")
        # the backward ends the last row's run at run_lengths' frame count (duration_path: t_cov <= t_y)
        ctx.save_for_backward(row_start, run_lengths, seg)
        ctx.shape = (B, C, Tx, S)
        ctx.mark_non_differentiable(*(t for t in (y_cut, attn_cut, mask, seg) if t is not None))
        return y_cut, mu_y_cut, attn_cut, mask, seg

    @staticmethod
    def backward(ctx, _dy, d_mu_y, _dattn, _dmask, _dseg):
        row_start, lengths, seg = ctx.saved_tensors
        B, C, Tx, S = ctx.shape
        d_mu_y = d_mu_y.to(torch.float32).contiguous()
        dx = torch.empty((B, C, Tx), dtype=torch.float32, device=d_mu_y.device)
        with torch.cuda.device(d_mu_y.device):
            N.check(N.lib().mtts_segment_crop_bwd(N.ptr(d_mu_y), N.ptr(row_start), N.ptr(lengths), N.ptr(seg), B, C, Tx,
                                                  S, N.ptr(dx), N.stream_handle(d_mu_y.device)),
                    "mtts_segment_crop_bwd")
        return (dx.to(ctx.in_dtype),) + (None,) * 9


def segment_crop(y: torch.Tensor, mu_x: torch.Tensor, col_row: torch.Tensor, row_start: torch.Tensor,
                 lengths: torch.Tensor, out_size: int, *, offsets: torch.Tensor | None = None,
                 words: torch.Tensor | None = None, want_attn: bool = True,
                 run_lengths: torch.Tensor | None = None):
    """The reference's random mel segment (matcha_tts.py:290-315, forward(out_size=...)) on the device, for the
    alignment prior_maximum_path returned: every utterance is cut to a window of ``out_size`` frames.

    y [B,C,Ty], mu_x [B,C,Tx] -> (y_cut [B,C,S], mu_y_cut [B,C,S] = the window of attn^T @ mu_x, attn_cut
    [B,Tx,S] (None with ``want_attn=False``), y_mask [B,1,S], seg int32 [B,2] = (offset, cut_len)), zeros past
    cut_len = min(t_y, S).  The gradient goes to mu_x only; y is data.
    ``offsets`` (int tensor [B]) injects the windows, clamped on the device to [0, max(t_y - S, 0)].  Otherwise
    one 31-bit word per utterance is drawn ON THE DEVICE from torch's generator (no host sync; a replayed HIP
    graph draws fresh windows) and mapped by segment_offset_host's rule; ``words`` (int32 [B], tests) gives
    the words instead.  ``run_lengths`` (int32 [B,2], duration_path's (t_x, t_cov); default: ``lengths``) is what
    the backward ends the last row's run at; the forward's window is drawn on ``lengths``."""
    N.require_device(y, mu_x, col_row, row_start, lengths, offsets, words, run_lengths)
    if mu_x.dim() != 3 or y.dim() != 3 or mu_x.shape[:2] != y.shape[:2]:
        raise ValueError(f"segment_crop expects y [B,C,Ty] and mu_x [B,C,Tx], got {tuple(y.shape)}, "
                         f"{tuple(mu_x.shape)}")
    B, Ty = y.shape[0], y.shape[2]
    if not 1 <= int(out_size) <= Ty:
        raise ValueError(f"segment_crop: out_size {out_size} outside [1, {Ty}] (the padded mel length)")
    if tuple(col_row.shape) != (B, Ty) or tuple(row_start.shape) != (B, mu_x.shape[2]) or \
            tuple(lengths.shape) != (B, 2):
        raise ValueError("segment_crop: col_row / row_start / lengths are not this batch's alignment")
    if run_lengths is None:
        run_lengths = lengths
    elif tuple(run_lengths.shape) != (B, 2) or run_lengths.dtype != torch.int32:
        raise ValueError(f"segment_crop: run_lengths must be int32 [B,2] = [{B},2]")
    y = y.detach().to(torch.float32).contiguous()
    if offsets is not None:
        if tuple(offsets.shape) != (B,):
            raise ValueError(f"segment_crop: offsets must be [B] = [{B}], got {tuple(offsets.shape)}")
        offsets = offsets.detach().to(torch.int32).contiguous()
        words = None
    elif words is not None:
        if tuple(words.shape) != (B,) or words.dtype != torch.int32:
            raise ValueError(f"segment_crop: words must be int32 [B] = [{B}]")
        words = words.contiguous()
    else:
        words = torch.randint(0, 2 ** 31 - 1, (B,), device=y.device, dtype=torch.int32)
    return _SegmentCrop.apply(mu_x, y, col_row.contiguous(), row_start.contiguous(), lengths.contiguous(),
                              int(out_size), offsets, words, want_attn, run_lengths.contiguous())
