"""Random mel segments on the device (MatchaTTS.forward(out_size=...), matcha_tts.py:290-315 of the reference):
the crop op (csrc/mas.hip segment_crop_fwd_kernel / the windowed expand_rows_bwd_kernel) against torch
restatements written here, bitwise; the device draw against the host's integer rule; the model against the CPU
oracle's pieces cropped with torch; the Trainer's captured step.

Bars: forward outputs and the backward's sums bit-exact (the backward against expand_rows' backward on the
zero-padded full-length gradient: the summation-order contract of include/mtts.h); losses at
test_headline_gpu's FP32_LOSS_RTOL / PARITY_RTOL."""
from __future__ import annotations

import collections
import math
import random

import numpy as np
import pytest
import torch

from test_headline_gpu import FP32_LOSS_RTOL, PARITY_RTOL, run_precision
from test_segment_cpu import HIST_HI, HIST_LO, HIST_MAX_OFF, hist_words

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 3


# ------------------------------------------------------------------------------------------ helpers
def _runs_from_durations(durs: list[list[int]], Tx: int, Ty: int):
    """Hand-written alignments: durs[b] = frames per text row -> (col_row [B,Ty], row_start [B,Tx], lengths
    [B,2], dense attn [B,Tx,Ty]) as prior_maximum_path writes them."""
    B = len(durs)
    col_row = torch.full((B, Ty), -1, dtype=torch.int32)
    row_start = torch.full((B, Tx), -1, dtype=torch.int32)
    lengths = torch.zeros((B, 2), dtype=torch.int32)
    attn = torch.zeros((B, Tx, Ty))
    for b, d in enumerate(durs):
        pos = 0
        for x, n in enumerate(d):
            row_start[b, x] = pos
            col_row[b, pos:pos + n] = x
            attn[b, x, pos:pos + n] = 1.0
            pos += n
        lengths[b, 0], lengths[b, 1] = len(d), pos
    return col_row.to(DEV), row_start.to(DEV), lengths.to(DEV), attn.to(DEV)


def _clamped(offsets, t_y, S):
    return [min(max(int(o), 0), max(int(t) - S, 0)) for o, t in zip(offsets, t_y)]


def _torch_crop(y, mu_x, attn, t_y, offsets, S):
    """The reference's crop (matcha_tts.py:296-315) restated with torch slices on the dense one-hot attn."""
    B, Cc, _ = y.shape
    y_cut = torch.zeros(B, Cc, S, device=y.device)
    attn_cut = torch.zeros(B, attn.shape[1], S, device=y.device)
    mask = torch.zeros(B, 1, S, device=y.device)
    seg = []
    for b, (ty, off) in enumerate(zip(t_y, offsets)):
        L = min(int(ty), S)
        y_cut[b, :, :L] = y[b, :, off:off + L]
        attn_cut[b, :, :L] = attn[b, :, off:off + L]
        mask[b, :, :L] = 1.0
        seg.append([off, L])
    mu_y = torch.matmul(attn_cut.transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
    return y_cut, mu_y, attn_cut, mask, torch.tensor(seg, dtype=torch.int32, device=y.device)


def _mas_case(Tx, Ty, xl, yl, seed):
    from matcha.utils.monotonic_align import prior_maximum_path

    g = torch.Generator().manual_seed(seed)
    B = len(xl)
    mu = torch.randn(B, C, Tx, generator=g).to(DEV)
    y = torch.randn(B, C, Ty, generator=g).to(DEV)
    attn, _, col_row, rs, lens = prior_maximum_path(mu, y, torch.tensor(xl, device=DEV), torch.tensor(yl, device=DEV))
    return mu, y, attn, col_row, rs, lens


def _check_forward(mu, y, attn, col_row, rs, lens, t_y, offsets, S):
    from matcha.utils.monotonic_align import segment_crop

    got = segment_crop(y, mu, col_row, rs, lens, S, offsets=torch.tensor(offsets, device=DEV))
    want = _torch_crop(y, mu, attn, t_y, _clamped(offsets, t_y, S), S)
    torch.cuda.synchronize()
    for name, a, b in zip(("y_cut", "mu_y_cut", "attn_cut", "y_mask", "seg"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------ 1, 2: forward
T_Y = [50, 16, 17, 9, 33, 50]


@pytest.mark.parametrize("Tx,S", [(7, 16), (7, 37), (1, 16)])
def test_forward_bitwise_vs_torch_crop(Tx, S):
    """S=16: 16-byte stores, offset 3 = a misaligned source row, t_y = 9 < S, t_y = S, t_y = S + 1 (max_off 1);
    S=37: odd S, the scalar tail stores (offset 34 clamps to 13 there); Tx=1: one row owns every frame."""
    xl = [min(Tx, t) for t in (7, 7, 5, 3, 7, 1)]
    case = _mas_case(Tx, 50, xl, T_Y, seed=11)
    _check_forward(*case, T_Y, [34, 0, 0, 0, 5, 3], S)


def test_out_of_range_offsets_clamp_on_the_device():
    from matcha.utils.monotonic_align import segment_crop

    mu, y, attn, col_row, rs, lens = _mas_case(7, 50, [7, 7, 5, 3, 7, 1], T_Y, seed=12)
    offsets = [-5, 16, -5, 9, 33, 50]  # -5 and t_y
    _check_forward(mu, y, attn, col_row, rs, lens, T_Y, offsets, 16)
    seg = segment_crop(y, mu, col_row, rs, lens, 16, offsets=torch.tensor(offsets, device=DEV))[4]
    assert seg.tolist() == [[0, 16], [0, 16], [0, 16], [0, 9], [17, 16], [34, 16]]


# ------------------------------------------------------------------------------------------ 3: backward
def _check_backward(durs, Tx, Ty, S, offsets, seed, zero_rows=()):
    from matcha.utils.monotonic_align import expand_rows, segment_crop

    col_row, rs, lens, attn = _runs_from_durations(durs, Tx, Ty)
    B = len(durs)
    t_y = [sum(d) for d in durs]
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, C, Tx, generator=g).to(DEV)
    y = torch.randn(B, C, Ty, generator=g).to(DEV)
    d = torch.randn(B, C, S, generator=g).to(DEV)  # nonzero past cut_len too: the kernel must not read it
    a = mu.clone().requires_grad_(True)
    out = segment_crop(y, a, col_row, rs, lens, S, offsets=torch.tensor(offsets, device=DEV))
    out[1].backward(d)
    # the contract: expand_rows' backward on the full-length gradient, zero outside the window
    dy = torch.zeros(B, C, Ty, device=DEV)
    for b, (ty, off) in enumerate(zip(t_y, offsets)):
        L = min(ty, S)
        dy[b, :, off:off + L] = d[b, :, :L]
    r = mu.clone().requires_grad_(True)
    expand_rows(r, col_row, rs, lens).backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(a.grad, r.grad)
    for b, x in zero_rows:
        assert (a.grad[b, :, x] == 0).all(), (b, x)
    # and the matmul path's gradient in float64, at test_mas_gpu's expand_rows bar (1e-6 of the largest entry)
    gref = torch.matmul(dy.double(), attn.double().transpose(1, 2))
    err = (a.grad.double() - gref).abs().max().item() / gref.abs().max().item()
    assert err < 1e-6, err
    assert a.grad.abs().max().item() > 0


def test_backward_bitwise_vs_expand_rows_on_padded_gradient():
    """Ty = 50, S = 16, rows of 10, 8, 2, 20, 6, 4 frames: window [5, 21) cuts row 0 at its start and row 3 at its
    end (rows 4, 5 wholly outside: gradient exactly 0); window [22, 38) lies inside row 3 (20 frames > S: the run
    is cut at both ends and covers the whole window; every other row is 0); window [34, 50) is the last one;
    utterance 3 is shorter than S (cut_len = 9)."""
    durs = [[10, 8, 2, 20, 6, 4]] * 3 + [[3, 3, 3]]
    zero = [(0, 4), (0, 5), (1, 0), (1, 1), (1, 2), (1, 4), (1, 5), (2, 0), (2, 1), (2, 2), (3, 3), (3, 4), (3, 5)]
    _check_backward(durs, 6, 50, 16, [5, 22, 34, 0], seed=21, zero_rows=zero)


def test_backward_crosses_the_4096_frame_slab():
    """B = 2, Ty = 4200, S = 4100: the window spans both slabs of the full-length frame axis and a row's run
    crosses frame 4096 (rows [3100, 4100) and [2000, 4150)); the slab partial sums add in the full kernel's order."""
    durs = [[100, 3000, 1000, 50, 50], [2000, 2150, 20, 20, 10]]
    _check_backward(durs, 5, 4200, 4100, [37, 100], seed=22)


# ------------------------------------------------------------------------------------------ 4: device draw
def _draw_case():
    S, B = 16, 2048
    col_row, rs, lens, _ = _runs_from_durations([[12, 12]], 2, S + HIST_MAX_OFF)
    g = torch.Generator().manual_seed(31)
    mu = torch.randn(B, 2, 2, generator=g).to(DEV)
    y = torch.randn(B, 2, S + HIST_MAX_OFF, generator=g).to(DEV)
    return S, y, mu, col_row.expand(B, -1).contiguous(), rs.expand(B, -1).contiguous(), lens.expand(B, -1).contiguous()


def _check_hist(offs: np.ndarray):
    assert offs.min() >= 0 and offs.max() <= HIST_MAX_OFF - 1, (offs.min(), offs.max())  # offset 8 never appears
    bins = np.bincount(offs, minlength=HIST_MAX_OFF)
    assert ((bins >= HIST_LO) & (bins <= HIST_HI)).all(), bins


def test_device_offsets_equal_the_host_rule():
    from matcha.utils.monotonic_align import segment_crop, segment_offset_host

    S, y, mu, col_row, rs, lens = _draw_case()
    words = hist_words()
    out = segment_crop(y, mu, col_row, rs, lens, S, words=torch.from_numpy(words.astype(np.int32)).to(DEV))
    seg = out[4].cpu().numpy()
    want = np.array([segment_offset_host(int(w), S + HIST_MAX_OFF, S) for w in words])
    np.testing.assert_array_equal(seg, want)
    _check_hist(seg[:, 0])
    b = int(np.argmax(seg[:, 0]))  # the data follows the drawn window
    assert torch.equal(out[0][b], y[b, :, seg[b, 0]:seg[b, 0] + S])


def test_device_draw_from_torch_generator():
    """No words given: one 31-bit word per utterance from torch's device generator; two calls draw different
    windows, both uniform on [0, max_off)."""
    from matcha.utils.monotonic_align import segment_crop

    S, y, mu, col_row, rs, lens = _draw_case()
    torch.manual_seed(5)
    s1 = segment_crop(y, mu, col_row, rs, lens, S)[4].cpu().numpy()
    s2 = segment_crop(y, mu, col_row, rs, lens, S)[4].cpu().numpy()
    assert (s1[:, 1] == S).all() and (s2[:, 1] == S).all()
    _check_hist(s1[:, 0])
    _check_hist(s2[:, 0])
    assert (s1[:, 0] != s2[:, 0]).any()


# ------------------------------------------------------------------------------------------ 5: model
M_B, M_TX, M_TY, M_S = 4, 20, 160, 64
M_XL, M_YL = [20, 15, 18, 12], [160, 120, 50, 97]  # utterance 2 is shorter than the window
M_OFF = [96, 13, 0, 7]
_MODEL = {}


def _model_case():
    """Inputs, the product model and the reference losses / attn assembled ONCE from the CPU oracle's pieces: its
    encoder, its maximum_path on its own log-prior lattice, a torch crop at M_OFF, its decoder.compute_loss and the
    prior formula (matcha_tts.py:296-323)."""
    if _MODEL:
        return _MODEL
    import oracle_bind as OB
    from golden.weights_recipe import apply_recipe
    from matcha.models.matcha_tts import MatchaTTS
    from oracle import matcha_oracle as MO

    def omp(value, mask):
        p, _ = OB.maximum_path(value.detach().float().numpy(), mask.detach().float().numpy())
        return torch.from_numpy(p)

    g = torch.Generator().manual_seed(51)
    xl, yl = torch.tensor(M_XL), torch.tensor(M_YL)
    x = torch.randint(1, 150, (M_B, M_TX), generator=g) * (torch.arange(M_TX)[None] < xl[:, None])
    y = torch.randn(M_B, 80, M_TY, generator=g) * (torch.arange(M_TY)[None, None] < yl[:, None, None])
    t = torch.rand(M_B, 1, 1, generator=g)
    z = torch.randn(M_B, 80, M_S, generator=g)
    ref = MO.MatchaTTSOracle(150, 80, 192, maximum_path=omp)
    apply_recipe(ref, 9)
    ref.eval()
    with torch.no_grad():
        mu_x, logw, x_mask = ref.encoder(x, xl)
        y_mask = MO.sequence_mask(yl, M_TY).unsqueeze(1).to(x_mask)
        *_, log_prior = ref(x, xl, y, yl, return_log_prior=True)
        attn = ref._maximum_path(log_prior, (x_mask.unsqueeze(-1) * y_mask.unsqueeze(2)).squeeze(1))
        logw_ = torch.log(1e-8 + torch.sum(attn.unsqueeze(1), -1)) * x_mask
        dur = torch.sum((logw - logw_) ** 2) / torch.sum(xl)
        y_cut, mu_y, attn_cut, mask, _ = _torch_crop(y, mu_x, attn, M_YL, M_OFF, M_S)
        diff, _ = ref.decoder.compute_loss(x1=y_cut, mask=mask, mu=mu_y, t=t, z=z)
        prior = torch.sum(0.5 * ((y_cut - mu_y) ** 2 + math.log(2 * math.pi)) * mask) / (torch.sum(mask) * 80)
    model = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(DEV)
    apply_recipe(model, 9)
    model.eval()
    d = lambda v: v.to(DEV)  # noqa: E731
    _MODEL.update(model=model, args=(d(x), d(xl), d(y), d(yl)), t=d(t), z=d(z),
                  want=np.array([dur.item(), prior.item(), diff.item()]), attn=attn_cut)
    return _MODEL


def _run_model(case, precision, offsets, sync_error):
    model = case["model"]

    def fn():
        for p in model.parameters():
            p.grad = None
        if sync_error:  # no device->host copy anywhere in the forward
            if precision not in case.setdefault("warm", set()):
                # the whole-utterance forward fills the model's one-time caches (rotary tables, weight packs);
                # the crop itself first runs under the error mode
                with torch.no_grad():
                    model(*case["args"], t=case["t"])
                case["warm"].add(precision)
            torch.cuda.set_sync_debug_mode("error")
        try:
            kw = {} if offsets is None else {"out_offset": offsets}
            dur, prior, diff, attn = model(*case["args"], out_size=M_S, t=case["t"], z=case["z"], **kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        (dur + prior + diff).backward()
        return dur, prior, diff, attn

    dur, prior, diff, attn = run_precision(model, precision, fn)
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    return np.array([dur.item(), prior.item(), diff.item()]), attn.detach().cpu()


@pytest.mark.parametrize("precision", ["32-true", "bf16-parity"])
def test_model_injected_offsets_vs_oracle_pieces(precision):
    case = _model_case()
    got, attn = _run_model(case, precision, torch.tensor(M_OFF, device=DEV), sync_error=True)
    err = np.abs(got - case["want"]) / np.abs(case["want"])
    print(f"{precision}: losses {got} oracle pieces {case['want']} rel err {err}")
    assert attn.shape == (M_B, M_TX, M_S)
    if precision == "32-true":
        assert torch.equal(attn, case["attn"])
        assert (err <= FP32_LOSS_RTOL).all(), err
    else:
        assert (err <= PARITY_RTOL).all(), err
    assert case["model"].last_seg.tolist() == [[o, min(t, M_S)] for o, t in zip(M_OFF, M_YL)]


@pytest.mark.parametrize("precision", ["32-true", "bf16-parity"])
def test_model_device_crop_vs_host_crop(precision, monkeypatch):
    """MTTS_SEGMENT_HOST=1 keeps the reference's host-side crop (Python's random, the dense attn matmul); Python's
    random replayed from the seed gives its offsets, and the device path at those offsets gives its losses."""
    case = _model_case()
    monkeypatch.setenv("MTTS_SEGMENT_HOST", "1")
    random.seed(77)
    host, host_attn = _run_model(case, precision, None, sync_error=False)
    random.seed(77)
    offs = [random.choice(range(0, e)) if e > 0 else 0 for e in (max(t - M_S, 0) for t in M_YL)]
    monkeypatch.delenv("MTTS_SEGMENT_HOST")
    got, attn = _run_model(case, precision, torch.tensor(offs, device=DEV), sync_error=True)
    err = np.abs(got - host) / np.abs(host)
    print(f"{precision}: offsets {offs} device {got} host {host} rel err {err}")
    assert (err <= (FP32_LOSS_RTOL if precision == "32-true" else PARITY_RTOL)).all(), err
    assert torch.equal(attn, host_attn)


def test_segment_forward_launch_budget(monkeypatch):
    """The crop costs one native launch each way and replaces the alignment's consumers: no expand_rows pair, no
    dense path (prior_maximum_path gets a null `path`, so mas_expand_kernel is not launched), and no torch
    operator beyond the whole-utterance forward's except the draw of the window words (one launch)."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from matcha import _native as N

    case = _model_case()
    model = case["model"]
    lib = N.lib()
    calls = {}

    def counted(name):
        fn = getattr(lib, name)

        def wrapper(*a):
            calls.setdefault(name, []).append(a)
            return fn(*a)

        return wrapper

    for name in ("mtts_segment_crop_fwd", "mtts_segment_crop_bwd", "mtts_expand_rows_fwd", "mtts_expand_rows_bwd",
                 "mtts_prior_maximum_path"):
        monkeypatch.setattr(lib, name, counted(name))

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(str(func))
            return func(*args, **(kwargs or {}))

    def forward_backward(**kw):
        calls.clear()
        with Ops() as ops:
            out = model(*case["args"], t=case["t"], **kw)
        sum(out[:3]).backward()
        torch.cuda.synchronize()
        return ops.names, {k: len(v) for k, v in calls.items()}, calls["mtts_prior_maximum_path"][0][8]

    whole_ops, whole_calls, whole_path = forward_backward()
    seg_ops, seg_calls, seg_path = forward_backward(out_size=M_S)
    assert whole_calls == {"mtts_prior_maximum_path": 1, "mtts_expand_rows_fwd": 1, "mtts_expand_rows_bwd": 1}
    assert seg_calls == {"mtts_prior_maximum_path": 1, "mtts_segment_crop_fwd": 1, "mtts_segment_crop_bwd": 1}
    assert whole_path is not None and seg_path is None  # the dense [B,Tx,Ty] path is not written
    # torch operators: none runs more often than in the whole-utterance forward (no crop matmul, no slicing
    # loop), except the draw of the window words (one launch) and allocations / detach (no launch)
    seg_n, whole_n = collections.Counter(seg_ops), collections.Counter(whole_ops)
    extra = {k: v - whole_n[k] for k, v in seg_n.items() if v > whole_n[k]}
    free = {"aten.empty.memory_format", "aten.detach.default"}
    assert {k: v for k, v in extra.items() if k not in free} == {"aten.randint.low": 1}, extra


# ------------------------------------------------------------------------------------------ 6: Trainer
def _train_model(seed=0):
    from matcha.models.matcha_tts import MatchaTTS

    torch.manual_seed(seed)
    m = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(DEV)
    m.eval()  # dropout off
    return m


def _train_batch(seed, inject_offsets=True):
    from matcha.training import synthetic_batch

    b = synthetic_batch(4, 20, 160, seed=seed, device=DEV)
    g = torch.Generator().manual_seed(100 + seed)
    b["t"] = torch.rand(4, 1, 1, generator=g).to(DEV)
    b["z"] = torch.randn(4, 80, 64, generator=g).to(DEV)
    if inject_offsets:
        b["out_offset"] = torch.tensor([40, 0, 17, 3], device=DEV)
    return b


@pytest.mark.parametrize("precision", ["32-true", "bf16-mixed"])
def test_graph_segment_step_matches_eager_step(precision):
    from matcha.training import TrainConfig, Trainer

    b = _train_batch(0)
    m1, m2 = _train_model(), _train_model()
    m2.load_state_dict(m1.state_dict())
    te = Trainer(m1, TrainConfig(precision=precision, graph=False, out_size=64))
    tg = Trainer(m2, TrainConfig(precision=precision, graph=True, out_size=64))
    le = te.step([b]).clone()
    lg = tg.step([b]).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(le).all()
    assert torch.equal(lg, le), (lg, le)  # same kernels, fixed-order sums: bitwise, as the whole-utterance step
    assert torch.equal(m1.last_seg, m2.last_seg)


def test_graph_replays_draw_new_windows():
    from matcha.training import TrainConfig, Trainer

    b = _train_batch(1, inject_offsets=False)
    m = _train_model(1)
    tr = Trainer(m, TrainConfig(precision="bf16-mixed", graph=True, out_size=64))
    losses, segs = [], []
    for _ in range(4):
        losses.append(tr.step([b]).clone())
        segs.append(m.last_seg.clone())
    torch.cuda.synchronize()
    assert torch.isfinite(torch.stack(losses)).all()
    segs = torch.stack(segs).cpu()
    assert (segs[..., 1] == 64).all()
    max_off = (b["y_lengths"].cpu() - 64).clamp(0)
    assert ((segs[..., 0] >= 0) & (segs[..., 0] < max_off.clamp(1)[None])).all()
    assert len({tuple(s[:, 0].tolist()) for s in segs}) > 1  # every replay draws its own windows


def test_merged_accumulation_with_segments_vs_separate_micro_batches():
    """accumulate_grad_batches=2 with out_size: the merged micro-batches (one forward of 8 utterances, the crop is
    per utterance) against two separate micro-batch forwards with torch's clip + AdamW, by
    test_accumulate_merged_micro_batches_vs_torch's criterion."""
    from matcha.training import TrainConfig, Trainer

    b1, b2 = _train_batch(1), _train_batch(2)
    m_tr, m_ref = _train_model(7), _train_model(7)
    m_ref.load_state_dict(m_tr.state_dict())
    tr = Trainer(m_tr, TrainConfig(accumulate_grad_batches=2, graph=True, out_size=64))
    assert tr._merge_ok([b1, b2])
    params = [p for p in m_ref.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)
    for step in range(2):
        logged = tr.step([b1, b2]).clone()
        tot = []
        for b in (b1, b2):
            dur, prior, diff, _ = m_ref(**b, out_size=64)
            tot.append((dur + prior + diff).detach())
            ((dur + prior + diff) / 2).backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.testing.assert_close(logged[3], (tot[0] + tot[1]) / 2, rtol=2e-6, atol=0.0)
        for (n, a), (_, r) in zip(m_tr.named_parameters(), m_ref.named_parameters()):
            d = (a.detach() - r.detach()).abs()
            ok = d <= 1e-6 * r.detach().abs() + 1e-9
            assert ok.all() or d.max().item() <= (step + 1) * 2e-4 * 1.01, (step, n, d.max().item())
