"""MatchaTTS(use_precomputed_durations=True) on the device path (matcha_tts.py:273-274 of the reference):
durations -> runs in one launch (monotonic_align.duration_path), then the MAS branch's consumers.

* round trip: ``align``'s durations fed to a twin model give the MAS model's losses, attn and gradients bit for
  bit (the runs are identical, so every kernel sees identical inputs);
* arbitrary durations (under-covered, over-covered, rows of length 0) against the CPU oracle with
  generate_path in place of its alignment search, at test_model_gpu's bars;
* the mode runs without the alignment search and without the dense builder;
* the Trainer: captured step == eager step, a replay reads new durations, merged accumulation."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from golden.weights_recipe import apply_recipe

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R_B, R_TX, R_TY, R_S = 4, 20, 80, 32
R_XL, R_YL = [20, 15, 18, 12], [80, 60, 25, 49]  # utterance 2 is shorter than the window
R_OFF = [40, 13, 0, 7]
_RT = {}


def _model(precomputed, seed=None):
    from matcha.models.matcha_tts import MatchaTTS

    if seed is not None:
        torch.manual_seed(seed)
    m = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192, use_precomputed_durations=precomputed).to(DEV)
    m.eval()  # dropout off
    return m


def _round_trip_case():
    if not _RT:
        g = torch.Generator().manual_seed(61)
        xl, yl = torch.tensor(R_XL), torch.tensor(R_YL)
        x = torch.randint(1, 150, (R_B, R_TX), generator=g) * (torch.arange(R_TX)[None] < xl[:, None])
        y = torch.randn(R_B, 80, R_TY, generator=g) * (torch.arange(R_TY)[None, None] < yl[:, None, None])
        mas, twin = _model(False), _model(True)
        apply_recipe(mas, 9)
        twin.load_state_dict(mas.state_dict())
        d = lambda v: v.to(DEV)  # noqa: E731
        _RT.update(mas=mas, twin=twin, args=(d(x), d(xl), d(y), d(yl)), t=d(torch.rand(R_B, 1, 1, generator=g)),
                   z=d(torch.randn(R_B, 80, R_TY, generator=g)), zs=d(torch.randn(R_B, 80, R_S, generator=g)),
                   off=torch.tensor(R_OFF, device=DEV))
    return _RT


def _fwd_bwd(model, args, **kw):
    for p in model.parameters():
        p.grad = None
    dur, prior, diff, attn = model(*args, **kw)
    (dur + prior + diff).backward()
    return (dur.detach(), prior.detach(), diff.detach(), attn.detach()), \
        {n: p.grad for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("crop", [False, True], ids=["whole", "out_size32"])
@pytest.mark.parametrize("precision", ["32-true", "bf16-parity"])
def test_round_trip_align_then_train_is_bitwise_the_mas_step(precision, crop):
    from matcha.precision import precision_context

    c = _round_trip_case()
    kw = dict(t=c["t"], z=c["zs"], out_size=R_S, out_offset=c["off"]) if crop else dict(t=c["t"], z=c["z"])
    with precision_context(precision):
        d = c["mas"].align(*c["args"])
        want, want_g = _fwd_bwd(c["mas"], c["args"], **kw)
        got, got_g = _fwd_bwd(c["twin"], c["args"], durations=d, **kw)
    torch.cuda.synchronize()
    assert d.dtype == torch.int64 and d.shape == (R_B, R_TX)
    assert d.sum(1).tolist() == R_YL and (d[1, R_XL[1]:] == 0).all()  # MAS covers every frame
    for name, a, b in zip(("dur", "prior", "diff", "attn"), got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b), (name, a, b)
    assert got[3].shape == (R_B, R_TX, R_S if crop else R_TY)
    assert set(got_g) == set(want_g) and len(got_g) > 100
    for n in want_g:
        assert torch.equal(got_g[n], want_g[n]), n
    if crop:
        assert torch.equal(c["twin"].last_seg, c["mas"].last_seg)


O_B, O_TX, O_TY = 2, 11, 40
O_XL, O_YL = [11, 8], [40, 29]
# utterance 0: 27 of 40 frames covered, rows 1 and 5 of length 0; utterance 1: 35 frames asked of 29 (row 6 is cut,
# row 7 gets nothing), row 2 of length 0; the rows past t_x = 8 hold what must not count
O_D = [[3, 0, 4, 2, 5, 0, 3, 4, 2, 3, 1], [5, 4, 0, 6, 3, 7, 4, 6, 9, 9, 9]]


def test_arbitrary_durations_vs_oracle_with_generate_path():
    from oracle import matcha_oracle as MO

    g = torch.Generator().manual_seed(3)
    xl, yl = torch.tensor(O_XL), torch.tensor(O_YL)
    x = torch.randint(1, 150, (O_B, O_TX), generator=g) * (torch.arange(O_TX)[None] < xl[:, None])
    y = torch.randn(O_B, 80, O_TY, generator=g) * (torch.arange(O_TY)[None, None] < yl[:, None, None])
    t = torch.rand(O_B, 1, 1, generator=g)
    z = torch.randn(O_B, 80, O_TY, generator=g)
    dd = torch.tensor(O_D, dtype=torch.float32)
    ref = MO.MatchaTTSOracle(150, 80, 192, maximum_path=lambda lp, m: MO.generate_path(dd, m))
    apply_recipe(ref, 7)
    ref.eval()
    exp = ref(x, xl, y, yl, t=t, z=z)
    sum(exp[:3]).backward()
    model = _model(True)
    apply_recipe(model, 7)
    d = lambda v: v.to(DEV)  # noqa: E731
    out, grads = _fwd_bwd(model, (d(x), d(xl), d(y), d(yl)), durations=d(dd).unsqueeze(1), t=d(t), z=d(z))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[3].cpu().numpy(), exp[3].detach().numpy())
    assert out[3].sum().item() == 27 + 29
    got = np.array([float(v) for v in out[:3]])
    want = np.array([float(v.detach()) for v in exp[:3]])
    print("losses", got, "oracle", want, "rel", np.abs(got - want) / np.abs(want))
    np.testing.assert_allclose(got, want, rtol=1e-4)
    names = [n for n, p in ref.named_parameters() if p.grad is not None]
    assert set(names) == set(grads)
    gn = np.array([grads[n].double().norm().item() for n in names])
    gw = np.array([dict(ref.named_parameters())[n].grad.double().norm().item() for n in names])
    np.testing.assert_allclose(gn, gw, rtol=5e-3, atol=1e-6)


def test_mode_runs_without_alignment_search_and_without_dense_builder(monkeypatch):
    import matcha.models.matcha_tts as MT
    import matcha.utils.model as UM
    import matcha.utils.monotonic_align as MA

    def boom(*a, **k):
        raise AssertionError("the precomputed-durations forward must not get here")

    c = _round_trip_case()
    with torch.no_grad():
        d = c["mas"].align(*c["args"])
    monkeypatch.setattr(MA, "prior_maximum_path", boom)
    monkeypatch.setattr(UM, "generate_path", boom)
    monkeypatch.setattr(MT, "generate_path", boom)
    torch.cuda.set_sync_debug_mode("error")  # and no device->host copy
    try:
        out, grads = _fwd_bwd(c["twin"], c["args"], durations=d, t=c["t"], z=c["zs"], out_size=R_S)
        out2, _ = _fwd_bwd(c["twin"], c["args"], durations=d, t=c["t"], z=c["z"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in out + out2) and len(grads) > 100


def test_missing_durations_raise():
    c = _round_trip_case()
    with pytest.raises(ValueError, match="durations"):
        c["twin"](*c["args"])


# ------------------------------------------------------------------------------------------ Trainer
def _train_batch(model, seed, out_size=None):
    from matcha.training import synthetic_batch

    b = synthetic_batch(4, 20, 80, seed=seed, device=DEV)
    g = torch.Generator().manual_seed(100 + seed)
    b["t"] = torch.rand(4, 1, 1, generator=g).to(DEV)
    b["z"] = torch.randn(4, 80, out_size or 80, generator=g).to(DEV)
    if out_size:
        b["out_offset"] = torch.tensor([40, 0, 17, 3], device=DEV)
    b["durations"] = model.align(b["x"], b["x_lengths"], b["y"], b["y_lengths"])
    return b


@pytest.mark.parametrize("out_size", [None, 32], ids=["whole", "out_size32"])
def test_graph_step_with_durations_matches_eager_step(out_size):
    from matcha.training import TrainConfig, Trainer

    m1, m2 = _model(True, seed=0), _model(True, seed=0)
    m2.load_state_dict(m1.state_dict())
    b = _train_batch(m1, 0, out_size)
    te = Trainer(m1, TrainConfig(graph=False, out_size=out_size))
    tg = Trainer(m2, TrainConfig(graph=True, out_size=out_size))
    le = te.step([b]).clone()
    lg = tg.step([b]).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(le).all()
    assert torch.equal(lg, le), (lg, le)  # same kernels, fixed-order sums: bitwise, as the MAS step


def test_graph_replay_reads_the_batch_durations():
    """The second replay gets other durations of the same shape: the logged duration loss is the one an eager
    forward computes on them (with the weights the first step left), not the first batch's."""
    from matcha.training import TrainConfig, Trainer

    m = _model(True, seed=1)
    b1 = _train_batch(m, 1)
    b2 = dict(b1)
    d2 = b1["durations"].clone()
    d2[:, 0] += 3  # three frames more for the first token: the last rows are cut at y_lengths
    b2["durations"] = d2
    tr = Trainer(m, TrainConfig(graph=True))
    tr.step([b1])
    with torch.no_grad():
        fwd = {k: v for k, v in b1.items() if k != "durations"}
        dur1 = m(**fwd, durations=b1["durations"])[0].clone()
        dur2 = m(**fwd, durations=d2)[0].clone()
    logged = tr.step([b2]).clone()
    torch.cuda.synchronize()
    assert len(tr._graphs) == 1  # a replay, not a new capture
    assert torch.equal(logged[0], dur2) and not torch.equal(dur1, dur2), (logged, dur1, dur2)


def test_merged_accumulation_with_durations_vs_separate_micro_batches():
    """accumulate_grad_batches=2: the merged micro-batches (one forward of 8 utterances, durations stacked with the
    rest of the batch) against two separate micro-batch forwards with torch's clip + AdamW, by
    test_segment_gpu's criterion."""
    from matcha.training import TrainConfig, Trainer

    m_tr, m_ref = _model(True, seed=7), _model(True, seed=7)
    m_ref.load_state_dict(m_tr.state_dict())
    b1, b2 = _train_batch(m_tr, 1, 32), _train_batch(m_tr, 2, 32)
    tr = Trainer(m_tr, TrainConfig(accumulate_grad_batches=2, graph=True, out_size=32))
    assert tr._merge_ok([b1, b2])
    params = [p for p in m_ref.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)
    for step in range(2):
        logged = tr.step([b1, b2]).clone()
        tot = []
        for b in (b1, b2):
            dur, prior, diff, _ = m_ref(**b, out_size=32)
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
