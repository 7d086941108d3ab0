"""Trainer.validation_step / validate, checkpoint + resume of the captured step, and Trainer.fit on the GPU
(matcha/training.py, matcha/checkpoint.py).  The state round trips themselves are checked bit for bit without a
GPU in tests/test_checkpoint_cpu.py; here a resumed run must continue a captured step exactly."""
from __future__ import annotations

import os

import pytest
import torch

import poison as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(seed=0):
    from matcha.models.matcha_tts import MatchaTTS

    torch.manual_seed(seed)
    return MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(DEV)


def _batch(seed=0, inject=True):
    from matcha.training import synthetic_batch

    b = synthetic_batch(4, 20, 80, seed=seed, device=DEV)
    if inject:
        g = torch.Generator().manual_seed(100 + seed)
        b["t"] = torch.rand(4, 1, 1, generator=g).to(DEV)
        b["z"] = torch.randn(4, 80, 80, generator=g).to(DEV)
    return b


def _trainer(model, **kw):
    from matcha.training import TrainConfig, Trainer

    return Trainer(model, TrainConfig(graph=True, **kw))


def _state(tr):
    o = tr.optimizer
    return [p.detach().clone() for p in tr.params] + [o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_t.clone()]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        d = P.difference(x, y)
        assert d is None, f"{what}: tensor {i}: {d}"


@pytest.mark.parametrize("precision", ["32-true", "bf16-parity"])
def test_validation_step(precision):
    m = _model()
    m.train()
    tr = _trainer(m, precision=precision)
    tr.step([_batch(7)])  # gradients, moments and a captured train step exist before validation runs
    before = _state(tr)
    grads = [p.grad for p in tr.params]
    grad_vals = [None if g is None else g.clone() for g in grads]
    b1, b2 = _batch(1), _batch(2)

    v1 = tr.validation_step(b1)
    assert v1.shape == (4,) and all(mod.training for mod in m.modules())
    v2 = tr.validation_step(b2)  # same shape: a replay
    torch.cuda.synchronize()
    assert len(tr._val_graphs) == 1 and len(tr._graphs) == 1
    assert not torch.equal(v1, v2) and torch.isfinite(v1).all() and torch.isfinite(v2).all()
    # nothing of the training state moved
    _assert_same(_state(tr), before, "validation changed the training state")
    assert tr.global_step == 1
    assert all(p.grad is g for p, g in zip(tr.params, grads))
    _assert_same([g for g in grad_vals if g is not None], [g for g in grads if g is not None], "a gradient changed")

    # eagerly: eval(), no_grad(), get_losses under the same precision context, the same t and z
    def eager(b):
        orig = m.decoder.compute_loss_and_prior
        m.decoder.compute_loss_and_prior = lambda *a, **k: orig(*a, **{**k, "t": b["t"], "z": b["z"]})
        try:
            with torch.no_grad(), tr._autocast():
                d = m.get_losses(b)
                # the module's own hook (baselightningmodule.py:164-202): the same total, the reference's names
                m.__dict__.pop("_logged", None)
                total = m.validation_step(b, 0)
            assert m.training or torch.equal(total, sum(d.values()))  # (dropout on: two forwards, two masks)
            assert torch.equal(m._logged["loss/val"], total)
            assert list(m._logged) == ["sub_loss/val_dur_loss", "sub_loss/val_prior_loss", "sub_loss/val_diff_loss",
                                       "loss/val"]
        finally:
            del m.decoder.compute_loss_and_prior
        return torch.stack([d["dur_loss"], d["prior_loss"], d["diff_loss"], sum(d.values())]).float()

    m.eval()
    want = eager(b1)
    m.train()
    assert P.difference(v1, want) is None, (v1, want)
    # the eval() toggle is real: with dropout on, the same t and z give other losses
    assert not torch.equal(eager(b1)[:3], want[:3])

    out = tr.validate([b1, b2])
    mean = ((v1 + v2).tolist())
    assert out == {n: s / 2 for n, s in zip(("sub_loss/val_dur_loss", "sub_loss/val_prior_loss",
                                              "sub_loss/val_diff_loss", "loss/val"), mean)}


@pytest.mark.parametrize("epochs", [False, True])
@pytest.mark.parametrize("precision", ["32-true", "bf16-parity"])
def test_resume_is_exact(tmp_path, precision, epochs):
    """A takes steps 1-2, saves, takes steps 3-4.  The same A -- its step captured long before -- loads the file
    again and repeats steps 3-4 (in place: the captured graphs read the restored weights, moments, step count and
    lr; the weight packs are rebuilt inside every step).  A fresh model and trainer B loads the file and takes
    steps 3-4.  All three agree bit for bit.  epochs=True: on_epoch_end after every step, so lr has moved and must
    be restored too."""
    bs = [_batch(s) for s in range(4)]
    cfg = dict(precision=precision, t_max_epochs=10)

    def steps(tr, which):
        out = []
        for i in which:
            out.append(tr.step([bs[i]]).clone())
            if epochs:
                tr.on_epoch_end()
        return out

    ma = _model(0)
    ma.eval()
    a = _trainer(ma, **cfg)
    steps(a, (0, 1))
    path = tmp_path / "step2.ckpt"
    a.save_checkpoint(path)
    want_l = steps(a, (2, 3))
    want = _state(a)
    want_lr = float(a.lr)

    a.load_checkpoint(path)
    assert a.global_step == 2 and a.epoch == (2 if epochs else 0)
    got_l = steps(a, (2, 3))
    assert len(a._graphs) == 1
    _assert_same(got_l, want_l, "live trainer after load: losses")
    _assert_same(_state(a), want, "live trainer after load")

    mb = _model(1)  # other initial weights: everything must come from the file
    mb.eval()
    b = _trainer(mb, **cfg)
    b.load_checkpoint(path)
    got_l = steps(b, (2, 3))
    _assert_same(got_l, want_l, "fresh trainer after load: losses")
    _assert_same(_state(b), want, "fresh trainer after load")
    assert float(b.lr) == want_lr and b.global_step == 4
    if epochs:
        assert want_lr != 1e-4


def test_resumed_runs_are_reproducible_with_dropout_on(tmp_path):
    """Two fresh trainers load the same file and take one step on the same batch, dropout on, t and z drawn by the
    step: bitwise equal, because the file restores the generators (whatever they held before the load)."""
    src = _trainer(_model(0))
    torch.cuda.manual_seed(77)
    src.save_checkpoint(tmp_path / "c.ckpt")
    b = _batch(3, inject=False)
    res = []
    for junk in (1, 2):
        m = _model(junk)
        m.train()
        tr = _trainer(m)
        torch.cuda.manual_seed(1000 + junk)
        torch.rand(junk * 3, device=DEV)
        tr.load_checkpoint(tmp_path / "c.ckpt")
        loss = tr.step([b]).clone()
        torch.cuda.synchronize()
        res.append([loss] + _state(tr))
    _assert_same(res[0], res[1], "two resumed runs")


def test_fit_end_to_end(tmp_path):
    from matcha.models.matcha_tts import MatchaTTS

    def train(epoch):
        return [_batch(10 * epoch + i, inject=False) for i in range(3)]

    def val(epoch):
        return [_batch(900 + i, inject=False) for i in range(2)]

    m = _model(0)
    tr = _trainer(m, precision="bf16-parity")
    hist = tr.fit(train, val, max_epochs=2, ckpt_dir=tmp_path, log_every_n_steps=1)
    assert m.training
    train_rows = [r for r in hist if "loss/train" in r]
    val_rows = [r for r in hist if "loss/val" in r]
    assert [r["step"] for r in train_rows] == [1, 2, 3, 4, 5, 6] and [r["epoch"] for r in val_rows] == [0, 1]
    for r in hist:
        assert all(v == v and abs(v) != float("inf") for v in r.values())
    assert (tmp_path / "metrics.csv").exists()
    names = sorted(os.listdir(tmp_path))
    last = [n for n in names if n.startswith("last-")]
    best = [n for n in names if n.startswith("best-")]
    assert last == ["last-epoch=01-step=6.ckpt"] and 1 <= len(best) <= 3
    assert len(tr._graphs) == 1 and len(tr._val_graphs) == 1

    seen = []

    def train2(epoch):
        seen.append((epoch, tr2.global_step))
        return train(epoch)

    tr2 = _trainer(_model(1), precision="bf16-parity")
    tr2.fit(train2, val, max_epochs=3, ckpt_dir=tmp_path, resume=True)
    assert seen == [(2, 6)] and tr2.epoch == 3 and tr2.global_step == 9
    assert [n for n in os.listdir(tmp_path) if n.startswith("last-")] == ["last-epoch=02-step=9.ckpt"]

    best_path = tmp_path / sorted(n for n in os.listdir(tmp_path) if n.startswith("best-"))[0]
    model = MatchaTTS.load_from_checkpoint(best_path, map_location=DEV)
    model.eval()
    b = _batch(5, inject=False)
    out = model.synthesise(b["x"], b["x_lengths"], n_timesteps=2)
    assert out["mel"].shape[1] == 80 and torch.isfinite(out["mel"]).all()
