"""Checkpoint, resume and load_from_checkpoint without a GPU (matcha/checkpoint.py, Trainer.save_checkpoint /
load_checkpoint / fit, BaseLightningClass.save_hyperparameters / load_from_checkpoint).

A graph-mode Trainer on the CPU constructs the flat optimizer and launches nothing (test_lr_schedule_cpu.py relies
on the same), so the state round trips are checked here bit for bit; the GPU side (resume of a captured step) is
tests/test_fit_gpu.py."""
from __future__ import annotations

import os
import re

import pytest
import torch

from matcha.checkpoint import find_latest_checkpoint
from matcha.models.matcha_tts import MatchaTTS
from matcha.training import TrainConfig, Trainer

pytestmark = pytest.mark.filterwarnings("ignore:Detected call")


class _Tiny(torch.nn.Module):
    """A stand-in with parameters of odd sizes (the flat array pads each to a multiple of 4) and a buffer."""

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.w = torch.nn.Linear(5, 3)
        self.v = torch.nn.Parameter(torch.randn(7))
        self.register_buffer("stat", torch.randn(2))

    def configure_optimizers(self):  # BaseLightningClass.configure_optimizers on this stand-in
        o = torch.optim.AdamW(self.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-6)
        return {"optimizer": o,
                "lr_scheduler": {"scheduler": torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=1000, eta_min=1e-6)}}


def _randomise(tr, seed):
    g = torch.Generator().manual_seed(seed)
    o = tr.optimizer
    o.exp_avg.copy_(torch.randn(o.exp_avg.shape, generator=g))
    o.exp_avg_sq.copy_(torch.rand(o.exp_avg_sq.shape, generator=g))
    o.step_t.fill_(float(torch.randint(1, 1000, (1,), generator=g)))


def _moments(tr):
    """Per parameter (exp_avg, exp_avg_sq, step) of either optimizer."""
    o = tr.optimizer
    if hasattr(o, "offsets"):
        return [(o.exp_avg[a:a + p.numel()].view_as(p).clone(), o.exp_avg_sq[a:a + p.numel()].view_as(p).clone(),
                 o.step_t.reshape(()).clone()) for p, a in zip(o.params, o.offsets)]
    return [(o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone(),
             torch.as_tensor(o.state[p]["step"]).float().reshape(()).clone()) for p in tr.params]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def test_state_round_trip_graph_mode(tmp_path):
    a = Trainer(_Tiny(1), TrainConfig(graph=True))
    _randomise(a, 3)
    for _ in range(3):
        a.on_epoch_end()
    a.global_step = 41
    path = tmp_path / "a.ckpt"
    a.save_checkpoint(path)
    b = Trainer(_Tiny(2), TrainConfig(graph=True))
    flat_ptr = b.optimizer.flat.data_ptr()
    b.load_checkpoint(path)
    assert b.optimizer.flat.data_ptr() == flat_ptr  # in place: a captured step would still point at it
    for (n, p), (_, q) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert _same(p, q), n
    # (per parameter: the flat arrays' padding between parameters is no state)
    for (m1, v1, s1), (m2, v2, s2) in zip(_moments(a), _moments(b)):
        assert _same(m1, m2) and _same(v1, v2) and _same(s1, s2)
    assert _same(a.optimizer.step_t, b.optimizer.step_t)
    assert (b.epoch, b.global_step) == (3, 41) == (a.epoch, a.global_step)
    assert float(a.lr) == float(b.lr) and float(b.lr) != 1e-4
    a.on_epoch_end()
    b.on_epoch_end()
    assert float(a.lr) == float(b.lr) and a.epoch == b.epoch == 4


def test_cross_mode_load(tmp_path):
    g = Trainer(_Tiny(1), TrainConfig(graph=True))
    _randomise(g, 5)
    g.on_epoch_end()
    g.on_epoch_end()
    g.save_checkpoint(tmp_path / "graph.ckpt")
    e = Trainer(_Tiny(2), TrainConfig(graph=False))
    e.load_checkpoint(tmp_path / "graph.ckpt")
    assert e.epoch == 2 and e.scheduler.last_epoch == 2
    assert abs(e.optimizer.param_groups[0]["lr"] - float(g.lr)) < 1e-15
    for (m1, v1, s1), (m2, v2, s2) in zip(_moments(g), _moments(e)):
        assert _same(m1, m2) and _same(v1, v2) and _same(s1, s2)
    for p, q in zip(g.model.parameters(), e.model.parameters()):
        assert _same(p.detach(), q.detach())
    e.on_epoch_end()
    e.save_checkpoint(tmp_path / "eager.ckpt")
    g2 = Trainer(_Tiny(3), TrainConfig(graph=True))
    g2.load_checkpoint(tmp_path / "eager.ckpt")
    assert g2.epoch == 3
    g.on_epoch_end()
    assert float(g2.lr) == float(g.lr)
    for (m1, v1, s1), (m2, v2, s2) in zip(_moments(g), _moments(g2)):
        assert _same(m1, m2) and _same(v1, v2) and _same(s1, s2)


def test_file_format(tmp_path):
    tr = Trainer(_Tiny(1), TrainConfig(graph=True))
    _randomise(tr, 7)
    tr.save_checkpoint(tmp_path / "f.ckpt")
    ck = torch.load(tmp_path / "f.ckpt", weights_only=True)
    for key in ("state_dict", "hyper_parameters", "epoch", "global_step", "optimizer_states", "lr_schedulers"):
        assert key in ck, key
    assert len(ck["optimizer_states"]) == 1
    st = ck["optimizer_states"][0]
    assert set(st) == {"state", "param_groups"} and len(st["state"]) == len(tr.params)
    assert set(st["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert st["state"][0]["exp_avg"].shape == tr.params[0].shape
    # every tensor owns its bytes: a parameter view must not drag the flat array into the file
    assert all(v.untyped_storage().nbytes() == v.numel() * v.element_size() for v in ck["state_dict"].values())
    assert ck["mtts"]["version"] == 1 and ck["mtts"]["precision"] == "32-true"
    assert set(ck["mtts"]["rng"]) == {"torch_cpu", "torch_cuda", "python"}
    # the file is what torch's own AdamW reads
    opt = torch.optim.AdamW(_Tiny(4).parameters(), lr=1.0)
    opt.load_state_dict(st)
    assert opt.param_groups[0]["lr"] == 1e-4


def test_rng_states_are_restored(tmp_path):
    import random

    tr = Trainer(_Tiny(1), TrainConfig(graph=True))
    torch.manual_seed(11)
    random.seed(11)
    tr.save_checkpoint(tmp_path / "r.ckpt")
    want = (torch.rand(3), random.random())
    torch.rand(5)
    random.random()
    tr.load_checkpoint(tmp_path / "r.ckpt")
    got = (torch.rand(3), random.random())
    assert torch.equal(got[0], want[0]) and got[1] == want[1]


def test_hyper_parameters_and_load_from_checkpoint(tmp_path):
    stats = {"mel_mean": -5.5, "mel_std": 2.25}
    model = MatchaTTS(n_vocab=20, out_channels=8, hidden_channels=16, data_statistics=stats, out_size=32,
                      use_precomputed_durations=True)
    assert model.hparams["data_statistics"] == stats and model.hparams["n_vocab"] == 20
    tr = Trainer(model, TrainConfig(graph=True))
    tr.save_checkpoint(tmp_path / "m.ckpt")
    back = MatchaTTS.load_from_checkpoint(tmp_path / "m.ckpt")
    assert back.out_size == 32 and back.use_precomputed_durations is True and back.n_vocab == 20
    assert back.hparams == model.hparams
    sd, sd2 = model.state_dict(), back.state_dict()
    assert list(sd) == list(sd2)
    for k in sd:
        assert _same(sd[k], sd2[k]), k
    assert float(back.mel_mean) == -5.5 and float(back.mel_std) == 2.25


def test_load_from_checkpoint_config_constructor(tmp_path):
    """The (encoder, decoder, cfm) constructor: the config namespaces are saved as dicts and come back as trees
    the constructors can read both ways (attributes and **)."""
    from types import SimpleNamespace as NS

    enc = NS(encoder_type="transformer",
             encoder_params=NS(n_feats=8, n_channels=16, filter_channels=32, n_heads=2, n_layers=1, kernel_size=3,
                               p_dropout=0.1, prenet=True),
             duration_predictor_params=NS(filter_channels_dp=16, kernel_size=3, p_dropout=0.1))
    dec = {"channels": (16, 16), "dropout": 0.05, "attention_head_dim": 8, "n_blocks": 1, "num_mid_blocks": 1,
           "num_heads": 2}
    model = MatchaTTS(n_vocab=20, n_feats=8, encoder=enc, decoder=dec, cfm=NS(solver="euler", sigma_min=1e-4))
    assert model.hparams["encoder"]["encoder_params"]["n_channels"] == 16
    Trainer(model, TrainConfig(graph=True)).save_checkpoint(tmp_path / "c.ckpt")
    back = MatchaTTS.load_from_checkpoint(tmp_path / "c.ckpt")
    for (k, a), (_, b) in zip(model.state_dict().items(), back.state_dict().items()):
        assert _same(a, b), k


def test_find_latest_checkpoint(tmp_path):
    assert find_latest_checkpoint(tmp_path) is None
    assert find_latest_checkpoint(tmp_path / "missing") is None
    (tmp_path / "sub").mkdir()
    files = [tmp_path / "a.ckpt", tmp_path / "sub" / "b.ckpt", tmp_path / "c.ckpt"]
    for i, (f, mtime) in enumerate(zip(files, (1000.0, 3000.0, 2000.0))):
        f.write_bytes(b"x")
        os.utime(f, (mtime, mtime))
    (tmp_path / "newest.txt").write_bytes(b"x")  # not a checkpoint
    assert find_latest_checkpoint(tmp_path) == str(files[1])
    assert find_latest_checkpoint(tmp_path, checkpoint_path=str(files[0])) == str(files[0])
    assert find_latest_checkpoint(tmp_path, checkpoint_path=str(tmp_path / "nope.ckpt")) is None


class _Scripted(Trainer):
    """fit's bookkeeping without a model step: step and validate return scripted values."""

    def __init__(self, val_losses):
        super().__init__(_Tiny(1), TrainConfig(graph=True))
        self.script = list(val_losses)
        self.val_calls = 0

    def step(self, batches):
        self.global_step += 1
        return torch.tensor([1.0, 2.0, 3.0, 6.0]) * self.global_step

    def validate(self, batches):
        self.val_calls += 1
        v = self.script[self.epoch]
        return {"sub_loss/val_dur_loss": v / 4, "sub_loss/val_prior_loss": v / 4, "sub_loss/val_diff_loss": v / 2,
                "loss/val": v}


def _ckpts(d):
    best = sorted(f for f in os.listdir(d) if f.startswith("best-"))
    last = sorted(f for f in os.listdir(d) if f.startswith("last-"))
    return best, last


def test_fit_top_k_bookkeeping(tmp_path):
    vals = [0.9, 0.5, 0.7, 0.3, 0.8, 0.6]
    tr = _Scripted(vals)
    seen = []

    def train(epoch):
        seen.append(epoch)
        return [{"x": torch.zeros(1)}] * 3

    hist = tr.fit(train, lambda epoch: [None], max_epochs=6, ckpt_dir=tmp_path, save_top_k=3, log_every_n_steps=2)
    assert seen == list(range(6)) and tr.epoch == 6 and tr.global_step == 18
    best, last = _ckpts(tmp_path)
    assert last == ["last-epoch=05-step=18.ckpt"]
    # the three lowest loss/val: epochs 3 (0.3), 1 (0.5), 5 (0.6)
    assert best == ["best-epoch=01-loss_val=0.500.ckpt", "best-epoch=03-loss_val=0.300.ckpt",
                    "best-epoch=05-loss_val=0.600.ckpt"]
    for f in best:
        ep = int(re.match(r"best-epoch=(\d+)-", f).group(1))
        assert torch.load(tmp_path / f, weights_only=True)["epoch"] == ep + 1  # epochs completed
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    train_rows = [r for r in hist if "loss/train" in r]
    val_rows = [r for r in hist if "loss/val" in r]
    assert [r["step"] for r in train_rows] == list(range(2, 19, 2))
    assert train_rows[0]["loss/train"] == 12.0 and train_rows[0]["sub_loss/train_dur_loss"] == 2.0
    assert [r["loss/val"] for r in val_rows] == vals
    lines = (tmp_path / "metrics.csv").read_text().strip().splitlines()
    assert len(lines) == 1 + len(hist) and "loss/val" in lines[0] and "loss/train" in lines[0]

    # resume: a fresh trainer continues at epoch 6 and keeps ranking against the files already there
    tr2 = _Scripted(vals + [0.1, 0.95])
    seen.clear()
    tr2.fit(train, lambda epoch: [None], max_epochs=8, ckpt_dir=tmp_path, save_top_k=3, resume=True)
    assert seen == [6, 7] and tr2.global_step == 24
    best, last = _ckpts(tmp_path)
    assert last == ["last-epoch=07-step=24.ckpt"]
    assert best == ["best-epoch=01-loss_val=0.500.ckpt", "best-epoch=03-loss_val=0.300.ckpt",
                    "best-epoch=06-loss_val=0.100.ckpt"]


def test_fit_accumulates_micro_batches_and_accepts_a_re_iterable(tmp_path):
    tr = _Scripted([1.0, 1.0])
    tr.cfg.accumulate_grad_batches = 2
    got = []
    tr.step = lambda batches: (got.append(len(batches)), setattr(tr, "global_step", tr.global_step + 1),
                               torch.zeros(4))[-1]
    hist = tr.fit([{"x": torch.zeros(1)}] * 5, None, max_epochs=2, log_every_n_steps=1)
    assert got == [2, 2, 2, 2] and tr.val_calls == 0  # the fifth micro-batch of each epoch has no partner
    assert len(hist) == 4 and not os.listdir(tmp_path)
