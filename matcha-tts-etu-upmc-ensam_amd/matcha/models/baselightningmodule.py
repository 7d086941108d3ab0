"""Training hooks of the reference's BaseLightningClass (matcha/models/baselightningmodule.py:19-246)
without pytorch_lightning (not part of this stack): the same get_losses / training_step /
configure_optimizers semantics, driven by matcha.training.Trainer instead of Lightning's loop.
"""
from __future__ import annotations

import os
from typing import Any

import torch
import torch.nn as nn


class Config(dict):
    """A config tree read back from a checkpoint: a dict whose keys are attributes too (what the model's
    constructors ask of the reference's OmegaConf nodes: ``params.n_feats`` and ``**params``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def plain(v):
    """A hyper-parameter as plain values: namespaces and mappings -> dict, sequences -> list / tuple, numbers,
    strings, bools and None as they are, 0-dim tensors -> float."""
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if hasattr(v, "__dict__") and not isinstance(v, (type, torch.Tensor, nn.Module)):
        return {k: plain(x) for k, x in vars(v).items()}
    if isinstance(v, (list, tuple)):
        return type(v)(plain(x) for x in v) if type(v) in (list, tuple) else [plain(x) for x in v]
    if isinstance(v, torch.Tensor) and v.numel() == 1:
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"hyper-parameter of type {type(v).__name__} has no plain form")


def config(v):
    """plain()'s dicts as Config trees."""
    if isinstance(v, dict):
        return Config({k: config(x) for k, x in v.items()})
    if isinstance(v, (list, tuple)):
        return type(v)(config(x) for x in v)
    return v


class BaseLightningClass(nn.Module):
    global_step: int = 0

    def update_data_statistics(self, data_statistics):
        if data_statistics is None:
            data_statistics = {"mel_mean": 0.0, "mel_std": 1.0}
        self.register_buffer("mel_mean", torch.tensor(data_statistics["mel_mean"]))
        self.register_buffer("mel_std", torch.tensor(data_statistics["mel_std"]))

    def save_hyperparameters(self, *args, ignore=(), logger=True, **kwargs):
        """Lightning API: records the constructor arguments in ``self.hparams`` (a checkpoint's
        ``hyper_parameters``, what load_from_checkpoint rebuilds the model from).  Lightning reads them off the
        caller's frame; here the caller passes them -- dicts positionally and / or keywords -- as plain values
        (config namespaces as dicts: plain())."""
        hp = {}
        for a in args:
            hp.update(a)
        hp.update(kwargs)
        ignore = (ignore,) if isinstance(ignore, str) else tuple(ignore)
        self.hparams = {k: plain(v) for k, v in hp.items() if k not in ignore}

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None):
        """Lightning's classmethod (generate.py:42, train.py:71): the model rebuilt from the file's
        ``hyper_parameters`` with its ``state_dict`` loaded, on map_location (CPU when None).  The file is read
        with weights_only=True (matcha/checkpoint.py writes nothing else)."""
        ck = torch.load(os.fspath(checkpoint_path), map_location="cpu", weights_only=True)
        model = cls(**{k: config(v) if k in cls._config_hparams else v for k, v in ck["hyper_parameters"].items()})
        model.load_state_dict(ck["state_dict"])
        return model.to(map_location) if map_location is not None else model

    _config_hparams: tuple = ()  # hyper-parameters that are config trees (rebuilt as Config, see config())

    def log(self, name, value, **kwargs):  # Lightning API: recorded for the driver to reduce/print
        self.__dict__.setdefault("_logged", {})[name] = value

    def log_dict(self, dictionary, **kwargs):  # Lightning API: one log() per item
        for name, value in dictionary.items():
            self.log(name, value, **kwargs)

    def on_before_optimizer_step(self, optimizer):
        """baselightningmodule.py:244-245: every parameter's gradient 2-norm and their total, logged as
        ``grad_norm/grad_2.0_norm/<parameter name>`` and ``grad_norm/grad_2.0_norm_total``.  (A driver that
        wants the log calls this between backward and the optimizer step; matcha.training.Trainer does not.)"""
        from matcha.utils.grad_norm import grad_norm

        self.log_dict({f"grad_norm/{k}": v for k, v in grad_norm(self, norm_type=2).items()})

    def configure_optimizers(self) -> dict[str, Any]:
        """baselightningmodule.py:57-92: AdamW(1e-4, (0.9, 0.999), wd 1e-6) + per-epoch cosine
        annealing (T_max 1000, eta_min 1e-6)."""
        # torch's default implementation, as the reference (multi-tensor on the GPU); the graph-mode
        # Trainer replaces it with the HIP clip + AdamW, equal to it within 2 ulp
        opt = torch.optim.AdamW(self.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-6)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=1000, eta_min=1e-6)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": sched, "interval": "epoch", "frequency": 1}}

    def get_losses(self, batch):
        """baselightningmodule.py:94-110."""
        dur_loss, prior_loss, diff_loss, *_ = self(
            x=batch["x"], x_lengths=batch["x_lengths"], y=batch["y"], y_lengths=batch["y_lengths"],
            out_size=self.out_size, durations=batch.get("durations", None))
        return {"dur_loss": dur_loss, "prior_loss": prior_loss, "diff_loss": diff_loss}

    def training_step(self, batch: Any, batch_idx: int):
        """baselightningmodule.py:115-162: total = dur + prior + diff."""
        loss_dict = self.get_losses(batch)
        total = sum(loss_dict.values())
        self.log("loss/train", total)
        return {"loss": total, "log": loss_dict}

    def validation_step(self, batch: Any, batch_idx: int):
        """baselightningmodule.py:164-202: the three sub-losses and their total, logged under the
        reference's names; returns the total.  (The caller sets eval() and no_grad(), as Lightning's loop does:
        matcha.training.Trainer.validation_step.)"""
        loss_dict = self.get_losses(batch)
        self.log("sub_loss/val_dur_loss", loss_dict["dur_loss"], sync_dist=True)
        self.log("sub_loss/val_prior_loss", loss_dict["prior_loss"], sync_dist=True)
        self.log("sub_loss/val_diff_loss", loss_dict["diff_loss"], sync_dist=True)
        total = sum(loss_dict.values())
        self.log("loss/val", total, sync_dist=True)
        return total
