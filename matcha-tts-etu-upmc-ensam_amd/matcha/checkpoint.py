"""Checkpoints: one file per checkpoint, written by torch.save in Lightning's top-level layout, so that the
reference's tooling (and ``MatchaTTS.load_from_checkpoint``, generate.py:42, train.py:71) finds what it expects:

    state_dict        the model's, CPU tensors
    hyper_parameters  the constructor arguments (BaseLightningClass.save_hyperparameters), plain values
    epoch, global_step
    optimizer_states  [torch.optim.AdamW.state_dict() form]: per parameter exp_avg / exp_avg_sq / step and the
                      param group -- in BOTH Trainer modes (the graph step's flat moment arrays are cut along
                      _FlatClipAdamW.offsets, its device step counter becomes every parameter's ``step``), so a
                      file written by one mode loads into the other
    lr_schedulers     [CosineAnnealingLR.state_dict()] (graph mode: the entries that define the schedule)
    mtts              {"version", "precision", "rng": torch CPU / torch CUDA of the trainer's device / Python random}

Only tensors and plain containers: ``torch.load(path, weights_only=True)`` reads it.

Loading into a graph-mode Trainer copies INTO the existing flat arrays, the parameters (views of the flat array),
the step counter and the lr scalar: every address stays, so steps captured before the load remain valid (the
weight packs and bf16 planes are rebuilt from the parameters inside every step -- DESIGN.md).
"""
from __future__ import annotations

import glob
import os
import random

import torch
import torch.distributed as dist

FORMAT_VERSION = 1
_ADAMW_GROUP = {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-6, "amsgrad": False, "maximize": False,
                "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                "decoupled_weight_decay": True}  # torch.optim.AdamW's own group keys


def find_latest_checkpoint(logs_dir="lightning_logs", checkpoint_path=None):
    """train.py:10-43: an explicit path if it exists (None if it does not), else the newest ``*.ckpt`` by mtime
    anywhere under logs_dir, else None."""
    if checkpoint_path is not None:
        return checkpoint_path if os.path.exists(checkpoint_path) else None
    if not os.path.exists(logs_dir):
        return None
    files = glob.glob(os.path.join(str(logs_dir), "**", "*.ckpt"), recursive=True)
    return max(files, key=os.path.getmtime) if files else None


def _cpu(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", copy=True).contiguous()  # a view's own bytes, not the flat array behind it


def _flat_optimizer_state(opt, lr: float) -> dict:
    """_FlatClipAdamW -> torch.optim.AdamW.state_dict() form."""
    step = _cpu(opt.step_t).reshape(())
    state = {}
    for i, (p, o) in enumerate(zip(opt.params, opt.offsets)):
        n = p.numel()
        state[i] = {"step": step.clone(), "exp_avg": _cpu(opt.exp_avg[o:o + n]).view(p.shape),
                    "exp_avg_sq": _cpu(opt.exp_avg_sq[o:o + n]).view(p.shape)}
    group = dict(_ADAMW_GROUP, lr=lr, betas=tuple(opt.betas), eps=opt.eps, weight_decay=opt.wd,
                 params=list(range(len(opt.params))))
    return {"state": state, "param_groups": [group]}


def _load_flat_optimizer_state(opt, sd: dict) -> None:
    """torch.optim.AdamW.state_dict() form -> the flat arrays, in place.  A parameter the file has no state for
    (torch creates it at the parameter's first step) gets zero moments; the one device step counter takes the
    largest ``step`` of the file."""
    state = sd["state"]
    if any(int(k) >= len(opt.params) for k in state):
        raise ValueError("checkpoint: the optimizer state covers more parameters than the model has")
    step = 0.0
    with torch.no_grad():
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        for k, st in state.items():
            p, o = opt.params[int(k)], opt.offsets[int(k)]
            n = p.numel()
            if st["exp_avg"].numel() != n:
                raise ValueError(f"checkpoint: optimizer state {k} has {st['exp_avg'].numel()} elements, "
                                 f"the parameter {n}")
            opt.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            opt.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            step = max(step, float(st["step"]))
        opt.step_t.fill_(step)


def _rng_state(dev: torch.device) -> dict:
    v, ints, gauss = random.getstate()
    return {"torch_cpu": torch.get_rng_state().clone(),
            "torch_cuda": torch.cuda.get_rng_state(dev).clone() if dev.type == "cuda" else None,
            "python": [v, list(ints), gauss]}


def _set_rng_state(rng: dict, dev: torch.device) -> None:
    torch.set_rng_state(rng["torch_cpu"].cpu())
    if dev.type == "cuda" and rng.get("torch_cuda") is not None:
        torch.cuda.set_rng_state(rng["torch_cuda"].cpu(), dev)
    v, ints, gauss = rng["python"]
    random.setstate((v, tuple(ints), gauss))


def trainer_state(tr) -> dict:
    from matcha.training import _FlatClipAdamW

    model = tr.model
    if isinstance(tr.optimizer, _FlatClipAdamW):
        lr = float(tr.lr)
        opt_sd = _flat_optimizer_state(tr.optimizer, lr)
        sched = {"T_max": tr.cfg.t_max_epochs, "eta_min": tr.cfg.eta_min, "base_lrs": [tr.cfg.lr],
                 "last_epoch": tr.epoch, "_step_count": tr.epoch + 1, "_last_lr": [lr]}
    else:
        opt_sd = tr.optimizer.state_dict()
        opt_sd = {"state": {k: {n: (_cpu(v) if torch.is_tensor(v) else v) for n, v in st.items()}
                            for k, st in opt_sd["state"].items()},
                  "param_groups": [dict(g) for g in opt_sd["param_groups"]]}
        sched = dict(tr.scheduler.state_dict()) if tr.scheduler is not None else {}
    return {"state_dict": {k: _cpu(v) for k, v in model.state_dict().items()},
            "hyper_parameters": dict(getattr(model, "hparams", None) or {}),
            "epoch": tr.epoch, "global_step": tr.global_step,
            "optimizer_states": [opt_sd], "lr_schedulers": [sched],
            # Trainer.fit's top-k bookkeeping (ModelCheckpoint's best_k_models): file name -> loss/val
            "callbacks": {"best_k_models": {str(k): float(v) for k, v in getattr(tr, "_best_k", {}).items()}},
            "mtts": {"version": FORMAT_VERSION, "precision": tr.cfg.precision, "rng": _rng_state(tr.dev)}}


def save(tr, path) -> None:
    """Trainer.save_checkpoint.  World size > 1: rank 0 writes path + ".tmp" and renames it over `path`; every
    rank leaves together."""
    path = os.fspath(path)
    multi = tr.world > 1 and dist.is_available() and dist.is_initialized()
    if not multi or dist.get_rank() == 0:
        state = trainer_state(tr)
        tmp = path + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, path)
    if multi:
        dist.barrier()


def load(tr, path) -> dict:
    """Trainer.load_checkpoint (every rank reads the file).  Returns the checkpoint dict."""
    from matcha.training import _FlatClipAdamW

    ck = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    ver = ck.get("mtts", {}).get("version", FORMAT_VERSION)
    if ver != FORMAT_VERSION:
        raise ValueError(f"checkpoint format version {ver}; this code reads {FORMAT_VERSION}")
    tr.model.load_state_dict(ck["state_dict"])  # copy_ into the existing tensors (graph mode: the flat views)
    tr.epoch, tr.global_step = int(ck["epoch"]), int(ck["global_step"])
    opt_sd = ck["optimizer_states"][0]
    if isinstance(tr.optimizer, _FlatClipAdamW):
        _load_flat_optimizer_state(tr.optimizer, opt_sd)
        tr.lr.fill_(tr.cosine_lr(tr.epoch))  # on_epoch_end's formula
    else:
        cur = tr.optimizer.state_dict()
        if len(opt_sd["param_groups"]) != len(cur["param_groups"]) or any(
                len(a["params"]) != len(b["params"]) for a, b in zip(opt_sd["param_groups"], cur["param_groups"])):
            raise ValueError("checkpoint: the optimizer's parameter groups do not match the model's")
        groups = [dict(g, **{k: v for k, v in sg.items() if k != "params" and k in g})
                  for g, sg in zip(cur["param_groups"], opt_sd["param_groups"])]
        tr.optimizer.load_state_dict({"state": opt_sd["state"], "param_groups": groups})
        sched = ck["lr_schedulers"][0] if ck.get("lr_schedulers") else {}
        if tr.scheduler is not None and sched:
            tr.scheduler.load_state_dict(sched)
    rng = ck.get("mtts", {}).get("rng")
    if rng is not None:
        _set_rng_state(rng, tr.dev)
    return ck
