"""pytorch_lightning.utilities.grad_norm without pytorch_lightning (not part of this stack): the gradient norms
the reference logs before every optimizer step (baselightningmodule.py:244-245).  Plain torch, any device."""
from __future__ import annotations

import torch


def key(name: str, norm_type: float = 2) -> str:
    """The key of parameter `name`'s gradient norm: ``grad_2.0_norm/<name>``."""
    return f"grad_{float(norm_type)}_norm/{name}"


def total_key(norm_type: float = 2) -> str:
    return f"grad_{float(norm_type)}_norm_total"


def grad_norm(module: torch.nn.Module, norm_type: float = 2) -> dict[str, torch.Tensor]:
    """Lightning's contract: for every named_parameters() entry whose .grad is not None, in that order,
    ``grad_{norm_type}_norm/{name}`` -> the norm_type-norm of the gradient (a 0-dim tensor); last,
    ``grad_{norm_type}_norm_total`` -> the norm_type-norm of those norms.  No parameter with a gradient: {}."""
    norm_type = float(norm_type)
    if norm_type <= 0:
        raise ValueError(f"`norm_type` must be a positive number or 'inf' (infinity norm). Got {norm_type}")
    norms = {key(name, norm_type): p.grad.detach().norm(norm_type)
             for name, p in module.named_parameters() if p.grad is not None}
    if norms:
        norms[total_key(norm_type)] = torch.stack(list(norms.values())).norm(norm_type)
    return norms
