"""Per-parameter gradient norms: Lightning's grad_norm utility (matcha/utils/grad_norm.py) and the module hook
that logs it as the reference does (baselightningmodule.py:244-245).  Plain torch: no GPU."""
from __future__ import annotations

import pytest
import torch


class _Three(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(4, 3, generator=g))
        self.skipped = torch.nn.Parameter(torch.randn(5, generator=g))  # its .grad stays None
        self.lin = torch.nn.Linear(3, 2)
        self.a.grad = torch.randn(4, 3, generator=g)
        self.lin.weight.grad = torch.randn(2, 3, generator=g) * 7.0


def test_grad_norm_keys_values_total():
    from matcha.utils.grad_norm import grad_norm

    m = _Three()  # lin.bias has no gradient either: two of four parameters are listed
    out = grad_norm(m, norm_type=2)
    assert list(out) == ["grad_2.0_norm/a", "grad_2.0_norm/lin.weight", "grad_2.0_norm_total"]
    assert not any("skipped" in k or "bias" in k for k in out)
    assert torch.equal(out["grad_2.0_norm/a"], m.a.grad.norm(2))
    assert torch.equal(out["grad_2.0_norm/lin.weight"], m.lin.weight.grad.norm(2))
    want = torch.stack([m.a.grad.norm(2), m.lin.weight.grad.norm(2)]).norm(2)
    assert torch.equal(out["grad_2.0_norm_total"], want)
    # another norm type: the key carries float(norm_type), the total is that norm of the norms
    one = grad_norm(m, norm_type=1)
    assert list(one) == ["grad_1.0_norm/a", "grad_1.0_norm/lin.weight", "grad_1.0_norm_total"]
    assert torch.equal(one["grad_1.0_norm_total"], m.a.grad.norm(1) + m.lin.weight.grad.norm(1))
    assert grad_norm(torch.nn.Linear(2, 2), 2) == {}  # no gradient anywhere: nothing, no total
    with pytest.raises(ValueError):
        grad_norm(m, norm_type=0)


def test_on_before_optimizer_step_logs_prefixed_keys():
    from matcha.models.baselightningmodule import BaseLightningClass

    class M(BaseLightningClass):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(3))
            self.v = torch.nn.Parameter(torch.ones(2))
            self.none = torch.nn.Parameter(torch.ones(2))

    m = M()
    m.w.grad = torch.tensor([3.0, 0.0, 4.0])
    m.v.grad = torch.tensor([0.0, 12.0])
    m.on_before_optimizer_step(optimizer=None)
    assert list(m._logged) == ["grad_norm/grad_2.0_norm/w", "grad_norm/grad_2.0_norm/v",
                               "grad_norm/grad_2.0_norm_total"]
    assert [float(v) for v in m._logged.values()] == [5.0, 12.0, 13.0]
    m.log_dict({"x": 1, "y": 2})
    assert m._logged["x"] == 1 and m._logged["y"] == 2
