"""The forward-precision policy's decisions (host Python, no device, no library): which operand kind a forward GEMM
packs for every combination of the switches, that every context restores what it found, the ambient text-encoder
precision, the two environment switches, and the Trainer precision names.

The truth table is DESIGN.md's "Precision modes" written out: `_pack_kind` returns `prec` unchanged for PREC_FP32 and
for a dgrad operand; for a bf16 forward operand the first matching row wins --
  one_plane and parity policy active and no precise_forward -> PREC_BF16 (1)
  precise "fp32" -> PREC_FP32 (0);  "bf16x6" -> PACK_BF16_SPLIT3 (3);  "bf16x3" -> PACK_BF16_SPLIT (2)
  process-wide split on, or parity policy active -> PACK_BF16_SPLIT (2);  otherwise PREC_BF16 (1)
(one_plane is ignored under set_weight_split(True) alone: ADVICE r4)."""
from __future__ import annotations

import contextlib
import itertools
import os
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

from matcha.models.components import _ops as O

PKG = Path(__file__).resolve().parent.parent / "matcha-tts-etu-upmc-ensam_amd"
PRECISE = (False, "bf16x3", "bf16x6", "fp32")  # the columns of every grid below
SWITCHES = ((False, False), (True, False), (False, True), (True, True))  # rows: (process-wide split, parity_policy())
# EXPECTED[(prec, dgrad, one_plane)]: rows SWITCHES x columns PRECISE -> the packed kind.  128 literal entries.
_FP32 = ("0 0 0 0",
         "0 0 0 0",
         "0 0 0 0",
         "0 0 0 0")
_DGRAD = ("1 1 1 1",
          "1 1 1 1",
          "1 1 1 1",
          "1 1 1 1")
EXPECTED = {
    (0, False, False): _FP32, (0, False, True): _FP32, (0, True, False): _FP32, (0, True, True): _FP32,
    (1, True, False): _DGRAD, (1, True, True): _DGRAD,
    (1, False, False): ("1 2 3 0",    # nothing set
                        "2 2 3 0",    # set_weight_split(True)
                        "2 2 3 0",    # parity_policy()
                        "2 2 3 0"),   # both
    (1, False, True): ("1 2 3 0",
                       "2 2 3 0",     # the process-wide split alone ignores one_plane
                       "1 2 3 0",     # the policy honours it, precise_forward overrides it
                       "1 2 3 0"),
}


def _spec(dgrad=False, one_plane=False):
    return O.PackSpec(("probe",), 8, 8, [], dgrad, one_plane)


def _state():
    """Everything the legacy names show of the policy: (split enabled, ambient encoder precision, the kind of a
    bf16 forward operand, the kind of a one-plane one)."""
    return (O.weight_split_enabled(), O.encoder_precision_default(), O._pack_kind(_spec(), O.PREC_BF16),
            O._pack_kind(_spec(one_plane=True), O.PREC_BF16))


DEFAULT = (False, "bf16", 1, 1)


@pytest.fixture(autouse=True)
def _clean():
    assert _state() == DEFAULT
    yield
    assert _state() == DEFAULT


def test_constants():
    assert (O.PREC_FP32, O.PREC_BF16, O.PACK_BF16_SPLIT, O.PACK_BF16_SPLIT3) == (0, 1, 2, 3)


def test_pack_kind_truth_table():
    seen = 0
    for (prec, dgrad, one_plane), grid in EXPECTED.items():
        for (split, parity), row in zip(SWITCHES, grid):
            for precise, want in zip(PRECISE, row.split()):
                old = O.set_weight_split(split)
                try:
                    with (O.parity_policy() if parity else contextlib.nullcontext()), O.precise_forward(precise):
                        got = O._pack_kind(_spec(dgrad, one_plane), prec)
                finally:
                    O.set_weight_split(old)
                assert got == int(want), (prec, dgrad, one_plane, split, parity, precise, got, want)
                seen += 1
    assert seen == 128 and len(EXPECTED) == 8
    assert set(EXPECTED) == set(itertools.product((0, 1), (False, True), (False, True)))


def test_precise_forward_true_is_bf16x3():
    with O.precise_forward():
        assert O._pack_kind(_spec(), O.PREC_BF16) == O.PACK_BF16_SPLIT
    with O.precise_forward(True):
        assert O._pack_kind(_spec(), O.PREC_BF16) == O.PACK_BF16_SPLIT


@pytest.mark.parametrize("ctx,inside", [
    (lambda: O.precise_forward(), (False, "bf16", 2, 2)),
    (lambda: O.precise_forward("bf16x6"), (False, "bf16", 3, 3)),
    (lambda: O.precise_forward("fp32"), (False, "bf16", 0, 0)),
    (lambda: O.parity_policy(), (True, None, 2, 1)),
])
def test_context_restores_when_body_raises(ctx, inside):
    want = tuple(O.encoder_precision_for_parity() if v is None else v for v in inside)
    with pytest.raises(RuntimeError, match="body"):
        with ctx():
            assert _state() == want
            raise RuntimeError("body")
    assert _state() == DEFAULT


def test_nested_contexts_unwind_in_order():
    enc = O.encoder_precision_for_parity()
    with O.parity_policy():
        assert _state() == (True, enc, 2, 1)
        with O.precise_forward("fp32"):
            assert _state() == (True, enc, 0, 0)
            with O.precise_forward("bf16x6"):
                assert _state() == (True, enc, 3, 3)
                with O.precise_forward(False):
                    assert _state() == (True, enc, 2, 1)
                    with O.parity_policy(False):
                        assert _state() == DEFAULT
                    assert _state() == (True, enc, 2, 1)
                assert _state() == (True, enc, 3, 3)
            assert _state() == (True, enc, 0, 0)
        assert _state() == (True, enc, 2, 1)
        with pytest.raises(RuntimeError):
            with O.precise_forward(), O.parity_policy(False):
                assert _state() == (False, "bf16", 2, 2)
                raise RuntimeError("body")
        assert _state() == (True, enc, 2, 1)
    assert _state() == DEFAULT


def test_set_weight_split_returns_previous_and_is_process_wide():
    assert O.set_weight_split(True) is False
    try:
        assert _state() == (True, "bf16", 2, 2)
        assert O.set_weight_split(True) is True
        assert O.set_weight_split(1) is True  # any truthy value; stored as a bool
        assert O.weight_split_enabled() is True
        # not a context variable: a fresh thread (autograd's device thread) sees it, and none of the contexts
        import threading

        seen = []
        with O.parity_policy(), O.precise_forward("fp32"):
            th = threading.Thread(target=lambda: seen.append(_state()))
            th.start()
            th.join()
        assert seen == [(True, "bf16", 2, 2)]
    finally:
        assert O.set_weight_split(False) is True
    assert O.set_weight_split(False) is False


def test_parity_policy_off_leaves_the_process_wide_split_in_force():
    enc = O.encoder_precision_for_parity()
    with O.parity_policy(False):
        assert _state() == DEFAULT
    old = O.set_weight_split(True)
    try:
        with O.parity_policy(False):  # split still on, one_plane ignored (no policy), ambient encoder bf16
            assert _state() == (True, "bf16", 2, 2)
        with O.parity_policy():
            assert _state() == (True, enc, 2, 1)
            with O.parity_policy(False):
                assert _state() == (True, "bf16", 2, 2)
            assert _state() == (True, enc, 2, 1)
    finally:
        O.set_weight_split(old)


def test_encoder_precision_defaults():
    assert O.encoder_precision_default() == "bf16"
    assert O.encoder_precision_for_parity() == os.environ.get("MTTS_PARITY_ENCODER", "fp32fwd")
    with O.parity_policy():
        assert O.encoder_precision_default() == O.encoder_precision_for_parity()
        with O.precise_forward("fp32"):  # the encoder's own context does not change the ambient name
            assert O.encoder_precision_default() == O.encoder_precision_for_parity()
    old = O.set_weight_split(True)  # the process-wide split is not the policy: the encoder stays bf16
    try:
        assert O.encoder_precision_default() == "bf16"
    finally:
        O.set_weight_split(old)


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from matcha.models.components import _ops as O
with O.parity_policy():
    inside = O.encoder_precision_default()
    one = O._pack_kind(O.spec_linear((__import__("torch").zeros(8, 8),), one_plane=not O._FF1_SPLIT), O.PREC_BF16)
print(repr((O._FF1_SPLIT, O.encoder_precision_for_parity(), inside, O.encoder_precision_default(), one)))
"""


@pytest.mark.parametrize("env,want", [
    ({}, (False, "fp32fwd", "fp32fwd", "bf16", 1)),
    ({"MTTS_PARITY_FF1_SPLIT": "1"}, (True, "fp32fwd", "fp32fwd", "bf16", 2)),
    ({"MTTS_PARITY_FF1_SPLIT": "0"}, (False, "fp32fwd", "fp32fwd", "bf16", 1)),
    ({"MTTS_PARITY_ENCODER": "bf16x6"}, (False, "bf16x6", "bf16x6", "bf16", 1)),
], ids=["default", "ff1_split", "ff1_split_0", "encoder_bf16x6"])
def test_environment_switches_in_a_fresh_process(env, want):
    """Read at import, so each in a child process: (_FF1_SPLIT, the parity encoder, the ambient encoder inside and
    outside parity_policy(), the kind the FF up-projection's spec packs as under the policy)."""
    e = {k: v for k, v in os.environ.items() if k not in ("MTTS_PARITY_FF1_SPLIT", "MTTS_PARITY_ENCODER")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(PKG)], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == repr(want)


class _Autocast:
    """Stands in for torch.autocast (which switches itself off on a machine without the device): records the
    regions entered."""
    active: list = []

    def __init__(self, device_type, dtype=None, enabled=True, cache_enabled=None):
        self.args = (device_type, dtype, enabled)

    def __enter__(self):
        _Autocast.active.append(self.args)
        return self

    def __exit__(self, *exc):
        _Autocast.active.pop()
        return False


def _trainer_state():
    return (tuple(_Autocast.active), O.weight_split_enabled(), O.encoder_precision_default())


AMP = ("cuda", torch.bfloat16, True)
TRAINER_STATES = {"32-true": ((), False, "bf16"), "bf16-mixed": ((AMP,), False, "bf16"),
                  "bf16-parity": ((AMP,), True, None)}


def _trainer_autocast(name):
    from matcha.training import Trainer

    return Trainer._autocast(types.SimpleNamespace(cfg=types.SimpleNamespace(precision=name), dev=torch.device("cuda")))


def _precision_context(name):
    from matcha.precision import precision_context

    return precision_context(name)


def _shared_table(name):
    from matcha.models.components._policy import trainer_precision

    return trainer_precision(name)


def test_precision_name_table_is_shared():
    from matcha.models.components import _policy
    from matcha.precision import PRECISIONS

    assert PRECISIONS == tuple(_policy.TRAINER_PRECISIONS) == tuple(TRAINER_STATES)
    with pytest.raises(KeyError):
        with _policy.trainer_precision("fp16-mixed"):
            pass
    with pytest.raises(KeyError):  # an unknown text-encoder precision is an error too, not a bf16 encoder
        _policy.encoder_context("fp16", "cuda")


@pytest.mark.parametrize("name", list(TRAINER_STATES))
@pytest.mark.parametrize("enter", [_trainer_autocast, _precision_context, _shared_table],
                         ids=["trainer", "precision_context", "table"])
def test_trainer_precision_names(monkeypatch, enter, name):
    monkeypatch.setattr(torch, "autocast", _Autocast)
    want = tuple(O.encoder_precision_for_parity() if v is None else v for v in TRAINER_STATES[name])
    with enter(name):
        assert _trainer_state() == want
    assert _trainer_state() == ((), False, "bf16")
    with pytest.raises(RuntimeError, match="body"):
        with enter(name):
            raise RuntimeError("body")
    assert _trainer_state() == ((), False, "bf16")


def test_trainer_autocast_off_the_device(monkeypatch):
    from matcha.training import Trainer

    monkeypatch.setattr(torch, "autocast", _Autocast)
    for name in TRAINER_STATES:
        me = types.SimpleNamespace(cfg=types.SimpleNamespace(precision=name), dev=torch.device("cpu"))
        with Trainer._autocast(me):
            assert _trainer_state() == ((), False, "bf16")


def test_precision_context_extra_duties(monkeypatch):
    """Besides the Trainer's contexts: the process-wide split is forced off and model.encoder_precision cleared for
    the duration, both restored after (also when the body raises); an unknown name is refused."""
    from matcha.precision import precision_context

    monkeypatch.setattr(torch, "autocast", _Autocast)
    model = types.SimpleNamespace(encoder_precision="bf16x3")
    old = O.set_weight_split(True)
    try:
        for name, want in TRAINER_STATES.items():
            want = tuple(O.encoder_precision_for_parity() if v is None else v for v in want)
            with pytest.raises(RuntimeError, match="body"):
                with precision_context(name, model):
                    assert _trainer_state() == want and model.encoder_precision is None
                    assert O._pack_kind(_spec(one_plane=True), O.PREC_BF16) == 1
                    raise RuntimeError("body")
            assert O.weight_split_enabled() is True and model.encoder_precision == "bf16x3"
        with pytest.raises(ValueError):
            with precision_context("fp16-mixed", model):
                pass
        assert O.weight_split_enabled() is True and model.encoder_precision == "bf16x3"
    finally:
        O.set_weight_split(old)


@pytest.mark.parametrize("own,kind,amp", [(None, 1, ()), ("bf16", 1, ()), ("bf16x3", 2, ()), ("bf16x6", 3, ()),
                                          ("fp32fwd", 0, ()), ("fp32", 1, (("cuda", None, False),))])
def test_model_encoder_context(monkeypatch, own, kind, amp):
    """MatchaTTS._encoder_ctx: the model's own encoder_precision, else the ambient one, as a context."""
    from matcha.models.matcha_tts import MatchaTTS

    monkeypatch.setattr(torch, "autocast", _Autocast)
    me = types.SimpleNamespace(encoder_precision=own)
    with MatchaTTS._encoder_ctx(me, "cuda"):
        assert (O._pack_kind(_spec(), O.PREC_BF16), tuple(_Autocast.active)) == (kind, amp)
    assert tuple(_Autocast.active) == ()
    with O.parity_policy():  # the ambient default applies only where the model sets none
        ambient = {"fp32fwd": 0, "bf16x6": 3}[O.encoder_precision_for_parity()]
        with MatchaTTS._encoder_ctx(me, "cuda"):
            assert O._pack_kind(_spec(), O.PREC_BF16) == (ambient if own is None else 2 if kind == 1 else kind)


def test_model_encoder_fp32_property():
    from matcha.models.matcha_tts import MatchaTTS

    assert MatchaTTS.encoder_precision is None
    me = MatchaTTS.__new__(MatchaTTS)
    torch.nn.Module.__init__(me)
    assert me.encoder_fp32 is False
    me.encoder_fp32 = True
    assert me.encoder_precision == "fp32" and me.encoder_fp32 is True
    me.encoder_fp32 = False
    assert me.encoder_precision is None
