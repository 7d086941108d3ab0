"""The HiFi-GAN vocoder's Python surface without a GPU: parameter names, weight-norm folding, checkpoint formats,
save_wav, config validation, the device-only rule, and the test restatement (tests/hifigan_ref.py) against the
fixture the reference's own Generator produced (tests/golden/_hifigan_golden.py)."""
from __future__ import annotations

import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from golden.weights_recipe import apply_recipe
from hifi_gan import AttrDict, Generator, save_wav
from hifigan_ref import CONFIGS, RefGenerator
from matcha import _native as N

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "hifigan_golden.npz")
CASES = sorted(CONFIGS)


def _model(case, cls=Generator):
    m = cls(AttrDict(CONFIGS[case]))
    apply_recipe(m, int(GOLD[case + "/seed"]))
    return m.eval()


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_equal_the_reference(case):
    want = [str(k) for k in GOLD[case + "/keys"]]
    assert list(Generator(AttrDict(CONFIGS[case])).state_dict().keys()) == want
    assert list(RefGenerator(AttrDict(CONFIGS[case])).state_dict().keys()) == want
    assert "conv_pre.weight_g" in want and "ups.0.weight_v" in want


@pytest.mark.parametrize("case", CASES)
def test_folded_weights_equal_torch_remove_weight_norm_bitwise(case):
    m = _model(case)
    folded = {k: v.clone() for k, v in m.folded_weights().items()}
    ref = _model(case, RefGenerator)
    for mod in ref.modules():
        if hasattr(mod, "weight_g"):
            torch.nn.utils.remove_weight_norm(mod)
    want = {k: v for k, v in ref.state_dict().items() if k.endswith(".weight")}
    assert sorted(folded) == sorted(want) and len(want) > 10
    for k in want:
        assert torch.equal(folded[k], want[k]), k
    m.remove_weight_norm()  # the module's own fold is the same tensor, and folding twice is harmless
    assert not any(k.endswith(("weight_g", "weight_v")) for k in m.state_dict())
    for k, v in m.folded_weights().items():
        assert torch.equal(v, want[k]), k
    m.remove_weight_norm()


def test_plain_weight_checkpoint_loads():
    src = _model("v3_small")
    want = {k: v.clone() for k, v in src.folded_weights().items()}
    sd = _model("v3_small").remove_weight_norm().state_dict()
    assert "conv_pre.weight" in sd and "conv_pre.weight_g" not in sd
    dst = Generator(AttrDict(CONFIGS["v3_small"]))
    dst.load_state_dict(sd)
    for k, v in dst.folded_weights().items():
        assert torch.equal(v, want[k]), k
    # and the weight-normed form, as a published checkpoint holds it under "generator"
    dst2 = Generator(AttrDict(CONFIGS["v3_small"]))
    dst2.load_state_dict({"generator": src.state_dict()}["generator"])
    for k, v in dst2.folded_weights().items():
        assert torch.equal(v, want[k]), k


def test_save_wav_round_trip(tmp_path):
    x = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.7, -3.0, 0.25])
    save_wav(tmp_path / "a.wav", x.view(1, -1), 22050)
    with wave.open(str(tmp_path / "a.wav"), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 22050, 8)
        pcm = np.frombuffer(f.readframes(8), "<i2")
    want = np.round(np.clip(x.numpy().astype(np.float64), -1, 1) * 32767).astype(np.int16)
    assert np.array_equal(pcm, want) and pcm[5] == 32767 and pcm[6] == -32767
    with pytest.raises(ValueError):
        save_wav(tmp_path / "b.wav", torch.zeros(2, 8), 22050)


@pytest.mark.parametrize("change", [
    dict(resblock_kernel_sizes=[3, 7, 13]),  # k > 11
    dict(resblock_kernel_sizes=[3, 4, 11]),  # even k
    dict(upsample_kernel_sizes=[16, 15, 4, 4]),  # k_up != 2u
    dict(upsample_initial_channel=64),  # 64 / 2^4 = 4 channels in the last stage
])
def test_unsupported_configs_raise_at_construction(change):
    with pytest.raises(ValueError):
        Generator(AttrDict(dict(CONFIGS["v1_small"], **change)))


def test_cpu_tensors_are_refused():
    m = _model("v3_small")
    with pytest.raises(N.NativeError):
        m(torch.zeros(1, 80, 4))


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference_fixture(case):
    """Both run torch's CPU convs on the same weights in the same op order, and on the machine that wrote the
    fixture the fp32 outputs are bitwise equal (printed below).  The assertion allows 1e-6 (the reference's own
    fp32 error against float64 is 2.4e-6) because torch's CPU conv picks its kernel, and with it the summation
    order, by the host's vector ISA and thread count: another host may legitimately differ in the last bits."""
    m = _model(case, RefGenerator)
    with torch.no_grad():
        y = m(torch.from_numpy(GOLD[case + "/mel"]))
        y64 = m.double()(torch.from_numpy(GOLD[case + "/mel"]).double())
    err = np.abs(y.numpy().astype(np.float64) - GOLD[case + "/out_f32"]).max()
    print(f"{case}: fp32 restatement vs fixture max abs {err:.3e}, bitwise {np.array_equal(y.numpy(), GOLD[case + '/out_f32'])}")
    assert err <= 1e-6
    assert np.abs(y64.numpy() - GOLD[case + "/out_f64"]).max() <= 1e-9
