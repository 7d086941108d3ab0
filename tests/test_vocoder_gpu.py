"""The HiFi-GAN vocoder on the MI355X: every kernel of include/mtts_vocoder.h against torch CPU float64 computed
here, the whole generator against the reference's fixture (tests/golden/_hifigan_golden.py) and the restatement
(tests/hifigan_ref.py), graph replay, determinism and MatchaTTS.synthesise(vocoder=).

Bounds: an op's max abs error <= 2e-5 * max|ref| (the project's fp32 op bound); conv_post
2e-5 absolute; the whole generator 1e-4 on the [-1, 1] signal."""
from __future__ import annotations

import itertools
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden.weights_recipe import apply_recipe
from hifi_gan import AttrDict, Generator
from hifi_gan import ops as V
from hifigan_ref import CONFIGS, RefGenerator

pytestmark = pytest.mark.gpu

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "hifigan_golden.npz")
DEV = torch.device("cuda:0")
OP_BOUND = 2e-5


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _close(got, ref, what, bound=OP_BOUND):
    ref = ref.double()
    err = float((got.double().cpu() - ref).abs().max())
    lim = bound * float(ref.abs().max())
    print(f"{what}: max abs err {err:.3e} (bound {lim:.3e})")
    assert torch.isfinite(got).all() and err <= lim, (what, err, lim)


def _ref_conv(a, w, bias, B, L, d, leaky, slope):
    """a [B*L, cin] -> float64 [B*L, N] of the "same" dilated Conv1d on the (leaky) input."""
    x = a.double().view(B, L, -1).transpose(1, 2)
    if leaky:
        x = F.leaky_relu(x, slope)
    k = w.shape[-1]
    y = F.conv1d(x, w.double(), bias.double(), padding=(k - 1) // 2 * d, dilation=d)
    return y.transpose(1, 2).reshape(B * L, -1)


EPILOGUES = ["plain", "leaky", "residual", "acc_init", "acc_add", "acc_mean"]


def _conv_cases():
    cases = []
    for i, (k, d, L) in enumerate(itertools.product([3, 7, 11], [1, 3, 5], [1, 7, 24, 129, 1000])):
        C = [8, 32, 64][(i // 6) % 3]  # the three walk at different periods: every epilogue meets both B,
        cases.append((k, d, C, C, [1, 3][(i // 6 + i) % 2], L, EPILOGUES[i % 6]))  # several C and several L
    cases.append((7, 1, 80, 64, 3, 129, "leaky"))  # N != cin, a channel chunk of 16
    cases.append((3, 1, 512, 512, 1, 40, "residual"))  # the widest published layer
    cases.append((11, 5, 512, 512, 1, 40, "acc_mean"))
    return cases


CONV_CASES = _conv_cases()


def test_conv_cases_cover_every_listed_value():
    col = lambda j: {c[j] for c in CONV_CASES}  # noqa: E731
    assert col(0) == {3, 7, 11} and col(1) == {1, 3, 5} and {8, 32, 64, 80, 512} == col(2)
    assert col(4) == {1, 3} and {1, 7, 24, 129, 1000} <= col(5) and col(6) == set(EPILOGUES)


@pytest.mark.parametrize("k,d,cin,N,B,L,epi", CONV_CASES)
def test_conv(k, d, cin, N, B, L, epi):
    seed = 1000 * k + 100 * d + L + cin
    a = _rand(B * L, cin, seed=seed)
    w = _rand(N, cin, k, seed=seed + 1) / (cin * k) ** 0.5
    bias = _rand(N, seed=seed + 2) * 0.1
    leaky = epi != "plain"
    v = _ref_conv(a, w, bias, B, L, d, leaky, 0.1)
    ad, wp, bd = a.to(DEV), V.pack_conv(w).to(DEV), bias.to(DEV)
    kw = dict(leaky=leaky, slope=0.1)
    if epi in ("plain", "leaky"):
        _close(V.conv(ad, wp, bd, B, L, k, d, **kw), v, epi)
    elif epi == "residual":  # C aliases the residual
        r = _rand(B * L, N, seed=seed + 3)
        buf = r.to(DEV)
        out = V.conv(ad, wp, bd, B, L, k, d, residual=buf, out=buf, **kw)
        assert out.data_ptr() == buf.data_ptr()
        _close(out, v + r.double(), epi)
    else:
        acc0 = _rand(B * L, N, seed=seed + 4)
        r = _rand(B * L, N, seed=seed + 3)
        acc = torch.full((B * L, N), float("nan"), device=DEV) if epi == "acc_init" else acc0.to(DEV)
        mode = {"acc_init": V.ACC_INIT, "acc_add": V.ACC_ADD, "acc_mean": V.ACC_MEAN}[epi]
        want_out = epi != "acc_mean"  # the last conv of a stage's last resblock writes only the mean
        out = V.conv(ad, wp, bd, B, L, k, d, residual=r.to(DEV), acc=acc, acc_mode=mode, acc_div=3.0,
                     want_out=want_out, **kw)
        vr = v + r.double()
        if want_out:
            _close(out, vr, epi + " C")
        else:
            assert out is None
        want = {"acc_init": vr, "acc_add": acc0.double() + vr, "acc_mean": (acc0.double() + vr) / 3.0}[epi]
        _close(acc, want, epi + " acc")


def test_conv_never_reads_the_neighbouring_utterance():
    """B = 3 with utterances 0 and 2 filled with 1e30: utterance 1 equals the B = 1 run bitwise."""
    k, d, C, L = 11, 5, 32, 129
    a1 = _rand(L, C, seed=77)
    w = _rand(C, C, k, seed=78) / (C * k) ** 0.5
    bias = _rand(C, seed=79)
    wp, bd = V.pack_conv(w).to(DEV), bias.to(DEV)
    a3 = torch.full((3, L, C), 1e30)
    a3[1] = a1
    one = V.conv(a1.to(DEV), wp, bd, 1, L, k, d, leaky=True)
    three = V.conv(a3.view(3 * L, C).to(DEV), wp, bd, 3, L, k, d, leaky=True)
    _close(one, _ref_conv(a1, w, bias, 1, L, d, True, 0.1), "B = 1")
    assert torch.equal(three[L:2 * L], one)
    for L in (1, 7):  # the halo is longer than the utterance
        s1 = V.conv(a1[:L].contiguous().to(DEV), wp, bd, 1, L, k, d)
        s3 = V.conv(a3[:, :L].reshape(3 * L, C).contiguous().to(DEV), wp, bd, 3, L, k, d)
        assert torch.equal(s3[L:2 * L], s1)


def test_conv_indexes_past_2_to_31_elements():
    """One utterance of 2^26 + 5 frames x 32 channels: element offsets cross 2^31 (the kernels index in 64 bits).
    The data is drawn on the device; windows at the start, around offset 2^31 and at the end are checked."""
    k, d, C, L = 3, 1, 32, (1 << 26) + 5
    a = torch.randn(L, C, device=DEV, generator=torch.Generator(DEV).manual_seed(11))
    w = _rand(C, C, k, seed=12) / (C * k) ** 0.5
    bias = _rand(C, seed=13) * 0.1
    out = V.conv(a, V.pack_conv(w).to(DEV), bias.to(DEV), 1, L, k, d, leaky=True)
    for lo, hi in ((0, 40), ((1 << 26) - 20, (1 << 26) + 5), (L - 40, L)):
        s0, s1 = max(lo - 1, 0), min(hi + 1, L)  # one halo frame each side where the utterance has one
        ref = _ref_conv(a[s0:s1].cpu(), w, bias, 1, s1 - s0, d, True, 0.1)[lo - s0:hi - s0]
        _close(out[lo:hi], ref, f"frames {lo}..{hi}")
    del a, out
    torch.cuda.empty_cache()


def test_conv_rejects_bad_shapes_and_aliasing_before_any_launch():
    a = torch.zeros(16, 16, device=DEV)
    out = torch.zeros(16, 16, device=DEV)
    w = lambda k, cin=16: torch.zeros(16, k * cin, device=DEV)  # noqa: E731
    assert V.conv_raw(a, w(13), None, 1, 16, 13, 1, out=out) == V.ERR_SHAPE  # k > 11
    assert V.conv_raw(a, w(4), None, 1, 16, 4, 1, out=out) == V.ERR_SHAPE  # even k
    assert V.conv_raw(a, w(3), None, 1, 16, 3, 0, out=out) == V.ERR_SHAPE  # d < 1
    a12 = torch.zeros(16, 12, device=DEV)
    assert V.conv_raw(a12, w(3, 12), None, 1, 16, 3, 1, out=out) == V.ERR_SHAPE  # cin % 8
    assert V.conv_raw(a, w(3), None, 1, 16, 3, 1, out=a) == V.ERR_INVALID_ARG  # C aliases A
    assert V.conv_raw(a, w(3), None, 1, 16, 3, 1, out=out, acc=a, acc_mode=V.ACC_ADD) == V.ERR_INVALID_ARG
    assert V.conv_raw(a, w(3), None, 1, 16, 3, 1) == V.ERR_INVALID_ARG  # nothing to write
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(a.abs().max()) == 0.0


@pytest.mark.parametrize("k,u,cin,cout,B,L", [
    (k, u, cin, cout, B, L) for (k, u), (cin, cout), B, L in
    itertools.product([(16, 8), (4, 2), (8, 4)], [(16, 8), (128, 64)], [1, 2], [1, 5, 33])])
def test_upsample(k, u, cin, cout, B, L):
    seed = 10 * k + cin + 3 * L + B
    a = _rand(B * L, cin, seed=seed)
    w = _rand(cin, cout, k, seed=seed + 1) / (2 * cin) ** 0.5
    bias = _rand(cout, seed=seed + 2) * 0.1
    x = F.leaky_relu(a.double().view(B, L, cin).transpose(1, 2), 0.1)
    ref = F.conv_transpose1d(x, w.double(), bias.double(), stride=u, padding=(k - u) // 2)
    assert ref.shape == (B, cout, L * u)
    ref = ref.transpose(1, 2).reshape(B * L * u, cout)
    got = V.upsample(a.to(DEV), V.pack_upsample(w, u).to(DEV), bias.to(DEV), B, L, k, u, 0.1)
    assert got.shape == ref.shape
    _close(got, ref, "upsample")
    g, r = got.view(B, L * u, cout).cpu().double(), ref.view(B, L * u, cout)
    lim = OP_BOUND * float(ref.abs().max())
    assert float((g[:, :u] - r[:, :u]).abs().max()) <= lim  # the first u samples: frame -1 is padding
    assert float((g[:, -u:] - r[:, -u:]).abs().max()) <= lim  # the last u: frame L is padding


def test_upsample_rejects_kernels_other_than_twice_the_rate():
    a, out = torch.zeros(8, 16, device=DEV), torch.zeros(24, 8, device=DEV)
    wp = torch.zeros(3 * 8, 2 * 16, device=DEV)
    assert V.upsample_raw(a, wp, None, out, 1, 8, 16, 8, 7, 3) == V.ERR_SHAPE
    assert V.upsample_raw(a, wp, None, out, 1, 8, 16, 8, 6, 3) == V.ERR_SHAPE  # odd rate: T*u + 1 samples in torch
    assert V.upsample_raw(a, wp, None, out, 1, 8, 16, 8, 16, 4) == V.ERR_SHAPE
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


@pytest.mark.parametrize("B,T,N", [(1, 1, 8), (2, 37, 64), (3, 130, 128)])
def test_pre(B, T, N):
    mel = _rand(B, 80, T, seed=T) * 1.5 - 5.5
    w = _rand(N, 80, 7, seed=T + 1) / 560 ** 0.5
    bias = _rand(N, seed=T + 2) * 0.1
    ref = F.conv1d(mel.double(), w.double(), bias.double(), padding=3).transpose(1, 2).reshape(B * T, N)
    _close(V.pre(mel.to(DEV), V.pack_conv(w).to(DEV), bias.to(DEV)), ref, "pre")


def _ref_post(a, w, bias, B, L, slope):
    x = F.leaky_relu(a.double().view(B, L, -1).transpose(1, 2), slope)
    return torch.tanh(F.conv1d(x, w.double(), bias.double(), padding=3))


@pytest.mark.parametrize("B,L,C", [(1, 1, 8), (2, 300, 8), (3, 1000, 32)])
def test_post(B, L, C):
    a = _rand(B * L, C, seed=L + C)
    w = _rand(1, C, 7, seed=L + 1) / (7 * C) ** 0.5
    bias = _rand(1, seed=L + 2) * 0.1
    got = V.post(a.to(DEV), V.pack_post(w).to(DEV), bias.to(DEV), B, L, 0.01)
    ref = _ref_post(a, w, bias, B, L, 0.01)
    assert got.shape == (B, 1, L)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"post: max abs err {err:.3e}")
    assert err <= 2e-5


def test_post_slope_is_torchs_default_not_lrelu_slope():
    """An all-negative input: with slope 0.1 instead of 0.01 the result would be far outside the bound."""
    B, L, C = 2, 257, 32
    a = -_rand(B * L, C, seed=5).abs() - 0.5
    w = _rand(1, C, 7, seed=6) / (7 * C) ** 0.5
    bias = torch.zeros(1)
    ref, wrong = _ref_post(a, w, bias, B, L, 0.01), _ref_post(a, w, bias, B, L, 0.1)
    assert float((ref - wrong).abs().max()) > 100 * 2e-5
    m = Generator(AttrDict(CONFIGS["v3_small"]))  # the generator passes POST_SLOPE itself
    from hifi_gan import models as M

    assert M.POST_SLOPE == 0.01 and M.LRELU_SLOPE == 0.1 and m.hop == 256
    got = V.post(a.to(DEV), V.pack_post(w).to(DEV), bias.to(DEV), B, L, M.POST_SLOPE)
    assert float((got.cpu().double() - ref).abs().max()) <= 2e-5


def _pair(case, seed=None):
    seed = int(GOLD[case + "/seed"]) if seed is None else seed
    m = Generator(AttrDict(CONFIGS[case]))
    apply_recipe(m, seed)
    ref = RefGenerator(AttrDict(CONFIGS[case]))
    apply_recipe(ref, seed)
    return m.to(DEV).eval(), ref.double().eval()


@pytest.mark.parametrize("case", sorted(CONFIGS))
def test_generator_against_the_reference_fixture(case):
    m, _ = _pair(case)
    with torch.no_grad():
        wav = m(torch.from_numpy(GOLD[case + "/mel"]).to(DEV))
    assert wav.shape == GOLD[case + "/out_f64"].shape
    err = float(np.abs(wav.cpu().numpy().astype(np.float64) - GOLD[case + "/out_f64"]).max())
    print(f"{case}: whole generator vs the reference in float64: max abs {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("case", sorted(CONFIGS))
@pytest.mark.parametrize("B,T", [(1, 3), (3, 50)])
def test_generator_against_the_restatement(case, B, T):
    m, ref = _pair(case)
    mel = _rand(B, 80, T, seed=B * T) * 1.5 - 5.5
    with torch.no_grad():
        want = ref(mel.double())
        wav = m(mel.to(DEV))
    assert wav.shape == (B, 1, T * m.hop)
    err = float((wav.cpu().double() - want).abs().max())
    print(f"{case} B={B} T={T}: max abs {err:.3e}, std {float(want.std()):.3f}")
    assert err <= 1e-4


def test_generator_refuses_a_mel_that_needs_a_gradient():
    m, _ = _pair("v3_small")
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 80, 4, device=DEV, requires_grad=True))


def test_graph_replay_equals_eager_and_eager_is_deterministic():
    m, _ = _pair("v3_small")
    assert Generator.graph is True
    mels = [(_rand(2, 80, 24, seed=s) * 1.5 - 5.5).to(DEV) for s in (1, 2, 3)]
    with torch.no_grad():
        replayed = [m(x) for x in mels]
        assert len(m._graphs) == 1
        other = m(mels[0][:, :, :11].contiguous())  # a second shape gets its own graph
        assert len(m._graphs) == 2 and other.shape == (2, 1, 11 * 256)
        m.graph = False
        eager = [m(x) for x in mels]
        again = [m(x) for x in mels]
        eager_other = m(mels[0][:, :, :11].contiguous())
    assert len(m._graphs) == 2
    for r, e, a in zip(replayed, eager, again):
        assert torch.equal(r, e) and torch.equal(e, a)
    assert torch.equal(other, eager_other)
    assert not torch.equal(replayed[0], replayed[1])


def test_repack_after_a_parameter_changes():
    m, _ = _pair("v3_small")
    mel = (_rand(1, 80, 8, seed=9) * 1.5 - 5.5).to(DEV)
    with torch.no_grad():
        before = m(mel)
        m.conv_post.bias.add_(0.25)
        after = m(mel)
    assert not torch.equal(before, after)


def test_synthesise_with_a_vocoder():
    from matcha.models.matcha_tts import MatchaTTS

    model = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(DEV)
    apply_recipe(model, 7)
    model.eval()
    voc, _ = _pair("v3_small")
    g = torch.Generator().manual_seed(3)
    xl = torch.tensor([9, 6])
    x = (torch.randint(1, 150, (2, 9), generator=g) * (torch.arange(9)[None] < xl[:, None])).to(DEV)
    plain = model.synthesise(x, xl.to(DEV), n_timesteps=2)
    assert set(plain) == {"encoder_outputs", "decoder_outputs", "attn", "mel", "mel_lengths", "rtf"}
    out = model.synthesise(x, xl.to(DEV), n_timesteps=2, vocoder=voc)
    assert set(out) == set(plain) | {"wav", "wav_lengths"}
    with torch.no_grad():
        want = voc(out["mel"]).squeeze(1).clamp(-1, 1)
    assert out["wav"].shape == (2, out["mel"].shape[-1] * 256) and torch.equal(out["wav"], want)
    assert torch.equal(out["wav_lengths"], out["mel_lengths"] * 256)
    assert float(out["wav"].abs().max()) <= 1.0
