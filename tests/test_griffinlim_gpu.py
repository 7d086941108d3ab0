"""Griffin-Lim on the MI355X (include/mtts_griffinlim.h, matcha/utils/audio_process.py) against the float64
restatement on torch.stft / torch.istft (tests/griffinlim_ref.py), computed here on the CPU.

Bounds.  One op (inverse mel, synthesis + gather, analysis): max abs error <= 2e-5 * max|ref| against float64, the
project's fp32 op bound.  A whole run divides by |reb - m * tprev|, ill-conditioned where that is
near zero, so no fixed bound can be derived: the same restatement run in fp32 on the CPU measures what fp32 costs on
that input, and the HIP error must stay within max(2e-5, 4 * err_torch_fp32) * max|ref| -- the factor 4 for another
FFT factorisation and summation order; a wrong twiddle, momentum or envelope is off by orders of magnitude.
Each shape's input seed is the one griffinlim_ref.SEEDS names, chosen from CPU runs alone (the rule is stated there).
Quality: the spectral convergence of the HIP waveform is at most 1.01 x the float64 reference's."""
from __future__ import annotations

import functools

import pytest
import torch

import griffinlim_ref as R
from matcha.utils.audio_process import GriffinLim, GriffinLimVocoder, InverseMelScale

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OP_BOUND = 2e-5
SHAPES = [(B, F) for F in (4, 5, 9, 40) for B in (1, 3)]
HOP = 256


def _err(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())


def _close(got, ref, what, bound=OP_BOUND):
    err, top = _err(got, ref)
    print(f"{what}: max abs err {err:.3e} = {err / max(top, 1e-300):.3e} x max|ref| (bound {bound:.3e})")
    assert torch.isfinite(got).all() and err <= bound * top, (what, err, bound * top)


def _gl(n_iter, **kw):
    return GriffinLim(n_fft=1024, n_iter=n_iter, hop_length=256, win_length=1024, power=1.0, **kw)


@functools.lru_cache(maxsize=None)
def _ref_run(B, F, n_iter):
    """(float64 waveform, err of the fp32 CPU run relative to max|ref|) with the injected [0, 1)^2 angles."""
    c = R.case(B, F)
    ref = R.griffinlim(c["lin"], c["angles_rand"], n_iter)
    w32 = R.griffinlim(c["lin"], c["angles_rand"], n_iter, dtype=torch.float32)
    err, top = _err(w32, ref)
    return ref, err / top


# ---- the operators ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_input", [True, False])
@pytest.mark.parametrize("B,F", SHAPES + [(2, 130)])  # 130: three frame tiles, the last partial
def test_inverse_mel(B, F, log_input):
    log_mel = R.case(B, F)["log_mel"]
    x = log_mel if log_input else torch.exp(log_mel)
    ref = R.inverse_mel(torch.exp(log_mel.double()) if log_input else x.double())
    got = InverseMelScale(513, 80, 22050, 0.0, 8000.0)(x.to(DEV), log_input=log_input)
    assert got.shape == (B, 513, F) and got.dtype == torch.float32
    _close(got, ref, f"inverse mel B={B} F={F} log={log_input}")
    assert not got[:, 372:].any(), "bins above 8 kHz must be exactly zero"
    assert float(got.min()) >= 0.0


@pytest.mark.parametrize("angles", ["angles_unit", "angles_rand"])
@pytest.mark.parametrize("B,F", SHAPES)
def test_synthesis_and_gather_zero_iterations(B, F, angles):
    c = R.case(B, F)
    ref = R.istft(c["lin"].double() * c[angles].to(torch.complex128))
    got = _gl(0)(c["lin"].to(DEV), angles=c[angles].to(DEV))
    assert got.shape == (B, (F - 1) * HOP)
    _close(got, ref, f"istft B={B} F={F} {angles}")


@pytest.mark.parametrize("B,F", SHAPES)
def test_known_answer_on_the_device(B, F):
    c = R.case(B, F)
    S = c["S"].float()
    angles = (c["X"] / c["S"].clamp(min=1e-300)).to(torch.complex64)
    got = _gl(0)(S.to(DEV), angles=angles.to(DEV))
    _close(got, c["x"], f"known answer B={B} F={F}")


@pytest.mark.parametrize("B,F", SHAPES)
def test_analysis_first_iteration(B, F):
    c = R.case(B, F)
    _, reb = R.griffinlim(c["lin"], c["angles_rand"], 1, first=True)
    got = _gl(1).rebuilt(c["lin"].to(DEV), angles=c["angles_rand"].to(DEV))
    assert got.shape == (B, 513, F) and got.is_complex()
    _close(torch.view_as_real(got), torch.view_as_real(reb), f"stft(istft) B={B} F={F}")


# ---- whole runs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [1, 4, 32])
@pytest.mark.parametrize("B,F", SHAPES)
def test_whole_run(B, F, n_iter):
    c = R.case(B, F)
    ref, e32 = _ref_run(B, F, n_iter)
    got = _gl(n_iter)(c["lin"].to(DEV), angles=c["angles_rand"].to(DEV))
    print(f"B={B} F={F} n_iter={n_iter}: err_torch_fp32 {e32:.3e} x max|ref|")
    _close(got, ref, f"whole run B={B} F={F} n_iter={n_iter}", bound=max(OP_BOUND, 4 * e32))


@pytest.mark.parametrize("B,F", [(1, 40), (3, 40), (3, 9)])
def test_quality_spectral_convergence(B, F):
    c = R.case(B, F)
    ref, _ = _ref_run(B, F, 32)
    got = _gl(32)(c["lin"].to(DEV), angles=c["angles_rand"].to(DEV)).cpu()
    sc_ref, sc_hip = R.spectral_convergence(ref, c["lin"]), R.spectral_convergence(got, c["lin"])
    print(f"spectral convergence B={B} F={F}: hip {sc_hip:.4f}, float64 {sc_ref:.4f}")
    assert sc_hip <= 1.01 * sc_ref


def test_silence_stays_finite():
    inv, gl = InverseMelScale(513, 80, 22050, 0.0, 8000.0), _gl(32)
    mel = torch.exp(R.case(3, 9)["log_mel"]).to(DEV)
    wav = gl(inv(torch.zeros_like(mel)))  # 0 / (0 + 1e-16) stays 0
    assert torch.isfinite(wav).all() and not wav.any()
    mel[1] = 0.0
    wav = gl(inv(mel))
    assert torch.isfinite(wav).all() and not wav[1].any() and wav[0].any() and wav[2].any()
    out = GriffinLimVocoder(n_iter=4)(torch.full((2, 80, 9), -11.5129, device=DEV))  # log(1e-5): the model's silence
    assert torch.isfinite(out).all() and float(out.abs().max()) < 1e-2


# ---- determinism, graph, random phase ---------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal():
    c = R.case(3, 9)
    gl = _gl(32)
    lin, ang = c["lin"].to(DEV), c["angles_rand"].to(DEV)
    assert torch.equal(gl(lin, angles=ang), gl(lin, angles=ang))


def test_graph_replay_equals_eager_and_caches_per_shape():
    gl, eager = _gl(4), _gl(4)
    eager.graph = False
    for n, (B, F) in enumerate([(3, 9), (1, 5)], 1):
        c = R.case(B, F)
        lin, ang = c["lin"].to(DEV), c["angles_rand"].to(DEV)
        first = gl(lin, angles=ang)  # captures, then replays
        again = gl(lin, angles=ang)  # replays
        assert len(gl._graphs) == n
        want = eager(lin, angles=ang)
        assert torch.equal(first, want) and torch.equal(again, want)
    assert not eager._graphs
    for F in range(10, 20):  # the cache is bounded
        gl(torch.rand(1, 513, F, device=DEV))
    assert len(gl._graphs) == GriffinLim._GRAPH_CACHE_MAX == 8
    first, second = list(gl._graphs)[:2]  # ... and evicts the least recently used shape, not the oldest capture
    gl(torch.rand(1, 513, first[1], device=DEV))
    gl(torch.rand(1, 513, 20, device=DEV))
    assert first in gl._graphs and second not in gl._graphs and len(gl._graphs) == 8


def test_rand_init_draws_from_torchs_generator():
    lin = R.case(1, 9)["lin"].to(DEV)
    gl = _gl(4)
    torch.manual_seed(5)
    a = gl(lin)
    b = gl(lin)
    torch.manual_seed(5)
    a2 = gl(lin)
    assert not torch.equal(a, b) and torch.equal(a, a2)
    assert torch.isfinite(a).all() and a.any()


@pytest.mark.parametrize("B,F", [(1, 9), (3, 5)])
def test_rand_init_false_starts_from_the_ones_phase(B, F):
    """torchaudio's rand_init=False: the phase 1 + 0i in every bin; repeatable without a seed.  Against float64 at
    zero iterations (one istft: the op bound) and at one (the whole-run bound); at four iterations the result is
    bitwise the one of the injected ones phase, the path test_whole_run checks.  (A real spectrum makes every frame
    an impulse at its centre, so the fp32 istft -- torch's as much as this one -- already costs 1e-4 of the peak
    after one iteration: that is precision, not chaos, and the fp32 CPU run measures it.)"""
    c = R.case(B, F)
    lin = c["lin"].to(DEV)
    ones = torch.ones(B, 513, F, dtype=torch.complex64)
    for n_iter in (0, 1):
        ref = R.griffinlim(c["lin"], ones, n_iter)
        err32, top = _err(R.griffinlim(c["lin"], ones, n_iter, dtype=torch.float32), ref)
        print(f"B={B} F={F} ones phase, n_iter={n_iter}: err_torch_fp32 {err32 / top:.3e} x max|ref|")
        bound = OP_BOUND if n_iter == 0 else max(OP_BOUND, 4 * err32 / top)
        _close(_gl(n_iter, rand_init=False)(lin), ref, f"rand_init=False B={B} F={F} n_iter={n_iter}", bound=bound)
    gl = _gl(4, rand_init=False)
    a = gl(lin)
    torch.rand(3, device=DEV)  # the generator moves on; the result must not
    b = gl(lin)
    assert torch.equal(a, b)
    assert torch.equal(a, _gl(4)(lin, angles=ones.to(DEV)))
    assert torch.isfinite(a).all() and a.any()


def test_synthesis_refuses_frames_aliasing_an_input():
    from matcha import _native as N

    B, F = 1, 4
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    lin, reb, frames, tw, win = z(B, F, 513), z(B, F, 513, 2), z(B, F, 1024), z(1024, 2), z(1024)
    call = lambda reb_, tprev_, fr_: N.lib().mtts_gl_synthesis(  # noqa: E731
        N.ptr(lin), N.ptr(reb_), N.ptr(tprev_), 0.5, 1, N.ptr(tw), N.ptr(win), N.ptr(fr_), B, F, 1024, 256,
        N.stream_handle(DEV))
    assert call(reb, frames, frames) == -1  # frames is tprev
    assert call(frames, None, frames) == -1  # frames is reb
    assert N.lib().mtts_gl_synthesis(N.ptr(frames), N.ptr(reb), None, 0.5, 1, N.ptr(tw), N.ptr(win), N.ptr(frames), B,
                                     F, 1024, 256, N.stream_handle(DEV)) == -1  # frames is lin
    torch.cuda.synchronize()


# ---- the vocoder ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 4), (3, 9)])
def test_vocoder_shape_and_padding(B, T):
    c = R.case(B, T)
    voc = GriffinLimVocoder(n_iter=4)
    out = voc(c["log_mel"].to(DEV), angles=c["angles_rand"].to(DEV))
    assert out.shape == (B, 1, T * HOP) and voc.hop == HOP
    assert not out[:, :, (T - 1) * HOP:].any()
    # the frame-major inverse mel inside the graph: with zero iterations the chain is two linear ops (inverse mel,
    # istft), each within the op bound
    out = GriffinLimVocoder(n_iter=0)(c["log_mel"].to(DEV), angles=c["angles_rand"].to(DEV))
    ref = R.istft(c["lin"].double() * c["angles_rand"].to(torch.complex128))
    _close(out[:, 0, :(T - 1) * HOP], ref, f"vocoder, zero iterations B={B} T={T}", bound=2 * OP_BOUND)


def test_synthesise_with_the_griffin_lim_vocoder():
    from golden.weights_recipe import apply_recipe
    from matcha.models.matcha_tts import MatchaTTS

    model = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(DEV)
    apply_recipe(model, 7)
    model.eval()
    g = torch.Generator().manual_seed(3)
    B, Tx = 2, 11
    xl = torch.tensor([11, 8])
    x = torch.randint(1, 150, (B, Tx), generator=g) * (torch.arange(Tx)[None] < xl[:, None])
    voc = GriffinLimVocoder(n_iter=4)
    torch.manual_seed(11)
    out = model.synthesise(x.to(DEV), xl.to(DEV), n_timesteps=2, vocoder=voc)
    torch.manual_seed(11)  # the same draws: the ODE's noise first, then the initial phase
    plain = model.synthesise(x.to(DEV), xl.to(DEV), n_timesteps=2)
    assert torch.equal(plain["mel"], out["mel"])
    with torch.no_grad():
        want = voc(plain["mel"]).squeeze(1).clamp(-1, 1)
    wav = out["wav"]
    assert set(out) == set(plain) | {"wav", "wav_lengths"}
    assert wav.shape == (B, out["mel"].shape[2] * HOP)
    assert torch.isfinite(wav).all() and float(wav.abs().max()) <= 1.0
    assert torch.equal(out["wav_lengths"].cpu(), out["mel_lengths"].cpu() * HOP)
    assert torch.equal(wav, want)
