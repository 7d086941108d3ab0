"""Griffin-Lim without a GPU: the float64 restatement (tests/griffinlim_ref.py) checked against facts that do not
depend on it, and the argument checking of the new API (matcha/utils/audio_process.py)."""
from __future__ import annotations

import pytest
import torch

import griffinlim_ref as R
from matcha import _native as N
from matcha.utils.audio_process import GriffinLim, GriffinLimVocoder, InverseMelScale


# ---- the restatement itself -------------------------------------------------------------------------------------
def test_pinv_is_the_lstsq_solution():
    M, P = R.mel_basis(), R.mel_pinv()
    y = torch.rand(80, 7, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    sol = torch.linalg.lstsq(M, y, driver="gelsd").solution
    rel = float((P @ y - sol).abs().max() / sol.abs().max())
    print(f"pinv vs lstsq(gelsd): {rel:.3e}")
    assert rel <= 1e-12


def test_basis_rank_and_zero_rows():
    M, P = R.mel_basis(), R.mel_pinv()
    assert int(torch.linalg.matrix_rank(M)) == 80
    unreached = (M == 0).all(0)  # bins no filter reaches: 0 Hz and the 141 bins above 8 kHz
    assert int(unreached.sum()) == 142 and bool(unreached[0]) and bool(unreached[-141:].all())
    # the minimum-norm solution is zero there: exactly above 8 kHz, to rounding (6e-15) at 0 Hz
    assert bool((P[-141:] == 0).all())
    assert float(P[unreached].abs().max()) <= 1e-12 * float(P.abs().max())
    assert int((P.abs().amax(1) > 1e-12 * float(P.abs().max())).sum()) == 371


def test_known_answer_zero_iterations_return_the_signal():
    x = R.signal(2, 9)
    X = R.stft(x)
    S = X.abs()
    angles = X / S.clamp(min=1e-300)
    wav = R.griffinlim(S, angles, 0)
    assert wav.shape == x.shape
    assert float((wav - x).abs().max()) <= 1e-12 * float(x.abs().max())


def test_spectral_convergence_falls_with_iterations():
    c = R.case(1, 40)
    sc = {n: R.spectral_convergence(R.griffinlim(c["lin"], c["angles_rand"], n), c["lin"]) for n in (0, 4, 32)}
    print("spectral convergence:", sc)
    assert sc[32] < sc[4] < sc[0]


# ---- the API, as far as it goes without a GPU -------------------------------------------------------------------
def test_constructors_build_on_the_cpu():
    inv = InverseMelScale(n_stft=513, n_mels=80, sample_rate=22050, f_min=0.0, f_max=8000.0, norm="slaney",
                          mel_scale="slaney")
    assert inv.pinv.shape == (513, 80) and inv.pinv.dtype == torch.float32
    assert inv.n_rows == 372 and not inv.pinv[inv.n_rows:].any()  # bins 1 .. 371 carry the 371 non-zero rows
    assert int((inv.pinv == 0).all(1).sum()) == 142
    assert float((inv.pinv.double() - R.mel_pinv()).abs().max()) <= 1e-6 * float(R.mel_pinv().abs().max())
    gl = GriffinLim(n_fft=1024, n_iter=32, hop_length=256, win_length=1024, power=1.0)
    assert (gl.n_iter, gl.momentum, gl.rand_init, gl.length) == (32, 0.99, True, None)
    v = GriffinLimVocoder()
    assert v.hop == 256 and v.griffin_lim.n_iter == 32 and v.griffin_lim.power == 1.0
    assert GriffinLimVocoder(n_iter=4).griffin_lim.n_iter == 4
    from hifi_gan import GriffinLimVocoder as exported

    assert exported is GriffinLimVocoder


@pytest.mark.parametrize("F", [0, 1, 3])
def test_too_few_frames_raise(F):
    gl = GriffinLim(hop_length=256, power=1.0)
    with pytest.raises(ValueError):
        gl(torch.zeros(1, 513, F))
    with pytest.raises(ValueError):
        GriffinLimVocoder()(torch.zeros(1, 80, F))


def test_unserved_settings_raise():
    with pytest.raises(ValueError):
        GriffinLim(n_fft=512, hop_length=128)
    with pytest.raises(ValueError):
        GriffinLim(n_fft=1024)  # torchaudio's default hop_length = win_length // 2 = 512
    with pytest.raises(ValueError):
        GriffinLim(n_fft=1024, hop_length=256, win_length=800)
    with pytest.raises(ValueError):
        GriffinLim(hop_length=256, length=5)
    with pytest.raises(ValueError):
        InverseMelScale(513, norm="htk")
    with pytest.raises(ValueError):
        InverseMelScale(513, mel_scale="htk")
    with pytest.raises(ValueError):
        GriffinLimVocoder(n_fft=2048)
    with pytest.raises(ValueError):
        GriffinLim(hop_length=256)(torch.zeros(1, 512, 8))  # wrong bin count


def test_cpu_tensors_are_refused():
    with pytest.raises(N.NativeError):
        InverseMelScale(513, f_max=8000.0)(torch.zeros(1, 80, 8))
    with pytest.raises(N.NativeError):
        GriffinLim(hop_length=256, power=1.0)(torch.zeros(1, 513, 8))
    with pytest.raises(N.NativeError):
        GriffinLimVocoder()(torch.zeros(1, 80, 8))


def test_library_refuses_other_geometries_without_aborting():
    """Shape and size checks come before any pointer is looked at, so no pointer is passed: nothing could launch."""
    lib = N.lib()
    none = None
    assert lib.mtts_gl_synthesis(none, none, none, 0.5, 1, none, none, none, 1, 8, 512, 128, None) == -2  # MTTS_ERR_SHAPE
    assert lib.mtts_gl_analysis(none, none, none, none, none, 1, 8, 1024, 512, None) == -2
    assert lib.mtts_gl_synthesis(none, none, none, 0.5, 1, none, none, none, 1, 3, 1024, 256, None) == -2  # F < 4
    assert lib.mtts_gl_analysis(none, none, none, none, none, 1, 3, 1024, 256, None) == -2
    assert lib.mtts_gl_synthesis(none, none, none, 0.5, 1, none, none, none, 1, 8, 1024, 256, None) == -1  # null pointer
    assert lib.mtts_gl_analysis(none, none, none, none, none, 1, 8, 1024, 256, None) == -1
    assert lib.mtts_gl_synthesis(none, none, none, 0.5, 1, none, none, none, -1, 8, 1024, 256, None) == -1  # bad size
    assert lib.mtts_gl_inverse_mel(none, none, none, 1, 80, 513, 371, 8, 1, 1.0, 0, None) == -1  # null pointer
    assert lib.mtts_gl_inverse_mel(none, none, none, 1, 80, 513, 600, 8, 1, 1.0, 0, None) == -1  # n_rows > n_stft
    assert lib.mtts_gl_inverse_mel(none, none, none, 1, 80, 513, 371, 8, 1, 0.0, 0, None) == -1  # power
    assert lib.mtts_gl_inverse_mel(none, none, none, 1, 97, 513, 371, 8, 1, 1.0, 0, None) == -2  # n_mels > 96
    assert lib.mtts_gl_inverse_mel(none, none, none, 0, 80, 513, 371, 8, 1, 1.0, 0, None) == 0  # empty batch
    assert lib.mtts_gl_synthesis(none, none, none, 0.5, 1, none, none, none, 0, 8, 1024, 256, None) == 0


def test_rand_init_false_is_stored():
    assert GriffinLim(hop_length=256, rand_init=False).rand_init is False


def test_fft_building_blocks_on_the_host(tmp_path):
    """tools/gl_fft_host_check.cpp drives the __host__ __device__ functions of csrc/gl_fft.h (FFT passes, split /
    merge, overlap-add geometry) lane by lane, in the kernels' order, against a direct float64 DFT.  Host pass only:
    no device code is compiled and no HIP call is made."""
    import subprocess
    from pathlib import Path

    import build_native

    root = Path(build_native.__file__).resolve().parent.parent
    exe = tmp_path / "gl_fft_host_check"
    subprocess.run([build_native._hipcc(), "-x", "hip", "--cuda-host-only", "-O1", f"-I{build_native.CSRC}",
                    str(root / "tools" / "gl_fft_host_check.cpp"), "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
