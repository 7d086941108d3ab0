"""The yardstick of the Griffin-Lim tests: torchaudio.transforms.InverseMelScale and torchaudio.functional.griffinlim
(as the reference's generate.py configures them) restated on torch.stft / torch.istft on the CPU.  ``dtype`` selects
float64 (the reference) or float32 (the same code, to measure what fp32 costs).  Imports nothing from the code under
test except ``slaney_mel_basis``.

Settings: n_fft = win_length = 1024, hop 256, periodic Hann, 80 slaney mels 0-8000 Hz at 22050 Hz, power 1,
momentum 0.99."""
from __future__ import annotations

import functools
import math

import torch

from matcha.utils.audio_process import slaney_mel_basis

N_FFT, HOP, N_MELS, SR, FMIN, FMAX = 1024, 256, 80, 22050, 0.0, 8000.0
N_STFT = N_FFT // 2 + 1


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


@functools.lru_cache(maxsize=None)
def mel_basis() -> torch.Tensor:
    """[80, 513] float64 (the project's fp32 basis, widened)."""
    return slaney_mel_basis(SR, N_FFT, N_MELS, FMIN, FMAX).double()


@functools.lru_cache(maxsize=None)
def mel_pinv() -> torch.Tensor:
    """[513, 80] float64."""
    return torch.linalg.pinv(mel_basis())


def inverse_mel(mel_linear: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """relu(pinv(M) @ mel_linear): [B, 80, F] -> [B, 513, F]."""
    return torch.relu(mel_pinv().to(dtype) @ mel_linear.to(dtype))


def stft(x: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    return torch.stft(x.to(dtype), N_FFT, hop_length=HOP, win_length=N_FFT,
                      window=torch.hann_window(N_FFT, dtype=dtype), center=True, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)


def istft(X: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    return torch.istft(X.to(_cdtype(dtype)), N_FFT, hop_length=HOP, win_length=N_FFT,
                       window=torch.hann_window(N_FFT, dtype=dtype), center=True, normalized=False, onesided=True,
                       length=None)


def griffinlim(lin: torch.Tensor, angles: torch.Tensor, n_iter: int, momentum: float = 0.99, dtype=torch.float64,
               first=False):
    """lin [B, 513, F] magnitudes (power 1), angles complex [B, 513, F] -> waveform [B, (F-1)*256].
    ``first=True`` returns (inv, reb) of the first iteration instead."""
    lin = lin.to(dtype)
    ang = angles.to(_cdtype(dtype))
    m = momentum / (1 + momentum)
    tprev = torch.zeros_like(ang)
    for _ in range(n_iter):
        inv = istft(lin * ang, dtype)
        reb = stft(inv, dtype)
        if first:
            return inv, reb
        ang = reb - tprev.mul(m)
        ang = ang.div(ang.abs().add(1e-16))
        tprev = reb
    return istft(lin * ang, dtype)


def spectral_convergence(wav: torch.Tensor, S: torch.Tensor) -> float:
    """|| |STFT(wav)| - S || / || S ||, in float64."""
    return float((stft(wav.double()).abs() - S.double()).norm() / S.double().norm())


def signal(B: int, F: int, seed: int = 0) -> torch.Tensor:
    """[B, (F-1)*256] float64: a chirp plus a tone plus noise, different per utterance."""
    L = (F - 1) * HOP
    g = torch.Generator().manual_seed(1000 * seed + 10 * F + B)
    t = torch.arange(L, dtype=torch.float64) / SR
    out = []
    for b in range(B):
        f0, f1 = 200.0 + 150.0 * b, 3000.0 + 900.0 * b
        dur = max(L / SR, 1e-3)
        chirp = torch.sin(2 * math.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t))
        tone = torch.sin(2 * math.pi * (440.0 * (b + 1)) * t + 0.3 * b)
        out.append(0.5 * chirp + 0.3 * tone + 0.05 * torch.randn(L, generator=g, dtype=torch.float64))
    return torch.stack(out)


def rounding_variant(lin, angles, n_iter, which, momentum=0.99):
    """The fp32 run with another rounding pattern of the same precision class: every iterate is stored in fp32, but
    one of the two transforms is computed in float64 ("B": istft, "C": stft).  Used only to choose SEEDS."""
    lin, ang, m = lin.float(), angles.to(torch.complex64), momentum / (1 + momentum)
    tprev = torch.zeros_like(ang)
    di, ds = (torch.float64, torch.float32) if which == "B" else (torch.float32, torch.float64)
    for _ in range(n_iter):
        inv = istft(lin * ang, di).float()
        reb = stft(inv, ds).to(torch.complex64)
        ang = reb - tprev.mul(m)
        ang = ang.div(ang.abs().add(1e-16))
        tprev = reb
    return istft(lin * ang, torch.float32)


def conditioning(B: int, F: int, seed: int, n_iter: int = 32):
    """Errors against float64, relative to max|ref|, of the fp32 run and its two rounding variants."""
    c = case(B, F, seed)
    ref = griffinlim(c["lin"], c["angles_rand"], n_iter)
    runs = [griffinlim(c["lin"], c["angles_rand"], n_iter, dtype=torch.float32),
            rounding_variant(c["lin"], c["angles_rand"], n_iter, "B"),
            rounding_variant(c["lin"], c["angles_rand"], n_iter, "C")]
    return [float((w.double() - ref).abs().max() / ref.abs().max()) for w in runs]


# The phase normalisation divides by |reb - m * tprev|; where that is near zero a rounding error of 1e-7 becomes a
# phase of its own, and after 32 iterations two fp32 runs of the same algorithm can differ by 100 x on one input
# and agree on the next (B = 1, F = 4, seed 2: 4e-2 and 2e-5).  On such an input the fp32 CPU run measures an
# accident, not what fp32 costs.  So each shape uses the smallest seed in 0 .. 11 on which the fp32 CPU run is
# reproducible under a change of rounding: its error and those of the two variants above lie within a factor 2 of
# one another (or all below 5e-6, a quarter of the op bound), and the fp32 error is at most 1e-3.
# The fp32 run also moves with the host's FFT library (no entry of the table was equal on two hosts; on one,
# B = 3, F = 40, seed 0 gave 2.1e-4, on the other 5.7e-3, which would loosen the whole-run bound to 2e-2), so the rule
# was evaluated on two hosts with different CPUs and a seed must pass on both.  Among the seeds that do, a shape takes
# the smallest that passes the same rule at 4 iterations on both hosts too (the other length the tests run; there the
# bound sits at its 2e-5 floor), or the smallest if none does (B = 3, F = 5: seed 7 is the only one, 6.6e-6 at 4
# iterations).  B = 3, F = 9 has no seed in 0 .. 11 that passes at 32 iterations on both hosts; it takes the seed
# whose worst spread over the two is smallest (seed 2: 2.1 x and 2.7 x, fp32 error 3.6e-5 and 3.1e-5).  With these
# seeds the fp32 error of every shape at 32 iterations agreed within 1.3 x between the hosts wherever it exceeds
# 5e-6.  Chosen from CPU runs alone; running this file prints one host's table for a given iteration count.
SEEDS = {(1, 4): 0, (3, 4): 2, (1, 5): 5, (3, 5): 7, (1, 9): 2, (3, 9): 2, (1, 40): 3, (3, 40): 4}


def well_conditioned(errs) -> bool:
    return (max(errs) <= 2 * min(errs) or max(errs) <= 5e-6) and errs[0] <= 1e-3


@functools.lru_cache(maxsize=None)
def case(B: int, F: int, seed: int | None = None) -> dict:
    """A seeded input chain: signal -> |STFT| -> mel basis -> log -> inverse mel, everything the tests share.
    fp32 tensors are what the device is given; the float64 reference starts from the same fp32 values."""
    seed = SEEDS.get((B, F), 0) if seed is None else seed
    x = signal(B, F, seed)
    X = stft(x)
    S = X.abs()
    log_mel = torch.log(torch.clamp(mel_basis() @ S, min=1e-5)).float()  # [B, 80, F], the model's output format
    lin = inverse_mel(torch.exp(log_mel.double())).float()  # [B, 513, F]
    g = torch.Generator().manual_seed(77 + 1000 * seed + 10 * F + B)
    rand = torch.rand(B, N_STFT, F, 2, generator=g, dtype=torch.float64)
    ph = torch.rand(B, N_STFT, F, generator=g, dtype=torch.float64) * (2 * math.pi)
    return {
        "x": x, "X": X, "S": S, "log_mel": log_mel, "lin": lin,
        "angles_rand": torch.view_as_complex(rand.float()),  # [0, 1)^2, torchaudio's rand_init
        "angles_unit": torch.polar(torch.ones_like(ph), ph).to(torch.complex64),
    }


if __name__ == "__main__":  # PYTHONPATH=matcha-tts-etu-upmc-ensam_amd python tests/griffinlim_ref.py [n_iter]
    import sys

    n_iter = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    for shape in SEEDS:
        for s in range(12):
            e = conditioning(*shape, s, n_iter)
            print(f"B={shape[0]} F={shape[1]} seed={s} n_iter={n_iter}: fp32 {e[0]:.2e}, variants {e[1]:.2e} {e[2]:.2e}"
                  f"{'  <- well conditioned' if well_conditioned(e) else ''}", flush=True)
