"""Log-mel features (reference: matcha/utils/audio_process.py:1-81) on the MI355X, two ways.

MelSpectrogram.batch(y, lengths): the whole front end in ONE HIP launch (csrc/mel_fused.hip, mtts_mel_from_wav) --
a zero-padded batch of int16 or fp32 waveforms and their lengths in, the padded log-mel batch and its frame counts
out.  Each utterance is reflect-padded at its own end, windowed, transformed (the 1024-point FFT of csrc/gl_fft.h in
LDS), projected on the band-sparse slaney basis and logged as the reference does on that utterance alone; exact zeros
follow its last frame, as collate pads; (mel - mel_mean) / mel_std is applied in the kernel on request.  Serves
n_fft = win_size = 1024, hop_size = 256, center=False.  MelStatistics accumulates the data_statistics
(mel_mean, mel_std) of a dataset from such batches on the device (mtts_mel_stats).

MelSpectrogram.__call__(y): torch.stft (rocFFT) produces the complex spectrum in HBM, then one HIP kernel
(csrc/mel.hip, mtts_mel_log_fwd) forms the magnitude sqrt(re^2+im^2+1e-9), projects it and applies
log(clamp(., 1e-5)).  Any geometry, but fp32 only, and it pads at the end of the padded row: right for rows of one
length (one call per utterance), wrong in the last frames of every shorter utterance of a padded batch.

Same names and argument meaning as the reference: MelSpectrogram(n_fft, num_mels, sampling_rate,
hop_size, win_size, fmin, fmax, center=False), __call__(y [B, T] float in [-1, 1]) -> [B, num_mels, F];
load_wav, load_and_process_audio, dynamic_range_compression_torch, spectral_normalize_torch,
MAX_WAV_VALUE.  Differences: __call__ takes DEVICE tensors (batched; the reference runs per utterance
on the CPU inside Dataset.__getitem__) and fails loudly without the HIP library -- there is no CPU
path.  librosa (reference :4) is not a dependency: `slaney_mel_basis` computes the same basis
(librosa.filters.mel, htk=False, norm="slaney") in float64 and stores it float32.

The way back, mel -> waveform without a vocoder checkpoint (reference: generate.py:66-113, which uses torchaudio):
InverseMelScale, GriffinLim and GriffinLimVocoder below, on the HIP kernels of include/mtts_griffinlim.h.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from matcha import _graphs as G
from matcha import _native as N
from matcha._abi import MTTS_GL_HOP as GL_HOP, MTTS_GL_NFFT as GL_NFFT  # the one STFT geometry the kernels serve

MAX_WAV_VALUE = 32768.0  # audio_process.py:9


def load_wav(full_path):
    """audio_process.py:13-15 (scipy.io.wavfile) -> (int16 samples, sampling rate)."""
    from scipy.io.wavfile import read

    sampling_rate, data = read(full_path)
    return data, sampling_rate


def dynamic_range_compression_torch(x, C=1, clip_val=1e-5):
    """audio_process.py:18-20."""
    return torch.log(torch.clamp(x, min=clip_val) * C)


def spectral_normalize_torch(magnitudes):
    """audio_process.py:23-25."""
    return dynamic_range_compression_torch(magnitudes)


def _hz_to_slaney_mel(hz: torch.Tensor) -> torch.Tensor:
    # linear below 1 kHz (200/3 Hz per mel), logarithmic above (ln 6.4 / 27 per mel)
    lin = hz * (3.0 / 200.0)
    return torch.where(hz >= 1000.0, 15.0 + torch.log(hz.clamp(min=1e-300) / 1000.0) * (27.0 / math.log(6.4)), lin)


def _slaney_mel_to_hz(mel: torch.Tensor) -> torch.Tensor:
    return torch.where(mel >= 15.0, 1000.0 * torch.exp((mel - 15.0) * (math.log(6.4) / 27.0)), mel * (200.0 / 3.0))


def slaney_mel_basis(sr: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: float | None = None) -> torch.Tensor:
    """[n_mels, n_fft//2 + 1] float32: triangular filters between consecutive slaney-mel-spaced edge
    frequencies, each scaled by 2 / (upper edge - lower edge) in Hz (librosa.filters.mel)."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    freqs = torch.arange(n_fft // 2 + 1, dtype=torch.float64) * (sr / n_fft)
    edges = _slaney_mel_to_hz(torch.linspace(float(_hz_to_slaney_mel(torch.tensor(float(fmin), dtype=torch.float64))),
                                             float(_hz_to_slaney_mel(torch.tensor(fmax, dtype=torch.float64))),
                                             n_mels + 2, dtype=torch.float64))
    lo, ce, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    rise = (freqs[None] - lo) / (ce - lo)
    fall = (hi - freqs[None]) / (hi - ce)
    tri = torch.clamp(torch.minimum(rise, fall), min=0.0).to(torch.float32)  # librosa stores float32 first
    return (tri.double() * (2.0 / (hi - lo))).to(torch.float32)


class MelSpectrogram:
    """audio_process.py:32-72.  One instance per configuration; buffers move to the input's device on
    first use and stay there."""

    def __init__(self, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
        self.n_fft = n_fft
        self.num_mels = num_mels
        self.sampling_rate = sampling_rate
        self.hop_size = hop_size
        self.win_size = win_size
        self.fmin = fmin
        self.fmax = fmax
        self.center = center
        self.mel_basis = slaney_mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax)
        nz = self.mel_basis != 0
        any_nz = nz.any(1)
        first = torch.where(any_nz, nz.float().argmax(1), torch.zeros_like(any_nz, dtype=torch.long))
        last = torch.where(any_nz, nz.shape[1] - nz.flip(1).float().argmax(1), torch.zeros_like(first))
        self.band_lo = first.to(torch.int32)
        self.band_hi = last.to(torch.int32)
        self.hann_window = torch.hann_window(win_size)
        self._dev = {}

    def _buffers(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.mel_basis.to(device).contiguous(), self.band_lo.to(device), self.band_hi.to(device),
                              self.hann_window.to(device))
        return self._dev[key]

    def _stft(self, y):
        pad_size = int((self.n_fft - self.hop_size) / 2)  # :47
        y = torch.nn.functional.pad(y.unsqueeze(1), (pad_size, pad_size), mode="reflect").squeeze(1)
        return torch.stft(y, self.n_fft, hop_length=self.hop_size, win_length=self.win_size,
                          window=self._buffers(y.device)[3], center=self.center, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True)

    def _apply_stft(self, y):
        """:45-58 (magnitude spectrogram, unfused; kept for API parity)."""
        spec = self._stft(y)
        return torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)

    def __call__(self, y):
        """:60-72 -> log-mel [B, num_mels, F] float32."""
        N.require_device(y)
        if y.dim() != 2:
            raise ValueError(f"MelSpectrogram expects y [B, T], got {tuple(y.shape)}")
        spec = torch.view_as_real(self._stft(y.to(torch.float32))).contiguous()  # [B, n_freq, F, 2]
        B, n_freq, F, _ = spec.shape
        basis, lo, hi, _ = self._buffers(y.device)
        out = torch.empty((B, self.num_mels, F), dtype=torch.float32, device=y.device)
        with torch.cuda.device(y.device):
            rc = N.lib().mtts_mel_log_fwd(N.ptr(spec), N.ptr(basis), N.ptr(lo), N.ptr(hi), B, n_freq, F,
                                          self.num_mels, 1e-5, N.ptr(out), N.stream_handle(y.device))
        N.check(rc, "mtts_mel_log_fwd")
        return out

    def _check_served(self):
        if (self.n_fft, self.win_size, self.hop_size) != (GL_NFFT, GL_NFFT, GL_HOP) or self.center or \
                not 1 <= self.num_mels <= 96:
            raise ValueError(f"MelSpectrogram.batch serves n_fft = win_size = {GL_NFFT}, hop_size = {GL_HOP}, "
                             f"center=False and num_mels <= 96 only, got n_fft={self.n_fft}, win_size={self.win_size}, "
                             f"hop_size={self.hop_size}, center={self.center}, num_mels={self.num_mels}")

    def batch(self, y, lengths=None, *, mel_mean=0.0, mel_std=1.0):
        """Padded waveform batch -> (log-mel [B, num_mels, L // 256] float32, mel_lengths int64 [B]) in one launch
        (mtts_mel_from_wav), each utterance computed on its own waveform as the reference's per-utterance call does:
        reflect-padded at its own end, ``mel_lengths[b] = lengths[b] // 256`` frames, exact zeros after them (what
        ``collate`` pads with).  ``(mel - mel_mean) / mel_std`` is applied to the valid frames inside the kernel; the
        defaults change no bit.

        y: [B, L] float32 in [-1, 1] or int16 (converted in the kernel as s / 32768), on the device.  lengths: samples
        per row, or None for L everywhere.  A device int tensor is converted on the device and the call does no
        host synchronisation (the kernel clamps it to [0, L]; a row shorter than 385 samples, the least a reflect
        pad by 384 accepts, gets mel_lengths 0 and zeros); a host tensor or list is validated (ValueError below 385 or
        above L) and copied.  With device lengths the call can be captured into an outer graph after one warm-up
        call."""
        self._check_served()
        if not isinstance(y, torch.Tensor) or y.dim() != 2:
            raise ValueError(f"MelSpectrogram.batch expects y [B, L], got {tuple(getattr(y, 'shape', ()))}")
        if y.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"MelSpectrogram.batch takes float32 or int16 waveforms, got {y.dtype}")
        if not float(mel_std) > 0.0:
            raise ValueError(f"mel_std must be positive, got {mel_std}")
        B, L = y.shape
        if B > 65535:
            raise ValueError(f"MelSpectrogram.batch serves B <= 65535, got {B}")
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            host = torch.as_tensor(lengths).reshape(-1)
            if host.is_floating_point() or host.numel() != B:
                raise ValueError(f"lengths must be {B} integers, got {host.dtype} x {host.numel()}")
            if B and (int(host.min()) < MEL_MIN_SAMPLES or int(host.max()) > L):
                raise ValueError(f"lengths must lie in [{MEL_MIN_SAMPLES}, L = {L}] (a reflect pad by "
                                 f"{MEL_MIN_SAMPLES - 1} needs {MEL_MIN_SAMPLES} samples), got {int(host.min())} .. "
                                 f"{int(host.max())}")
            N.require_device(y)
            lengths = host.to(torch.int32).to(y.device)
        N.require_device(y, lengths)
        if lengths is not None:
            if lengths.dim() != 1 or lengths.numel() != B or lengths.is_floating_point():
                raise ValueError(f"lengths must be an integer tensor [{B}], got {lengths.dtype} {tuple(lengths.shape)}")
            lengths = lengths.to(torch.int32).contiguous()
        y = y.contiguous()
        basis, lo, hi, _ = self._buffers(y.device)
        tw, win = _gl_device_tables(y.device)
        out = torch.empty((B, self.num_mels, L // GL_HOP), dtype=torch.float32, device=y.device)
        mel_lengths = torch.empty((B,), dtype=torch.int32, device=y.device)
        with torch.cuda.device(y.device):
            rc = N.lib().mtts_mel_from_wav(N.ptr(y), int(y.dtype == torch.int16), N.ptr(lengths), N.ptr(basis),
                                           N.ptr(lo), N.ptr(hi), N.ptr(tw), N.ptr(win), B, L, self.n_fft,
                                           self.win_size, self.hop_size, self.num_mels, 1e-5, float(mel_mean),
                                           float(mel_std), 0.0, N.ptr(out), N.ptr(mel_lengths),
                                           N.stream_handle(y.device))
        N.check(rc, "mtts_mel_from_wav")
        return out, mel_lengths.to(torch.int64)


class MelStatistics:
    """The ``data_statistics`` of a dataset from its mel batches: ``update(mel, mel_lengths)`` adds the float64 sums
    of the valid frames (one launch of mtts_mel_stats, accumulators stay on the device, no synchronisation);
    ``result()`` returns ``{"mel_mean", "mel_std"}`` for ``MatchaTTS(data_statistics=...)`` and for the ``mel_mean`` /
    ``mel_std`` of ``MelSpectrogram.batch``.  mean = sum v / n, std = sqrt(sum v^2 / n - mean^2) with n = num_mels *
    sum mel_lengths: the population form of upstream Matcha's data-statistics script."""

    def __init__(self):
        self._sums = None  # float64 [2] on the device: sum v, sum v^2
        self._frames = None  # int64 [] on the device
        self._num_mels = None

    def update(self, mel, mel_lengths):
        if mel.dim() != 3 or mel.dtype != torch.float32:
            raise ValueError(f"MelStatistics.update expects mel float32 [B, num_mels, F], got {mel.dtype} "
                             f"{tuple(mel.shape)}")
        N.require_device(mel)
        B, n_mels, F = mel.shape
        if self._num_mels not in (None, n_mels):
            raise ValueError(f"num_mels changed between updates: {self._num_mels} then {n_mels}")
        ml = torch.as_tensor(mel_lengths).reshape(-1)
        if ml.is_floating_point() or ml.numel() != B:
            raise ValueError(f"mel_lengths must be {B} integers, got {ml.dtype} x {ml.numel()}")
        ml = ml.to(device=mel.device, dtype=torch.int32).clamp(0, F).contiguous()
        mel = mel.detach().contiguous()
        stats = torch.empty((B, 2), dtype=torch.float64, device=mel.device)
        with torch.cuda.device(mel.device):
            rc = N.lib().mtts_mel_stats(N.ptr(mel), N.ptr(ml), B, n_mels, F, N.ptr(stats), N.stream_handle(mel.device))
        N.check(rc, "mtts_mel_stats")
        sums, frames = stats.sum(0), ml.sum(dtype=torch.int64)
        self._sums = sums if self._sums is None else self._sums + sums
        self._frames = frames if self._frames is None else self._frames + frames
        self._num_mels = n_mels
        return self

    def state(self):
        """(float64 [2]: sum v and sum v^2, int64 []: frames added) on the device, without synchronising; None before
        the first update."""
        return None if self._sums is None else (self._sums, self._frames)

    @staticmethod
    def from_sums(total, total_sq, count):
        """{"mel_mean", "mel_std"} from sum v, sum v^2 and the number of values."""
        if count <= 0:
            raise ValueError("MelStatistics: no frames were added")
        mean = float(total) / count
        return {"mel_mean": mean, "mel_std": math.sqrt(max(float(total_sq) / count - mean * mean, 0.0))}

    def result(self):
        if self._sums is None:
            raise ValueError("MelStatistics: no frames were added")
        total, total_sq = self._sums.tolist()
        return self.from_sums(total, total_sq, self._num_mels * int(self._frames))


# ---- mel -> waveform without a vocoder checkpoint (reference: generate.py:66-113) ----------------------------------
MEL_MIN_SAMPLES = (GL_NFFT - GL_HOP) // 2 + 1  # MelSpectrogram.batch: the shortest utterance a reflect pad by 384 accepts

_gl_tables: dict = {}


def _gl_device_tables(device):
    """(twiddle [1024, 2], window [1024]) on `device`: exp(-2 pi i k / 1024) computed in float64, stored fp32, and
    the periodic Hann window."""
    key = str(device)
    if key not in _gl_tables:
        a = torch.arange(GL_NFFT, dtype=torch.float64) * (-2.0 * math.pi / GL_NFFT)
        tw = torch.stack([torch.cos(a), torch.sin(a)], 1).to(torch.float32)
        _gl_tables[key] = (tw.to(device).contiguous(), torch.hann_window(GL_NFFT).to(device))
    return _gl_tables[key]


class InverseMelScale:
    """torchaudio.transforms.InverseMelScale (same argument names and defaults) on one HIP kernel
    (mtts_gl_inverse_mel): relu(pinv(M) @ mel), M this module's ``slaney_mel_basis``.  The pseudo-inverse is computed
    once on the host in float64 and stored fp32; it is the minimum-norm least-squares solution torchaudio's
    ``lstsq`` returns (M has full row rank).  Bins above f_max are written as exact zeros.

    ``__call__(mel [B, n_mels, F], *, log_input=False) -> [B, n_stft, F]``.  The reference decides whether to
    exponentiate a log-mel with a host-side ``if mel.min() < 0`` (generate.py:102); ``log_input=True`` applies the
    exp inside the kernel instead, with no device-to-host synchronisation.  Device fp32 tensors only."""

    def __init__(self, n_stft, n_mels=80, sample_rate=22050, f_min=0.0, f_max=None, norm="slaney", mel_scale="slaney"):
        if norm != "slaney" or mel_scale != "slaney":
            raise ValueError(f"InverseMelScale serves norm='slaney', mel_scale='slaney' only, got {norm!r}, "
                             f"{mel_scale!r}")
        if n_stft < 2 or not 1 <= n_mels <= 96:  # the kernel stages a tile's mel channels in LDS
            raise ValueError(f"bad n_stft / n_mels (1 .. 96): {n_stft}, {n_mels}")
        self.n_stft, self.n_mels, self.sample_rate = int(n_stft), int(n_mels), int(sample_rate)
        self.f_min, self.f_max = float(f_min), float(sample_rate) / 2 if f_max is None else float(f_max)
        basis = slaney_mel_basis(self.sample_rate, 2 * (self.n_stft - 1), self.n_mels, self.f_min, self.f_max)
        pinv = torch.linalg.pinv(basis.double())  # [n_stft, n_mels]
        reached = (basis != 0).any(0)
        pinv[~reached] = 0.0  # a bin no filter reaches is zero in the minimum-norm solution (0 Hz, above f_max)
        self.n_rows = int(reached.nonzero().max()) + 1 if reached.any() else 0  # rows from here on: never read
        self.pinv = pinv.to(torch.float32).contiguous()
        self._dev = {}

    def to(self, *args, **kwargs):
        """Accepted for torchaudio's call pattern; buffers follow the input's device on first use."""
        return self

    def _pinv_on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.pinv.to(device)
        return self._dev[key]

    def _launch(self, mel, out, *, log_input, inv_power=1.0, frame_major=False):
        B, _, F = mel.shape
        with torch.cuda.device(mel.device):
            rc = N.lib().mtts_gl_inverse_mel(N.ptr(mel), N.ptr(self._pinv_on(mel.device)), N.ptr(out), B, self.n_mels,
                                             self.n_stft, self.n_rows, F, int(bool(log_input)), float(inv_power),
                                             int(frame_major), N.stream_handle(mel.device))
        N.check(rc, "mtts_gl_inverse_mel")

    def __call__(self, mel, *, log_input=False):
        if mel.dim() != 3 or mel.shape[1] != self.n_mels:
            raise ValueError(f"InverseMelScale expects mel [B, {self.n_mels}, F], got {tuple(mel.shape)}")
        N.require_device(mel)
        mel = mel.detach().to(torch.float32).contiguous()
        out = torch.empty((mel.shape[0], self.n_stft, mel.shape[2]), dtype=torch.float32, device=mel.device)
        self._launch(mel, out, log_input=log_input)
        return out

    forward = __call__


class _GLState:
    """The caller-owned buffers of one Griffin-Lim run on (B, F): spectra frame-major (include/mtts_griffinlim.h)."""

    def __init__(self, B, F, device, n_mels=None):
        with torch.inference_mode(False):  # graph-static buffers: later calls outside inference mode copy into them
            e = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
            self.mel = e(B, n_mels, F) if n_mels else None
            self.lin = e(B, F, GL_NFFT // 2 + 1)
            self.ang0 = e(B, F, GL_NFFT // 2 + 1, 2)
            self.spec = e(2, B, F, GL_NFFT // 2 + 1, 2)  # reb / tprev, ping-pong
            self.frames = e(B, F, GL_NFFT)
            self.wav = e(B, (F - 1) * GL_HOP)
        self.graph = None


class GriffinLim:
    """torchaudio.transforms.GriffinLim (same argument names and defaults) on the HIP kernels of
    include/mtts_griffinlim.h: ``__call__(spec [B, n_fft//2 + 1, F], *, angles=None) -> [B, (F - 1) * hop]``.

    One run is a synthesis launch (phase update + inverse FFT + window) and an analysis launch (overlap-add gather +
    window + FFT) per iteration, plus the first synthesis and the final gather; it is captured once per
    (B, F, n_iter) into a HIP graph (the 8 most recently used stay cached) and replayed; under an outer capture, or
    with ``graph = False``, the same launches run eagerly.  With ``rand_init`` the initial phase has real and
    imaginary parts uniform in [0, 1) -- not unit magnitude; torchaudio's behaviour -- drawn with torch's generator before the replay;
    ``rand_init=False`` starts from the phase 1 + 0i in every bin, as torchaudio does, and is repeatable unseeded;
    ``angles`` (complex [B, n_fft//2 + 1, F]) injects it instead.

    Only n_fft = win_length = 1024 and hop_length = 256 are served (torchaudio's default hop_length = win_length // 2
    is not: pass hop_length=256), ``length`` must be None and F >= 4 (fewer frames cannot be reflect-padded).
    Device fp32 tensors only."""

    _GRAPH_CACHE_MAX = 8
    graph = True

    def __init__(self, n_fft=1024, n_iter=32, win_length=None, hop_length=None, power=2.0, momentum=0.99, length=None,
                 rand_init=True):
        win_length = n_fft if win_length is None else win_length
        hop_length = win_length // 2 if hop_length is None else hop_length
        if (n_fft, win_length, hop_length) != (GL_NFFT, GL_NFFT, GL_HOP):
            raise ValueError(f"GriffinLim serves n_fft = win_length = {GL_NFFT}, hop_length = {GL_HOP} only, got "
                             f"n_fft={n_fft}, win_length={win_length}, hop_length={hop_length}")
        if length is not None:
            raise ValueError(f"GriffinLim serves length=None only, got {length}")
        if not 0 <= momentum < 1:
            raise ValueError(f"momentum must be in [0, 1), got {momentum}")
        if n_iter < 0 or not power > 0:
            raise ValueError(f"bad n_iter / power: {n_iter}, {power}")
        self.n_fft, self.n_iter, self.win_length, self.hop_length = n_fft, int(n_iter), win_length, hop_length
        self.power, self.momentum, self.length, self.rand_init = float(power), float(momentum), length, bool(rand_init)
        self._graphs = G.GraphCache(self._GRAPH_CACHE_MAX)

    def to(self, *args, **kwargs):
        return self

    # ---- launches -------------------------------------------------------------------------------------------
    def _launch(self, st, B, F, device, inverse_mel=None, n_iter=None):
        """Every launch of one run on the current stream: (inverse mel,) synthesis, n_iter x (analysis, synthesis),
        gather."""
        lib, s = N.lib(), N.stream_handle(device)
        tw, win = _gl_device_tables(device)
        m = self.momentum / (1.0 + self.momentum)
        n_iter = self.n_iter if n_iter is None else n_iter
        with torch.cuda.device(device):
            if inverse_mel is not None:
                inverse_mel._launch(st.mel, st.lin, log_input=True, inv_power=1.0 / self.power, frame_major=True)

            def synthesis(reb, tprev, normalize):
                N.check(lib.mtts_gl_synthesis(N.ptr(st.lin), N.ptr(reb), N.ptr(tprev), m, normalize, N.ptr(tw),
                                              N.ptr(win), N.ptr(st.frames), B, F, GL_NFFT, GL_HOP, s),
                        "mtts_gl_synthesis")

            synthesis(st.ang0, None, 0)
            for i in range(n_iter):
                N.check(lib.mtts_gl_analysis(N.ptr(st.frames), N.ptr(tw), N.ptr(win), N.ptr(st.spec[i % 2]), None, B, F,
                                             GL_NFFT, GL_HOP, s), "mtts_gl_analysis")
                synthesis(st.spec[i % 2], st.spec[(i + 1) % 2] if i else None, 1)
            N.check(lib.mtts_gl_analysis(N.ptr(st.frames), None, N.ptr(win), None, N.ptr(st.wav), B, F, GL_NFFT,
                                         GL_HOP, s), "mtts_gl_analysis")

    def _fill(self, st, spec, mel, angles):
        if mel is not None:
            st.mel.copy_(mel)
        else:
            st.lin.copy_((spec if self.power == 1.0 else spec.pow(1.0 / self.power)).transpose(1, 2))
        if angles is not None:
            st.ang0.copy_(torch.view_as_real(angles.transpose(1, 2).to(torch.complex64).resolve_conj()))
        elif self.rand_init:
            st.ang0.uniform_(0.0, 1.0)
        else:  # torchaudio: angles = torch.full(specgram.size(), 1) -- the phase 1 + 0i, deterministic
            st.ang0[..., 0].fill_(1.0)
            st.ang0[..., 1].zero_()

    def _run(self, B, F, device, *, spec=None, mel=None, inverse_mel=None, angles=None):
        if self.graph and not torch.cuda.is_current_stream_capturing():
            key = (B, F, self.n_iter, str(device), inverse_mel is not None)

            def build():
                st = _GLState(B, F, device, inverse_mel.n_mels if inverse_mel is not None else None)

                def launch(n_iter=None):
                    self._launch(st, B, F, device, inverse_mel, n_iter)

                # the warm-up runs on the zeroed buffers, shortened: it only has to load the code objects
                st.graph, _ = G.capture(launch, device, warmup=lambda: launch(min(self.n_iter, 2)))
                return st

            st = self._graphs.lookup(key, build)
            self._fill(st, spec, mel, angles)
            st.graph.replay()
            return st.wav.clone()
        st = _GLState(B, F, device, inverse_mel.n_mels if inverse_mel is not None else None)
        self._fill(st, spec, mel, angles)
        self._launch(st, B, F, device, inverse_mel)
        return st.wav

    def _check(self, x, rows, what, angles):
        if x.dim() != 3 or x.shape[1] != rows:
            raise ValueError(f"{what} must be [B, {rows}, F], got {tuple(x.shape)}")
        if x.shape[2] < 4:
            raise ValueError(f"Griffin-Lim needs at least 4 frames (fewer cannot be reflect-padded by "
                             f"{GL_NFFT // 2} samples), got {x.shape[2]}")
        if angles is not None and (not angles.is_complex() or
                                   tuple(angles.shape) != (x.shape[0], GL_NFFT // 2 + 1, x.shape[2])):
            raise ValueError(f"angles must be complex [B, {GL_NFFT // 2 + 1}, F], got {tuple(angles.shape)}")
        N.require_device(x, angles)

    def __call__(self, spec, *, angles=None):
        self._check(spec, GL_NFFT // 2 + 1, "spec", angles)
        with torch.no_grad():
            spec = spec.detach().to(torch.float32)
            B, _, F = spec.shape
            if B == 0:
                return torch.zeros(0, (F - 1) * GL_HOP, dtype=torch.float32, device=spec.device)
            return self._run(B, F, spec.device, spec=spec, angles=angles)

    forward = __call__

    def rebuilt(self, spec, *, angles):
        """Test hook: the first iteration's ``stft(istft(spec ** (1/power) * angles))`` as complex
        [B, n_fft//2 + 1, F] (one synthesis and one analysis launch, eager)."""
        self._check(spec, GL_NFFT // 2 + 1, "spec", angles)
        B, _, F = spec.shape
        dev = spec.device
        with torch.no_grad():
            st = _GLState(B, F, dev)
            self._fill(st, spec.detach().to(torch.float32), None, angles)
            tw, win = _gl_device_tables(dev)
            with torch.cuda.device(dev):
                s = N.stream_handle(dev)
                N.check(N.lib().mtts_gl_synthesis(N.ptr(st.lin), N.ptr(st.ang0), None, 0.0, 0, N.ptr(tw), N.ptr(win),
                                                  N.ptr(st.frames), B, F, GL_NFFT, GL_HOP, s), "mtts_gl_synthesis")
                N.check(N.lib().mtts_gl_analysis(N.ptr(st.frames), N.ptr(tw), N.ptr(win), N.ptr(st.spec[0]), None, B,
                                                 F, GL_NFFT, GL_HOP, s), "mtts_gl_analysis")
            return torch.view_as_complex(st.spec[0]).transpose(1, 2).contiguous()


class GriffinLimVocoder:
    """The reference's checkpoint-free mel -> waveform path (generate.py:73-109: exp, InverseMelScale, 32 iterations
    of GriffinLim with power 1), shaped like ``hifi_gan.Generator``: ``__call__(log_mel [B, num_mels, T]) ->
    [B, 1, T * hop]`` with ``.hop`` samples per frame, so ``MatchaTTS.synthesise(..., vocoder=GriffinLimVocoder())``
    works unchanged.  Griffin-Lim yields (T - 1) * hop samples; the last hop is zero padding.  Padded frames are
    vocoded unmasked, like the HiFi-GAN path: cut at ``wav_lengths``.  The inverse mel runs inside the captured
    graph: 2 * n_iter + 3 launches per call."""

    def __init__(self, n_fft=1024, hop_size=256, num_mels=80, sampling_rate=22050, fmin=0, fmax=8000, n_iter=32):
        self.griffin_lim = GriffinLim(n_fft=n_fft, n_iter=n_iter, win_length=n_fft, hop_length=hop_size, power=1.0)
        self.inverse_mel = InverseMelScale(n_fft // 2 + 1, num_mels, sampling_rate, float(fmin),
                                           None if fmax is None else float(fmax))
        self.hop = hop_size
        self.num_mels = num_mels

    def to(self, *args, **kwargs):
        return self

    def eval(self):
        return self

    def __call__(self, log_mel, *, angles=None):
        self.griffin_lim._check(log_mel, self.num_mels, "log_mel", angles)
        with torch.no_grad():
            mel = log_mel.detach().to(torch.float32)
            B, _, T = mel.shape
            out = torch.zeros(B, 1, T * self.hop, dtype=torch.float32, device=mel.device)
            if B:
                wav = self.griffin_lim._run(B, T, mel.device, mel=mel, inverse_mel=self.inverse_mel, angles=angles)
                out[:, 0, :(T - 1) * self.hop] = wav
            return out

    forward = __call__


def load_and_process_audio(file_path, mel_processor, device="cuda"):
    """audio_process.py:75-81: int16 wav -> float / 32768 -> [1, T] on `device` -> mel_processor."""
    sampling_rate, data = load_wav(file_path)[::-1]
    y = torch.from_numpy(np.asarray(data, dtype=np.float32)) / MAX_WAV_VALUE
    return mel_processor(y.unsqueeze(0).to(device))
