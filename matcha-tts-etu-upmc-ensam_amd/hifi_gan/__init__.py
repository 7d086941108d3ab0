"""HiFi-GAN generator inference on the HIP kernels of include/mtts_vocoder.h (mel -> waveform).

    from hifi_gan import AttrDict, Generator, GriffinLimVocoder, save_wav
"""
from __future__ import annotations

import wave

import numpy as np
import torch

from matcha.utils.audio_process import GriffinLimVocoder  # the checkpoint-free vocoder, same call shape

from .env import AttrDict
from .models import Generator

__all__ = ["AttrDict", "Generator", "GriffinLimVocoder", "save_wav"]


def save_wav(path, wav, sampling_rate: int) -> None:
    """Writes one mono utterance as 16-bit PCM with the standard library's ``wave`` module.  ``wav``: a tensor or
    array of samples in [-1, 1] (values outside are clipped), shape [L], [1, L] or [1, 1, L]."""
    if isinstance(wav, torch.Tensor):
        wav = wav.detach().float().cpu().numpy()
    a = np.asarray(wav, dtype=np.float64)
    if a.size != max(a.shape, default=0):
        raise ValueError(f"save_wav takes one mono utterance, got shape {a.shape}")
    pcm = np.round(np.clip(a.reshape(-1), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sampling_rate))
        f.writeframes(pcm.tobytes())
