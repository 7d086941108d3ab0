"""The fused mel front end without a GPU: the index arithmetic and the per-lane frame pipeline of csrc/mel_frame.h
driven on the host (tools/mel_frame_host_check.cpp) against numpy.pad(mode="reflect") and the reference's own mel
(tests/golden/mel_golden.npz), collate_wav, and the argument checking of MelSpectrogram.batch / MelStatistics."""
from __future__ import annotations

import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from matcha import _native as N
from matcha.data_management.ljspeech_datamodule import collate_wav
from matcha.utils.audio_process import MelSpectrogram, MelStatistics

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "mel_golden.npz")
CFG = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000)
MEL_TOL = 1e-4  # the bound tests/test_data_path.py holds the mel path to


def test_index_header_and_frame_pipeline_on_the_host(tmp_path):
    """Every length 385 .. 1400, every frame and sample: the source index equals numpy.pad(mode="reflect") and lies
    in [0, len), the frame count equals len // 256, the wide-load predicate holds exactly on aligned interior frames;
    then the kernel's per-lane pipeline over pcm_0 (4 frames) against mel_0 within MEL_TOL.  Host pass only: no
    device code is compiled and no HIP call is made."""
    import build_native

    root = Path(build_native.__file__).resolve().parent.parent
    exe = tmp_path / "mel_frame_host_check"
    subprocess.run([build_native._hipcc(), "-x", "hip", "--cuda-host-only", "-O1", f"-I{build_native.CSRC}",
                    str(root / "tools" / "mel_frame_host_check.cpp"), "-o", str(exe)], check=True, capture_output=True)
    records = []
    for n in range(385, 1401):
        records += [np.array([n, n // 256], dtype=np.int32),
                    np.pad(np.arange(n, dtype=np.int32), 384, mode="reflect")]
    np.concatenate(records).tofile(tmp_path / "reflect.i32")
    pcm, mel = GOLD["pcm_0"], GOLD["mel_0"]
    assert pcm.dtype == np.int16 and pcm.shape == (1024,) and mel.shape == (80, 4)
    pcm.tofile(tmp_path / "pcm.i16")
    np.ascontiguousarray(GOLD["basis"], dtype=np.float32).tofile(tmp_path / "basis.f32")
    np.ascontiguousarray(mel, dtype=np.float32).tofile(tmp_path / "mel.f32")
    r = subprocess.run([str(exe), *(str(tmp_path / f) for f in ("reflect.i32", "pcm.i16", "basis.f32", "mel.f32")),
                        repr(MEL_TOL)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


# ---- collate_wav ------------------------------------------------------------------------------------------------
def _items(sizes):
    g = torch.Generator().manual_seed(0)
    return [{"x": torch.randint(1, 150, (tx,), generator=g), "x_lengths": torch.tensor(tx),
             "wav": torch.randint(-32768, 32768, (n,), generator=g).to(torch.int16)} for tx, n in sizes]


def test_collate_wav_pads_with_zeros_to_the_quantum():
    items = _items([(5, 1000), (9, 4097), (3, 385)])
    out = collate_wav(items)
    assert set(out) == {"x", "x_lengths", "wav", "wav_lengths"}
    assert out["x"].shape == (3, 9) and out["x"].dtype == torch.int64
    assert out["wav"].shape == (3, 4352) and out["wav"].dtype == torch.int16  # 4097 up to a multiple of 256
    assert out["x_lengths"].tolist() == [5, 9, 3] and out["wav_lengths"].tolist() == [1000, 4097, 385]
    for b, it in enumerate(items):
        tx, n = it["x"].numel(), it["wav"].numel()
        assert torch.equal(out["x"][b, :tx], it["x"]) and (out["x"][b, tx:] == 0).all()
        assert torch.equal(out["wav"][b, :n], it["wav"]) and (out["wav"][b, n:] == 0).all()
    out = collate_wav(items, x_quantum=16, wav_quantum=4096)
    assert out["x"].shape == (3, 16) and out["wav"].shape == (3, 8192)
    assert (out["x"][:, 9:] == 0).all() and (out["wav"][:, 4097:] == 0).all()
    assert collate_wav(_items([(4, 512)]))["wav"].shape == (1, 512)  # already a multiple: nothing added
    assert collate_wav(items, wav_quantum=1)["wav"].shape == (3, 4097)


def test_collate_wav_checks_its_items():
    items = _items([(5, 1000), (9, 600)])
    collate_wav(items, n_vocab=150)
    with pytest.raises(ValueError):
        collate_wav(items, n_vocab=int(max(it["x"].max() for it in items)))  # the largest id is out of range
    bad = _items([(5, 1000)])
    bad[0]["wav"] = bad[0]["wav"].float()
    with pytest.raises(ValueError):
        collate_wav(bad)
    with pytest.raises(ValueError):
        collate_wav(items, wav_quantum=0)


# ---- MelSpectrogram.batch: what it refuses before any launch --------------------------------------------------------
@pytest.mark.parametrize("change", [dict(n_fft=2048, win_size=2048), dict(win_size=800), dict(hop_size=128),
                                    dict(center=True), dict(num_mels=97)])
def test_batch_refuses_unserved_geometry(change):
    m = MelSpectrogram(**{**CFG, **change})
    with pytest.raises(ValueError, match="1024"):
        m.batch(torch.zeros(1, 4096), [4096])


def test_batch_validates_host_lengths_and_inputs():
    m = MelSpectrogram(**CFG)
    y = torch.zeros(2, 4096)
    for bad in ([384, 4096], [4096, 4097], torch.tensor([0, 1000]), [1000], [1000.0, 2000.0]):
        with pytest.raises(ValueError):
            m.batch(y, bad)
    with pytest.raises(ValueError):
        m.batch(torch.zeros(4096), [4096])  # not [B, L]
    with pytest.raises(ValueError):
        m.batch(y.double(), [385, 4096])
    with pytest.raises(ValueError):
        m.batch(y, [385, 4096], mel_std=0.0)


def test_batch_refuses_cpu_tensors():
    m = MelSpectrogram(**CFG)
    with pytest.raises(N.NativeError):
        m.batch(torch.zeros(2, 4096), [385, 4096])
    with pytest.raises(N.NativeError):
        m.batch(torch.zeros(2, 4096, dtype=torch.int16), None)
    with pytest.raises(N.NativeError):
        MelStatistics().update(torch.zeros(1, 80, 4), [4])


def test_library_refuses_other_geometries_without_launching():
    """Size and geometry checks come before any pointer is looked at, so no pointer is passed: nothing could launch."""
    lib = N.lib()

    def call(B=1, L=4096, n_fft=1024, win=1024, hop=256, n_mels=80, clip=1e-5, std=1.0):
        return lib.mtts_mel_from_wav(None, 0, None, None, None, None, None, None, B, L, n_fft, win, hop, n_mels, clip,
                                     0.0, std, 0.0, None, None, None)

    assert call(n_fft=2048, win=2048) == -2 and call(win=800) == -2 and call(hop=128) == -2  # MTTS_ERR_SHAPE
    assert call(n_mels=97) == -2 and call(B=65536) == -2
    assert call(B=-1) == -1 and call(clip=0.0) == -1 and call(std=0.0) == -1  # MTTS_ERR_INVALID_ARG
    assert call() == -1 and b"null pointer" in lib.mtts_last_error()
    assert call(B=0) == 0
    assert lib.mtts_mel_stats(None, None, 0, 80, 10, None, None) == 0
    assert lib.mtts_mel_stats(None, None, 2, 80, 10, None, None) == -1
    assert lib.mtts_mel_stats(None, None, 2, 0, 10, None, None) == -1


# ---- MelStatistics arithmetic ---------------------------------------------------------------------------------------
def test_statistics_arithmetic_on_hand_made_sums():
    v = np.array([-1.5, 0.25, 2.0, -7.0, 3.5, 0.0], dtype=np.float64)
    got = MelStatistics.from_sums(v.sum(), (v * v).sum(), v.size)
    assert set(got) == {"mel_mean", "mel_std"} and all(isinstance(x, float) for x in got.values())
    assert got["mel_mean"] == pytest.approx(v.mean(), rel=1e-15)
    assert got["mel_std"] == pytest.approx(v.std(), rel=1e-14)  # the population form (ddof = 0)
    assert MelStatistics.from_sums(6.0, 12.0, 3) == {"mel_mean": 2.0, "mel_std": 0.0}
    assert math.isfinite(MelStatistics.from_sums(0.3, 0.03 - 1e-18, 3)["mel_std"])  # rounding below zero: clamped
    with pytest.raises(ValueError):
        MelStatistics.from_sums(0.0, 0.0, 0)
    with pytest.raises(ValueError):
        MelStatistics().result()
