"""The fused mel front end on the MI355X (csrc/mel_fused.hip through MelSpectrogram.batch and MelStatistics): ragged
batches against the reference's own per-utterance mels (tests/golden/mel_golden.npz) and the numpy oracle
(oracle/mel_oracle.py), within the 1e-4 absolute bound on log-mel that tests/test_data_path.py holds the mel path to;
padding, batch independence, normalisation, statistics, no host synchronisation, graph capture, poisoned buffers."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

import poison
from matcha.utils.audio_process import MelSpectrogram, MelStatistics
from oracle.mel_oracle import mel_spectrogram

pytestmark = pytest.mark.gpu

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "mel_golden.npz")
CFG = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000)
MEL_TOL = 1e-4
GOLD_LENGTHS = [1024, 5000, 22050]
EDGE_LENGTHS = [385, 511, 512, 639, 640, 1023, 1025]
EDGE_L = 1301  # odd: rows 1, 3, 5 start off the 8-byte (fp32) / 4-byte (int16) boundary


@pytest.fixture(scope="module")
def mel():
    return MelSpectrogram(**CFG)


@pytest.fixture(scope="module")
def golden_batch():
    pcm = np.zeros((3, 22050), dtype=np.int16)
    for i, n in enumerate(GOLD_LENGTHS):
        assert GOLD[f"pcm_{i}"].shape == (n,)
        pcm[i, :n] = GOLD[f"pcm_{i}"]
    return torch.from_numpy(pcm).cuda()


@pytest.fixture(scope="module")
def edge_pcm():
    g = torch.Generator().manual_seed(21)
    x = (0.3 * torch.randn(len(EDGE_LENGTHS), EDGE_L, generator=g)).clamp(-1, 1)
    return (x * 32767).round().to(torch.int16)  # no zero padding: what lies past an utterance's end must not matter


def _as_float(pcm):
    return pcm.to(torch.float32) / 32768.0


def _oracle(pcm_row, n):
    return mel_spectrogram(_as_float(pcm_row[:n]).numpy()[None], **CFG)[0]


def test_ragged_golden_batch_int16_and_fp32(mel, golden_batch):
    got16, len16 = mel.batch(golden_batch, GOLD_LENGTHS)
    got32, len32 = mel.batch(_as_float(golden_batch), torch.tensor(GOLD_LENGTHS, device="cuda"))
    assert got16.shape == (3, 80, 86) and got16.dtype == torch.float32
    assert len16.dtype == torch.int64 and len16.tolist() == [4, 19, 86] and len32.tolist() == [4, 19, 86]
    assert poison.bits_equal(got16, got32)
    out = got16.cpu().numpy()
    for i, F in enumerate([4, 19, 86]):
        err = np.abs(out[i, :, :F] - GOLD[f"mel_{i}"]).max()
        print(f"utterance {i}: {F} frames, max |log-mel - reference| = {err:.3e}")
        assert err < MEL_TOL, (i, err)
        assert (out[i, :, F:] == 0.0).all() and not np.signbit(out[i, :, F:]).any()


def test_edge_lengths_in_one_batch_with_misaligned_rows(mel, edge_pcm):
    for y in (edge_pcm.cuda(), _as_float(edge_pcm).cuda()):
        got, lens = mel.batch(y, EDGE_LENGTHS)
        assert got.shape == (7, 80, EDGE_L // 256)
        assert lens.tolist() == [n // 256 for n in EDGE_LENGTHS] == [1, 1, 2, 2, 2, 3, 4]
        out = got.cpu().numpy()
        for b, n in enumerate(EDGE_LENGTHS):
            ref = _oracle(edge_pcm[b], n)
            assert ref.shape == (80, n // 256)
            err = np.abs(out[b, :, :n // 256] - ref).max()
            print(f"{y.dtype} len {n}: max |log-mel - oracle| = {err:.3e}")
            assert err < MEL_TOL, (n, err)
            assert (out[b, :, n // 256:] == 0.0).all()


def test_device_lengths_outside_the_range(mel, edge_pcm):
    y = edge_pcm[:4].cuda()
    lengths = torch.tensor([384, 0, EDGE_L + 7, -5], device="cuda")
    got, lens = mel.batch(y, lengths)
    assert lens.tolist() == [0, 0, EDGE_L // 256, 0]
    assert (got[[0, 1, 3]] == 0.0).all()
    full, _ = mel.batch(y[2:3], [EDGE_L])
    assert poison.bits_equal(got[2:3], full)  # L + 7 is treated as L
    assert np.abs(got[2].cpu().numpy() - _oracle(edge_pcm[2], EDGE_L)).max() < MEL_TOL
    none, lens = mel.batch(y, None)  # no lengths: every row has L samples
    assert lens.tolist() == [EDGE_L // 256] * 4 and poison.bits_equal(none[2:3], full)
    short, lens = mel.batch(y[:, :200], torch.tensor([200, 200, 100, 0], device="cuda"))  # L < 256: no frame at all
    assert short.shape == (4, 80, 0) and lens.tolist() == [0, 0, 0, 0]


def test_rows_do_not_depend_on_the_batch_and_calls_repeat(mel, golden_batch, edge_pcm):
    for y, lengths in ((golden_batch, GOLD_LENGTHS), (_as_float(golden_batch), GOLD_LENGTHS),
                       (edge_pcm.cuda(), EDGE_LENGTHS), (_as_float(edge_pcm).cuda(), EDGE_LENGTHS)):
        got, lens = mel.batch(y, lengths)
        again, _ = mel.batch(y, lengths)
        assert poison.bits_equal(got, again)
        for b, n in enumerate(lengths):
            alone, one = mel.batch(y[b:b + 1, :n], [n])
            assert one.tolist() == [n // 256]
            d = poison.difference(got[b:b + 1, :, :n // 256].contiguous(), alone)
            assert d is None, (y.dtype, n, d)


def test_normalisation_inside_the_kernel(mel, golden_batch):
    plain, lens = mel.batch(golden_batch, GOLD_LENGTHS)
    same, _ = mel.batch(golden_batch, GOLD_LENGTHS, mel_mean=0.0, mel_std=1.0)
    assert poison.bits_equal(plain, same)
    mean, std = -5.5, 2.0
    got, lens2 = mel.batch(golden_batch, GOLD_LENGTHS, mel_mean=mean, mel_std=std)
    assert torch.equal(lens, lens2)
    valid = torch.arange(plain.shape[2], device="cuda")[None, None] < lens[:, None, None]
    want = (plain - mean) / std  # fp32: both constants are exact in it
    ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
    worst = ((got - want).abs() / ulp)[valid.expand_as(got)].max()
    print(f"normalised vs (plain - mean) / std: {float(worst):.2f} ulp")
    assert float(worst) <= 1.0
    assert (got[~valid.expand_as(got)] == 0.0).all()  # the padding is not normalised


def test_statistics_over_two_batches(mel, golden_batch, edge_pcm):
    st = MelStatistics()
    values, frames = [], 0
    for y, lengths in ((golden_batch, GOLD_LENGTHS), (edge_pcm.cuda(), EDGE_LENGTHS)):
        m, lens = mel.batch(y, lengths)
        assert st.update(m, lens) is st
        for b, F in enumerate(lens.tolist()):
            values.append(m[b, :, :F].cpu().numpy().astype(np.float64).reshape(-1))
            frames += F
    v = np.concatenate(values)
    sums, n = st.state()
    assert int(n) == frames and v.size == 80 * frames
    s = sums.cpu().numpy()
    rel = [abs(s[0] - v.sum()) / abs(v.sum()), abs(s[1] - (v * v).sum()) / (v * v).sum()]
    got = st.result()
    rel += [abs(got["mel_mean"] - v.mean()) / abs(v.mean()), abs(got["mel_std"] - v.std()) / v.std()]
    print("relative errors (sum, sum of squares, mean, std):", ["%.2e" % r for r in rel], got)
    assert max(rel) <= 1e-10
    from matcha.models.matcha_tts import MatchaTTS

    model = MatchaTTS(n_vocab=20, out_channels=80, hidden_channels=192, data_statistics=got)
    assert float(model.mel_mean) == pytest.approx(got["mel_mean"]) and float(model.mel_std) == pytest.approx(got["mel_std"])


def test_no_host_synchronisation_and_graph_capture(mel, golden_batch):
    lengths = torch.tensor(GOLD_LENGTHS, device="cuda", dtype=torch.int32)
    y = golden_batch.clone()
    want, want_len = mel.batch(y, lengths)  # warm-up: the tables reach the device, the code object is loaded
    st = MelStatistics().update(want, want_len)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got, got_len = mel.batch(y, lengths, mel_mean=0.0, mel_std=1.0)
        st.update(got, got_len)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert poison.bits_equal(got, want) and torch.equal(got_len, want_len)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_mel, g_len = mel.batch(y, lengths)
    # new contents of the same shape: the rows rotated, other lengths
    y.copy_(golden_batch.roll(1, 0))
    lengths.copy_(torch.tensor([22050, 1000, 4999], device="cuda", dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager, eager_len = mel.batch(y.clone(), lengths.clone())
    assert g_len.tolist() == eager_len.tolist() == [86, 3, 19]
    assert poison.bits_equal(g_mel, eager)


def test_poisoned_buffers(mel, golden_batch, edge_pcm):
    y = edge_pcm.cuda()
    lengths = torch.tensor(EDGE_LENGTHS, device="cuda")
    mel.batch(y, lengths)  # the cached device tables are not what this test is about

    def fn():
        a, a_len = mel.batch(golden_batch, GOLD_LENGTHS, mel_mean=-5.5, mel_std=2.0)
        b, b_len = mel.batch(y, lengths)
        st = MelStatistics().update(a, a_len).update(b, b_len)
        return [a, a_len, b, b_len, *st.state()]

    poison.run_under_fills(fn)
