"""monotonic_align.duration_path on the device (csrc/mas.hip duration_path_kernel -> mas_expand_kernel): every
output against the reference's recorded paths (tests/golden/duration_path_golden.npz), the CPU oracle's
generate_path and the rule in Python numbers (duration_runs_host), bit for bit; and the existing consumers
(expand_rows, segment_crop) on alignments that cover fewer or more frames than t_y, against torch on the dense
path.  Everything is exact: integer outputs, one-hot products, and sums of integer-valued gradients."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from test_duration_path_cpu import B, CASES, attn_mask, golden, host_rule
from test_segment_gpu import _clamped, _torch_crop

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("attn", "dur", "col_row", "row_start", "lengths", "run_lengths")


def _call(name, d, xl, yl, Ty, **kw):
    from matcha.utils.monotonic_align import duration_path

    t = torch.from_numpy(d)
    if name.startswith("int64"):
        t = t.to(torch.int64)
    elif name.startswith("b1t"):
        t = t.unsqueeze(1)
    return duration_path(t.to(DEV), torch.from_numpy(xl).to(DEV), torch.from_numpy(yl).to(DEV), Ty, **kw)


@pytest.mark.parametrize("name,d,xl,yl,Ty", CASES, ids=[c[0] for c in CASES])
def test_op_vs_reference_fixture_oracle_and_rule(name, d, xl, yl, Ty):
    from oracle.matcha_oracle import generate_path

    got = _call(name, d, xl, yl, Ty)
    sparse = _call(name, d, xl, yl, Ty, dense=False)
    again = _call(name, d, xl, yl, Ty)
    torch.cuda.synchronize()
    attn = got[0].cpu().numpy()
    assert attn.dtype == np.float32 and attn.shape == (B, d.shape[1], Ty)
    np.testing.assert_array_equal(attn, golden()[name + "_path"])
    np.testing.assert_array_equal(attn, generate_path(torch.from_numpy(d), attn_mask(xl, yl, d.shape[1], Ty)).numpy())
    np.testing.assert_array_equal(got[1].cpu().numpy(), attn.sum(-1))
    want = host_rule(d, xl, yl, Ty)
    for n, a, w in zip(NAMES, got, want):
        a = a.cpu().numpy()
        assert a.dtype == (np.float32 if n in ("attn", "dur") else np.int32), n
        np.testing.assert_array_equal(a, w, err_msg=n)
    assert sparse[0] is None  # dense=False: no [B,Tx,Ty] write, nothing else changes
    for n, a, s, r in zip(NAMES[1:], got[1:], sparse[1:], again[1:]):
        assert torch.equal(a, s) and torch.equal(a, r), n
    assert torch.equal(got[0], again[0])  # two calls: bitwise


def test_longest_text_8192_rows_vs_numpy_repeat():
    """Tx = 8192 (32 rows per thread, the cap), Ty = 9000, runs only: ones, two rows of length 0 -- one at a
    thread's first row, one at a wave's last -- and one row of 500 frames; 8689 of the 9000 frames are covered."""
    from matcha.utils.monotonic_align import duration_path

    Tx, Ty = 8192, 9000
    d = np.ones(Tx, dtype=np.int64)
    d[[64, 2047]] = 0
    d[5000] = 500
    attn, dur, col_row, row_start, lengths, run_lengths = duration_path(
        torch.from_numpy(d)[None].to(DEV), torch.tensor([Tx], device=DEV), torch.tensor([Ty], device=DEV), Ty,
        dense=False)
    torch.cuda.synchronize()
    assert attn is None
    cov = int(d.sum())
    assert cov == 8689 and lengths.tolist() == [[Tx, Ty]] and run_lengths.tolist() == [[Tx, cov]]
    np.testing.assert_array_equal(col_row[0, :cov].cpu().numpy(), np.repeat(np.arange(Tx), d))
    assert (col_row[0, cov:] == -1).all()
    np.testing.assert_array_equal(dur[0].cpu().numpy(), d.astype(np.float32))
    np.testing.assert_array_equal(row_start[0].cpu().numpy(), np.cumsum(d) - d)


def test_errors():
    from matcha import _native as N
    from matcha.utils.monotonic_align import duration_path

    one = torch.ones(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="8192"):
        duration_path(torch.ones(1, 8193, device=DEV), one, one, 16)
    with pytest.raises(ValueError, match="x_lengths"):
        duration_path(torch.ones(2, 5, device=DEV), one, torch.ones(2, dtype=torch.int64, device=DEV), 16)
    with pytest.raises(ValueError):
        duration_path(torch.ones(2, 3, 5, device=DEV), one, one, 16)
    out = torch.empty(64, dtype=torch.int32, device=DEV)
    rc = N.lib().mtts_duration_path(None, N.ptr(one), N.ptr(one), 1, 5, 16, None, N.ptr(out), N.ptr(out), N.ptr(out),
                                    None, None, None)
    assert rc == -1 and b"duration_path" in N.lib().mtts_last_error()  # MTTS_ERR_INVALID_ARG, before any launch
    rc = N.lib().mtts_duration_path(N.ptr(out), N.ptr(one), N.ptr(one), 1, 8193, 16, None, None, None, None, None,
                                    None, None)
    assert rc == -2  # MTTS_ERR_SHAPE


# ------------------------------------------------------------------------- the consumers on run_lengths
C_TX, C_TY, C_S, C_CH = 6, 50, 16, 3
# utterance 0 covers 30 of its 50 frames (a row of length 0 inside); utterance 1 asks for 55 of its 40 (row 3 is
# cut at t_y, rows 4 and 5 get nothing: two trailing rows of length 0 that share their start with t_cov)
C_D = [[10, 0, 8, 2, 6, 4], [12, 9, 9, 25, 3, 0]]
C_XL, C_YL = [6, 6], [50, 40]
C_OFF = [25, 24]  # window [25, 41): frames 30.. are unaligned; window [24, 40): ends where utterance 1 does
_CONS = {}


def _consumer_case():
    if not _CONS:
        from matcha.utils.monotonic_align import duration_path

        g = torch.Generator().manual_seed(7)
        out = duration_path(torch.tensor(C_D, device=DEV), torch.tensor(C_XL, device=DEV),
                            torch.tensor(C_YL, device=DEV), C_TY)
        assert out[5].tolist() == [[6, 30], [6, 40]] and out[4].tolist() == [[6, 50], [6, 40]]
        _CONS.update(out=out, mu=torch.randn(2, C_CH, C_TX, generator=g).to(DEV),
                     y=torch.randn(2, C_CH, C_TY, generator=g).to(DEV),
                     dy=torch.randint(-8, 9, (2, C_CH, C_TY), generator=g).float().to(DEV),
                     ds=torch.randint(-8, 9, (2, C_CH, C_S), generator=g).float().to(DEV))
    return _CONS


def test_expand_rows_on_under_and_over_covered_runs_vs_bmm():
    from matcha.utils.monotonic_align import expand_rows

    c = _consumer_case()
    attn, _, col_row, row_start, _, run_lengths = c["out"]
    a = c["mu"].clone().requires_grad_(True)
    r = c["mu"].clone().requires_grad_(True)
    got = expand_rows(a, col_row, row_start, run_lengths)
    want = torch.matmul(attn.transpose(1, 2), r.transpose(1, 2)).transpose(1, 2)
    got.backward(c["dy"])  # integer-valued: every order of summation gives the same bits
    want.backward(c["dy"])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert (got[0, :, 30:] == 0).all() and (got[1, :, 40:] == 0).all()
    assert torch.equal(a.grad, r.grad)
    assert (a.grad[0, :, 1] == 0).all() and (a.grad[1, :, 4:] == 0).all() and a.grad.abs().max() > 0


def test_segment_crop_with_run_lengths_vs_torch_crop():
    from matcha.utils.monotonic_align import segment_crop

    c = _consumer_case()
    attn, _, col_row, row_start, lengths, run_lengths = c["out"]
    a = c["mu"].clone().requires_grad_(True)
    r = c["mu"].clone().requires_grad_(True)
    got = segment_crop(c["y"], a, col_row, row_start, lengths, C_S, offsets=torch.tensor(C_OFF, device=DEV),
                       run_lengths=run_lengths)
    want = _torch_crop(c["y"], r, attn, C_YL, _clamped(C_OFF, C_YL, C_S), C_S)
    got[1].backward(c["ds"])
    want[1].backward(c["ds"])
    torch.cuda.synchronize()
    for name, g_, w_ in zip(("y_cut", "mu_y_cut", "attn_cut", "y_mask", "seg"), got, want):
        assert g_.shape == w_.shape and torch.equal(g_.detach(), w_.detach()), name
    assert got[4].tolist() == [[25, 16], [24, 16]]
    assert (got[1][0, :, 5:] == 0).all()  # frames 30.. of utterance 0: inside the window, aligned to nothing
    assert torch.equal(a.grad, r.grad)
    assert a.grad.abs().max() > 0
