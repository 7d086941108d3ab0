"""Explicit schedule ids after the forward-GEMM tables were pruned: an id that left the tables (0 and 13 of the
register-staged table, 33 and 43 of the LDS-DMA one) is refused before any launch -- the library error is raised and
the output buffer keeps its fill -- and a kept id still runs: 7, which is also the heuristic's pick at this shape,
gives the heuristic call's output bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, T, CIN, COUT = 2, 33, 64, 64
SENTINEL = -123.5
_OPERANDS = []


def _operands():
    """x, w and the packed bf16 weight, built once and never modified."""
    from matcha.models.components import _ops as O

    if not _OPERANDS:
        g = torch.Generator(device="cpu").manual_seed(17)
        x = torch.randn(B, T, CIN, generator=g).to(DEV)
        w = (torch.randn(COUT, CIN, generator=g) / CIN ** 0.5).to(DEV)
        _OPERANDS.extend([x, w, *O.pack_weight(w, O.PREC_BF16)])
    return _OPERANDS


def _gemm_into_sentinel(tile_cfg):
    """The output buffer, filled with the sentinel before the call; the call's exception, if any."""
    from matcha import _native as N
    from matcha.models.components import _ops as O

    x, _, Wp, Kp = _operands()
    y = torch.full((B, T, COUT), SENTINEL, device=DEV)
    err = None
    try:
        O._gemm(x, T, T, B, 1, [0], CIN, Wp, Kp, COUT, y, T, prec=O.PREC_BF16, tile_cfg=tile_cfg)
    except N.NativeError as e:
        err = e
    torch.cuda.synchronize()
    return y, err


@pytest.mark.parametrize("cfg", [0, 13, 33, 43])
def test_removed_id_raises_and_launches_nothing(cfg):
    y, err = _gemm_into_sentinel(cfg)
    assert err is not None and "bad tile config" in str(err), err
    assert (y == SENTINEL).all()


def test_kept_id_matches_the_heuristic_call_bitwise():
    auto, err = _gemm_into_sentinel(-1)
    assert err is None
    seven, err = _gemm_into_sentinel(7)
    assert err is None
    assert torch.isfinite(auto).all() and not (auto == SENTINEL).any()
    assert torch.equal(seven, auto)
    # and it is the GEMM: bf16 operands (products exact in fp32), K = 64 fp32 accumulations of 2^-24 each
    x, w = _operands()[:2]
    xb, wb = x.bfloat16().double().reshape(-1, CIN), w.bfloat16().double()
    bound = CIN * 2.0 ** -24 * (xb.abs() @ wb.abs().T)
    assert ((auto.double().reshape(-1, COUT) - xb @ wb.T).abs() <= bound).all()


@pytest.mark.parametrize("cin", [64, 96])  # whole-tap K steps: the scalar-addressed loop; 96: the register-addressed one
def test_three_plane_fallbacks_bitwise(cin):
    """Three weight planes (bf16x6) are built on the 64 x 64 tiles only: 45 (two stages) runs its own kernel and
    every other LDS-DMA id falls back by its stage count -- 41 and 46 to 45, 42 and 47 to 44.  The stage count does
    not change the order of the products, so every id gives the heuristic's (44) output bit for bit."""
    from matcha.models.components import _ops as O

    g = torch.Generator(device="cpu").manual_seed(cin)
    x = torch.randn(B, T, cin, generator=g).to(DEV)
    w = (torch.randn(COUT, cin, 3, generator=g) / (3 * cin) ** 0.5).to(DEV)
    outs = {}
    with O.precise_forward("bf16x6"):
        Wp, Kp = O.packed(O.spec_conv_fwd(w), O.PREC_BF16)
        assert Wp._mtts_w_split3
        for cfg in (-1, 44, 45, 41, 42, 46, 47):
            y = torch.full((B, T, COUT), SENTINEL, device=DEV)
            O._gemm(x, T, T, B, 1, [-1, 0, 1], cin, Wp, Kp, COUT, y, T, prec=O.PREC_BF16, tile_cfg=cfg)
            outs[cfg] = y
    torch.cuda.synchronize()
    conv = lambda a, b_: torch.nn.functional.conv1d(a.double().transpose(1, 2), b_.double(), padding=1).transpose(1, 2)  # noqa: E731
    # fp32-class: per element 6 K products into fp32 accumulators (each addition rounds by <= 2^-24 of the running
    # sum of magnitudes) and the omitted plane products, each below 2^-24 of |x||w|: a worst-case bound, far above
    # the measured distance (tests/test_weight_split_gpu.py: ~1e-7 .. 6e-7 of the output scale)
    bound = (6 * 3 * cin + 8) * 2.0 ** -24 * conv(x.abs(), w.abs())
    assert ((outs[-1].double() - conv(x, w)).abs() <= bound).all()
    for cfg, y in outs.items():
        assert torch.equal(y, outs[-1]), cfg
