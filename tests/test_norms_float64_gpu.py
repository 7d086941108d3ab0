"""GroupNorm+Mish, LayerNorm (csrc/norms.hip) and the fused CFM / prior losses (csrc/losses.hip) against the
float64 restatements of tests/norm_ref.py, element-wise, at every kernel variant the launchers choose by
shape, on both sides of each switch, with idle threads, row tails and partly filled chunks.

Inputs are drawn on the CPU with a seeded generator; the same fp32 values go to the device and, widened to
float64, to the reference.  Error of an output or gradient: max|got - ref| / max|ref|, printed for every
case.  Bounds: the project's fp32 op bound (TOL["fp32"]) per element -- 2e-5 forward,
1e-4 gradients; the two conditioning cases (mean 30, std 0.5) instead 4 x the error of the same formulas run
in plain fp32 on the CPU; the losses 1e-5 (the existing test's rtol).  The case tables are checked on the
CPU (tests/test_norm_ref_cpu.py) for the variants and boundaries they claim."""
from __future__ import annotations

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FWD_BOUND, GRAD_BOUND = 2e-5, 1e-4
LOSS_BOUND = 1e-5
COND_FACTOR = 4.0  # kernel error <= 4 x the plain fp32 restatement's (summation order, one-exponential Mish)
WORST: dict = {}  # (op, output) -> worst relative error seen, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (op, name), v in sorted(WORST.items()):
        print(f"worst {op} {name}: {v:.3e}")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _err(got, ref):
    ref = ref.double()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _close(op, name, got, ref, bound, case=""):
    e = _err(got, ref)
    WORST[(op, name)] = max(WORST.get((op, name), 0.0), e)
    print(f"{op} {case} {name}: err {e:.3e} (bound {bound:.1e})")
    assert torch.isfinite(got).all() and e <= bound, (op, case, name, e, bound)
    return e


def _ragged_mask(B, T, lengths=None):
    """Utterance 0 full, utterance 1 of length 1, a third one half full."""
    if lengths is None:
        lengths = [T, 1, max(1, T // 2)][:B]
    m = torch.zeros(B, T)
    for b, n in enumerate(lengths):
        m[b, :n] = 1
    return m


# ------------------------------------------------------------------------------------ GroupNorm + Mish
# (B, T, C, G, masked, add)
GN_CASES = (
    [(2, T, 256, 8, True, True) for T in (512, 513, 768, 769, 1024, 1025)]  # cpg 32 (the model's), rpp 128
    + [(3, T, 512, 2, True, True) for T in (64, 65, 96, 97, 128, 129)]  # cpg 256: cols 64, rpp 16
    + [(2, T, 24, 2, True, True) for T in (1364, 1365, 300)]  # cpg 12: cols 3, rpp 341, one idle thread
    + [(2, 817, 40, 2, True, True)]  # cpg 20: cols 5, rpp 204, 5 passes
    + [(2, T, 472, 2, True, True) for T in (17, 69, 140)]  # cpg 236: cols 59, rpp 17, 21 idle threads
    + [(2, 1, 32, 8, False, False), (2, 5, 32, 8, True, True)]  # cpg 4: one column
    + [(2, 300, 256, 8, False, False), (1, 600, 256, 8, True, True)]  # no mask / add; B = 1
)
GN_BF16_CASES = [(2, 513, 256, 8), (2, 769, 256, 8), (2, 1025, 256, 8), (2, 300, 24, 2)]
GN_OUTPUTS = ("y", "dh", "dgamma", "dbeta", "dadd")


def _gn_inputs(B, T, C, G, masked=True, add=True, seed=None, scale=3.0, shift=1.0):
    g = _gen(1000003 * B + 1009 * T + 7 * C + G if seed is None else seed)
    return dict(h=torch.randn(B, T, C, generator=g) * scale + shift, gamma=1 + 0.1 * torch.randn(C, generator=g),
                beta=0.1 * torch.randn(C, generator=g), G=G, mask=_ragged_mask(B, T) if masked else None,
                add=torch.randn(B, C, generator=g) if add else None, dy=torch.randn(B, T, C, generator=g))


def _gn_eval(fn, x, dtype, dev):
    """y and the gradients of fn(h, gamma, beta, G, mask, add) for the output gradient dy."""
    to = lambda t: None if t is None else t.to(device=dev, dtype=dtype)  # noqa: E731
    h, gamma, beta = (to(x[k]).requires_grad_(True) for k in ("h", "gamma", "beta"))
    add = None if x["add"] is None else to(x["add"]).requires_grad_(True)
    y = fn(h, gamma, beta, x["G"], to(x["mask"]), add)
    y.backward(to(x["dy"]))
    out = dict(y=y.detach(), dh=h.grad, dgamma=gamma.grad, dbeta=beta.grad)
    if add is not None:
        out["dadd"] = add.grad
    return out


def _gn_kernel(x):
    from matcha.models.components._ops import group_norm_mish_tm

    return _gn_eval(group_norm_mish_tm, x, torch.float32, DEV)


def _gn_reference(x, dtype=torch.float64):
    return _gn_eval(R.gn_mish_ref, x, dtype, "cpu")


def _gn_compare(got, ref, case, op="gn_mish"):
    assert set(got) == set(ref)
    for name in GN_OUTPUTS:
        if name in ref:
            _close(op, name, got[name], ref[name], FWD_BOUND if name == "y" else GRAD_BOUND, case)


@pytest.mark.parametrize("B,T,C,G,masked,add", GN_CASES)
def test_group_norm_mish_float64(B, T, C, G, masked, add):
    x = _gn_inputs(B, T, C, G, masked, add)
    _gn_compare(_gn_kernel(x), _gn_reference(x), f"{(B, T, C, G)} {R.gn_variant(T, C, G)}")


def test_group_norm_mish_padded_frames_count_in_statistics():
    """Utterance 1 has 40 valid frames of 130 and h = 50 on the padded ones: the statistics run over all 130
    frames, as the reference's do, so the valid frames' output depends on the padding."""
    B, T, C, G = 2, 130, 256, 8
    x = _gn_inputs(B, T, C, G)
    x["mask"] = _ragged_mask(B, T, [T, 40])
    x["h"][1, 40:] = 50.0
    got, ref = _gn_kernel(x), _gn_reference(x)
    valid = x["mask"].bool()
    _close("gn_mish", "y", got["y"].cpu()[valid], ref["y"][valid], FWD_BOUND, "padded h=50, valid frames")
    _gn_compare(got, ref, "padded h=50")
    x["h"][1, 40:] = 0.0  # the padding does move the valid frames: the case can see it ignored
    assert _err(_gn_reference(x)["y"][valid], ref["y"][valid]) > 0.1


def _conditioning(op, got, ref, plain, names):
    for name in names:
        ek, ep = _err(got[name], ref[name]), _err(plain[name], ref[name])
        print(f"{op} conditioning {name}: kernel {ek:.3e}, fp32 restatement {ep:.3e}, ratio {ek / ep:.2f}")
        WORST[(op + " conditioning ratio", name)] = ek / ep
        assert ek <= COND_FACTOR * ep, (op, name, ek, ep)


def test_group_norm_mish_conditioning():
    """mean 30, std 0.5: a one-pass variance loses about 240 times the two-pass form's accuracy here.  The
    kernel may err at most 4 x what the two-pass formulas give in plain fp32 on the CPU."""
    x = _gn_inputs(2, 600, 256, 8, scale=0.5, shift=30.0)
    _conditioning("gn_mish", _gn_kernel(x), _gn_reference(x), _gn_reference(x, torch.float32), ("y", "dh"))


def test_group_norm_mish_eps_inside_sqrt():
    """var ~ 1e-6 < eps = 1e-5: with eps outside the sqrt, or missing, the result is off by a factor ~3."""
    x = _gn_inputs(2, 300, 256, 8, scale=1e-3, shift=0.0)
    _gn_compare(_gn_kernel(x), _gn_reference(x), "h ~ 1e-3")


def test_group_norm_mish_range():
    """gamma = 40, beta in {-20, 0, 20}: u spans about +-160, through the exp clamp at 15 and the underflow
    of exp(u).  Forward bound per band of |u|, so the small outputs are not hidden behind the large ones."""
    B, T, C, G = 1, 1024, 32, 8
    x = _gn_inputs(B, T, C, G, masked=False, add=False)
    x["gamma"] = torch.full((C,), 40.0)
    x["beta"] = torch.tensor([-20.0, 0.0, 20.0]).repeat(C)[:C].contiguous()
    got, ref = _gn_kernel(x), _gn_reference(x)
    for v in got.values():
        assert torch.isfinite(v).all()
    u = R.gn_u_ref(x["h"].double(), x["gamma"].double(), x["beta"].double(), G).abs()
    assert float(u.max()) > 100
    for name, band in (("|u|<=4", u <= 4), ("4<|u|<=20", (u > 4) & (u <= 20)), ("|u|>20", u > 20)):
        assert int(band.sum()) > 100, name
        _close("gn_mish range", "y " + name, got["y"].cpu()[band], ref["y"][band], FWD_BOUND)
    _close("gn_mish range", "dh", got["dh"], ref["dh"], GRAD_BOUND)


@pytest.mark.parametrize("dy16", [False, True])
@pytest.mark.parametrize("B,T,C,G", GN_BF16_CASES)
def test_group_norm_mish_bf16_storage_at_boundaries(B, T, C, G, dy16):
    """test_group_norm_mish_bf16_storage's bitwise statement (the bf16-stored result equals the fp32-storage
    result rounded once) just past each `passes` boundary and with an idle thread."""
    from matcha.models.components import _ops as O

    g = _gen(B * T + G)
    h = (torch.randn(B, T, C, generator=g) * 2 + 0.5).bfloat16().to(DEV)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    m = _ragged_mask(B, T, [T, T - 9]).to(DEV)
    add = torch.randn(B, C, generator=g).to(DEV)
    dy = torch.randn(B, T, C, generator=g).to(DEV)
    if dy16:
        dy = dy.bfloat16().float()
    outs = []
    for x, o16 in ((h.float(), False), (h, dy16)):
        xx = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = O.group_norm_mish_tm(xx, gamma, beta, G, m, add, out_bf16=o16)
        y.backward(dy.to(y.dtype))
        outs.append((y.detach(), xx.grad))
    (y32, g32), (y16, g16) = outs
    assert y32.dtype == torch.float32 and g32.dtype == torch.float32
    assert y16.dtype == (torch.bfloat16 if dy16 else torch.float32) and g16.dtype == torch.bfloat16
    torch.testing.assert_close(y16.float(), y32.to(y16.dtype).float(), rtol=0, atol=0)
    torch.testing.assert_close(g16.float(), g32.bfloat16().float(), rtol=0, atol=0)


@pytest.mark.parametrize("B,T,C,G", [(2, 1025, 256, 8), (2, 69, 472, 2)])
def test_group_norm_mish_deterministic(B, T, C, G):
    x = _gn_inputs(B, T, C, G)
    a, b = _gn_kernel(x), _gn_kernel(x)
    for name in GN_OUTPUTS:
        assert torch.equal(a[name], b[name]), name


def test_group_norm_mish_limits():
    """The backward takes C/G <= 256 and a full workspace; it refuses anything else before launching (dh
    stays as filled).  The forward takes C/G = 260 (cols 65, rpp 15) and must be right there."""
    from matcha import _native as N
    from matcha.models.components import _ops as O

    lib = N.lib()

    def bwd(B, T, C, G, short):
        g = _gen(C)
        dy, h = (torch.randn(B, T, C, generator=g).to(DEV) for _ in range(2))
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        mean, rstd = torch.zeros(B, G, device=DEV), torch.ones(B, G, device=DEV)
        dh = torch.full((B, T, C), 7.0, device=DEV)
        dgamma, dbeta, dadd = (torch.full(s, 7.0, device=DEV) for s in ((C,), (C,), (B, C)))
        need = int(lib.mtts_gn_mish_bwd_workspace_size(B, C))
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        rc = lib.mtts_gn_mish_bwd_ex(dy.data_ptr(), h.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None,
                                     mean.data_ptr(), rstd.data_ptr(), dh.data_ptr(), dgamma.data_ptr(),
                                     dbeta.data_ptr(), dadd.data_ptr(), B, T, C, G, 0, ws.data_ptr(), need - short,
                                     torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        for t in (dh, dgamma, dbeta, dadd):
            assert bool((t == 7.0).all())
        return rc

    # include/mtts.h: MTTS_ERR_INVALID_ARG = -1 for a refused shape, MTTS_ERR_WORKSPACE = -3 (the ABI's own
    # code for this invalid argument) for a workspace one byte short
    assert bwd(1, 8, 520, 2, 0) == -1
    assert bwd(1, 8, 512, 2, 1) == -3
    x = _gn_inputs(1, 8, 520, 2)
    with torch.no_grad():
        y = O.group_norm_mish_tm(x["h"].to(DEV), x["gamma"].to(DEV), x["beta"].to(DEV), 2, x["mask"].to(DEV),
                                 x["add"].to(DEV))
    want = R.gn_mish_ref(*(x[k].double() for k in ("h", "gamma", "beta")), 2, x["mask"].double(), x["add"].double())
    _close("gn_mish", "y", y, want, FWD_BOUND, "(1, 8, 520, 2) forward only")


# ------------------------------------------------------------------------------------------ LayerNorm
LN_CASES = [
    (8195, 256), (8192 + 13, 32),  # forward four rows per wave, with a row tail
    (8191, 256),  # one row per wave, just below the switch
    (17, 256),  # backward: a second block of one row
    (12289, 192),  # backward: 32 rows per block
    (98305, 32),  # backward: the cap of 128 rows per block
    (77, 260), (33, 772), (5, 1024), (9, 4), (64, 252),  # partly filled chunks, one float4, C just under 256
]
LN_RES_CASES = [(8195, 256), (77, 772)]
LN_RELU_CASE = (8195, 256)


def _ln_inputs(M, C, scale=3.0, shift=1.0):
    g = _gen(131 * M + C)
    return dict(x=torch.randn(M, C, generator=g) * scale + shift, w=1 + 0.1 * torch.randn(C, generator=g),
                b=0.1 * torch.randn(C, generator=g), dy=torch.randn(M, C, generator=g))


def _ln_eval(fn, v, dtype, dev):
    x, w, b = (v[k].to(device=dev, dtype=dtype).requires_grad_(True) for k in ("x", "w", "b"))
    y = fn(x, w, b)
    y.backward(v["dy"].to(device=dev, dtype=dtype))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad)


def _ln_kernel(v, **kw):
    from matcha.models.components._ops import layer_norm_tm

    return _ln_eval(lambda x, w, b: layer_norm_tm(x, w, b, **kw), v, torch.float32, DEV)


def _ln_reference(v, dtype=torch.float64, fn=R.layer_norm_ref):
    return _ln_eval(fn, v, dtype, "cpu")


@pytest.mark.parametrize("M,C", LN_CASES)
def test_layer_norm_float64(M, C):
    v = _ln_inputs(M, C)
    got, ref = _ln_kernel(v), _ln_reference(v)
    case = f"{(M, C)} fwd {R.ln_fwd_variant(M, C)} bwd rows {R.ln_bwd_rows_per_block(M, C)}"
    for name in ("y", "dx", "dw", "db"):  # mean and rstd are checked through dx
        _close("layer_norm", name, got[name], ref[name], FWD_BOUND if name == "y" else GRAD_BOUND, case)


def test_layer_norm_conditioning():
    v = _ln_inputs(33, 772, scale=0.5, shift=30.0)
    _conditioning("layer_norm", _ln_kernel(v), _ln_reference(v), _ln_reference(v, torch.float32), ("y", "dx"))


@pytest.mark.parametrize("M,C", LN_RES_CASES)
def test_layer_norm_bwd_res_float64(M, C):
    """mtts_layernorm_bwd_res (the pre-LN blocks' backward): dx = LN-backward(dn) + dres."""
    from matcha.models.components import _ops as O

    v = _ln_inputs(M, C)
    dres = torch.randn(M, C, generator=_gen(M + C))
    x, w, b, dn = (v[k].to(DEV) for k in ("x", "w", "b", "dy"))
    n, mean, rstd = O._ln_fwd(x, w, b, 1e-5, False)
    dx, dw, db = O._ln_bwd_res(dn, x, w, b, mean, rstd, dres.to(DEV))
    ref = _ln_reference(v)
    case = f"{(M, C)} bwd_res"
    _close("layer_norm", "y", n, ref["y"], FWD_BOUND, case)
    _close("layer_norm_bwd_res", "dx", dx, ref["dx"] + dres.double(), GRAD_BOUND, case)
    _close("layer_norm_bwd_res", "dw", dw, ref["dw"], GRAD_BOUND, case)
    _close("layer_norm_bwd_res", "db", db, ref["db"], GRAD_BOUND, case)


def test_layer_norm_relu_float64():
    """The fused ReLU tail without dropout: gradients gated by the reference's LN(x) > 0.  Elements whose
    LN(x) lies within 1e-4 of the gate are left out of the element-wise comparisons; with w ~ 1 and b ~ 0.1
    that is about 0.01 % of them."""
    M, C = LN_RELU_CASE
    v = _ln_inputs(M, C)
    got = _ln_kernel(v, relu=True)
    ref = _ln_reference(v, fn=lambda x, w, b: torch.relu(R.layer_norm_ref(x, w, b)))
    ln = R.layer_norm_ref(*(v[k].double() for k in ("x", "w", "b")))
    keep = ln.abs() >= 1e-4
    left_out = 1.0 - float(keep.double().mean())
    print(f"layer_norm relu: {left_out:.4%} of the elements within 1e-4 of the gate")
    assert left_out < 1e-3
    case = f"{(M, C)} relu"
    _close("layer_norm relu", "y", got["y"].cpu()[keep], ref["y"][keep], FWD_BOUND, case)
    for name in ("dx", "dw", "db"):
        a, r = got[name].cpu(), ref[name]
        if name == "dx":
            e = float((a.double() - r)[keep].abs().max() / r.abs().max())
            WORST[("layer_norm relu", name)] = e
            print(f"layer_norm relu {case} dx: err {e:.3e} (bound {GRAD_BOUND:.1e})")
            assert torch.isfinite(a).all() and e <= GRAD_BOUND, e
        else:
            _close("layer_norm relu", name, a, r, GRAD_BOUND, case)


# ------------------------------------------------------------------------------------------ fused losses
LOSS_CASES = [(1, 1, 1), (2, 7, 64), (3, 80, 65), (2, 128, 128), (2, 80, 63), (4, 80, 129)]  # (B, C, T)
SIGMA_MIN = 1e-4


def _loss_inputs(B, C, T):
    g = _gen(10007 * B + 101 * C + T)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    lengths = [T, 1, max(1, T // 2), max(1, T - 3)][:B]
    mask = torch.zeros(B, T)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    return dict(u_pred=r(B, T, C), mu_y=r(B, C, T), x1=r(B, C, T), z=r(B, C, T), mask=mask)


def _loss_eval(fn, v, dtype, dev, with_u=True):
    to = lambda t: t.to(device=dev, dtype=dtype)  # noqa: E731
    u = to(v["u_pred"]).requires_grad_(True) if with_u else None
    mu = to(v["mu_y"]).requires_grad_(True)
    # fused_losses takes one tensor for x1 and y (the step's y is the flow's x1; _FusedLosses passes x1 for
    # both pointers), so y cannot be made distinct from x1 through the op
    diff, prior = fn(u, mu, to(v["x1"]), to(v["z"]), to(v["mask"]), SIGMA_MIN)
    (diff + 0.5 * prior).backward()
    return dict(diff=diff.detach(), prior=prior.detach(), du_pred=u.grad if with_u else None, dmu_y=mu.grad)


def _loss_compare(got, ref, mask, case, with_u=True):
    for name in ("diff", "prior") if with_u else ("prior",):
        e = abs(float(got[name]) - float(ref[name])) / abs(float(ref[name]))
        WORST[("losses", name)] = max(WORST.get(("losses", name), 0.0), e)
        print(f"losses {case} {name}: rel err {e:.3e} (bound {LOSS_BOUND:.1e})")
        assert e <= LOSS_BOUND, (case, name, float(got[name]), float(ref[name]))
    pad = mask == 0  # [B, T]
    _close("losses", "dmu_y", got["dmu_y"], ref["dmu_y"], LOSS_BOUND, case)
    dmu = got["dmu_y"].cpu().transpose(1, 2)  # [B, T, C]
    assert bool((dmu[pad] == 0).all())  # the prior loss is masked: exactly 0 on the padded frames
    if with_u:
        _close("losses", "du_pred", got["du_pred"], ref["du_pred"], LOSS_BOUND, case)
        assert bool((got["du_pred"].cpu()[pad] != 0).all())  # the diff loss is not: they contribute


@pytest.mark.parametrize("B,C,T", LOSS_CASES)
def test_fused_losses_float64(B, C, T):
    from matcha.models.components.flow_matching import fused_losses

    v = _loss_inputs(B, C, T)
    got = _loss_eval(fused_losses, v, torch.float32, DEV)
    ref = _loss_eval(R.losses_ref, v, torch.float64, "cpu")
    _loss_compare(got, ref, v["mask"], (B, C, T))


def test_fused_prior_loss_only_float64():
    from matcha.models.components.flow_matching import fused_losses

    v = _loss_inputs(2, 7, 64)
    got = _loss_eval(fused_losses, v, torch.float32, DEV, with_u=False)
    ref = _loss_eval(R.losses_ref, v, torch.float64, "cpu", with_u=False)
    assert float(got["diff"]) == 0.0
    _loss_compare(got, ref, v["mask"], "(2, 7, 64) prior only", with_u=False)


def test_fused_losses_refuse_more_than_128_channels():
    from matcha import _native as N
    from matcha.models.components.flow_matching import fused_losses

    v = {k: t.to(DEV) for k, t in _loss_inputs(1, 129, 4).items()}
    with pytest.raises(N.NativeError, match="C > 128"):
        fused_losses(v["u_pred"], v["mu_y"], v["x1"], v["z"], v["mask"], SIGMA_MIN)
