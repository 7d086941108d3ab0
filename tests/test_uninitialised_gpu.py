"""No result may depend on what a `torch.empty` buffer held before the kernels ran.

Every case runs under tests/poison.py's `run_under_fills`: all `torch.empty` / `torch.empty_like` buffers (outputs,
saved activations, bf16 pre-activations, lse, mean / rstd, split-K and weight-gradient workspaces, packed weight
planes, MAS workspaces, the vocoder's ping-pong buffers) are filled with 0x00, 0x00 again, 0x7F (3.39e38, int32
2139062143) and 0xFF (NaN, int32 -1); everything the caller can see -- every returned tensor in full, padded rows
and columns included, and every input / parameter gradient -- must be finite and bitwise the same under all of them.
Where a case drives an internal entry point (`O._gemm`, `O._wgrad`, `_attn_fwd/_bwd`, `mtts_colsum`,
`mtts_reduce_partials`) the test allocates the output with `torch.empty` inside the poisoned run and the whole
buffer is compared, except the regions the call documents as untouched (the other stride-2 output phase, the
columns N..ldc of a wider C): those must still hold the fill byte.

Workspaces and scratch outputs: what the kernels read before writing, and who initialises it (read from csrc/
before the first poisoned run; no region is used as an index, count or flag, so poison cannot turn into a wild
access or an endless wait):

| entry point (file) | buffer from torch.empty | read before written? | initialised by |
|---|---|---|---|
| mtts_conv_gemm_ws (conv_gemm.hip, _glds, _wreg) | split-K partial slabs `ws` | no: the combine pass reads only the slabs its own launch wrote | the GEMM kernel |
| same | C, C_pre | no; the other stride-2 phase and columns N..ldc are never touched | the epilogue |
| mtts_pack_weights (pack.hip) | packed planes [rows, Kp] | no; columns K..Kp are written as zeros | the pack kernel |
| mtts_conv_wgrad_tile (conv_gemm.hip) | `ws`: partial dW / db slabs, one per row split | no: every split's kernel writes its whole slab, the reduction reads `splits` slabs | the wgrad kernel; for an empty batch (M = 0) hipMemsetAsync in the entry point, on the launch stream |
| mtts_reduce_partials, mtts_colsum (reduce.hip) | column partials | no | colsum_partials_kernel |
| mtts_gn_mish_bwd, mtts_layernorm_bwd (norms.hip) | per-block dgamma / dbeta partials | no | the backward kernel's first pass |
| mtts_attention_bwd (attention.hip) | `Drow` [B,H,T] | no | the Drow pre-pass of the same call |
| mtts_attention_fwd | o, lse | no; rows past the key length are written too | the forward kernel |
| mtts_losses_fwd (losses.hip) | per-block partial sums | no | the first kernel of the call |
| mtts_maximum_path_f32 / mtts_prior_maximum_path (mas.hip) | `ws`: lengths, row_start, direction bits, transposed lattice | bits: only the words of rows < t_x and columns <= t_y, which the DP wrote; row_start past t_x: -1 from the LDS copy (`rs` is initialised in LDS); `mw_done` is LDS, workgroup scope | the DP kernel |
| mtts_duration_path, expand_rows, segment_crop | dur, col_row, row_start, lengths, seg, outputs | no; rows / frames past the lengths are written (-1 / 0) | the kernels |
| mtts_clip_adamw_scaled (optim.hip) | `_ws`: nchunks partial norms + t_next | no | adamw_sumsq_kernel |
| mtts_rows_linear_* (time_mlp.hip) | `part` of the chunked backward | no | the kernel; its split-K partials and ticket counters live in a torch.zeros buffer (_ops._rows_ws) and the kernel resets the counters |
| mtts_embedding_bwd (embedding.hip) | dw [V,C] | no: one workgroup per vocabulary entry writes its row, zeros for unused ids | the kernel |
| mtts_voc_* (vocoder.hip) | `ws` (token-major mel), acc / tmp / h0 / h1 | no: ACC_INIT writes acc before ACC_ADD / ACC_MEAN read it | the kernels |
| mtts_gl_* (griffinlim.hip), mtts_mel (mel.hip) | outputs | no | the kernels |

Buffers allocated on the main stream and first written on the deferral's side stream (Decoder.prefetch: packed
planes, time embedding, time MLP outputs) are allocated before the fork: the captured Trainer cases below failed
(a non-finite CFM loss on the second step) while the fork came first, because the fill, like anything else the
main stream does with that memory after the fork, was not ordered before the side-stream writers.

`O._gemm` accepts only cin % 8 == 0, so K = taps * cin is a multiple of 8 and no accepted GEMM shape has Kp > K;
the packed rows wider than their K are the transposed (dgrad) operands of an output count that is no multiple of
8, which the one-channel `linear_tm` case below packs inside the poisoned run (N = 1 -> Kp = 8).
"""
import math

import pytest
import torch

import poison as P
from golden.weights_recipe import apply_recipe

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PRECS = ["fp32", "bf16"]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _mask(B, T, seed=0):
    lens = torch.randint(T // 2, T + 1, (B,), generator=_gen(seed))
    lens[0] = T
    return (torch.arange(T)[None] < lens[:, None]).float().to(DEV)


def _flat(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, dict):
        out = list(out.values())
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _flat(o)]
    return []


def _fwd_bwd(fn, params, prec="fp32"):
    """fn(*leaves) under the fills: every tensor it returns and the gradient of every leaf (the output gradients are
    drawn once and shared by the runs)."""
    dys = []

    def run():
        xs = [p.detach().clone().requires_grad_(True) for p in params]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
            outs = _flat(fn(*xs))
        diff = [o for o in outs if o.requires_grad]
        if not dys:
            g = _gen(99)
            dys.extend(torch.randn(o.shape, generator=g).to(o.device, o.dtype) for o in diff)
        torch.autograd.backward(diff, dys)
        assert all(x.grad is not None for x in xs)
        return outs + [x.grad for x in xs]

    return P.run_under_fills(run)


def _r(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _holds_fill(t, byte):
    return bool((t.contiguous().view(torch.uint8) == byte).all())


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,T,Cin,Cout,k,stride", [(2, 37, 32, 64, 3, 1), (2, 41, 32, 32, 3, 2), (2, 33, 256, 80, 1, 1)])
def test_conv_tm(B, T, Cin, Cout, k, stride, prec):
    from matcha.models.components import _ops as O

    g = _gen(B * T + Cin + k)
    x, w, b = _r(g, B, T, Cin), _r(g, Cout, Cin, k, scale=(Cin * k) ** -0.5), _r(g, Cout, scale=0.1)
    m = _mask(B, T, 1)
    _fwd_bwd(lambda x_, w_, b_: O.conv_tm(x_, w_, b_, mask=m, stride=stride), [x, w, b], prec)


@pytest.mark.parametrize("prec", PRECS)
def test_conv_tm_out_scale_residual_and_relu_dropout(prec):
    from matcha.models.components import _ops as O

    B, T, C = 2, 37, 32
    g = _gen(5)
    x, r = _r(g, B, T, C), _r(g, B, T, C)
    w3, w5, b = _r(g, C, C, 3, scale=0.1), _r(g, C, C, 5, scale=0.1), _r(g, C, scale=0.1)
    m = _mask(B, T, 2)
    _fwd_bwd(lambda x_, r_, w_, b_: O.conv_tm(x_, w_, b_, residual=r_, out_scale=m), [x, r, w3, b], prec)
    _fwd_bwd(lambda x_, w_, b_: O.conv_tm(x_, w_, b_, mask=m, relu=True, dropout_p=0.1), [x, w5, b], prec)
    _fwd_bwd(lambda x_, w_, b_: O.conv_tm(x_, w_, b_, mask=m, out_bf16=prec == "bf16"), [x, w3, b], prec)


@pytest.mark.parametrize("prec", PRECS)
def test_conv_transpose_tm(prec):
    from matcha.models.components import _ops as O

    B, T, C = 2, 19, 32
    g = _gen(6)
    x, w, b = _r(g, B, T, C), _r(g, C, C, 4, scale=0.1), _r(g, C, scale=0.1)
    m = _mask(B, T, 3)
    _fwd_bwd(lambda x_, w_, b_: O.conv_transpose_tm(x_, w_, b_, m), [x, w, b], prec)


@pytest.mark.parametrize("prec", PRECS)
def test_linear_tm(prec):
    from matcha.models.components import _ops as O

    g = _gen(7)
    x, w, b, r = _r(g, 77, 32), _r(g, 96, 32, scale=32 ** -0.5), _r(g, 96, scale=0.1), _r(g, 77, 96)
    _fwd_bwd(lambda x_, w_, b_, r_: O.linear_tm(x_, w_, b_, residual=r_, dropout_p=0.1), [x, w, b, r], prec)
    # [2, 77, 256] x [256, 256]: the LDS-DMA schedules in bf16
    x, w, b = _r(g, 2, 77, 256), _r(g, 256, 256, scale=1 / 16), _r(g, 256, scale=0.1)
    m = _mask(2, 77, 4)
    _fwd_bwd(lambda x_, w_, b_: O.linear_tm(x_, w_, b_), [x, w, b], prec)
    _fwd_bwd(lambda x_, w_, b_: O.linear_tm(x_, w_, b_, in_scale=m, out_scale=m), [x, w, b], prec)
    # q|k|v stacked along N, no bias
    ws = [_r(g, 256, 256, scale=1 / 16) for _ in range(3)]
    _fwd_bwd(lambda x_, a, b_, c: O.linear_tm(x_, (a, b_, c), None), [x] + ws, prec)
    # one output channel: the dgrad operand [K][Kp = 8] is a packed row wider than its K = 1
    w1, b1 = _r(g, 1, 256, scale=1 / 16), _r(g, 1, scale=0.1)
    _fwd_bwd(lambda x_, w_, b_: O.linear_tm(x_, w_, b_, in_scale=m, out_scale=m), [x, w1, b1], prec)


@pytest.mark.parametrize("prec", PRECS)
def test_ff_tm(prec):
    from matcha.models.components import _ops as O

    M, C = 130, 32
    g = _gen(8)
    x, r = _r(g, M, C), _r(g, M, C)
    w1, b1, w2, b2 = _r(g, 4 * C, C, scale=C ** -0.5), _r(g, 4 * C, scale=0.1), _r(g, C, 4 * C, scale=0.09), _r(g, C, scale=0.1)
    _fwd_bwd(lambda x_, a, b, c, d, r_: O.ff_tm(x_, a, b, c, d, residual=r_, dropout_p=0.25), [x, w1, b1, w2, b2, r], prec)


@pytest.mark.parametrize("prec", PRECS)
def test_conv_ffn_tm(prec):
    from matcha.models.components import _ops as O

    B, T, C, Fc = 3, 45, 64, 128
    g = _gen(9)
    x = _r(g, B, T, C)
    w1, b1 = _r(g, Fc, C, 3, scale=(3 * C) ** -0.5), _r(g, Fc, scale=0.1)
    w2, b2 = _r(g, C, Fc, 3, scale=(3 * Fc) ** -0.5), _r(g, C, scale=0.1)
    m = _mask(B, T, 5)
    _fwd_bwd(lambda x_, a, b, c, d: O.conv_ffn_tm(x_, a, b, c, d, m, residual=x_, p_in=0.1, p_out=0.19),
             [x, w1, b1, w2, b2], prec)


@pytest.mark.parametrize("prec,out_bf16", [("fp32", False), ("bf16", False), ("bf16", True)])
def test_group_norm_mish_tm(prec, out_bf16):
    from matcha.models.components import _ops as O

    B, T, C, G = 2, 37, 32, 8
    g = _gen(10)
    h, gamma, beta, add = _r(g, B, T, C), 1 + _r(g, C, scale=0.1), _r(g, C, scale=0.1), _r(g, B, C)
    m = _mask(B, T, 6)
    _fwd_bwd(lambda h_, ga, be, ad: O.group_norm_mish_tm(h_, ga, be, G, m, ad, out_bf16=out_bf16), [h, gamma, beta, add],
             prec)
    _fwd_bwd(lambda h_, ga, be: O.group_norm_mish_tm(h_, ga, be, G, m, out_bf16=out_bf16), [h, gamma, beta], prec)


@pytest.mark.parametrize("M,C", [(77, 32), (5, 1024)])
@pytest.mark.parametrize("relu,p", [(False, 0.0), (True, 0.1)])
def test_layer_norm_tm(M, C, relu, p):
    from matcha.models.components import _ops as O

    g = _gen(M + C)
    x, w, b = _r(g, M, C), 1 + _r(g, C, scale=0.1), _r(g, C, scale=0.1)
    _fwd_bwd(lambda x_, w_, b_: O.layer_norm_tm(x_, w_, b_, 1e-5, relu=relu, dropout_p=p), [x, w, b])


ATTN_SHAPES = [(3, 33, 2, 96), (2, 130, 2, 64), (2, 77, 2, 16)]  # short kernels; long kernels; zero-padded head dim


def _key_bias(B, T, seed):
    from matcha.models.components import _ops as O

    lens = torch.randint(T // 2, T + 1, (B,), generator=_gen(seed))
    lens[0] = T
    return O.sequence_mask_f32(lens.to(DEV), T, key_bias=True)[1]  # ragged: (mask - 1) * 1e4


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,H,D", ATTN_SHAPES)
def test_attention_tm(B, T, H, D, p, prec):
    from matcha.models.components import _ops as O

    qkv = _r(_gen(B * T + D), B, T, 3 * H * D)
    kb = _key_bias(B, T, 7)
    _fwd_bwd(lambda q: O.attention_tm(q, kb, H, dropout_p=p), [qkv], prec)


@pytest.mark.parametrize("merged", ["1", "0"])
@pytest.mark.parametrize("io16", [False, True])
@pytest.mark.parametrize("B,T,H,D", ATTN_SHAPES)
def test_attention_entry_points(monkeypatch, B, T, H, D, io16, merged):
    """_attn_fwd / _attn_bwd with o and lse allocated here; bf16 storage (MTTS_ATTN_F_IO_BF16); the merged and the
    two-launch backward."""
    from matcha.models.components import _ops as O

    monkeypatch.setenv("MTTS_ATTN_BWD_MERGED", merged)
    g = _gen(B + T + D)
    dt = torch.bfloat16 if io16 else torch.float32
    qkv, do = _r(g, B, T, 3 * H * D).to(dt), _r(g, B, T, H * D).to(dt)
    kb = _key_bias(B, T, 8)
    seed = torch.tensor([4321, 765], dtype=torch.int32, device=DEV)
    prec = O.PREC_BF16 if io16 else O.PREC_FP32

    def run():
        o = torch.empty(B, T, H * D, device=DEV, dtype=dt)
        lse = torch.empty(B, H, T, device=DEV, dtype=torch.float32)
        O._attn_fwd(qkv, kb, o, lse, H, prec, dropout_p=0.1, seed=seed)
        return [o, lse, O._attn_bwd(do, qkv, kb, o, lse, H, prec, dropout_p=0.1, seed=seed)]

    P.run_under_fills(run)


@pytest.mark.parametrize("prec", PRECS)
def test_preln_blocks(prec):
    from matcha.models.components import _ops as O

    B, T, C, H = 3, 37, 64, 2
    g = _gen(11)
    h = _r(g, B, T, C)
    ln_w, ln_b = 1 + _r(g, C, scale=0.1), _r(g, C, scale=0.1)
    wq, wk, wv, wo = (_r(g, C, C, scale=C ** -0.5) for _ in range(4))
    bo = _r(g, C, scale=0.1)
    w1, b1, w2, b2 = _r(g, 4 * C, C, scale=C ** -0.5), _r(g, 4 * C, scale=0.1), _r(g, C, 4 * C, scale=0.06), _r(g, C, scale=0.1)
    kb = torch.zeros(B, T, device=DEV)
    for b in range(B):
        kb[b, : T - 7 * b] = 1  # the decoder's float 0/1 mask, added to the scores
    _fwd_bwd(lambda h_, a, b_, q, k, v, o, ob: O.preln_attention_tm(h_, a, b_, 1e-5, kb, H, q, k, v, o, ob, dropout_p=0.1),
             [h, ln_w, ln_b, wq, wk, wv, wo, bo], prec)
    _fwd_bwd(lambda h_, a, b_, c, d, e, f: O.preln_ff_tm(h_, a, b_, 1e-5, c, d, e, f, dropout_p=0.1),
             [h, ln_w, ln_b, w1, b1, w2, b2], prec)


@pytest.mark.parametrize("d", [96, 20])
def test_rope_tm(d):
    from matcha.models.components import _ops as O
    from matcha.models.components.text_encoder import RotaryPositionalEmbeddings

    B, T, H = 3, 37, 2
    rp = RotaryPositionalEmbeddings(d * 0.5)
    cos, sin = rp.tables(T, DEV)
    _fwd_bwd(lambda q: O.rope_tm(q, cos, sin, H, rp.feature_dim), [_r(_gen(d), B, T, 3 * H * d)])


def test_cat_skip_feeds_a_conv():
    """cat_skip_tm allocates nothing itself; its row-strided gradient slices reach the conv's dgrad GEMM."""
    from matcha.models.components import _ops as O

    B, T, C = 2, 37, 32
    g = _gen(12)
    h, s, w, b = _r(g, B, T, C), _r(g, B, T, C), _r(g, C, 2 * C, 3, scale=0.1), _r(g, C, scale=0.1)
    m = _mask(B, T, 9)
    _fwd_bwd(lambda h_, s_, w_, b_: O.conv_tm(O.cat_skip_tm(O.conv_tm(h_, w_[:, :C], b_, m), s_), w_, b_, m), [h, s, w, b])


def test_embedding_forward_and_backward():
    from matcha.models.components.text_encoder import _Embedding

    B, T, V, C = 3, 17, 150, 192
    g = _gen(13)
    ids = torch.randint(1, 40, (B, T), generator=g).to(DEV)  # ids 40..149 (and 0) unused: their dw rows are the point
    w = _r(g, V, C)
    outs = _fwd_bwd(lambda w_: _Embedding.apply(ids, w_, math.sqrt(C)), [w])
    assert (outs[-1][40:] == 0).all() and (outs[-1][0] == 0).all()


def test_step_glue_ops():
    from matcha.models.components import _ops as O
    from matcha.models.components.decoder import SinusoidalPosEmb
    from matcha.models.components.flow_matching import _CfmPack, fused_losses

    g = _gen(14)
    B, T, C = 3, 77, 80
    lens = torch.tensor([77, 40, 12], device=DEV)
    P.run_under_fills(lambda: list(O.sequence_mask_f32(lens, T, key_bias=True)) + [O.sequence_mask_f32(lens.int(), T)])
    mask = O.sequence_mask_f32(lens, T)
    dur = torch.randint(0, 12, (B, T), generator=g).float().to(DEV) * mask
    logw = _r(g, B, 1, T) * mask.unsqueeze(1)
    _fwd_bwd(lambda lw: O.duration_loss_fused(lw, dur, lens), [logw])
    vals = [torch.tensor(v, device=DEV) for v in (0.75, 2.5, 4.125)]
    _fwd_bwd(lambda a, b, c: O.loss_sum(a, b, c), vals)
    _fwd_bwd(lambda a, c: O.loss_sum(a, 0, c), vals[::2])
    x1, z, mu = _r(g, B, C, T), _r(g, B, C, T), _r(g, B, C, T)
    t = torch.rand(B, 1, 1, generator=g).to(DEV)
    _fwd_bwd(lambda mu_: _CfmPack.apply(x1, z, t, mu_, 1e-4), [mu])
    u = _r(g, B, T, C)
    m3 = mask.unsqueeze(1)
    _fwd_bwd(lambda u_, mu_: fused_losses(u_, mu_, x1, z, m3, 1e-4), [u, mu])
    _fwd_bwd(lambda mu_: fused_losses(None, mu_, x1, z, m3, 1e-4)[1], [mu])
    tt = torch.rand(7, generator=g).to(DEV)
    P.run_under_fills(lambda: [SinusoidalPosEmb(80)(tt, scale=1000)])


@pytest.mark.parametrize("B,width,dim", [(5, 256, 1024), (7, 96, 200)])
def test_time_mlp(B, width, dim):
    from matcha.models.components import _ops as O
    from matcha.models.components.decoder import TimeStepEmbeddingNet

    torch.manual_seed(B)
    mlp = TimeStepEmbeddingNet(160, dim).to(DEV)
    projs = [torch.nn.Linear(dim, width).to(DEV) for _ in range(6)]
    e = torch.randn(B, 160, generator=_gen(15)).to(DEV) * 3
    params = list(mlp.parameters()) + [q for lin in projs for q in lin.parameters()]
    ws = [_r(_gen(16 + i), B, width) for i in range(6)]

    def run():
        for p in params:
            p.grad = None
        temb, tps = O.time_mlp(e, mlp.linear_1, mlp.linear_2, projs)
        sum((tp * wi).sum() for tp, wi in zip(tps, ws)).backward()
        return [temb, *tps] + [p.grad for p in params]

    P.run_under_fills(run)


def test_decoder_with_nine_resnets():
    """channels=(32, 32, 32), num_mid_blocks=3: the time path's chunked rows-linear backward with its `part`
    buffer (the shape of test_decoder_more_than_eight_resnets_vs_oracle), train mode."""
    from matcha.models.components.decoder import Decoder

    dec = Decoder(16, 8, channels=(32, 32, 32), attention_head_dim=16, num_heads=2, num_mid_blocks=3).to(DEV)
    apply_recipe(dec, 5)
    dec.train()
    g = _gen(9)
    B, T = 2, 48
    x, mu = _r(g, B, 8, T), _r(g, B, 8, T)
    mask = (torch.arange(T)[None, None] < torch.tensor([48, 37])[:, None, None]).float().to(DEV)
    t = torch.rand(B, generator=g).to(DEV)
    params = list(dec.parameters())

    def run():
        for p in params:
            p.grad = None
        xd = x.clone().requires_grad_(True)
        u = dec(xd, mask, mu, t)
        u.square().sum().backward()
        return [u, xd.grad] + [p.grad for p in params if p.grad is not None]

    run()  # the first forward records the pack plan and the dropout-seed count the later ones replay
    P.run_under_fills(run)


# ------------------------------------------------------------------------------------------------ GEMM schedules
WREG = 96


def _gemm_case(B, T, cin, taps, N, cfg, splits, planes, *, prec="bf16", a16=False, full_epilogue=False, ldc=None,
               precise=None):
    from matcha.models.components import _ops as O

    g = _gen(B * T + cin + N + taps)
    x = _r(g, B, T, cin)
    x = x.bfloat16() if a16 else x
    w = _r(g, N, cin, taps, scale=(cin * taps) ** -0.5)
    msk = (torch.rand(B * T, generator=g) > 0.2).float().to(DEV)
    bias = _r(g, N)
    stride2 = full_epilogue
    To_full = 2 * T if stride2 else T
    res, cs = _r(g, B, To_full, N), torch.rand(B * To_full, generator=g).to(DEV)
    seed = torch.tensor([12345, 678], dtype=torch.int32, device=DEV)
    offs = [j - (taps - 1) // 2 for j in range(taps)]
    ldc = N if ldc is None else ldc
    p = O.PREC_BF16 if prec == "bf16" else O.PREC_FP32

    def run():
        byte = P.current().byte
        spec = O.spec_conv_fwd(w)
        if precise:
            with O.precise_forward(precise):
                Wp, Kp = O.packed(spec, p)
        else:
            kind = O.PACK_BF16_SPLIT if planes == 2 else p
            Wp, Kp = O._run_pack([spec], kind)[0], spec.Kp
        assert Kp == taps * cin  # cin % 8 == 0: no accepted GEMM shape has Kp > K (module docstring)
        y = torch.empty(B, To_full, ldc, device=DEV)
        kw = dict(a_scale=msk, bias=bias)
        yp = None
        if full_epilogue:
            yp = torch.empty(B, To_full, ldc, device=DEV)
            kw.update(act=O.ACT_GELU, residual=res, c_scale=cs, C_pre=yp, dropout_p=0.1, seed=seed)
        pos = (2, 1) if stride2 else ()
        ctx = O.precise_forward(precise) if precise else torch.autocast("cuda", enabled=False)
        before = P.current().count
        with ctx:
            O._gemm(x, T, T, B, 1, offs, cin, Wp, Kp, N, y, To_full, *pos, prec=p, tile_cfg=cfg, splits=splits, **kw)
        if splits > 1:  # the call's own allocation, not the test's: the split-K workspace was poisoned
            assert P.current().count - before >= 1, "split K asked for, but _gemm allocated no workspace"
        torch.cuda.synchronize()
        outs = [Wp]  # the packed planes are compared in full too
        for t in (y, yp):
            if t is None:
                continue
            if stride2:
                assert _holds_fill(t[:, 0::2], byte), "the other stride-2 output phase was written"
                t = t[:, 1::2]
            if ldc > N:
                assert _holds_fill(t[..., N:], byte), "columns N..ldc were written"
                t = t[..., :N]
            outs.append(t)
        return outs

    P.run_under_fills(run)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("cfg,splits", [(7, 1), (12, 1), (41, 1), (42, 3), (44, 4), (-1, 0)])
def test_gemm_schedules_full_epilogue(cfg, splits, planes):
    """bias, GELU with C_pre, dropout, residual, c_scale and a stride-2 output phase; 3 taps, ragged 0/1 a_scale;
    the split-K workspace is _gemm's own torch.empty."""
    _gemm_case(5, 77, 256, 3, 320, cfg, splits, planes, full_epilogue=True)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("cfg", [46, 47])
def test_gemm_160_row_schedules(cfg, planes):
    _gemm_case(2, 170, 96, 3, 62, cfg, 0, planes, a16=True)


@pytest.mark.parametrize("planes", [1, 2])
def test_gemm_weight_stationary(planes):
    _gemm_case(4, 77, 160, 1, 320, WREG, 0, planes)


def test_gemm_fp32_and_wider_c():
    _gemm_case(2, 37, 32, 1, 80, -1, 0, 1, prec="fp32")
    _gemm_case(2, 37, 32, 1, 80, -1, 0, 1, prec="fp32", ldc=88)
    _gemm_case(2, 37, 32, 1, 80, -1, 0, 1, ldc=88)


def test_gemm_three_planes():
    _gemm_case(5, 77, 256, 3, 320, -1, 0, 3, precise="bf16x6")


# (a bf16 A runs with one step in flight only: the entry point refuses depth 2 for it)
@pytest.mark.parametrize("sched,a16", [((-1, -1, -1), False), ((32, -1, 1), False), ((32, 512, 2), False),
                                       ((-1, -1, -1), True), ((32, -1, 1), True)])
@pytest.mark.parametrize("B,T,Cin,Cout,k,stride", [(4, 64, 512, 160, 1, 1), (6, 77, 192, 768, 5, 1), (8, 301, 256, 256, 3, 2)])
def test_wgrad(B, T, Cin, Cout, k, stride, sched, a16):
    from matcha.models.components import _ops as O

    g = _gen(B * T + Cin + k + stride)
    x = _r(g, B, T, Cin).bfloat16()
    x = x if a16 else x.float()
    lens = torch.randint(T // 3, T + 1, (B,), generator=g)
    lens[0] = T
    m = (torch.arange(T)[None] < lens[:, None]).float().to(DEV)
    pad = k // 2
    To = (T + 2 * pad - k) // stride + 1
    dy = _r(g, B, To, Cout)

    def run():
        dw = torch.empty(Cout, Cin, k, device=DEV)
        db = torch.empty(Cout, device=DEV)
        before = P.current().count
        O._wgrad(dy, To, 1, 0, x, T, To, B, stride, [j - pad for j in range(k)], Cin, Cout, dw, (Cin * k, k, 1),
                 prec=O.PREC_BF16, a_scale=m, db=db, rows_per_step=sched[0], target_blocks=sched[1], depth=sched[2])
        assert P.current().count - before >= 1, "_wgrad allocated no slab workspace of its own"
        return [dw, db]

    P.run_under_fills(run)


def test_wgrad_fp32():
    from matcha.models.components import _ops as O

    B, T, Cin, Cout, k = 4, 64, 512, 160, 1
    g = _gen(21)
    x, dy = _r(g, B, T, Cin), _r(g, B, T, Cout)
    m = _mask(B, T, 10)

    def run():
        dw = torch.empty(Cout, Cin, k, device=DEV)
        db = torch.empty(Cout, device=DEV)
        before = P.current().count
        O._wgrad(dy, T, 1, 0, x, T, T, B, 1, [0], Cin, Cout, dw, (Cin * k, k, 1), prec=O.PREC_FP32, a_scale=m, db=db)
        assert P.current().count - before >= 1, "_wgrad allocated no slab workspace of its own"
        return [dw, db]

    P.run_under_fills(run)


def test_colsum_and_reduce_partials():
    from matcha import _native as N
    from matcha._abi import ReduceJob as Job
    from matcha.models.components import _ops as O

    lib = N.lib()
    rows, n, ld = 77, 5, 8
    x = _r(_gen(22), rows, ld)

    def colsum():  # the C entry point directly: the workspace it is handed is this poisoned buffer
        ws = torch.empty(int(lib.mtts_colsum_workspace_size(rows, n)) // 4, device=DEV)
        out = torch.empty(n, device=DEV)
        N.check(lib.mtts_colsum(x.data_ptr(), rows, n, ld, out.data_ptr(), 0, ws.data_ptr(), ws.numel() * 4, O._stream(x)),
                "mtts_colsum")
        return [out]

    P.run_under_fills(colsum)

    g = _gen(5)  # the jobs of test_reduce_partials_jobs; the non-accumulating outputs come from torch.empty here
    p0, o0 = _r(g, 7, 1024), _r(g, 1024)
    p1 = _r(g, 300, 258)
    Nn, cin, taps, S = 24, 16, 3, 5
    p2 = _r(g, S, Nn * cin * taps)

    def reduce():
        outs = [o0.clone(), torch.empty(255, device=DEV), torch.empty(Nn, cin, taps, device=DEV)]
        kws = [dict(stride=1024, n=1024, splits=7, accumulate=1), dict(stride=258, n=255, splits=300, accumulate=0),
               dict(stride=Nn * cin * taps, n=Nn * cin * taps, splits=S, accumulate=0, cols=cin * taps, cin=cin,
                    sr=cin * taps, sc=taps, sj=1)]
        jobs = (Job * 3)()
        for i, (p, o, kw) in enumerate(zip((p0, p1, p2), outs, kws)):
            jobs[i] = Job(part=p.data_ptr(), out=o.data_ptr(), **kw)
        N.check(lib.mtts_reduce_partials(jobs, 3, torch.cuda.current_stream().cuda_stream), "mtts_reduce_partials")
        return outs

    P.run_under_fills(reduce)


# ------------------------------------------------------------------------------------------------ MAS
def _ragged(B, T, g):
    lens = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g)
    lens[0] = T
    return lens


@pytest.mark.parametrize("tr", ["0", "1"])
@pytest.mark.parametrize("Tx,Ty", [(5, 7), (65, 130), (129, 301), (300, 999)])
def test_maximum_path(monkeypatch, Tx, Ty, tr):
    from matcha.utils.monotonic_align import maximum_path

    monkeypatch.setenv("MTTS_MAS_TR", tr)
    B = 3
    g = _gen(Tx + Ty)
    xl, yl = _ragged(B, Tx, g), _ragged(B, Ty, g)
    yl = torch.maximum(yl, xl)
    mask = ((torch.arange(Tx)[None, :, None] < xl[:, None, None]) & (torch.arange(Ty)[None, None, :] < yl[:, None, None]))
    value, mask = _r(g, B, Tx, Ty), mask.float().to(DEV)
    P.run_under_fills(lambda: list(maximum_path(value, mask, return_row_start=True)))


@pytest.mark.parametrize("B,C,Tx,Ty", [(4, 80, 13, 37), (3, 80, 300, 301)])
def test_prior_maximum_path_and_consumers(B, C, Tx, Ty):
    from matcha.utils.monotonic_align import expand_rows, prior_maximum_path, segment_crop

    g = _gen(B + Tx + Ty)
    xl, yl = _ragged(B, Tx, g), _ragged(B, Ty, g)
    yl = torch.maximum(yl, xl).to(DEV)
    xl = xl.to(DEV)
    mu, y = _r(g, B, C, Tx), _r(g, B, C, Ty)
    P.run_under_fills(lambda: list(prior_maximum_path(mu, y, xl, yl)))
    P.run_under_fills(lambda: list(prior_maximum_path(mu, y, xl, yl, return_lattice=True)))
    P.run_under_fills(lambda: list(prior_maximum_path(mu, y, xl, yl, dense=False)))
    _, _, col_row, rs, lens = prior_maximum_path(mu, y, xl, yl)
    _fwd_bwd(lambda a: expand_rows(a, col_row, rs, lens), [mu])
    S = 16
    offs = torch.randint(0, Ty, (B,), generator=g).to(DEV)
    _fwd_bwd(lambda a: segment_crop(y, a, col_row, rs, lens, S, offsets=offs), [mu])
    words = torch.randint(0, 2 ** 31 - 1, (B,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
    _fwd_bwd(lambda a: segment_crop(y, a, col_row, rs, lens, S, words=words, want_attn=False), [mu])


def test_duration_path_and_consumers():
    from matcha.utils.monotonic_align import duration_path, expand_rows, segment_crop

    B, Tx, Ty, C = 3, 9, 40, 8
    g = _gen(31)
    d = (torch.rand(B, Tx, generator=g) * 6).to(DEV)
    d[1, 2] = float("nan")  # counts as 0 by the rule
    xl, yl = torch.tensor([9, 6, 1], device=DEV), torch.tensor([40, 23, 5], device=DEV)
    P.run_under_fills(lambda: list(duration_path(d, xl, yl, Ty)))
    P.run_under_fills(lambda: list(duration_path(d, xl, yl, Ty, dense=False)))
    _, _, col_row, rs, lens, run_lens = duration_path(d, xl, yl, Ty)
    mu, y = _r(g, B, C, Tx), _r(g, B, C, Ty)
    _fwd_bwd(lambda a: expand_rows(a, col_row, rs, run_lens), [mu])
    offs = torch.tensor([3, 0, 2], device=DEV)
    _fwd_bwd(lambda a: segment_crop(y, a, col_row, rs, lens, 16, offsets=offs, run_lengths=run_lens), [mu])


# ------------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("grad_scale", [10.0, 1e-3])  # clipping active / inactive
def test_flat_clip_adamw(grad_scale):
    from matcha.training import _FlatClipAdamW

    g = _gen(5)
    shapes = [(256, 160, 3), (256,), (1000,), (7, 5), (1,), (80, 256, 1), (3,)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[(torch.randn(s, generator=g) * grad_scale / math.sqrt(len(shapes))).to(DEV) for s in shapes] for _ in range(3)]

    def run():
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        opt = _FlatClipAdamW(ps, torch.tensor(1e-4, device=DEV, dtype=torch.float64), 1.0)
        for step in range(3):
            for p, gr in zip(ps, grads[step]):
                p.grad = gr.clone()
            opt.step()
        return [opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_t]

    P.run_under_fills(run)


# ------------------------------------------------------------------------------------------------ model
def _model(seed):
    from matcha.models.matcha_tts import MatchaTTS

    model = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(DEV)
    apply_recipe(model, seed)
    return model


@pytest.mark.parametrize("precision", ["32-true", "bf16-mixed", "bf16-parity"])
def test_model_forward_backward(precision):
    from matcha.precision import loss_and_grads
    from matcha.training import synthetic_batch

    model = _model(7)
    model.train()
    b = synthetic_batch(4, 24, 96, device=DEV)
    g = _gen(3)
    t, z = torch.rand(4, 1, 1, generator=g).to(DEV), _r(g, 4, 80, 96)

    def run():
        losses, grads, attn = loss_and_grads(model, b, precision, t=t, z=z)
        assert len(grads) == len(list(model.parameters()))
        return [torch.tensor(losses, dtype=torch.float64), attn] + [grads[n] for n in sorted(grads)]

    torch.cuda.manual_seed(1234)
    run()  # the first forward records the pack plan and the dropout-seed count the later ones replay
    P.run_under_fills(run)


def _trainer_case(precision, graph, accumulate=1):
    from matcha.training import TrainConfig, Trainer, synthetic_batch

    batches = [synthetic_batch(4, 24, 96, seed=s, device=DEV) for s in range(accumulate)]

    def run():
        # a fresh model and Trainer per fill, built inside the poisoned context: warm-up, capture and replays all
        # run on poisoned buffers, and the fills become graph nodes
        torch.manual_seed(0)
        model = _model(11)
        model.train()
        tr = Trainer(model, TrainConfig(precision=precision, graph=graph, accumulate_grad_batches=accumulate))
        losses = [tr.step(batches).clone() for _ in range(2)]
        torch.cuda.synchronize()
        return losses + [p.detach() for p in model.parameters()]

    P.run_under_fills(run)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("precision", ["32-true", "bf16-parity"])
def test_trainer_two_steps(precision, graph):
    _trainer_case(precision, graph)


def test_trainer_accumulates_two_micro_batches():
    _trainer_case("bf16-parity", True, accumulate=2)


# ------------------------------------------------------------------------------------------------ inference
def test_synthesise():
    model = _model(17)
    model.eval()
    g = _gen(3)
    B, Tx = 2, 11
    xl = torch.tensor([11, 8])
    x = (torch.randint(1, 150, (B, Tx), generator=g) * (torch.arange(Tx)[None] < xl[:, None])).to(DEV)
    xl = xl.to(DEV)
    from matcha.utils.model import fix_len_compatibility

    T = fix_len_compatibility(int(model.synthesise(x, xl, 3)["mel_lengths"].max()))  # the padded length the solver runs at
    z = _r(g, B, 80, T)
    P.run_under_fills(lambda: _flat(model.synthesise(x, xl, 3, z=z)))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B,T", [(3, 50), (1, 3)])
def test_hifigan_generator(B, T, graph):
    from hifi_gan import AttrDict, Generator
    from hifigan_ref import CONFIGS

    mel = (_r(_gen(B * T), B, 80, T) * 1.5 - 5.5)

    def run():
        m = Generator(AttrDict(CONFIGS["v3_small"]))  # a fresh module per fill: packing and capture are poisoned too
        apply_recipe(m, 3)
        m = m.to(DEV).eval()
        m.graph = graph
        with torch.no_grad():
            return [m(mel), m(mel)]  # graph: capture + replay, then a replay

    P.run_under_fills(run)


@pytest.mark.parametrize("B,F", [(3, 9), (1, 4)])
def test_griffin_lim(B, F):
    import griffinlim_ref as R
    from matcha.utils.audio_process import GriffinLim, GriffinLimVocoder, InverseMelScale

    c = R.case(B, F)
    log_mel, lin, ang = c["log_mel"].to(DEV), c["lin"].to(DEV), c["angles_rand"].to(DEV)
    inv = InverseMelScale(513, 80, 22050, 0.0, 8000.0)
    P.run_under_fills(lambda: [inv(log_mel, log_input=True), inv(torch.exp(log_mel), log_input=False)])

    def run():  # GriffinLim's own buffers are graph-static torch.zeros: the poisoned ones here are InverseMelScale's
        gl = GriffinLim(n_fft=1024, n_iter=4, hop_length=256, win_length=1024, power=1.0)
        return [gl(inv(log_mel, log_input=True), angles=ang), gl(lin, angles=ang)] + \
            _flat(GriffinLimVocoder(n_iter=4)(log_mel, angles=ang))

    P.run_under_fills(run)


def test_mel_front_end():
    from matcha.utils.audio_process import MelSpectrogram

    m = MelSpectrogram(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000)
    y = (0.3 * torch.randn(4, 30000, generator=_gen(11))).clamp(-1, 1).to(DEV)
    P.run_under_fills(lambda: [m(y), m(torch.zeros(1, 8192, device=DEV))])
