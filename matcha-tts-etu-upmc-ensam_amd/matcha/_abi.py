"""The Python mirror of libmtts_hip.so's C ABI (include/*.h): every constant, argument struct and entry-point
signature, by hand, grouped by header and in header order.  Nothing else lives here and nothing else declares
any of it: _native.lib() binds SIGNATURES, the op modules alias the structs and constants they use.

tests/test_abi_mirror_cpu.py holds this file to the headers (prototypes parsed from them; struct layouts and macro
values printed by the host C compiler), so a header change and its change here land together.

Pointer parameters are c_void_p (callers pass device addresses, byref() or None) except the few typed POINTER(...)
below, which take a ctypes struct or array by reference.
"""
import ctypes

_P, _F, _D, _SZ, _ptr = ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.POINTER
_INT, _I32, _I64 = ctypes.c_int, ctypes.c_int32, ctypes.c_int64

# ================================================================================== include/mtts.h: constants
MTTS_ABI_VERSION = 1
# enum mtts_status: bad argument or flag / unsupported shape / workspace too small / HIP call failed / not built in
MTTS_OK = 0
MTTS_ERR_INVALID_ARG, MTTS_ERR_SHAPE, MTTS_ERR_WORKSPACE, MTTS_ERR_HIP, MTTS_ERR_UNSUPPORTED = -1, -2, -3, -4, -5

# flags of mtts_maximum_path_f32
MTTS_MAS_VALUE_PREMASKED = 0x1  # value already holds value*mask: skip the multiply
MTTS_MAS_NO_DENSE_PATH = 0x2  # only row_start_out / lengths_out: do not write `path`
MTTS_MAS_MAX_TX = 8192  # longest text of maximum_path / prior_maximum_path / duration_path
MTTS_MAS_MAX_TX_ROW_MAJOR = 4096  # longest text of compute_batch_alignments

# ========================================================================== include/mtts_decoder.h: constants
MTTS_PREC_FP32, MTTS_PREC_BF16 = 0, 1  # exact-fp32 MFMA / bf16 operands with fp32 accumulation
# DGELU / DRELU: the backward through a GELU / ReLU (multiply by GELU'(aux) / zero where aux <= 0)
MTTS_ACT_NONE, MTTS_ACT_GELU, MTTS_ACT_DGELU, MTTS_ACT_RELU, MTTS_ACT_DRELU = 0, 1, 2, 3, 4
MTTS_CONV_MAX_TAPS = 8
MTTS_GEMM_GLDS = 32  # first LDS-DMA schedule id
MTTS_GEMM_WREG = 96  # the bf16 weight-stationary schedule's id

# mtts_conv_gemm_args.flags (A_BF16 and BINARY_SCALE also mtts_conv_wgrad_args.flags)
MTTS_GEMM_F_BINARY_SCALE = 0x1  # a_scale holds only 0 / 1 (a sequence mask)
MTTS_GEMM_F_A_BF16 = 0x2  # A operand stored bf16 (bf16-mixed activations)
MTTS_GEMM_F_C_BF16 = 0x4  # output stored bf16
MTTS_GEMM_F_FAST_ACT = 0x8  # 5e-7-accurate erf in GELU epilogues (bf16-mixed only)
MTTS_GEMM_F_PRE_BF16 = 0x10  # C_pre written / aux read as bf16
MTTS_GEMM_F_W_SPLIT = 0x40  # W holds a hi and a lo bf16 plane (two MFMAs per product)
MTTS_GEMM_F_A_SPLIT = 0x80  # with W_SPLIT, fp32 A split into hi + lo planes (bf16x3)
MTTS_GEMM_F_SPLIT3 = 0x100  # three weight planes, fp32 A split in the kernel (bf16x6)
MTTS_WGRAD_F_DY_BF16 = 0x20  # mtts_conv_wgrad_args.flags: the weight gradient's dY holds bf16

# or'ed into a norm's `act` / `flags`
MTTS_NORM_F_Y_BF16 = 0x100  # y is written as bf16
MTTS_NORM_F_X_BF16 = 0x200  # GroupNorm: the input h holds bf16
MTTS_NORM_F_DY_BF16 = 0x400  # GroupNorm backward: dy holds bf16
MTTS_PACK_THREE_PLANES = 1 << 62  # or'ed into mtts_pack_job.lo_off: hi / mid / lo planes
MTTS_ATTN_F_IO_BF16 = 0x1  # mtts_attn_args.flags: q/k/v/o and their gradients hold bf16
MTTS_ROWS_MAX_MATS = 8  # matrices per rows-linear launch
MTTS_ROWS_ACT_NONE, MTTS_ROWS_ACT_SILU, MTTS_ROWS_ACT_MISH = 0, 1, 2

# ========================================================================== include/mtts_vocoder.h: constants
MTTS_VOC_MAX_TAPS = 11
# mtts_voc_conv_args.acc_mode, the stage's running sum: untouched / acc = v / acc += v / acc = (acc + v) / acc_div
MTTS_VOC_ACC_NONE, MTTS_VOC_ACC_INIT, MTTS_VOC_ACC_ADD, MTTS_VOC_ACC_MEAN = 0, 1, 2, 3

# ======================================================================= include/mtts_griffinlim.h: constants
MTTS_GL_NFFT, MTTS_GL_HOP = 1024, 256  # the one STFT geometry the kernels serve


# ============================================================================ include/mtts_decoder.h: structs
class ConvGemmArgs(ctypes.Structure):
    _c_name_ = "mtts_conv_gemm_args"
    _fields_ = [("A", _P), ("a_scale", _P), ("lda", _I32), ("Ti", _I32), ("To", _I32), ("nb", _I32),
                ("in_stride", _I32), ("ntaps", _I32), ("off", _I32 * MTTS_CONV_MAX_TAPS), ("cin", _I32), ("W", _P),
                ("N", _I32), ("K", _I32), ("Kp", _I32), ("bias", _P), ("act", _I32), ("residual", _P), ("ldr", _I32),
                ("c_scale", _P), ("C", _P), ("ldc", _I32), ("To_full", _I32), ("out_stride", _I32),
                ("out_off", _I32), ("C_pre", _P), ("aux", _P), ("ldaux", _I32), ("dropout_p", _F), ("seed", _P),
                ("flags", _I32)]


class ConvWgradArgs(ctypes.Structure):
    _c_name_ = "mtts_conv_wgrad_args"
    _fields_ = [("dY", _P), ("ldy", _I32), ("To_full", _I32), ("out_stride", _I32), ("out_off", _I32), ("A", _P),
                ("a_scale", _P), ("lda", _I32), ("Ti", _I32), ("To", _I32), ("nb", _I32), ("in_stride", _I32),
                ("ntaps", _I32), ("off", _I32 * MTTS_CONV_MAX_TAPS), ("cin", _I32), ("N", _I32), ("K", _I32),
                ("flags", _I32)]


class PackJob(ctypes.Structure):
    _c_name_ = "mtts_pack_job"
    _fields_ = [("src", _P), ("dst", _P), ("rows", _I32), ("C", _I32), ("ntaps", _I32), ("Kp", _I32), ("ld", _I32),
                ("sr", _I64), ("sc", _I64), ("sj", _I64), ("j0", _I32), ("js", _I32), ("lo_off", _I64)]


class AttnArgs(ctypes.Structure):
    _c_name_ = "mtts_attn_args"
    _fields_ = [("q", _P), ("k", _P), ("v", _P), ("ldq", _I32), ("key_bias", _P), ("o", _P), ("ldo", _I32),
                ("lse", _P), ("B", _I32), ("T", _I32), ("H", _I32), ("D", _I32), ("scale", _F), ("dropout_p", _F),
                ("seed", _P), ("flags", _I32)]


class AttnGrads(ctypes.Structure):
    _c_name_ = "mtts_attn_grads"
    _fields_ = [("dout", _P), ("lddo", _I32), ("dq", _P), ("dk", _P), ("dv", _P), ("ldd", _I32)]


class AdamWChunk(ctypes.Structure):
    _c_name_ = "mtts_adamw_chunk"
    _fields_ = [("grad", _P), ("offset", _I64), ("n", _I32), ("pad_", _I32)]


class ReduceJob(ctypes.Structure):
    _c_name_ = "mtts_reduce_job"
    _fields_ = [("part", _P), ("out", _P), ("stride", _I64), ("n", _I64), ("splits", _I32), ("accumulate", _I32),
                ("cols", _I32), ("cin", _I32), ("sr", _I64), ("sc", _I64), ("sj", _I64)]


# ============================================================================ include/mtts_vocoder.h: structs
class VocConvArgs(ctypes.Structure):
    _c_name_ = "mtts_voc_conv_args"
    _fields_ = [("A", _P), ("W", _P), ("bias", _P), ("residual", _P), ("C", _P), ("acc", _P), ("B", _I32),
                ("L", _I32), ("cin", _I32), ("N", _I32), ("k", _I32), ("d", _I32), ("leaky", _I32), ("slope", _F),
                ("acc_mode", _I32), ("acc_div", _F)]


_GEMM, _WGRAD = _ptr(ConvGemmArgs), _ptr(ConvWgradArgs)

# name -> (restype, argtypes), in the order of the header declarations
SIGNATURES: dict[str, tuple] = {
    # ------------------------------------------------------------------------------------------ include/mtts.h
    "mtts_abi_version": (_INT, []),
    "mtts_last_error": (ctypes.c_char_p, []),
    "mtts_maximum_path_workspace_size": (_SZ, [_I32, _I32, _I32]),
    "mtts_maximum_path_f32": (_INT, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _SZ, _P]),
    "mtts_compute_batch_alignments": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _F, _P, _SZ, _P]),
    "mtts_prior_maximum_path_workspace_size": (_SZ, [_I32, _I32, _I32]),
    "mtts_prior_maximum_path": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "mtts_duration_path": (_INT, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "mtts_expand_rows_fwd": (_INT, [_P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "mtts_expand_rows_bwd": (_INT, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "mtts_segment_crop_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "mtts_segment_crop_bwd": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "mtts_mel_log_fwd": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _P, _P]),
    "mtts_mel_from_wav": (_INT, [_P, _I32, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _F, _F, _F,
                                 _P, _P, _P]),
    "mtts_mel_stats": (_INT, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "mtts_losses_workspace_size": (_SZ, [_I32, _I32]),
    "mtts_losses_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _F, _P, _P, _SZ, _P]),
    "mtts_losses_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _F, _P, _P, _P]),
    "mtts_sequence_mask_f32": (_INT, [_P, _I32, _I32, _P, _P, _P]),
    "mtts_duration_loss_fwd": (_INT, [_P, _P, _P, _I32, _I32, _P, _P]),
    "mtts_duration_loss_bwd": (_INT, [_P, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "mtts_loss_sum": (_INT, [_P, _P, _P, _P, _P, _P]),
    # ---------------------------------------------------------------------------------- include/mtts_decoder.h
    "mtts_conv_gemm": (_INT, [_GEMM, _I32, _P]),
    "mtts_conv_gemm_tile": (_INT, [_GEMM, _I32, _I32, _P]),
    "mtts_conv_gemm_workspace_size": (_SZ, [_GEMM, _I32, _I32, _I32]),
    "mtts_conv_gemm_ws": (_INT, [_GEMM, _I32, _I32, _I32, _P, _SZ, _P]),
    # (args, precision, tile_cfg, splits, out[6]) -> schedule id, splits, workgroups, resident per CU, rounds, fill
    "mtts_conv_gemm_plan": (_INT, [_P, _I32, _I32, _I32, _ptr(_I32 * 6)]),
    "mtts_conv_gemm_glds_occupancy": (_INT, [_I32, _I32, _I32, _ptr(_I32 * 2)]),
    "mtts_conv_wgrad_workspace_size": (_SZ, [_WGRAD]),
    "mtts_conv_wgrad": (_INT, [_WGRAD, _I32, _P, _I64, _I64, _I64, _P, _I32, _P, _SZ, _P]),
    "mtts_conv_wgrad_tile": (_INT, [_WGRAD, _I32, _I32, _I32, _I32, _P, _I64, _I64, _I64, _P, _I32, _P, _SZ, _P]),
    "mtts_wgrad_plan_mode": (None, [_I32]),
    "mtts_wgrad_flush_cap": (None, [_I32]),
    "mtts_gn_mish_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _P]),
    "mtts_gn_mish_bwd_workspace_size": (_SZ, [_I32, _I32]),
    "mtts_gn_mish_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _SZ, _P]),
    "mtts_gn_mish_fwd_ex": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _I32, _P]),
    "mtts_gn_mish_bwd_ex": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _SZ,
                                   _P]),
    "mtts_dropout_apply": (_INT, [_P, _P, _I32, _I32, _I32, _F, _P, _P]),
    "mtts_act_dropout_bwd": (_INT, [_P, _P, _P, _I32, _I32, _I32, _I32, _F, _P, _P]),
    "mtts_act_dropout_bwd_scaled": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _P, _P]),
    "mtts_layernorm_fwd": (_INT, [_P, _P, _P, _P, _P, _P, _I32, _I32, _F, _I32, _F, _P, _P]),
    "mtts_layernorm_bwd_workspace_size": (_SZ, [_I32, _I32]),
    "mtts_layernorm_bwd": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _F, _P, _P, _SZ, _P]),
    "mtts_layernorm_bwd_res": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _P, _SZ, _P]),
    "mtts_pack_weights": (_INT, [_ptr(PackJob), _I32, _I32, _P]),
    "mtts_attention_fwd": (_INT, [_ptr(AttnArgs), _I32, _P]),
    "mtts_attention_bwd_workspace_size": (_SZ, [_I32, _I32, _I32]),
    "mtts_attention_bwd": (_INT, [_ptr(AttnArgs), _ptr(AttnGrads), _I32, _P, _SZ, _P]),
    "mtts_rope_qk": (_INT, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _I32, _P]),
    "mtts_clip_adamw_workspace_size": (_SZ, [_I32]),
    "mtts_clip_adamw": (_INT, [_P, _I32, _P, _P, _P, _P, _P, _F, _D, _D, _D, _D, _P, _SZ, _P]),
    "mtts_clip_adamw_scaled": (_INT, [_P, _I32, _P, _P, _P, _P, _P, _F, _D, _D, _D, _D, _F, _P, _SZ, _P]),
    "mtts_reduce_partials": (_INT, [_P, _I32, _P]),  # (mtts_reduce_job *, njobs, stream)
    "mtts_colsum_workspace_size": (_SZ, [_I64, _I32]),
    "mtts_colsum": (_INT, [_P, _I64, _I32, _I32, _P, _I32, _P, _SZ, _P]),
    "mtts_defer_reductions": (None, [_I32]),
    "mtts_pending_reductions": (_I32, []),
    "mtts_flush_reductions": (_INT, [_P]),
    "mtts_discard_reductions": (None, []),
    "mtts_cfm_pack_fwd": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _F, _P, _P]),
    "mtts_cfm_pack_bwd": (_INT, [_P, _I32, _I32, _I32, _P, _P]),
    "mtts_time_embedding": (_INT, [_P, _I32, _I32, _F, _P, _P]),
    "mtts_embedding_fwd": (_INT, [_P, _P, _I64, _I32, _I32, _F, _P, _P]),
    "mtts_embedding_bwd": (_INT, [_P, _P, _I64, _I32, _I32, _F, _P, _P]),
    "mtts_rows_linear_workspace_size": (_SZ, [_I32, _I32, _I32, _P]),
    "mtts_rows_linear_fwd": (_INT, [_P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _I32, _P, _SZ, _P]),
    "mtts_rows_linear_bwd": (_INT, [_P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    # --------------------------------------------------------------------------------------- include/mtts_dp.h
    "mtts_dp_unique_id": (_INT, [_P, _SZ]),
    "mtts_dp_comm_init": (_INT, [_P, _SZ, _I32, _I32, _ptr(_P)]),
    "mtts_dp_allreduce_f32": (_INT, [_P, _P, _I64, _I32, _P]),
    "mtts_dp_comm_query": (_INT, [_P, _ptr(_I32), _ptr(_I32)]),
    "mtts_dp_comm_destroy": (_INT, [_P]),
    "mtts_dp_rccl_version": (_INT, []),
    "mtts_dp_progress_create": (_INT, [_I32, _ptr(_P), _ptr(_ptr(_I32))]),
    "mtts_dp_progress_mark": (_INT, [_P, _I32, _I32, _P]),
    "mtts_dp_progress_destroy": (_INT, [_P]),
    # ---------------------------------------------------------------------------------- include/mtts_vocoder.h
    "mtts_voc_conv": (_INT, [_P, _P]),  # (mtts_voc_conv_args *, stream)
    "mtts_voc_upsample": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _P]),
    "mtts_voc_pre_workspace_size": (_SZ, [_I32, _I32, _I32]),
    "mtts_voc_pre": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _SZ, _P]),
    "mtts_voc_post": (_INT, [_P, _P, _P, _P, _I32, _I32, _I32, _F, _P]),
    # ------------------------------------------------------------------------------ include/mtts_griffinlim.h
    "mtts_gl_inverse_mel": (_INT, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P]),
    "mtts_gl_synthesis": (_INT, [_P, _P, _P, _F, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mtts_gl_analysis": (_INT, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
}
