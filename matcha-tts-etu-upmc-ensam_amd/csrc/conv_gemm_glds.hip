// bf16 implicit GEMM with LDS-DMA staging (global_load_lds_dwordx4) of both operands -- the default
// bf16 schedule of mtts_conv_gemm for the decoder / encoder convs and linears.
//
// Same contract as conv_gemm_kernel (include/mtts_decoder.h), for precision MTTS_PREC_BF16 with
// a_scale either NULL or a 0/1 row mask (MTTS_GEMM_F_BINARY_SCALE).  Why a second kernel: the
// register-staged kernel spends ~45 VALU instructions per MFMA on staging (fp32 loads, row-mask
// multiply, bf16 conversion, validity selects, LDS stores; SQ_INSTS_VALU / SQ_INSTS_MFMA on the step's
// 19200 x 256 x 768 conv) and is issue-bound at ~9 % of MFMA peak.  Here the operands go
// HBM/L2 -> LDS with no VGPR round trip:
//   A (fp32 activations): each lane DMAs one 16-byte chunk (4 channels) of one tap row; a row that
//     lies outside [0, Ti) or whose mask is 0 is read from a 16-byte zero constant instead, so the
//     masked / zero-padded operand is formed by address selection alone.  The fp32 -> bf16 conversion
//     moves to the fragment read (4 v_cvt_pk_bf16_f32 per 8 elements).
//   W (packed bf16 [N][Kp]): DMA'd as is.
// LDS images are XOR-swizzled through the per-lane SOURCE address (an LDS-DMA wave instruction fills
// 1 KiB lane-linearly): A rows are 256 B (64 fp32 of one K step), 16-byte chunk c of row r sits at
// c ^ (r & 15); W rows are 128 B, chunk c of row n at c ^ ((n >> 1) & 7).  Both make the MFMA
// fragment reads (ds_read_b128, 16-lane groups) bank-conflict free.
// Pipeline: STAGES LDS buffers, K step 64, loads for step kt + STAGES - 1 issued right after the
// barrier that retires step kt - 1's reads; a counted s_waitcnt vmcnt (never 0 inside the loop) and a
// raw s_barrier (no fence: __syncthreads() would drain the in-flight DMAs) order each buffer.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "gemm_epilogue.h"
#include "lds_dma.h"
#include "mtts_common.h"
#include "mtts_decoder.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
using mtts::f32x16;

__device__ uint4 g_zero16 = {0u, 0u, 0u, 0u};  // never written: source of every masked / out-of-range chunk

// -DMTTS_GEMM_TIMELINE=1 (diagnostic builds only, tools/r6/glds_timeline.py): lane 0 of every wave stamps the
// 100 MHz wall clock into g_tlg ([wave][kTlSlots]: HW ids, start, prologue issued, then per K step: data landed +
// barrier passed / MFMAs issued, loop end, epilogue end); read back by mtts_glds_timeline_read.
#ifndef MTTS_GEMM_TIMELINE
#define MTTS_GEMM_TIMELINE 0
#endif
#if MTTS_GEMM_TIMELINE
constexpr int kTlSlots = 128, kTlWaves = 16384, kTlSteps = 60;
__device__ long long g_tlg[kTlWaves * kTlSlots];
#define MTTS_TLG(slot)                                                                                   \
    do {                                                                                                 \
        const int tl_w = (int)blockIdx.x * NW + wave;                                                    \
        if (lane == 0 && tl_w < kTlWaves && (slot) < kTlSlots) g_tlg[tl_w * kTlSlots + (slot)] = wall_clock64(); \
    } while (0)
#else
#define MTTS_TLG(slot) \
    do {               \
    } while (0)
#endif

constexpr int kBK = 64;

__device__ __forceinline__ uint32_t pack2(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2));
}

using mtts::bload16;
using mtts::glds16;
using mtts::make_rsrc;
using mtts::u32x4;
using mtts::wait_vmcnt;
constexpr uint32_t MTTS_GLDS_OOB = mtts::kDmaOob;

template <int WM, int WN, int TM, int TN, int STAGES, bool ABF16 = false, int NPL = 1>
struct GldsGeom {
    static constexpr int NT = 64 * WM * WN, NW = WM * WN;
    static constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN;
    static constexpr int A_BYTES = BM * kBK * (ABF16 ? 2 : 4);  // fp32 rows of 256 B / bf16 rows of 128 B
    static constexpr int W_BYTES = NPL * BN * kBK * 2;  // bf16 rows of 128 B (NPL weight planes: BN rows each)
    // An image is NIA / NIW wave instructions of 1 KiB.  Wave w issues instructions w, w + NW, ...: GA / GW
    // per K step, the last one only by the waves below RA / RW when the image does not divide over the waves
    // (160-row tiles: five or ten waves on a 16 KiB W image) -- a ragged split, RA / RW != 0
    static constexpr int NIA = A_BYTES / 1024, NIW = W_BYTES / 1024;
    static constexpr int GA = (NIA + NW - 1) / NW, GW = (NIW + NW - 1) / NW;
    static constexpr int RA = NIA % NW, RW = NIW % NW;
    static constexpr bool RAGGED = RA != 0 || RW != 0;
    static_assert(A_BYTES % 1024 == 0 && W_BYTES % 1024 == 0, "whole DMA instructions");
    static_assert(STAGES >= 2 && STAGES <= 4, "two to four stage buffers");
    // Epilogue staging: one 4 KiB image per wave, carved from the first two stages' buffers.  Up to 8 waves keep
    // the (wave % 4 -> buffer, wave / 4 -> slot) layout; more waves take consecutive slots of sA0, sW0, sA1, sW1
    static constexpr int SA = A_BYTES / 4096, SW = W_BYTES / 4096;
    static_assert(NW <= 8 ? (SA >= (NW + 3) / 4 && SW >= (NW + 2) / 4) : 2 * (SA + SW) >= NW,
                  "the epilogue's per-wave staging images fit the stage buffers");
};

// ABF16: A is bf16 in HBM (MTTS_GEMM_F_A_BF16): 128-byte rows, the same image and swizzle as W, and
// the fragment read needs no conversion.
// LEAN (cin % 64 == 0, so every K step lies inside one tap and K % 64 == 0; 32-bit byte offsets): the
// operands are read through buffer descriptors, the K step advance is a scalar offset and only a tap
// change touches per-lane state -- the register-addressed loop spent ~12 vector instructions per DMA
// on pointer and tap bookkeeping (~26 VALU per MFMA on the 19200 x 256 x 768 conv, SQ counters).
// WS (MTTS_GEMM_F_W_SPLIT): the W image holds BN hi rows then BN lo rows (the lo plane starts N*Kp
// elements after W); each fragment pair issues A*hi and A*lo.
// X3 (MTTS_GEMM_F_SPLIT3, fp32 A, round 4): bf16x6 -- W holds three planes hi / mid / lo (hi + mid + lo = w
// exactly, packed by mtts_pack_weights), the fp32 A fragment is split the same way at the fragment read, and
// every product is the six terms of combined order <= 2^-16 (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid),
// smallest first, into the fp32 accumulator: ~2^-24 relative per product, fp32-faithful (the parity policy's
// text encoder forward at bf16 MFMA rates)
template <int WM, int WN, int TM, int TN, int STAGES, bool ABF16, bool LEAN, bool WS = false, bool X3 = false>
__global__ __launch_bounds__(64 * WM * WN) void conv_gemm_glds_kernel(mtts_conv_gemm_args p, int ksteps, float *part) {
    static_assert(!X3 || (!ABF16 && !WS), "bf16x6: fp32 A, three weight planes");
    constexpr int NPL = X3 ? 3 : (WS ? 2 : 1);
    using G = GldsGeom<WM, WN, TM, TN, STAGES, ABF16, NPL>;
    constexpr int ES = ABF16 ? 2 : 4;        // bytes per A element
    constexpr int RPI = ABF16 ? 8 : 4;       // A rows per 1 KiB DMA instruction
    constexpr int CPR = ABF16 ? 8 : 16;      // 16-byte chunks per A row of one K step
    constexpr int EPC = 16 / ES;             // A elements per chunk
    constexpr int NT = G::NT, BM = G::BM, BN = G::BN, GA = G::GA, GW = G::GW, NW = G::NW;
    // one __shared__ object per stage and operand, and a K loop unrolled by STAGES so every access
    // names its buffer statically: hipcc then sees that a DMA into one buffer cannot alias the
    // ds_reads of another and does not insert vmcnt(0) before them (one shared array with a runtime
    // stage offset gets a full drain of the in-flight DMAs before every fragment read)
    __shared__ __attribute__((aligned(1024))) unsigned char sA0[G::A_BYTES], sW0[G::W_BYTES];
    __shared__ __attribute__((aligned(1024))) unsigned char sA1[G::A_BYTES], sW1[G::W_BYTES];
    __shared__ __attribute__((aligned(1024))) unsigned char sA2[STAGES > 2 ? G::A_BYTES : 16],
        sW2[STAGES > 2 ? G::W_BYTES : 16];
    __shared__ __attribute__((aligned(1024))) unsigned char sA3[STAGES > 3 ? G::A_BYTES : 16],
        sW3[STAGES > 3 ? G::W_BYTES : 16];
    auto abuf = [&](auto S) -> unsigned char * {
        if constexpr (decltype(S)::value == 0) return sA0;
        else if constexpr (decltype(S)::value == 1) return sA1;
        else if constexpr (decltype(S)::value == 2) return sA2;
        else return sA3;
    };
    auto wbuf = [&](auto S) -> unsigned char * {
        if constexpr (decltype(S)::value == 0) return sW0;
        else if constexpr (decltype(S)::value == 1) return sW1;
        else if constexpr (decltype(S)::value == 2) return sW2;
        else return sW3;
    };
    // LDS byte addresses of the stage buffers, cast from the __shared__ objects themselves (a constant:
    // no generic-pointer null check)
    typedef __attribute__((address_space(3))) unsigned char lds_u8;
    auto lds_addr = [](const lds_u8 *q) { return (uint32_t)(uintptr_t)q; };
    auto abuf_l = [&](auto S) -> uint32_t {
        if constexpr (decltype(S)::value == 0) return lds_addr((const lds_u8 *)sA0);
        else if constexpr (decltype(S)::value == 1) return lds_addr((const lds_u8 *)sA1);
        else if constexpr (decltype(S)::value == 2) return lds_addr((const lds_u8 *)sA2);
        else return lds_addr((const lds_u8 *)sA3);
    };
    auto wbuf_l = [&](auto S) -> uint32_t {
        if constexpr (decltype(S)::value == 0) return lds_addr((const lds_u8 *)sW0);
        else if constexpr (decltype(S)::value == 1) return lds_addr((const lds_u8 *)sW1);
        else if constexpr (decltype(S)::value == 2) return lds_addr((const lds_u8 *)sW2);
        else return lds_addr((const lds_u8 *)sW3);
    };

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WN, wc = wave % WN;
    const int lr = lane & 31, lh = lane >> 5;
    const int M = p.nb * p.To;
    // ragged split: whether this wave issues the last A / W instruction of a K step (wave-uniform)
    const bool a_last = G::RA == 0 || wave < G::RA, w_last = G::RW == 0 || wave < G::RW;
    // split-K (part != NULL): grid = tiles x S, the S splits of a tile adjacent (same XCD); split s
    // reduces K steps [s*ksteps, min(nk, (s+1)*ksteps)) and stores raw fp32 partials to part[s][M][N]
    int m0, n0, kstep0 = 0, nk = (p.K + kBK - 1) / kBK;
    {
        const int nt = (p.N + BN - 1) / BN;
        const int ntiles = ((M + BM - 1) / BM) * nt;
        const int S = gridDim.x / ntiles;
        int t = mtts::xcd_relabel(blockIdx.x, gridDim.x);
        if (S > 1) {
            const int tile = t / S, split = t - tile * S;
            t = tile;
            kstep0 = split * ksteps;
            nk = min(ksteps, nk - kstep0);
        }
        const int mt = t / nt;
        m0 = mt * BM;
        n0 = (t - mt * nt) * BN;
    }
    const float inv_to = 1.0f / (float)p.To;
    const int off0 = p.off[0], offstep = p.ntaps > 1 ? p.off[1] - p.off[0] : 0;

    // ---- A chunk state: DMA instruction i of this wave covers tile rows 4q..4q+3 (q = i*NW + wave);
    // lane -> row 4q + lane/16, LDS slot lane%16 <- logical chunk (lane%16) ^ (row & 15)
    const float *zero = reinterpret_cast<const float *>(&g_zero16);
    const long long tap_delta = ((long long)offstep * p.lda - p.cin) * ES;  // source bytes when a chunk changes tap
    const char *a_src[GA];   // the lane's chunk in the current step (valid when its tap's bit is set)
    int a_ch[GA], a_j[GA];   // channel of the lane's chunk within its tap, and the tap
    uint32_t a_ok[GA];       // bit j: tap j's source row exists and is unmasked
#pragma unroll
    for (int i = 0; i < GA; ++i) {
        const int r = RPI * (i * NW + wave) + lane / CPR;
        const int lc = (lane % CPR) ^ (ABF16 ? ((r >> 1) & 7) : (r & 15));
        const int m = m0 + r;
        int b = 0, u = 0;
        const bool mv = m < M;
        mtts::divmod_fast(mv ? m : 0, p.To, inv_to, b, u);
        uint32_t ok = 0;
        for (int j = 0; j < p.ntaps; ++j) {
            const int irow = u * p.in_stride + off0 + j * offstep;
            bool v = mv && irow >= 0 && irow < p.Ti;
            if (v && p.a_scale) v = p.a_scale[(size_t)b * p.Ti + irow] != 0.f;
            ok |= (uint32_t)v << j;
        }
        a_ok[i] = ok;
        const int k = kstep0 * kBK + lc * EPC;  // the lane's element within the first K step
        a_j[i] = k / p.cin;
        a_ch[i] = k - a_j[i] * p.cin;
        a_src[i] = reinterpret_cast<const char *>(p.A) +
                   ((long long)(b * p.Ti + u * p.in_stride + off0 + a_j[i] * offstep) * p.lda + a_ch[i]) * ES;
    }
    // ---- W chunk state: instruction i covers W rows 8q..8q+7; lane -> row 8q + lane/8, LDS slot lane%8
    // <- logical chunk (lane%8) ^ ((row >> 1) & 7)
    const uint16_t *w_ptr[GW];
    int w_k[GW];
    bool w_nok[GW];
    const size_t w_plane = (size_t)p.N * p.Kp;  // WS / X3: elements from one weight plane to the next
#pragma unroll
    for (int i = 0; i < GW; ++i) {
        const int ni = 8 * (i * NW + wave) + (lane >> 3);  // row of the W image
        const int pl = NPL > 1 ? ni / BN : 0;
        const int n = ni - pl * BN;
        const int lc = (lane & 7) ^ ((ni >> 1) & 7);  // BN % 16 == 0: the lo rows swizzle like the hi rows
        w_nok[i] = n0 + n < p.N;
        w_k[i] = kstep0 * kBK + lc * 8;
        w_ptr[i] = static_cast<const uint16_t *>(p.W) + pl * w_plane + (size_t)(w_nok[i] ? n0 + n : 0) * p.Kp + w_k[i];
    }

    // ---- LEAN state: per chunk the tap-0 element index of its row and the byte offset of the current
    // tap (MTTS_GLDS_OOB when that tap's row is absent or masked); scalar tap / channel-block counters
    const int tapstride = offstep * p.lda;
    int l_row[LEAN ? GA : 1];
    uint32_t l_vo[LEAN ? GA : 1], l_vw[LEAN ? GW : 1];
    int l_tap = 0, l_chs = 0;
    uint32_t l_soa = 0, l_sow = 0;
    u32x4 l_rsa, l_rsw;
    if constexpr (LEAN) {
        const int k0 = kstep0 * kBK;
        l_tap = __builtin_amdgcn_readfirstlane(k0 / p.cin);
        const int ch0 = k0 - l_tap * p.cin;
        l_chs = __builtin_amdgcn_readfirstlane((p.cin - ch0) / kBK);
        l_soa = __builtin_amdgcn_readfirstlane((uint32_t)(ch0 * ES));
        l_sow = __builtin_amdgcn_readfirstlane((uint32_t)(k0 * 2));
        l_rsa = make_rsrc(p.A, (uint32_t)((long long)p.nb * p.Ti * p.lda * ES));
        l_rsw = make_rsrc(p.W, (uint32_t)((long long)NPL * p.N * p.Kp * 2));
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const int r = RPI * (i * NW + wave) + lane / CPR;
            const int lc = (lane % CPR) ^ (ABF16 ? ((r >> 1) & 7) : (r & 15));
            int b = 0, u = 0;
            mtts::divmod_fast(m0 + r < M ? m0 + r : 0, p.To, inv_to, b, u);
            l_row[i] = (b * p.Ti + u * p.in_stride + off0) * p.lda + lc * EPC;
            l_vo[i] = ((a_ok[i] >> min(l_tap, 31)) & 1u) ? (uint32_t)((l_row[i] + l_tap * tapstride) * ES) : MTTS_GLDS_OOB;
        }
#pragma unroll
        for (int i = 0; i < GW; ++i) {
            const int ni = 8 * (i * NW + wave) + (lane >> 3);
            const int pl = NPL > 1 ? ni / BN : 0;
            const int n = ni - pl * BN;
            const int lc = (lane & 7) ^ ((ni >> 1) & 7);
            l_vw[i] = w_nok[i] ? (uint32_t)((pl * w_plane + (size_t)(n0 + n) * p.Kp + lc * 8) * 2) : MTTS_GLDS_OOB;
        }
    }

    auto issue = [&](auto S) {
        unsigned char *abase = abuf(S);
        unsigned char *wbase = wbuf(S);
        if constexpr (LEAN) {
            const uint32_t la = abuf_l(S), lw = wbuf_l(S);
#pragma unroll
            for (int i = 0; i < GA; ++i)
                if (i < GA - 1 || a_last)
                    bload16(l_vo[i], l_rsa, l_soa, __builtin_amdgcn_readfirstlane(la + (i * NW + wave) * 1024));
#pragma unroll
            for (int i = 0; i < GW; ++i)
                if (i < GW - 1 || w_last)
                    bload16(l_vw[i], l_rsw, l_sow, __builtin_amdgcn_readfirstlane(lw + (i * NW + wave) * 1024));
            l_sow += kBK * 2;
            l_soa += kBK * ES;
            if (--l_chs == 0) {  // next tap (wave-uniform branch; nothing in flight depends on registers)
                ++l_tap;
                l_chs = p.cin / kBK;
                l_soa = 0;
#pragma unroll
                for (int i = 0; i < GA; ++i)
                    l_vo[i] = ((a_ok[i] >> min(l_tap, 31)) & 1u) ? (uint32_t)((l_row[i] + l_tap * tapstride) * ES)
                                                                 : MTTS_GLDS_OOB;
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const bool ok = (a_ok[i] >> min(a_j[i], 31)) & 1u;  // a_j >= ntaps (past K): bit is 0
            if (i < GA - 1 || a_last)
                glds16(ok ? static_cast<const void *>(a_src[i]) : static_cast<const void *>(zero),
                       abase + (i * NW + wave) * 1024);
            a_ch[i] += kBK;
            a_src[i] += kBK * ES;
            const bool w = a_ch[i] >= p.cin;  // cin >= 64: at most one tap change per step
            a_ch[i] -= w ? p.cin : 0;
            a_j[i] += w;
            a_src[i] += w ? tap_delta : 0;
        }
#pragma unroll
        for (int i = 0; i < GW; ++i) {
            const bool ok = w_nok[i] && w_k[i] < p.Kp;
            if (i < GW - 1 || w_last)
                glds16(ok ? static_cast<const void *>(w_ptr[i]) : static_cast<const void *>(zero),
                       wbase + (i * NW + wave) * 1024);
            w_ptr[i] += kBK;
            w_k[i] += kBK;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    auto compute = [&](auto S) {
        const unsigned char *abase = abuf(S);
        const unsigned char *wbase = wbuf(S);
        if constexpr (X3) {
#pragma unroll
            for (int ks = 0; ks < kBK / 16; ++ks) {
                bf16x8 ah[TM], am[TM], al[TM], bh[TN], bm[TN], bl[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int r = wr * 32 * TM + i * 32 + lr;
                    const int c = 4 * ks + 2 * lh;
                    const float4 x0 = *reinterpret_cast<const float4 *>(abase + r * 256 + ((c ^ (r & 15)) << 4));
                    const float4 x1 = *reinterpret_cast<const float4 *>(abase + r * 256 + (((c + 1) ^ (r & 15)) << 4));
                    float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                    uint32_t wh[4], wm[4], wl[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {  // every residual is exact in fp32
                        wh[q] = pack2(v[2 * q], v[2 * q + 1]);
                        v[2 * q] -= __uint_as_float(wh[q] << 16);
                        v[2 * q + 1] -= __uint_as_float(wh[q] & 0xffff0000u);
                        wm[q] = pack2(v[2 * q], v[2 * q + 1]);
                        v[2 * q] -= __uint_as_float(wm[q] << 16);
                        v[2 * q + 1] -= __uint_as_float(wm[q] & 0xffff0000u);
                        wl[q] = pack2(v[2 * q], v[2 * q + 1]);
                    }
                    ah[i] = __builtin_bit_cast(bf16x8, make_uint4(wh[0], wh[1], wh[2], wh[3]));
                    am[i] = __builtin_bit_cast(bf16x8, make_uint4(wm[0], wm[1], wm[2], wm[3]));
                    al[i] = __builtin_bit_cast(bf16x8, make_uint4(wl[0], wl[1], wl[2], wl[3]));
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = wc * 32 * TN + j * 32 + lr;
                    const int c = 2 * ks + lh;
                    const int sw = (c ^ ((n >> 1) & 7)) << 4;  // BN % 16 == 0: every plane swizzles alike
                    bh[j] = *reinterpret_cast<const bf16x8 *>(wbase + n * 128 + sw);
                    bm[j] = *reinterpret_cast<const bf16x8 *>(wbase + (n + BN) * 128 + sw);
                    bl[j] = *reinterpret_cast<const bf16x8 *>(wbase + (n + 2 * BN) * 128 + sw);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bm[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                    }
            }
            return;
        }
#pragma unroll
        for (int ks = 0; ks < kBK / 16; ++ks) {
            bf16x8 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int r = wr * 32 * TM + i * 32 + lr;
                if constexpr (ABF16) {
                    const int c = 2 * ks + lh;
                    af[i] = *reinterpret_cast<const bf16x8 *>(abase + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
                } else {
                    const int c = 4 * ks + 2 * lh;
                    const float4 x0 = *reinterpret_cast<const float4 *>(abase + r * 256 + ((c ^ (r & 15)) << 4));
                    const float4 x1 =
                        *reinterpret_cast<const float4 *>(abase + r * 256 + (((c + 1) ^ (r & 15)) << 4));
                    const uint4 w =
                        make_uint4(pack2(x0.x, x0.y), pack2(x0.z, x0.w), pack2(x1.x, x1.y), pack2(x1.z, x1.w));
                    af[i] = __builtin_bit_cast(bf16x8, w);
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = wc * 32 * TN + j * 32 + lr;
                const int c = 2 * ks + lh;
                bfr[j] = *reinterpret_cast<const bf16x8 *>(wbase + n * 128 + ((c ^ ((n >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            if constexpr (WS) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = BN + wc * 32 * TN + j * 32 + lr;
                    const int c = 2 * ks + lh;
                    bfr[j] = *reinterpret_cast<const bf16x8 *>(wbase + n * 128 + ((c ^ ((n >> 1) & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
    };

#if MTTS_GEMM_TIMELINE
    if (lane == 0 && (int)blockIdx.x * NW + wave < kTlWaves)
        g_tlg[((int)blockIdx.x * NW + wave) * kTlSlots] =
            ((long long)__smid() << 32) | (long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
    MTTS_TLG(1);
#endif
    // prologue: steps 0 .. STAGES-2 in flight (steps past nk DMA zeros into their buffer: harmless)
    issue(std::integral_constant<int, 0>{});
    if constexpr (STAGES > 2) issue(std::integral_constant<int, 1>{});
    if constexpr (STAGES > 3) issue(std::integral_constant<int, 2>{});
    MTTS_TLG(2);
    // step kt uses buffer kt % STAGES and refills buffer (kt + STAGES - 1) % STAGES, which step kt-1 read
    int tl_k = 0;
    (void)tl_k;
    auto step = [&](auto S) {
        constexpr int cur = decltype(S)::value, nxt = (cur + STAGES - 1) % STAGES;
        // this wave's DMAs for step kt have landed: all but the STAGES - 2 later steps' -- a count of the wave's
        // own instructions per step, so with a ragged split each wave waits on its own constant
        constexpr int F = (GA + GW) * (STAGES - 2);
        if constexpr (!G::RAGGED || STAGES == 2) {
            wait_vmcnt<F>();
        } else {
            const int less = (a_last ? 0 : 1) + (w_last ? 0 : 1);  // wave-uniform
            if (less == 0) wait_vmcnt<F>();
            else if (less == 1) wait_vmcnt<F - (STAGES - 2)>();
            else wait_vmcnt<F - 2 * (STAGES - 2)>();
        }
        mtts::lds_barrier();                       // ... everyone's, and step kt-1's reads are done
#if MTTS_GEMM_TIMELINE
        if (tl_k < kTlSteps) MTTS_TLG(3 + 2 * tl_k);
#endif
        issue(std::integral_constant<int, nxt>{});
        compute(S);
#if MTTS_GEMM_TIMELINE
        __builtin_amdgcn_sched_barrier(0);
        if (tl_k < kTlSteps) MTTS_TLG(4 + 2 * tl_k);
        ++tl_k;
#endif
    };
    for (int kt = 0; kt < nk; kt += STAGES) {
        step(std::integral_constant<int, 0>{});
        if (kt + 1 >= nk) break;
        step(std::integral_constant<int, 1>{});
        if constexpr (STAGES > 2) {
            if (kt + 2 >= nk) break;
            step(std::integral_constant<int, 2>{});
        }
        if constexpr (STAGES > 3) {
            if (kt + 3 >= nk) break;
            step(std::integral_constant<int, 3>{});
        }
    }
    wait_vmcnt<0>();  // no DMA may still target this workgroup's LDS when it retires
    MTTS_TLG(kTlSlots - 2);
    if (part || mtts::gemm_epilogue_vec_ok(p)) {
        mtts::lds_barrier();  // every wave is past its last fragment read: the buffers are free
        unsigned char *stage;
        if constexpr (NW <= 8) {
            stage = (wave % 4 == 0 ? sA0 : wave % 4 == 1 ? sW0 : wave % 4 == 2 ? sA1 : sW1) + (wave / 4) * 4096;
        } else {  // consecutive 4 KiB slots of sA0, sW0, sA1, sW1 (GldsGeom asserts that they hold NW images)
            constexpr int SA = G::SA, SW = G::SW;
            stage = wave < SA ? sA0 + wave * 4096
                    : wave < SA + SW ? sW0 + (wave - SA) * 4096
                    : wave < 2 * SA + SW ? sA1 + (wave - SA - SW) * 4096
                                         : sW1 + (wave - 2 * SA - SW) * 4096;
        }
        float *st = reinterpret_cast<float *>(stage);
        if (part)
            mtts::gemm_store_partial<TM, TN>(p, acc, st, part + (size_t)(kstep0 / ksteps) * M * p.N,
                                             m0 + wr * 32 * TM, n0 + wc * 32 * TN, lane);
        else
            mtts::gemm_epilogue_vec<TM, TN>(p, acc, st, m0 + wr * 32 * TM, n0 + wc * 32 * TN, lane);
    } else {
        mtts::gemm_epilogue<TM, TN>(p, acc, m0 + wr * 32 * TM, n0 + wc * 32 * TN, lr, lh);
    }
    MTTS_TLG(kTlSlots - 1);
}

// Split-K combine: out = epilogue(sum_s part[s][m][n..n+3]) summed in split order (deterministic).
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(mtts_conv_gemm_args p, const float *__restrict__ part,
                                                              int S) {
    const int M = p.nb * p.To, n4 = p.N >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)M * n4) return;
    const int m = (int)(idx / n4), n = (int)(idx - (long long)m * n4) * 4;
    const size_t slab = (size_t)M * p.N;
    float4 a = *reinterpret_cast<const float4 *>(part + (size_t)m * p.N + n);
    for (int s = 1; s < S; ++s) {
        const float4 b = *reinterpret_cast<const float4 *>(part + s * slab + (size_t)m * p.N + n);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float4 bn = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bn = *reinterpret_cast<const float4 *>(p.bias + n);
    float e[4] = {a.x + bn.x, a.y + bn.y, a.z + bn.z, a.w + bn.w};
    int b, u;
    mtts::divmod_fast(m, p.To, 1.0f / (float)p.To, b, u);
    uint32_t s0 = 0, s1 = 0;
    float keep = 1.f;
    if (p.dropout_p > 0.f) {
        s0 = p.seed[0];
        s1 = p.seed[1];
        keep = mtts::dropout_scale(p.dropout_p);
    }
    mtts::epilogue_row4(p, b * p.To_full + u * p.out_stride + p.out_off, n, e, s0, s1, keep);
}

// Operand kinds: A storage x weight planes.  A schedule has an instantiation per kind in its mask.
enum : unsigned { kF32 = 1u, kB16 = 2u, kF32WS = 4u, kB16WS = 8u, kX3 = 16u };
constexpr int kNumKinds = 5;
constexpr bool kind_a16(int kind) { return kind == 1 || kind == 3; }
constexpr int kind_planes(int kind) { return kind == 4 ? 3 : kind >= 2 ? 2 : 1; }
inline int kind_of(const mtts_conv_gemm_args &p) {
    if (p.flags & MTTS_GEMM_F_SPLIT3) return 4;
    return ((p.flags & MTTS_GEMM_F_W_SPLIT) ? 2 : 0) + ((p.flags & MTTS_GEMM_F_A_BF16) ? 1 : 0);
}

struct GldsCfg {
    int id;  // the public schedule id (MTTS_GEMM_GLDS + its place in the tuning rounds' table: DESIGN.md §3)
    int wm, wn, tm, tn, stages;
    unsigned kinds;  // operand kinds with an instantiation (LDS <= 160 KiB, registers)
    bool lean_only = false;  // only the scalar-addressed loop is built (the register-addressed one spills)
};
// Stage bytes = A image + W image of one K step (64 x BM x 2 or 4 bytes, planes x 64 x BN x 2 bytes); LDS per
// workgroup = stages x stage bytes; resident workgroups per CU = min(160 KiB / LDS, 2048 threads / workgroup)
// (glds_resident, which also names the one instantiation whose registers bind; the 160-row figures are below).  Two figures size a
// schedule: resident x LDS <= 160 KiB, and the bytes in flight per CU during the K loop,
// (stages - 1) x stage bytes x resident, near or above the ~96 KB that cover the 1.1 us DMA latency at the
// 75-95 GB/s per-CU fill ceiling.  The 160-row tiles (46, 47; 160 = 5 x 32 divides the decoder's 9600 and 19200
// rows: 60 / 120 row tiles instead of 150 / 300, so 240 or 480 workgroups on the chip's 256 or 512 slots) per
// kind, stage bytes -> LDS, resident, in flight:
//   46 160 x 64  2 st  bf16 A 2 pl  20+16 = 36 KiB ->  72 KiB, 2 resident (144 KiB),  72 KiB in flight
//                      bf16 A 1 pl  20+ 8 = 28 KiB ->  56 KiB, 2 resident (112 KiB),  56 KiB
//                      fp32 A 2 pl  40+16 = 56 KiB -> 112 KiB, 1 resident,            56 KiB (thin)
//                      fp32 A 1 pl  40+ 8 = 48 KiB ->  96 KiB, 1 resident,            48 KiB (thin)
//   47 160 x 128 3 st  bf16 A 2 pl  20+32 = 52 KiB -> 156 KiB, 1 resident, 104 KiB; 1 pl 36 KiB -> 108 KiB, 1, 72 KiB
// Registers (kernel-resource-usage; no AGPRs, scratch 0): 46 with bf16 A, two resident = 5 waves per SIMD, so <= 96:
// 80 / 77 VGPRs (2 / 1 planes; register-addressed loop 93 / 86); 46 with fp32 A, one resident = 3 waves per SIMD, so
// <= 168: 94 / 94 (123 / 114); 47, one resident: 165 / 150 -- its register-addressed loop needs 168 + 148 bytes of
// scratch with two planes, so 47 is built for whole-tap K steps only and runs 41 otherwise.
// Measured and not kept: 160 x 64 with four stages (one resident, 108 KiB in flight: 2-5 % behind the
// two-stage 46 on every 9600-row shape, 3-27 % on the 19200-row ones) and 160 x 32 with three stages for fp32 A
// (five waves, 1.7-2x slower than 46: ten DMA instructions per wave and step).
constexpr GldsCfg kGlds[] = {
    {41, 2, 4, 1, 2, 2, kF32 | kB16 | kF32WS | kB16WS},  // 64 x 256, 512 thr (waves 32 x 64), 2 stages (96 KiB; split
                                                          // W: 144 KiB with bf16 A, 160 KiB with fp32 A)
    {42, 2, 4, 1, 2, 3, kF32 | kB16},                     // 64 x 256, 512 thr, 3 stages (144 KiB)
    {44, 2, 2, 1, 1, 3, kF32 | kB16 | kF32WS | kB16WS | kX3},  // 64 x 64, 3 stages (72 KiB; bf16x6: 120 KiB)
    {45, 2, 2, 1, 1, 2, kF32 | kF32WS | kX3},             // 64 x 64, 2 stages (48 KiB)
    {46, 5, 2, 1, 1, 2, kF32 | kB16 | kF32WS | kB16WS},   // 160 x 64, 640 thr (waves 32 x 32), 2 stages
    {47, 5, 2, 1, 2, 3, kB16 | kB16WS, true},             // 160 x 128, 640 thr (waves 32 x 64), 3 stages
};
constexpr int kNumGlds = sizeof(kGlds) / sizeof(kGlds[0]);
// The table index of public schedule id (-1: none).  Everything below the mtts:: interface works on indices.
constexpr int glds_ix(int id) {
    for (int c = 0; c < kNumGlds; ++c)
        if (kGlds[c].id == id) return c;
    return -1;
}

// The instantiation schedule c runs for an operand kind: its own where it has one (47: for whole-tap K steps); else
//  * three planes (bf16x6): 64 x 64 three-stage (44) or two-stage (45) by the schedule's stage count;
//  * one or two planes: 64 x 256 two-stage (41), the one schedule with all four kinds.
constexpr int glds_run_id(int c, int kind, bool lean = true) {
    if (kGlds[c].lean_only && !lean) return glds_ix(41);
    if (kGlds[c].kinds & (1u << kind)) return c;
    if (kind == 4) return glds_ix(kGlds[c].stages >= 3 ? 44 : 45);
    return glds_ix(41);
}
constexpr int glds_bm(int c) { return 32 * kGlds[c].wm * kGlds[c].tm; }
constexpr int glds_bn(int c) { return 32 * kGlds[c].wn * kGlds[c].tn; }
constexpr int glds_stage_bytes(int c, int kind) {
    return glds_bm(c) * kBK * (kind_a16(kind) ? 2 : 4) + kind_planes(kind) * glds_bn(c) * kBK * 2;
}
constexpr int glds_resident(int c, int kind, bool lean = true) {
    // the one instantiation whose registers bind: 41 with a bf16 A and one plane, register-addressed loop -- 140 VGPRs,
    // three waves per SIMD, one 8-wave workgroup (80 KiB of LDS would admit two; its scalar-addressed loop: 108, two)
    if (c == glds_ix(41) && kind == 1 && !lean) return 1;
    const int lds = kGlds[c].stages * glds_stage_bytes(c, kind), nt = 64 * kGlds[c].wm * kGlds[c].wn;
    const int by_lds = 160 * 1024 / lds, by_thr = 2048 / nt;
    return by_lds < by_thr ? by_lds : by_thr;
}

}  // namespace

namespace mtts {
// The LEAN loop needs whole-tap K steps and 32-bit byte offsets with room for MTTS_GLDS_OOB.
bool conv_gemm_glds_lean(const mtts_conv_gemm_args &p) {
    const int es = (p.flags & MTTS_GEMM_F_A_BF16) ? 2 : 4;
    return p.cin % kBK == 0 && (long long)p.nb * p.Ti * p.lda * es < (1ll << 31) &&
           (long long)p.N * p.Kp * 2 < (1ll << 31);
}
}  // namespace mtts

namespace {

template <int C, int KIND>
auto glds_kernel(bool lean) {
    constexpr GldsCfg c = kGlds[C];
    constexpr bool A16 = kind_a16(KIND), WS = KIND == 2 || KIND == 3, X3 = KIND == 4;
    if constexpr (c.lean_only) {
        return conv_gemm_glds_kernel<c.wm, c.wn, c.tm, c.tn, c.stages, A16, true, WS, X3>;
    } else {
        return lean ? conv_gemm_glds_kernel<c.wm, c.wn, c.tm, c.tn, c.stages, A16, true, WS, X3>
                    : conv_gemm_glds_kernel<c.wm, c.wn, c.tm, c.tn, c.stages, A16, false, WS, X3>;
    }
}

template <int C, int KIND>
int launch_glds_t(const mtts_conv_gemm_args &p, int M, int splits, float *part, hipStream_t st) {
    static_assert(kGlds[C].kinds & (1u << KIND), "an instantiated kind");
    static_assert(glds_resident(C, KIND) >= 1, "the stages fit LDS");
    constexpr int BM = glds_bm(C), BN = glds_bn(C), NT = 64 * kGlds[C].wm * kGlds[C].wn;
    auto kern = glds_kernel<C, KIND>(mtts::conv_gemm_glds_lean(p));
    const int nk = (p.K + kBK - 1) / kBK;
    const int ksteps = (nk + splits - 1) / splits;
    const int S = splits > 1 ? (nk + ksteps - 1) / ksteps : 1;  // every split non-empty
    dim3 grid((unsigned)(((M + BM - 1) / BM) * ((p.N + BN - 1) / BN) * S));
    hipLaunchKernelGGL(kern, grid, dim3(NT), 0, st, p, ksteps, S > 1 ? part : nullptr);
    int rc = mtts::check_launch("conv_gemm_glds");
    if (rc || S == 1) return rc;
    const long long n4 = (long long)M * (p.N / 4);
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, p,
                       (const float *)part, S);
    return mtts::check_launch("splitk_epilogue_kernel");
}

template <int C>
int launch_glds(const mtts_conv_gemm_args &p, int M, int splits, float *part, hipStream_t st) {
    if constexpr (kGlds[C].lean_only) {
        if (!mtts::conv_gemm_glds_lean(p)) return launch_glds<glds_ix(41)>(p, M, splits, part, st);
    }
    switch (kind_of(p)) {
        case 4: return launch_glds_t<glds_run_id(C, 4), 4>(p, M, splits, part, st);
        case 3: return launch_glds_t<glds_run_id(C, 3), 3>(p, M, splits, part, st);
        case 2: return launch_glds_t<glds_run_id(C, 2), 2>(p, M, splits, part, st);
        case 1: return launch_glds_t<glds_run_id(C, 1), 1>(p, M, splits, part, st);
        default: return launch_glds_t<glds_run_id(C, 0), 0>(p, M, splits, part, st);
    }
}

// hipOccupancyMaxActiveBlocksPerMultiprocessor of schedule C's own instantiation for a kind (-1: none)
template <int C>
int occupancy_glds(int kind, bool lean) {
    int n = -1;
    auto ask = [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        if constexpr ((kGlds[C].kinds & (1u << KIND)) != 0) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, glds_kernel<C, KIND>(lean), 64 * kGlds[C].wm * kGlds[C].wn,
                                                             0) != hipSuccess)
                n = -2;
        }
    };
    switch (kind) {
        case 0: ask(std::integral_constant<int, 0>{}); break;
        case 1: ask(std::integral_constant<int, 1>{}); break;
        case 2: ask(std::integral_constant<int, 2>{}); break;
        case 3: ask(std::integral_constant<int, 3>{}); break;
        case 4: ask(std::integral_constant<int, 4>{}); break;
        default: break;
    }
    return n;
}

template <int... I>
int occupancy_glds_ix(int c, int kind, bool lean, std::integer_sequence<int, I...>) {
    int n = -1;
    ((c == I ? (n = occupancy_glds<I>(kind, lean), true) : false) || ...);
    return n;
}

template <int... I>
int launch_glds_ix(int c, const mtts_conv_gemm_args &p, int M, int splits, float *part, hipStream_t st,
                   std::integer_sequence<int, I...>) {
    int rc = MTTS_ERR_INVALID_ARG;
    ((c == I ? (rc = launch_glds<I>(p, M, splits, part, st), true) : false) || ...);
    return rc;
}

}  // namespace

namespace mtts {

bool conv_gemm_glds_has(int id) { return glds_ix(id) >= 0; }

// Whether the LDS-DMA kernels can run this GEMM (bf16; 16-byte aligned rows; 0/1 row mask or none;
// 32-bit element offsets).
bool conv_gemm_glds_applies(const mtts_conv_gemm_args &p) {
    if (p.a_scale && !(p.flags & MTTS_GEMM_F_BINARY_SCALE)) return false;
    if (p.cin < kBK || p.cin % 4 || p.lda % 4 || p.Kp % 8) return false;
    if ((p.flags & MTTS_GEMM_F_A_BF16) && (p.cin % 8 || p.lda % 8 || (uintptr_t)p.A % 16)) return false;
    const long long arows = (long long)p.nb * p.Ti;
    if (arows * p.lda >= (1ll << 31) - (1ll << 20)) return false;
    return true;
}

size_t conv_gemm_glds_splitk_bytes(const mtts_conv_gemm_args &p, int splits) {
    if (splits <= 1) return 0;
    const int nk = (p.K + kBK - 1) / kBK;
    const int ksteps = (nk + splits - 1) / splits;
    const int S = (nk + ksteps - 1) / ksteps;
    return S > 1 ? (size_t)S * p.nb * p.To * p.N * sizeof(float) : 0;
}

int splitk_combine(const mtts_conv_gemm_args &p, int M, const float *part, int S, hipStream_t st) {
    const long long n4 = (long long)M * (p.N / 4);
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, p, part, S);
    return mtts::check_launch("splitk_epilogue_kernel");
}

int conv_gemm_glds_launch(int id, const mtts_conv_gemm_args &p, int M, int splits, float *part, hipStream_t st) {
    return launch_glds_ix(glds_ix(id), p, M, splits, part, st, std::make_integer_sequence<int, kNumGlds>{});
}

// The tile, stage bytes and resident workgroups per CU of the instantiation that schedule `id` runs for p's
// operand kind (glds_run_id: the launch's own mapping), from the table beside kGlds[].
GldsInfo conv_gemm_glds_info(int id, const mtts_conv_gemm_args &p) {
    const int kind = kind_of(p);
    GldsInfo g = {};
    const int c = glds_ix(id);
    if (c < 0) return g;
    const int r = glds_run_id(c, kind, conv_gemm_glds_lean(p));
    g.run_id = kGlds[r].id;
    g.bm = glds_bm(r);
    g.bn = glds_bn(r);
    g.stages = kGlds[r].stages;
    g.stage_bytes = glds_stage_bytes(r, kind);
    g.resident = glds_resident(r, kind, conv_gemm_glds_lean(p));
    g.own = r == c;
    return g;
}
}  // namespace mtts

// Table figure and the runtime's answer for one instantiation (tests): out[0] = the table's resident workgroups per
// CU, out[1] = hipOccupancyMaxActiveBlocksPerMultiprocessor.  kind: 0 fp32 A, 1 bf16 A, 2 / 3 the same with split
// weights, 4 three planes.  MTTS_ERR_INVALID_ARG when the schedule has no instantiation of its own for the kind.
extern "C" int mtts_conv_gemm_glds_occupancy(int32_t schedule, int32_t kind, int32_t lean, int32_t out[2]) {
    const int c = glds_ix(schedule);
    MTTS_CHECK_ARG(out && c >= 0 && kind >= 0 && kind < kNumKinds && (kGlds[c].kinds & (1u << kind)) &&
                       (lean || !kGlds[c].lean_only),
                   "conv_gemm_glds_occupancy: no such instantiation");
    out[0] = glds_resident(c, kind, lean != 0);
    out[1] = occupancy_glds_ix(c, kind, lean != 0, std::make_integer_sequence<int, kNumGlds>{});
    if (out[1] < 0) return mtts::fail(MTTS_ERR_HIP, "conv_gemm_glds_occupancy: occupancy query failed");
    return MTTS_OK;
}

#if MTTS_GEMM_TIMELINE
// diagnostic builds: copy (or zero, host == NULL) the LDS-DMA kernels' timeline buffer; returns its size in bytes
extern "C" long long mtts_glds_timeline_read(void *host) {
    const size_t bytes = sizeof(long long) * kTlWaves * kTlSlots;
    if (host) {
        if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_tlg), bytes) != hipSuccess) return -1;
    } else {
        void *d = nullptr;
        if (hipGetSymbolAddress(&d, HIP_SYMBOL(g_tlg)) != hipSuccess || hipMemset(d, 0, bytes) != hipSuccess) return -1;
    }
    return (long long)bytes;
}
#endif
