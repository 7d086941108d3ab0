// HiFi-GAN generator inference on gfx950 (reference: hifi_gan/models.py:11-125), include/mtts_vocoder.h.
//
// One implicit-GEMM kernel on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) serves every conv of the generator:
//   mtts_voc_conv     : the dilated "same" Conv1d of the resblocks, k <= 11 taps,
//   mtts_voc_upsample : ConvTranspose1d with k == 2u as two 2-tap launches (phases p < u/2 read frames
//                       (t-1, t), phases p >= u/2 read (t, t+1)); a launch writes u/2 * cout columns of the
//                       output seen as [B*L, u*cout], which is token-major [B*L*u, cout],
//   mtts_voc_pre      : conv_pre, k = 7, after one transposing launch of the channel-major mel.
// mtts_voc_post (N = 1) is a VALU kernel.
//
// The conv kernel.  A workgroup (4 waves) owns 128 output frames of ONE utterance x BN output channels
// (BN = 32 / 64 / 128; wave w owns frames 32w .. 32w+31, BN/32 accumulators).  K = taps x channels is walked
// in steps of one tap x 32 channels:
//   - the A window -- the tile's 128 frames plus the halo of `tps` taps, 128 + (tps-1)*d <= 192 rows x 32
//     channels -- is staged in LDS once per (channel chunk, tap group) and serves tps steps; the leaky ReLU
//     is applied at that LDS store, frames outside [0, L) of the tile's own utterance are stored as zeros
//     (the tile never addresses another utterance), so a halo longer than L is just a window of zeros;
//     its global loads (6 x 16 B per thread) are issued together one window ahead, during the MFMAs of the
//     step before the restage (loaded one by one at the restage they cost 10 % of the B = 8 forward);
//   - the W slab of a step (BN x 32) is double-buffered: the next step's global loads are issued before
//     the MFMAs of this one and stored to the other LDS buffer after them; one LDS-only barrier per step.
// LDS rows have a pitch of 36 floats, so the 16-byte fragment reads of 16 consecutive rows hit 16 distinct
// 4-bank groups.  The k index inside a step is permuted (lane half h takes channels 8q+4h .. 8q+4h+3 of both
// operands): A and W use the same map, so the sum is the same set of products.
// Late stages are byte-bound: BN covers all of N there (N = 32 / 64), so A is read from HBM once and only its
// halo rows come again from L2.
// Deterministic: no atomics, a fixed summation order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mtts_base.h"
#include "mtts_vocoder.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kBM = 128;      // output frames per workgroup
constexpr int kKC = 32;       // channels per K step
constexpr int kPitch = 36;    // LDS row pitch in floats
constexpr int kWinMax = 192;  // A window rows: 128 + (tps - 1) * d
constexpr int kThreads = 256;
constexpr int kAQ = kWinMax * (kKC / 4) / kThreads;  // float4 of the A window per thread: 6

struct VocP {
    const float *A;
    const float *W;
    const float *bias;
    const float *res;
    float *C;
    float *acc;
    int L, cin, N, ntaps, off0, d, tps, tilesL;
    int ldw, ldc, bias_n;
    int leaky, acc_mode;
    float slope, acc_div;
};

__device__ __forceinline__ float lrelu(float v, float s) { return v > 0.f ? v : v * s; }

template <int BN>
__global__ __launch_bounds__(kThreads) void voc_conv_kernel(const VocP p) {
    constexpr int NT = BN / 32;
    constexpr int WQ = BN * (kKC / 4) / kThreads;  // float4 of W per thread and step
    __shared__ __attribute__((aligned(16))) float As[kWinMax * kPitch];
    __shared__ __attribute__((aligned(16))) float Ws[2][BN * kPitch];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.x / p.tilesL, u0 = (blockIdx.x - b * p.tilesL) * kBM;
    const int n0 = blockIdx.y * BN;
    const size_t row0 = (size_t)b * p.L;  // first row of this tile's utterance
    const int win = kBM + (p.tps - 1) * p.d;
    const int nchunks = (p.cin + kKC - 1) / kKC;
    const int nsteps = nchunks * p.ntaps;

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    float4 wreg[WQ];
    auto load_w = [&](int tap, int c0) {
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int i = tid + q * kThreads, n = n0 + (i >> 3), c = c0 + 4 * (i & 7);
            wreg[q] = (n < p.N && c < p.cin)
                          ? *reinterpret_cast<const float4 *>(p.W + (size_t)n * p.ldw + (size_t)tap * p.cin + c)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // The A window goes through registers too: all of its loads are issued together, from clamped always-valid
    // addresses with no branch around them, one window ahead (during the MFMAs of the step before the restage);
    // validity, the zero padding and the leaky ReLU are applied at the LDS store.  Rows past `win` (up to the 192
    // the LDS image holds) are stored from a clamped address and never read.
    float4 areg[kAQ];
    auto load_a = [&](int tap, int c0) {
        const int ubase = u0 + p.off0 + tap * p.d;
#pragma unroll
        for (int q = 0; q < kAQ; ++q) {
            const int i = tid + q * kThreads;
            const int u = min(max(ubase + min(i >> 3, win - 1), 0), p.L - 1), c = min(c0 + 4 * (i & 7), p.cin - 4);
            areg[q] = *reinterpret_cast<const float4 *>(p.A + (row0 + u) * p.cin + c);
        }
    };
    auto store_a = [&](int tap, int c0) {
        const int ubase = u0 + p.off0 + tap * p.d;
#pragma unroll
        for (int q = 0; q < kAQ; ++q) {
            const int i = tid + q * kThreads, u = ubase + (i >> 3);
            const bool ok = u >= 0 && u < p.L && c0 + 4 * (i & 7) < p.cin;
            float4 v = areg[q];
            if (p.leaky) {
                v.x = lrelu(v.x, p.slope); v.y = lrelu(v.y, p.slope);
                v.z = lrelu(v.z, p.slope); v.w = lrelu(v.w, p.slope);
            }
            v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
            *reinterpret_cast<float4 *>(As + (i >> 3) * kPitch + 4 * (i & 7)) = v;
        }
    };
    load_w(0, 0);
    load_a(0, 0);

    int tap = 0, c0 = 0;
    for (int s = 0; s < nsteps; ++s) {
        const int tj = tap % p.tps;
        if (tj == 0) {
            // every wave is done with the previous window
            if (s) mtts::lds_barrier();
            store_a(tap, c0);
        }
        float *wb = Ws[s & 1];
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int i = tid + q * kThreads;
            *reinterpret_cast<float4 *>(wb + (i >> 3) * kPitch + 4 * (i & 7)) = wreg[q];
        }
        mtts::lds_barrier();
        // next step's coordinates; its W loads (and its A window's, if it restages) fly during this step's MFMAs
        int ntap = tap + 1, nc0 = c0;
        if (ntap == p.ntaps) { ntap = 0; nc0 += kKC; }
        if (s + 1 < nsteps) {
            load_w(ntap, nc0);
            if (ntap % p.tps == 0) load_a(ntap, nc0);
        }

        const float *arow = As + (wave * 32 + r + tj * p.d) * kPitch + 4 * h;
        const float *wrow = wb + r * kPitch + 4 * h;
#pragma unroll
        for (int q = 0; q < kKC / 8; ++q) {
            const float4 a = *reinterpret_cast<const float4 *>(arow + 8 * q);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 w = *reinterpret_cast<const float4 *>(wrow + nt * 32 * kPitch + 8 * q);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc[nt], 0, 0, 0);
            }
        }
        tap = ntap;
        c0 = nc0;
    }

    // epilogue: accumulator register e of lane (r, h) is frame (e & 3) + 8 * (e >> 2) + 4 * h, column r
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + nt * 32 + r;
        if (col >= p.N) continue;
        const float bv = p.bias ? p.bias[col % p.bias_n] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int u = u0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (u >= p.L) continue;
            const size_t o = (row0 + u) * p.ldc + col;
            float v = acc[nt][e] + bv;
            if (p.res) v += p.res[o];
            if (p.C) p.C[o] = v;
            if (p.acc_mode == MTTS_VOC_ACC_INIT) p.acc[o] = v;
            else if (p.acc_mode == MTTS_VOC_ACC_ADD) p.acc[o] = p.acc[o] + v;
            else if (p.acc_mode == MTTS_VOC_ACC_MEAN) p.acc[o] = (p.acc[o] + v) / p.acc_div;
        }
    }
}

// [B, C, T] channel-major -> [B*T, C] token-major, 32 x 32 tiles through LDS
__global__ __launch_bounds__(kThreads) void voc_transpose_kernel(const float *__restrict__ x, int C, int T,
                                                                  float *__restrict__ y) {
    __shared__ float s[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, t = t0 + tx;
        if (c < C && t < T) s[i][tx] = x[((size_t)b * C + c) * T + t];
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, c = c0 + tx;
        if (c < C && t < T) y[((size_t)b * T + t) * C + c] = s[tx][i];
    }
}

// conv_post: one thread per output sample; rows u-3 .. u+3 of a token-major input are one contiguous run
__global__ __launch_bounds__(kThreads) void voc_post_kernel(const float *__restrict__ A, const float *__restrict__ w,
                                                             const float *__restrict__ bias, float *__restrict__ out,
                                                             long long rows, int L, int C, float slope) {
    extern __shared__ float sw[];  // [7 * C]
    for (int i = threadIdx.x; i < 7 * C; i += kThreads) sw[i] = w[i];
    __syncthreads();
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= rows) return;
    const int u = (int)(row % L);
    float sum = 0.f;
    for (int j = 0; j < 7; ++j) {
        const int uu = u + j - 3;
        if (uu < 0 || uu >= L) continue;  // zero padding inside the utterance
        const float4 *a = reinterpret_cast<const float4 *>(A + (size_t)(row + j - 3) * C);
        const float *wj = sw + j * C;
        for (int c = 0; c < C / 4; ++c) {
            const float4 v = a[c];
            sum = fmaf(lrelu(v.x, slope), wj[4 * c], sum);
            sum = fmaf(lrelu(v.y, slope), wj[4 * c + 1], sum);
            sum = fmaf(lrelu(v.z, slope), wj[4 * c + 2], sum);
            sum = fmaf(lrelu(v.w, slope), wj[4 * c + 3], sum);
        }
    }
    out[row] = tanhf(sum + (bias ? bias[0] : 0.f));
}

bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

bool aligned16(const void *q) { return ((uintptr_t)q & 15) == 0; }

// The shared launch: ntaps taps at rows u + off0 + j*d, N columns of a C with row stride ldc.
int launch_conv(VocP p, int B, hipStream_t st) {
    p.tilesL = (p.L + kBM - 1) / kBM;
    p.tps = 1;
    while (p.tps < p.ntaps && kBM + (long long)p.tps * p.d <= kWinMax) ++p.tps;
    const long long gx = (long long)B * p.tilesL;
    if (gx > 0x7fffffffLL) return mtts::fail(MTTS_ERR_SHAPE, "mtts_voc_conv: too many row tiles");
    // the widest column tile that still gives every CU a workgroup (256 CUs); A comes from L2 for the others
    int bn = p.N <= 32 ? 32 : p.N <= 64 ? 64 : 128;
    while (bn > 32 && gx * ((p.N + bn - 1) / bn) < 256) bn >>= 1;
    const dim3 grid((unsigned)gx, (unsigned)((p.N + bn - 1) / bn));
    if (bn == 128) hipLaunchKernelGGL(voc_conv_kernel<128>, grid, dim3(kThreads), 0, st, p);
    else if (bn == 64) hipLaunchKernelGGL(voc_conv_kernel<64>, grid, dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL(voc_conv_kernel<32>, grid, dim3(kThreads), 0, st, p);
    return mtts::check_launch("voc_conv_kernel");
}

int check_dims(const char *who, long long B, long long L, int cin, int N) {
    if (B < 0 || L < 0 || cin <= 0 || N <= 0) {
        mtts::set_error("%s: bad size", who);
        return MTTS_ERR_INVALID_ARG;
    }
    if (cin % 8 || N % 8 || B * L >= (1ll << 31)) {
        mtts::set_error("%s: channels must be multiples of 8 and B*L < 2^31 (cin %d, N %d, rows %lld)", who, cin, N,
                        B * L);
        return MTTS_ERR_SHAPE;
    }
    return MTTS_OK;
}

}  // namespace

extern "C" int mtts_voc_conv(const mtts_voc_conv_args *a, void *hip_stream) {
    MTTS_CHECK_ARG(a != nullptr, "mtts_voc_conv: null args");
    if (int rc = check_dims("mtts_voc_conv", a->B, a->L, a->cin, a->N)) return rc;
    if (a->k < 1 || a->k > MTTS_VOC_MAX_TAPS || a->k % 2 == 0 || a->d < 1 || a->d >= (1 << 24))
        return mtts::fail(MTTS_ERR_SHAPE, "mtts_voc_conv: k must be odd and <= 11, 1 <= d < 2^24");
    MTTS_CHECK_ARG(a->acc_mode >= MTTS_VOC_ACC_NONE && a->acc_mode <= MTTS_VOC_ACC_MEAN, "mtts_voc_conv: bad acc_mode");
    if ((long long)a->B * a->L == 0) return MTTS_OK;
    MTTS_CHECK_ARG(a->A && a->W, "mtts_voc_conv: null A or W");
    MTTS_CHECK_ARG(a->C || a->acc_mode != MTTS_VOC_ACC_NONE, "mtts_voc_conv: neither C nor acc to write");
    MTTS_CHECK_ARG(a->acc || a->acc_mode == MTTS_VOC_ACC_NONE, "mtts_voc_conv: acc_mode without acc");
    MTTS_CHECK_ARG(a->acc_mode != MTTS_VOC_ACC_MEAN || a->acc_div != 0.f, "mtts_voc_conv: acc_div is zero");
    MTTS_CHECK_ARG(aligned16(a->A) && aligned16(a->W), "mtts_voc_conv: A and W must be 16-byte aligned");
    const size_t rows = (size_t)a->B * a->L, na = rows * a->cin * sizeof(float), nc = rows * a->N * sizeof(float);
    MTTS_CHECK_ARG(!overlaps(a->A, na, a->C, nc), "mtts_voc_conv: C overlaps A");
    MTTS_CHECK_ARG(a->acc_mode == MTTS_VOC_ACC_NONE || !overlaps(a->A, na, a->acc, nc),
                   "mtts_voc_conv: acc overlaps A");
    MTTS_CHECK_ARG(a->acc_mode == MTTS_VOC_ACC_NONE || !overlaps(a->C, nc, a->acc, nc),
                   "mtts_voc_conv: acc overlaps C");
    VocP p{};
    p.A = a->A; p.W = a->W; p.bias = a->bias; p.res = a->residual; p.C = a->C;
    p.acc = a->acc_mode == MTTS_VOC_ACC_NONE ? nullptr : a->acc;
    p.L = a->L; p.cin = a->cin; p.N = a->N; p.ntaps = a->k; p.off0 = -((a->k - 1) / 2) * a->d; p.d = a->d;
    p.ldw = a->k * a->cin; p.ldc = a->N; p.bias_n = a->N;
    p.leaky = a->leaky != 0; p.slope = a->slope; p.acc_mode = a->acc_mode; p.acc_div = a->acc_div;
    return launch_conv(p, a->B, (hipStream_t)hip_stream);
}

extern "C" int mtts_voc_upsample(const float *A, const float *Wp, const float *bias, float *C, int32_t B, int32_t L,
                                 int32_t cin, int32_t cout, int32_t k, int32_t u, float slope, void *hip_stream) {
    if (int rc = check_dims("mtts_voc_upsample", B, L, cin, cout)) return rc;
    if (u < 2 || u % 2 || k != 2 * u || (long long)B * L * u >= (1ll << 31))
        return mtts::fail(MTTS_ERR_SHAPE, "mtts_voc_upsample: needs k == 2u, u even and B*L*u < 2^31");
    if ((long long)B * L == 0) return MTTS_OK;
    MTTS_CHECK_ARG(A && Wp && C, "mtts_voc_upsample: null pointer");
    MTTS_CHECK_ARG(aligned16(A) && aligned16(Wp), "mtts_voc_upsample: A and Wp must be 16-byte aligned");
    const size_t rows = (size_t)B * L;
    MTTS_CHECK_ARG(!overlaps(A, rows * cin * sizeof(float), C, rows * u * cout * sizeof(float)),
                   "mtts_voc_upsample: C overlaps A");
    const int half = (u / 2) * cout;
    VocP p{};
    p.A = A; p.bias = bias; p.L = L; p.cin = cin; p.N = half; p.ntaps = 2; p.d = 1;
    p.ldw = 2 * cin; p.ldc = u * cout; p.bias_n = cout;  // half is a multiple of cout: bias[col % cout]
    p.leaky = 1; p.slope = slope; p.acc_mode = MTTS_VOC_ACC_NONE;
    p.W = Wp; p.C = C; p.off0 = -1;  // phases p < u/2: frames (t-1, t)
    if (int rc = launch_conv(p, B, (hipStream_t)hip_stream)) return rc;
    p.W = Wp + (size_t)half * 2 * cin; p.C = C + half; p.off0 = 0;  // phases p >= u/2: frames (t, t+1)
    return launch_conv(p, B, (hipStream_t)hip_stream);
}

extern "C" size_t mtts_voc_pre_workspace_size(int32_t B, int32_t T, int32_t cin) {
    if (B <= 0 || T <= 0 || cin <= 0) return 0;
    return (size_t)B * T * cin * sizeof(float);
}

extern "C" int mtts_voc_pre(const float *mel, const float *W, const float *bias, float *C, int32_t B, int32_t T,
                            int32_t cin, int32_t N, void *workspace, size_t workspace_bytes, void *hip_stream) {
    if (int rc = check_dims("mtts_voc_pre", B, T, cin, N)) return rc;
    if ((long long)B * T == 0) return MTTS_OK;
    if (B > 65535) return mtts::fail(MTTS_ERR_SHAPE, "mtts_voc_pre: B > 65535");
    MTTS_CHECK_ARG(mel && W && C, "mtts_voc_pre: null pointer");
    MTTS_CHECK_ARG(aligned16(W) && aligned16(workspace), "mtts_voc_pre: W and the workspace must be 16-byte aligned");
    if (!workspace || workspace_bytes < mtts_voc_pre_workspace_size(B, T, cin))
        return mtts::fail(MTTS_ERR_WORKSPACE, "mtts_voc_pre: workspace too small");
    MTTS_CHECK_ARG(!overlaps(workspace, workspace_bytes, C, (size_t)B * T * N * sizeof(float)),
                   "mtts_voc_pre: C overlaps the workspace");
    hipStream_t st = (hipStream_t)hip_stream;
    float *tm = static_cast<float *>(workspace);
    hipLaunchKernelGGL(voc_transpose_kernel, dim3((T + 31) / 32, (cin + 31) / 32, B), dim3(kThreads), 0, st, mel, cin,
                       T, tm);
    if (int rc = mtts::check_launch("voc_transpose_kernel")) return rc;
    VocP p{};
    p.A = tm; p.W = W; p.bias = bias; p.C = C;
    p.L = T; p.cin = cin; p.N = N; p.ntaps = 7; p.off0 = -3; p.d = 1;
    p.ldw = 7 * cin; p.ldc = N; p.bias_n = N;
    p.acc_mode = MTTS_VOC_ACC_NONE;
    return launch_conv(p, B, st);
}

extern "C" int mtts_voc_post(const float *A, const float *w, const float *bias, float *out, int32_t B, int32_t L,
                             int32_t C, float slope, void *hip_stream) {
    if (B < 0 || L < 0 || C <= 0) return mtts::fail(MTTS_ERR_INVALID_ARG, "mtts_voc_post: bad size");
    if (C % 4 || C > 512 || (long long)B * L >= (1ll << 31))
        return mtts::fail(MTTS_ERR_SHAPE, "mtts_voc_post: needs C % 4 == 0, C <= 512 and B*L < 2^31");
    const long long rows = (long long)B * L;
    if (rows == 0) return MTTS_OK;
    MTTS_CHECK_ARG(A && w && out, "mtts_voc_post: null pointer");
    MTTS_CHECK_ARG(aligned16(A), "mtts_voc_post: A must be 16-byte aligned");
    hipLaunchKernelGGL(voc_post_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads),
                       (size_t)7 * C * sizeof(float), (hipStream_t)hip_stream, A, w, bias, out, rows, L, C, slope);
    return mtts::check_launch("voc_post_kernel");
}
