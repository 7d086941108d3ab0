// Griffin-Lim on gfx950: mel -> linear magnitude -> waveform without a vocoder checkpoint (include/mtts_griffinlim.h;
// restates torchaudio.transforms.InverseMelScale and torchaudio.functional.griffinlim as the reference's generate.py
// configures them: n_fft = win_length = 1024, hop 256).
//
// Three kernels, all plain fp32, no atomics, a fixed summation order (two runs are bitwise equal):
//
//   inverse_mel_kernel  lin = relu(pinv(M) @ exp(mel)) ** (1/power).  A workgroup (4 waves) owns 64 frames x 64
//       spectrum rows; exp(mel) of its frames and its pinv rows are staged in LDS with every load in flight at once
//       (walking the 80 mel channels with one global load each took 104 us, all latency); lanes are frames, each
//       thread keeps 16 rows and reads their pinv entries as 16-byte LDS broadcasts.  Only the first n_rows rows
//       (the bins the mel filters reach) are computed; the rest are written as zeros.  It can write frame-major
//       [B, F, 513] through an LDS transpose: the layout the two kernels below read with lanes along the bins.
//
//   synthesis_kernel    one wave per frame, 4 frames per workgroup.  Prologue: the phase update
//       ang = reb - m * tprev; ang /= |ang| + 1e-16 and X = lin * ang, read from the frame-major spectra (lane = bin,
//       coalesced); merge to the 512-point complex spectrum; inverse FFT in LDS (gl_fft.h); times window / 512;
//       frames [B, F, 1024] written as one float2 per lane and point.
//
//   analysis_kernel     one wave per frame.  Each of the frame's 1024 samples is gathered from the at most four
//       windowed frames that cover it (ascending frame order), divided by the window envelope summed the same way,
//       with the reflect mapping of center=True at the edges; times window; forward FFT; split; reb written
//       frame-major.  The only ordering between the overlap-add and its readers is the kernel boundary.
//
//   gather_kernel       the final waveform: the same gather, one thread per sample, no FFT.
//
// The work is small (2.4 MB of frames and 5 MB of spectrum per iteration at 600 frames) and lives in L2; the design
// aim is two launches per iteration, not bandwidth.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "gl_fft.h"
#include "mtts_base.h"
#include "mtts_griffinlim.h"

namespace {

using namespace mtts::gl;

constexpr int kWaves = 4;  // frames per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kTile = 64;      // inverse mel: frames and rows per workgroup
constexpr int kRowsPerThread = kTile / kWaves;
constexpr int kPinvPitch = kTile + 4;  // floats per mel channel of the staged pinv rows (16-byte aligned rows of 64)
constexpr int kMaxMels = 96;           // 53 KiB of LDS

// dynamic LDS: sx [n_mels][64] (g(mel) of the tile's frames; reused as the [64][65] transpose tile), then
// sp [n_mels][kPinvPitch] (the tile's 64 pinv rows, transposed: a thread's 16 rows are four 16-byte broadcast reads)
__host__ __device__ inline int inverse_mel_sx_floats(int n_mels) {
    return n_mels * kTile > kTile * (kTile + 1) ? n_mels * kTile : kTile * (kTile + 1);
}

__global__ __launch_bounds__(kThreads) void inverse_mel_kernel(const float *__restrict__ mel,
                                                               const float *__restrict__ pinv, float *__restrict__ lin,
                                                               int n_mels, int n_stft, int n_rows, int F, int log_input,
                                                               float inv_power, int frame_major) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sx = smem;
    float *sp = smem + inverse_mel_sx_floats(n_mels);
    const int tx = threadIdx.x, ty = threadIdx.y, b = blockIdx.z;
    const int tid = ty * kTile + tx;
    const int f0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
    // every load of the tile is issued before the first use: the kernel is latency-bound otherwise
    const int n_stage = r0 < n_rows ? n_mels * kTile : 0;  // a tile of zero rows stages nothing
    for (int idx = tid; idx < n_stage; idx += kThreads) {
        const int m = idx / kTile, ff = idx % kTile;
        const float x = mel[((size_t)b * n_mels + m) * F + min(f0 + ff, F - 1)];
        sx[idx] = log_input ? expf(x) : x;
    }
    for (int idx = tid; idx < n_stage; idx += kThreads) {
        const int r = idx / n_mels, m = idx % n_mels;
        sp[m * kPinvPitch + r] = r0 + r < n_rows ? pinv[(size_t)r0 * n_mels + idx] : 0.f;
    }
    __syncthreads();
    float acc[kRowsPerThread];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) acc[i] = 0.f;
    if (r0 + ty * kRowsPerThread < n_rows) {  // wave-uniform
        for (int m = 0; m < n_mels; ++m) {
            const float x = sx[m * kTile + tx];
            const float4 *p4 = reinterpret_cast<const float4 *>(sp + m * kPinvPitch + ty * kRowsPerThread);
#pragma unroll
            for (int i = 0; i < kRowsPerThread / 4; ++i) {
                const float4 p = p4[i];
                acc[4 * i] = fmaf(p.x, x, acc[4 * i]);
                acc[4 * i + 1] = fmaf(p.y, x, acc[4 * i + 1]);
                acc[4 * i + 2] = fmaf(p.z, x, acc[4 * i + 2]);
                acc[4 * i + 3] = fmaf(p.w, x, acc[4 * i + 3]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        float v = fmaxf(acc[i], 0.f);
        if (inv_power != 1.f) v = powf(v, inv_power);
        acc[i] = v;
    }
    const int k0 = r0 + ty * kRowsPerThread;
    if (!frame_major) {
#pragma unroll
        for (int i = 0; i < kRowsPerThread; ++i)
            if (f0 + tx < F && k0 + i < n_stft) lin[((size_t)b * n_stft + k0 + i) * F + f0 + tx] = acc[i];
        return;
    }
    __syncthreads();  // sx is read no more: it becomes the transpose tile
    float *tile = sx;
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) tile[(ty * kRowsPerThread + i) * (kTile + 1) + tx] = acc[i];
    __syncthreads();
    const int k = r0 + tx;
    for (int ff = ty; ff < kTile; ff += kWaves) {
        const int fr = f0 + ff;
        if (fr < F && k < n_stft) lin[((size_t)b * F + fr) * n_stft + k] = tile[tx * (kTile + 1) + ff];
    }
}

// X[k] = lin[k] * ang[k] of one frame (row: its offset in the frame-major spectra)
__device__ __forceinline__ float2 phase_times_mag(const float *__restrict__ lin, const float2 *__restrict__ reb,
                                                  const float2 *__restrict__ tprev, float m, int normalize,
                                                  size_t row, int k) {
    float2 a = reb[row + k];
    if (tprev) {
        const float2 t = tprev[row + k];
        a.x -= m * t.x;
        a.y -= m * t.y;
    }
    if (normalize) {
        const float d = sqrtf(a.x * a.x + a.y * a.y) + 1e-16f;
        a.x /= d;
        a.y /= d;
    }
    const float g = lin[row + k];
    return make_float2(g * a.x, g * a.y);
}

__global__ __launch_bounds__(kThreads) void synthesis_kernel(const float *__restrict__ lin,
                                                             const float2 *__restrict__ reb,
                                                             const float2 *__restrict__ tprev, float m, int normalize,
                                                             const float2 *__restrict__ tw,
                                                             const float *__restrict__ window,
                                                             float2 *__restrict__ frames, long long total) {
    __shared__ float lds[kWaves][2][kPlane];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *re = lds[wave][0], *im = lds[wave][1];
    const long long frame = (long long)blockIdx.x * kWaves + wave;
    const bool live = frame < total;  // a dead wave repeats the last frame and stores nothing (uniform barriers)
    const size_t gf = (size_t)(live ? frame : total - 1);
    const size_t row = gf * kBins;

    // merge: lane k and its mirror 512 - k, k = lane + 64 c (0 .. 255), and k = 256 on lane 0
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const int k = lane + 64 * c;
        if (k > kHalf / 2) break;
        const float2 a = phase_times_mag(lin, reb, tprev, m, normalize, row, k);
        const float2 b = phase_times_mag(lin, reb, tprev, m, normalize, row, kHalf - k);
        float2 zk, zn;
        merge_inv(k, a, b, tw[k], zk, zn);
        lds_put(k, zk, re, im);
        if (k != 0 && k != kHalf / 2) lds_put(kHalf - k, zn, re, im);
    }
    __syncthreads();

    float2 v[8];
    lds_gather(v, lane, re, im);
    fft_pass<true, 1>(v, lane, tw);
    __syncthreads();
    lds_scatter<1>(v, lane, re, im);
    __syncthreads();
    lds_gather(v, lane, re, im);
    fft_pass<true, 8>(v, lane, tw);
    __syncthreads();
    lds_scatter<8>(v, lane, re, im);
    __syncthreads();
    lds_gather(v, lane, re, im);
    fft_pass<true, 64>(v, lane, tw);

    if (!live) return;
    const float2 *w2 = reinterpret_cast<const float2 *>(window);
    float2 *dst = frames + gf * kHalf;
    constexpr float s = 1.0f / kHalf;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = lane + 64 * r;
        const float2 w = w2[n];
        dst[n] = make_float2(v[r].x * s * w.x, v[r].y * s * w.y);
    }
}

// overlap-add value at position p of an utterance's untrimmed signal, divided by the window envelope there.
// Always four loads, issued together; a frame that does not cover p is the first one again, weighted zero.
__device__ __forceinline__ float ola_sample(const float *__restrict__ fr, const float *window, int F, int p) {
    int f_lo, f_hi;
    cover(p, F, f_lo, f_hi);
    float v[4], w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = f_lo + j <= f_hi;
        const int f = in ? f_lo + j : f_lo;
        const int o = p - kHop * f;
        const float x = fr[(size_t)f * kNfft + o], ww = window[o];
        v[j] = in ? x : 0.f;
        w[j] = in ? ww : 0.f;
    }
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        num += v[j];
        den = fmaf(w[j], w[j], den);
    }
    return num / den;
}

__global__ __launch_bounds__(kThreads) void analysis_kernel(const float *__restrict__ frames,
                                                            const float2 *__restrict__ tw,
                                                            const float *__restrict__ window,
                                                            float2 *__restrict__ reb, int F, long long total) {
    __shared__ float lds[kWaves][2][kPlane];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *re = lds[wave][0], *im = lds[wave][1];
    const long long frame = (long long)blockIdx.x * kWaves + wave;
    const bool live = frame < total;
    const size_t gf = (size_t)(live ? frame : total - 1);
    const int g = (int)(gf % (size_t)F);
    const float *fr = frames + (gf - g) * kNfft;  // the utterance's first frame
    __shared__ float swin[kNfft];
    for (int i = threadIdx.x; i < kNfft; i += kThreads) swin[i] = window[i];
    __syncthreads();

    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n = 2 * (lane + 64 * r);
        const int q = kHop * g + n;
        v[r].x = ola_sample(fr, swin, F, reflect_pos(q, F)) * swin[n];
        v[r].y = ola_sample(fr, swin, F, reflect_pos(q + 1, F)) * swin[n + 1];
    }
    fft_pass<false, 1>(v, lane, tw);
    lds_scatter<1>(v, lane, re, im);
    __syncthreads();
    lds_gather(v, lane, re, im);
    fft_pass<false, 8>(v, lane, tw);
    __syncthreads();
    lds_scatter<8>(v, lane, re, im);
    __syncthreads();
    lds_gather(v, lane, re, im);
    fft_pass<false, 64>(v, lane, tw);
    __syncthreads();
    lds_scatter<64>(v, lane, re, im);
    __syncthreads();

    if (!live) return;
    float2 *dst = reb + gf * kBins;
    for (int c = 0; c < 5; ++c) {
        const int k = lane + 64 * c;
        if (k > kHalf / 2) break;
        float2 xk, xn;
        split_fwd(lds_at(k, re, im), lds_at((kHalf - k) & (kHalf - 1), re, im), tw[k], xk, xn);
        dst[k] = xk;
        if (k != kHalf / 2) dst[kHalf - k] = xn;
    }
}

__global__ __launch_bounds__(kThreads) void gather_kernel(const float *__restrict__ frames,
                                                          const float *__restrict__ window, float *__restrict__ wav,
                                                          int F, int L) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (t >= L) return;
    wav[(size_t)b * L + t] = ola_sample(frames + (size_t)b * F * kNfft, window, F, t + kHalf);
}

inline bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

int check_stft_shape(const char *what, int32_t B, int32_t F, int32_t n_fft, int32_t hop) {
    if (B < 0 || F < 0 || n_fft <= 0 || hop <= 0) {
        mtts::set_error("%s: bad size", what);
        return MTTS_ERR_INVALID_ARG;
    }
    if (n_fft != kNfft || hop != kHop) {
        mtts::set_error("%s: only n_fft = 1024, hop = 256 (got %d, %d)", what, n_fft, hop);
        return MTTS_ERR_SHAPE;
    }
    if (B > 0 && F < 4) {
        mtts::set_error("%s: needs F >= 4 frames (reflect padding by 512 samples), got %d", what, F);
        return MTTS_ERR_SHAPE;
    }
    if (B > 65535 || (long long)B * F >= (1ll << 20)) {
        mtts::set_error("%s: needs B <= 65535 and B*F < 2^20", what);
        return MTTS_ERR_SHAPE;
    }
    return MTTS_OK;
}

}  // namespace

extern "C" int mtts_gl_inverse_mel(const float *mel, const float *pinv, float *lin, int32_t B, int32_t n_mels,
                                   int32_t n_stft, int32_t n_rows, int32_t F, int32_t log_input, float inv_power,
                                   int32_t frame_major, void *hip_stream) {
    if (B < 0 || F < 0 || n_mels <= 0 || n_stft <= 0 || n_rows < 0 || n_rows > n_stft || !(inv_power > 0.f))
        return mtts::fail(MTTS_ERR_INVALID_ARG, "mtts_gl_inverse_mel: bad size or power");
    if (B > 65535 || (long long)B * F >= (1ll << 20) || n_stft > (1 << 20) || n_mels > kMaxMels)
        return mtts::fail(MTTS_ERR_SHAPE, "mtts_gl_inverse_mel: needs B <= 65535, B*F < 2^20, n_stft <= 2^20, "
                                          "n_mels <= 96");
    if ((size_t)B * F == 0) return MTTS_OK;
    MTTS_CHECK_ARG(mel && pinv && lin, "mtts_gl_inverse_mel: null pointer");
    dim3 grid((unsigned)((F + kTile - 1) / kTile), (unsigned)((n_stft + kTile - 1) / kTile), (unsigned)B);
    const size_t lds = (size_t)(inverse_mel_sx_floats(n_mels) + n_mels * kPinvPitch) * sizeof(float);
    hipLaunchKernelGGL(inverse_mel_kernel, grid, dim3(64, kWaves), lds, static_cast<hipStream_t>(hip_stream), mel,
                       pinv, lin, n_mels, n_stft, n_rows, F, log_input != 0, inv_power, frame_major != 0);
    return mtts::check_launch("inverse_mel_kernel");
}

extern "C" int mtts_gl_synthesis(const float *lin, const float *reb, const float *tprev, float m, int32_t normalize,
                                 const float *twiddle, const float *window, float *frames, int32_t B, int32_t F,
                                 int32_t n_fft, int32_t hop, void *hip_stream) {
    if (int rc = check_stft_shape("mtts_gl_synthesis", B, F, n_fft, hop)) return rc;
    const long long total = (long long)B * F;
    if (total == 0) return MTTS_OK;
    MTTS_CHECK_ARG(lin && reb && twiddle && window && frames, "mtts_gl_synthesis: null pointer");
    MTTS_CHECK_ARG(aligned8(reb) && aligned8(tprev) && aligned8(twiddle) && aligned8(window) && aligned8(frames),
                   "mtts_gl_synthesis: reb, tprev, twiddle, window and frames must be 8-byte aligned");
    MTTS_CHECK_ARG((const void *)frames != (const void *)reb && (const void *)frames != (const void *)lin &&
                       (const void *)frames != (const void *)tprev,
                   "mtts_gl_synthesis: frames must not alias an input");
    hipLaunchKernelGGL(synthesis_kernel, dim3((unsigned)((total + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(hip_stream), lin, reinterpret_cast<const float2 *>(reb),
                       reinterpret_cast<const float2 *>(tprev), m, normalize != 0,
                       reinterpret_cast<const float2 *>(twiddle), window, reinterpret_cast<float2 *>(frames), total);
    return mtts::check_launch("synthesis_kernel");
}

extern "C" int mtts_gl_analysis(const float *frames, const float *twiddle, const float *window, float *reb,
                                float *wav, int32_t B, int32_t F, int32_t n_fft, int32_t hop, void *hip_stream) {
    if (int rc = check_stft_shape("mtts_gl_analysis", B, F, n_fft, hop)) return rc;
    const long long total = (long long)B * F;
    if (total == 0) return MTTS_OK;
    MTTS_CHECK_ARG(frames && window && (reb || wav), "mtts_gl_analysis: null pointer");
    MTTS_CHECK_ARG(!reb || twiddle, "mtts_gl_analysis: the spectrum needs the twiddle table");
    MTTS_CHECK_ARG(aligned8(reb) && aligned8(twiddle), "mtts_gl_analysis: reb and twiddle must be 8-byte aligned");
    MTTS_CHECK_ARG((const void *)reb != (const void *)frames && (const void *)wav != (const void *)frames,
                   "mtts_gl_analysis: an output must not alias frames");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (reb) {
        hipLaunchKernelGGL(analysis_kernel, dim3((unsigned)((total + kWaves - 1) / kWaves)), dim3(kThreads), 0, st,
                           frames, reinterpret_cast<const float2 *>(twiddle), window, reinterpret_cast<float2 *>(reb),
                           F, total);
        if (int rc = mtts::check_launch("analysis_kernel")) return rc;
    }
    if (wav) {
        const int L = (F - 1) * kHop;
        hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((L + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads),
                           0, st, frames, window, wav, F, L);
        if (int rc = mtts::check_launch("gather_kernel")) return rc;
    }
    return MTTS_OK;
}
