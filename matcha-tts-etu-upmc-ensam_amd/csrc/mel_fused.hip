// The mel front end on gfx950 in one launch: ragged waveform batch in, padded log-mel and frame counts out
// (include/mtts.h, mtts_mel_from_wav; reference: matcha/utils/audio_process.py:45-72 run per utterance, then
// ljspeech_datamodule.py:84-109 collate).  Plus mtts_mel_stats, the per-utterance float64 sums behind data_statistics.
//
// mel_from_wav_kernel<T>: a workgroup of 4 waves owns 8 consecutive frames of one utterance, a wave 2 of them in
// turn.  Per frame (one wave): lane j loads the points j + 64 r of z[n] = x[2n] + i x[2n+1] -- one 8-byte (fp32) or
// 4-byte (int16) load per point where the frame is interior and its first sample aligned, a scalar gather through
// the utterance's own reflect mapping otherwise (the choice is wave-uniform; mel_frame.h) -- times the Hann
// window; the radix-8 512-point FFT of gl_fft.h in the wave's LDS planes; the split to the 513 real-transform bins;
// their magnitudes sqrt(re^2 + im^2 + 1e-9) into the workgroup's [8][513] LDS tile.  Then the whole workgroup
// projects the tile: each group of 8 lanes is the 8 frames of one mel channel, so every weight load is shared by
// 8 lanes, their magnitude reads fall in 8 distinct banks (pitch 513 = 1 mod 32) and each store instruction writes
// 32-byte runs along f.  Neither the spectrum nor the magnitudes reach HBM.  35 KB of LDS and 114 VGPRs: four
// workgroups (16 waves) per CU.
//
// Frames at or past the utterance's count are written as pad_value; a workgroup wholly past it does only that.
// No sample outside [0, len) of a row is read whatever `lengths` holds (clamped; see reflect_src).  No atomics, a
// fixed summation order: two calls give equal bits, and a row's result does not depend on the rest of the batch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gl_fft.h"
#include "mel_frame.h"
#include "mtts_base.h"

namespace {

using namespace mtts::gl;
using namespace mtts::melf;

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kFramesPerWave = 2;  // 4 / 2 / 1 ran 58 / 44 / 42 us at B = 32 x 7 s; 2 keeps 32-byte output runs
constexpr int kTileFrames = kWaves * kFramesPerWave;  // 8
constexpr int kMelGroups = kThreads / kTileFrames;     // mel channels projected at once
constexpr int kMaxMels = 96;
constexpr int kStatsThreads = 256;

template <class T>
__global__ __launch_bounds__(kThreads) void mel_from_wav_kernel(
    const T *__restrict__ wav, const int32_t *__restrict__ lengths, const float *__restrict__ mel_w,
    const int32_t *__restrict__ band_lo, const int32_t *__restrict__ band_hi, const float2 *__restrict__ tw,
    const float2 *__restrict__ window, int L, int F_out, int n_mels, float clip_val, float mean, float std,
    float pad_value, float *__restrict__ out, int32_t *__restrict__ mel_lengths) {
    __shared__ float planes[kWaves][2][kPlane];
    __shared__ float mags[kTileFrames][kFreq];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int f0 = blockIdx.x * kTileFrames;
    const int len = clamp_len(lengths ? lengths[b] : L, L);
    const int Fb = frame_count(len);
    if (blockIdx.x == 0 && threadIdx.x == 0) mel_lengths[b] = Fb;

    const int fl = threadIdx.x & (kTileFrames - 1), mg = threadIdx.x / kTileFrames;
    const int fo = f0 + fl;
    float *dst = out + (size_t)b * n_mels * F_out + fo;
    if (f0 >= Fb) {  // workgroup-uniform: nothing but padding here
        if (fo < F_out)
            for (int m = mg; m < n_mels; m += kMelGroups) dst[(size_t)m * F_out] = pad_value;
        return;
    }

    const T *row = wav + (size_t)b * L;
    float *re = planes[wave][0], *im = planes[wave][1];
    for (int i = 0; i < kFramesPerWave; ++i) {
        const int t = wave * kFramesPerWave + i;
        const int f = f0 + t;
        const bool live = f < Fb;  // wave-uniform; a dead wave only keeps the barriers
        float2 v[8];
        if (live) {
            const bool wide = wide_ok(row, f, len);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int n = lane + 64 * r;
                const float2 x = load_pair(row, f, len, n, wide);
                const float2 w = window[n];
                v[r] = make_float2(x.x * w.x, x.y * w.y);
            }
            fft_pass<false, 1>(v, lane, tw);
            lds_scatter<1>(v, lane, re, im);  // the planes were last read before the barrier that ended frame i - 1
        }
        __syncthreads();
        if (live) {
            lds_gather(v, lane, re, im);
            fft_pass<false, 8>(v, lane, tw);
        }
        __syncthreads();
        if (live) lds_scatter<8>(v, lane, re, im);
        __syncthreads();
        if (live) {
            lds_gather(v, lane, re, im);
            fft_pass<false, 64>(v, lane, tw);
        }
        __syncthreads();
        if (live) lds_scatter<64>(v, lane, re, im);
        __syncthreads();
        if (live) {
            float *mg_t = mags[t];
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                const int k = lane + 64 * c;
                if (k > kHalf / 2) break;
                float2 xk, xn;
                split_fwd(lds_at(k, re, im), lds_at((kHalf - k) & (kHalf - 1), re, im), tw[k], xk, xn);
                mg_t[k] = magnitude(xk);
                if (k != kHalf / 2) mg_t[kHalf - k] = magnitude(xn);
            }
        }
        __syncthreads();
    }

    if (fo >= F_out) return;
    const bool valid = fo < Fb;
    for (int m = mg; m < n_mels; m += kMelGroups) {
        float val = pad_value;
        if (valid)
            val = log_norm(project(mel_w + (size_t)m * kFreq, mags[fl], band_lo[m], band_hi[m]), clip_val, mean, std);
        dst[(size_t)m * F_out] = val;
    }
}

// (sum v, sum v^2) in float64 over out[b, :, :mel_lengths[b]]: one workgroup per utterance, each thread its strided
// share in ascending order, then a fixed tree over the 256 partial sums
__global__ __launch_bounds__(kStatsThreads) void mel_stats_kernel(const float *__restrict__ mel,
                                                                  const int32_t *__restrict__ mel_lengths, int n_mels,
                                                                  int F, double *__restrict__ stats) {
    __shared__ double s1[kStatsThreads], s2[kStatsThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    int Fb = mel_lengths[b];
    Fb = Fb < 0 ? 0 : (Fb > F ? F : Fb);
    const float *src = mel + (size_t)b * n_mels * F;
    double a1 = 0.0, a2 = 0.0;
    for (int m = 0; m < n_mels; ++m)
        for (int f = tid; f < Fb; f += kStatsThreads) {
            const double v = (double)src[(size_t)m * F + f];
            a1 += v;
            a2 += v * v;
        }
    s1[tid] = a1;
    s2[tid] = a2;
    __syncthreads();
    for (int h = kStatsThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s1[tid] += s1[tid + h];
            s2[tid] += s2[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[2 * (size_t)b] = s1[0];
        stats[2 * (size_t)b + 1] = s2[0];
    }
}

inline bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

extern "C" int mtts_mel_from_wav(const void *wav, int32_t wav_is_int16, const int32_t *lengths, const float *mel_w,
                                 const int32_t *band_lo, const int32_t *band_hi, const float *twiddle,
                                 const float *window, int32_t B, int32_t L, int32_t n_fft, int32_t win_size,
                                 int32_t hop, int32_t n_mels, float clip_val, float mean, float std, float pad_value,
                                 float *out, int32_t *mel_lengths, void *hip_stream) {
    MTTS_CHECK_ARG(B >= 0 && L >= 0 && n_fft > 0 && win_size > 0 && hop > 0 && n_mels >= 1 && clip_val > 0.f &&
                       std != 0.f && std == std && mean == mean,
                   "mtts_mel_from_wav: bad size, clip_val, mean or std");
    if (n_fft != kNfft || win_size != kNfft || hop != kHop) {
        mtts::set_error("mtts_mel_from_wav: only n_fft = win_size = 1024, hop = 256 (got %d, %d, %d)", n_fft, win_size,
                        hop);
        return MTTS_ERR_SHAPE;
    }
    if (B > 65535 || n_mels > kMaxMels || L > (1 << 30))  // padded positions stay far inside int32
        return mtts::fail(MTTS_ERR_SHAPE, "mtts_mel_from_wav: needs B <= 65535, n_mels <= 96 and L <= 2^30");
    if (B == 0) return MTTS_OK;
    const int F_out = L / kHop;
    // an empty tensor's pointer may be null: wav is not read at L = 0, out not written at F_out = 0
    MTTS_CHECK_ARG((wav || L == 0) && mel_w && band_lo && band_hi && twiddle && window && (out || F_out == 0) &&
                       mel_lengths,
                   "mtts_mel_from_wav: null pointer");
    MTTS_CHECK_ARG(aligned_to(twiddle, 8) && aligned_to(window, 8) && aligned_to(wav, wav_is_int16 ? 2 : 4),
                   "mtts_mel_from_wav: twiddle and window must be 8-byte aligned, wav aligned to its sample type");
    // F_out == 0 still launches one workgroup per row: it writes mel_lengths (all zero) and nothing else
    dim3 grid((unsigned)((F_out + kTileFrames - 1) / kTileFrames > 0 ? (F_out + kTileFrames - 1) / kTileFrames : 1),
              (unsigned)B);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const float2 *tw2 = reinterpret_cast<const float2 *>(twiddle), *win2 = reinterpret_cast<const float2 *>(window);
    if (wav_is_int16)
        hipLaunchKernelGGL(mel_from_wav_kernel<int16_t>, grid, dim3(kThreads), 0, st,
                           static_cast<const int16_t *>(wav), lengths, mel_w, band_lo, band_hi, tw2, win2, L, F_out,
                           n_mels, clip_val, mean, std, pad_value, out, mel_lengths);
    else
        hipLaunchKernelGGL(mel_from_wav_kernel<float>, grid, dim3(kThreads), 0, st, static_cast<const float *>(wav),
                           lengths, mel_w, band_lo, band_hi, tw2, win2, L, F_out, n_mels, clip_val, mean, std,
                           pad_value, out, mel_lengths);
    return mtts::check_launch("mel_from_wav_kernel");
}

extern "C" int mtts_mel_stats(const float *mel, const int32_t *mel_lengths, int32_t B, int32_t n_mels, int32_t F,
                              double *stats, void *hip_stream) {
    MTTS_CHECK_ARG(B >= 0 && n_mels >= 1 && F >= 0, "mtts_mel_stats: bad size");
    if (B == 0) return MTTS_OK;
    MTTS_CHECK_ARG(mel_lengths && stats && (mel || F == 0), "mtts_mel_stats: null pointer");
    MTTS_CHECK_ARG(aligned_to(stats, 8), "mtts_mel_stats: stats must be 8-byte aligned");
    hipLaunchKernelGGL(mel_stats_kernel, dim3((unsigned)B), dim3(kStatsThreads), 0, static_cast<hipStream_t>(hip_stream),
                       mel, mel_lengths, n_mels, F, stats);
    return mtts::check_launch("mel_stats_kernel");
}
