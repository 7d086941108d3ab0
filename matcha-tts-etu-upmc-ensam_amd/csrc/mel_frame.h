// Index arithmetic and per-lane steps of the fused mel front end (mel_fused.hip): which frames an utterance has,
// which sample of it a position of its reflect-padded signal reads, when a frame may be loaded with wide loads,
// and the magnitude / projection / log steps that follow the FFT of gl_fft.h.  Everything here is
// __host__ __device__ so that tools/mel_frame_host_check.cpp drives the same functions lane by lane on the host.
//
// Geometry (fixed, the reference's MelSpectrogram with center=False): n_fft = win = 1024, hop = 256, a manual reflect
// pad of (1024 - 256) / 2 = 384 samples on each side.  Frame f covers the padded positions 256 f .. 256 f + 1023.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gl_fft.h"

namespace mtts {
namespace melf {

constexpr int kPad = (gl::kNfft - gl::kHop) / 2;  // 384
constexpr int kMinLen = kPad + 1;                 // the shortest waveform a reflect pad by 384 accepts
constexpr int kFreq = gl::kBins;                  // 513 rows of the mel basis

// samples of row b that count: lengths may hold anything
MTTS_GL_HD int clamp_len(int len, int L) { return len < 0 ? 0 : (len > L ? L : len); }

// frames of an utterance of `len` (clamped) samples: (len + 768 - 1024) / 256 + 1 = len / 256; none below 385
MTTS_GL_HD int frame_count(int len) { return len >= kMinLen ? len / gl::kHop : 0; }

// Padded position p -> the sample of the utterance it reads.  s = p - 384; s < 0 reflects to -s, s >= len to
// 2 (len - 1) - s.  For len >= 385 and a frame f < frame_count(len), p <= 256 (len / 256) + 767 <= len + 767, so
// -s <= 384 < len and s <= len + 383 gives 2 (len - 1) - s >= len - 385 >= 0: one reflection always lands inside
// [0, len), and no sample outside the utterance is ever read.
MTTS_GL_HD int reflect_src(int p, int len) {
    int s = p - kPad;
    s = s < 0 ? -s : s;
    return s >= len ? 2 * (len - 1) - s : s;
}

// frame f reads 1024 consecutive samples of the utterance, none reflected
MTTS_GL_HD bool frame_interior(int f, int len) {
    const int s0 = gl::kHop * f - kPad;
    return s0 >= 0 && s0 + gl::kNfft <= len;
}

// The wide-load fast path: an interior frame whose first sample sits on a boundary of two samples (8 bytes for fp32,
// 4 for int16).  Row starts need not be aligned (L may be odd), so the address itself is tested.
template <class T>
MTTS_GL_HD bool wide_ok(const T *row, int f, int len) {
    return frame_interior(f, len) && (reinterpret_cast<uintptr_t>(row + (gl::kHop * f - kPad)) % (2 * sizeof(T))) == 0;
}

MTTS_GL_HD float to_float(float s) { return s; }
MTTS_GL_HD float to_float(int16_t s) { return (float)s * (1.0f / 32768.0f); }  // exact: float(s) / 32768

template <class T>
struct Pair;
template <>
struct Pair<float> {
    typedef float2 type;
};
template <>
struct Pair<int16_t> {
    typedef short2 type;
};

// samples 2 n and 2 n + 1 of frame f (before the window): point n of z[n] = x[2n] + i x[2n+1]
template <class T>
MTTS_GL_HD float2 load_pair(const T *row, int f, int len, int n, bool wide) {
    const int p = gl::kHop * f + 2 * n;
    if (wide) {
        const typename Pair<T>::type v = *reinterpret_cast<const typename Pair<T>::type *>(row + (p - kPad));
        return make_float2(to_float(v.x), to_float(v.y));
    }
    return make_float2(to_float(row[reflect_src(p, len)]), to_float(row[reflect_src(p + 1, len)]));
}

MTTS_GL_HD float magnitude(float2 x) { return sqrtf(x.x * x.x + x.y * x.y + 1e-9f); }

// sum_{k in [lo, hi)} w[k] * mag[k], ascending k (the order of mtts_mel_log_fwd); the band is cut to the basis' rows
MTTS_GL_HD float project(const float *w, const float *mag, int lo, int hi) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > kFreq ? kFreq : hi;
    float acc = 0.f;
    int k = lo;
    for (; k + 4 <= hi; k += 4) {  // four weight loads in flight; the sum keeps its order
        const float w0 = w[k], w1 = w[k + 1], w2 = w[k + 2], w3 = w[k + 3];
        acc = fmaf(w0, mag[k], acc);
        acc = fmaf(w1, mag[k + 1], acc);
        acc = fmaf(w2, mag[k + 2], acc);
        acc = fmaf(w3, mag[k + 3], acc);
    }
    for (; k < hi; ++k) acc = fmaf(w[k], mag[k], acc);
    return acc;
}

// a true division: mean = 0, std = 1 change no bit
MTTS_GL_HD float log_norm(float acc, float clip_val, float mean, float std) {
    return (logf(fmaxf(acc, clip_val)) - mean) / std;
}

}  // namespace melf
}  // namespace mtts
