// Building blocks of the Griffin-Lim kernels (griffinlim.hip): the 1024-point real transform as a 512-point
// complex FFT plus a split / merge pass, and the index arithmetic of the overlap-add gather.  Everything here is
// __host__ __device__ so that the same functions can be driven lane by lane from a host program.
//
// FFT: Stockham autosort, radix 8, three passes (Ns = 1, 8, 64).  One wave owns one frame; lane j holds the
// eight points j + 64 r.  Pass Ns multiplies point r by exp(-+2 pi i r (j mod Ns) / (8 Ns)), takes an 8-point
// DFT in registers and scatters point r to (j / Ns) * 8 Ns + (j mod Ns) + r Ns; the next pass reads j + 64 r
// again.  After the third pass lane j holds the outputs j + 64 r in natural order.
//
// LDS image of a frame: separate re[] and im[] planes (ds_read_b32 / ds_write_b32: a wave is served in two
// groups of 32 lanes over 32 banks), element a at a + (a >> 3).  The scatter of pass 1 has a lane stride of
// 8 elements and that of pass 2 runs 8 consecutive elements per 64; the pad makes them 9 and 72 dwords, so the
// 32 lanes of a group hit 32 distinct banks in both.  The strided read j + 64 r becomes j + (j >> 3) + 72 r:
// 35 consecutive dwords per group, i.e. three banks are hit twice (one extra LDS cycle per read).
#pragma once

#include <hip/hip_runtime.h>

namespace mtts {
namespace gl {

constexpr int kNfft = 1024;
constexpr int kHop = 256;
constexpr int kHalf = kNfft / 2;      // points of the complex FFT
constexpr int kBins = kNfft / 2 + 1;  // one-sided spectrum
constexpr int kPlane = kHalf + kHalf / 8;  // padded floats per LDS plane

#define MTTS_GL_HD __host__ __device__ __forceinline__

MTTS_GL_HD int lds_pad(int a) { return a + (a >> 3); }

MTTS_GL_HD float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
MTTS_GL_HD float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
MTTS_GL_HD float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
MTTS_GL_HD float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
MTTS_GL_HD float2 cscale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }

// a * w (forward) or a * conj(w) (inverse); w = exp(-2 pi i k / 1024) from the table
template <bool INV>
MTTS_GL_HD float2 mul_tw(float2 a, float2 w) {
    return cmul(a, INV ? cconj(w) : w);
}

// a * (-i) (forward) or a * (+i) (inverse)
template <bool INV>
MTTS_GL_HD float2 rot4(float2 a) {
    return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x);
}

// a * exp(-+ 2 pi i / 8)
template <bool INV>
MTTS_GL_HD float2 rot8(float2 a) {
    constexpr float c = 0.70710678118654752440f;
    return INV ? make_float2(c * (a.x - a.y), c * (a.x + a.y)) : make_float2(c * (a.x + a.y), c * (a.y - a.x));
}

// 8-point DFT in place, natural order in and out (decimation in time: two 4-point DFTs of the even and odd points)
template <bool INV>
MTTS_GL_HD void dft8(float2 (&v)[8]) {
    const float2 e0 = cadd(v[0], v[4]), e1 = csub(v[0], v[4]), e2 = cadd(v[2], v[6]), e3 = rot4<INV>(csub(v[2], v[6]));
    const float2 o0 = cadd(v[1], v[5]), o1 = csub(v[1], v[5]), o2 = cadd(v[3], v[7]), o3 = rot4<INV>(csub(v[3], v[7]));
    const float2 E0 = cadd(e0, e2), E1 = cadd(e1, e3), E2 = csub(e0, e2), E3 = csub(e1, e3);
    const float2 O0 = cadd(o0, o2);
    const float2 O1 = rot8<INV>(cadd(o1, o3));
    const float2 O2 = rot4<INV>(csub(o0, o2));
    const float2 O3 = rot4<INV>(rot8<INV>(csub(o1, o3)));
    v[0] = cadd(E0, O0); v[4] = csub(E0, O0);
    v[1] = cadd(E1, O1); v[5] = csub(E1, O1);
    v[2] = cadd(E2, O2); v[6] = csub(E2, O2);
    v[3] = cadd(E3, O3); v[7] = csub(E3, O3);
}

// One radix-8 pass on the eight points of lane j: twiddle, then the 8-point DFT.  tw: the 1024-entry table.
template <bool INV, int NS>
MTTS_GL_HD void fft_pass(float2 (&v)[8], int j, const float2 *tw) {
    if (NS > 1) {
        const int base = (j & (NS - 1)) * (128 / NS);  // r * base <= 7 * 63 * 2 = 882 < 1024
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = mul_tw<INV>(v[r], tw[r * base]);
    }
    dft8<INV>(v);
}

// the scatter that follows pass NS; NS = 64 stores lane j's natural-order outputs j + 64 r
template <int NS>
MTTS_GL_HD void lds_scatter(const float2 (&v)[8], int j, float *re, float *im) {
    const int base = (j / NS) * (NS * 8) + (j & (NS - 1));
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int a = lds_pad(base + r * NS);
        re[a] = v[r].x;
        im[a] = v[r].y;
    }
}

MTTS_GL_HD void lds_gather(float2 (&v)[8], int j, const float *re, const float *im) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int a = lds_pad(j + 64 * r);
        v[r] = make_float2(re[a], im[a]);
    }
}

MTTS_GL_HD float2 lds_at(int k, const float *re, const float *im) {
    const int a = lds_pad(k);
    return make_float2(re[a], im[a]);
}

MTTS_GL_HD void lds_put(int k, float2 z, float *re, float *im) {
    const int a = lds_pad(k);
    re[a] = z.x;
    im[a] = z.y;
}

// Forward split.  Z = FFT512(x[2n] + i x[2n+1]); zk = Z[k], zn = Z[(512 - k) mod 512], w = exp(-2 pi i k / 1024).
// Gives X[k] and X[512 - k] of the 1024-point transform of the real x, for 0 <= k <= 256.
MTTS_GL_HD void split_fwd(float2 zk, float2 zn, float2 w, float2 &xk, float2 &xn) {
    const float2 e = cscale(cadd(zk, cconj(zn)), 0.5f);
    const float2 d = cscale(csub(zk, cconj(zn)), 0.5f);
    const float2 t = cmul(make_float2(d.y, -d.x), w);  // W^k * O[k],  O = -i d
    xk = cadd(e, t);
    xn = cconj(csub(e, t));
}

// Inverse merge.  a = X[k], b = X[512 - k] (Hermitian half spectrum), w as above.  Gives Z[k] and Z[512 - k] with
// IFFT512(Z)[n] = 512 * (x[2n] + i x[2n+1]) of the inverse real transform x (unnormalised by 512: the caller
// folds 1/512 into the window).  At k = 0 the imaginary parts of X[0] and X[512] are dropped, as a
// complex-to-real transform does.
MTTS_GL_HD void merge_inv(int k, float2 a, float2 b, float2 w, float2 &zk, float2 &zn) {
    if (k == 0) a.y = 0.f, b.y = 0.f;
    const float2 bc = cconj(b);
    const float2 e = cscale(cadd(a, bc), 0.5f);
    const float2 o = cmul(cscale(csub(a, bc), 0.5f), cconj(w));
    zk = make_float2(e.x - o.y, e.y + o.x);   // E + i O
    zn = make_float2(e.x + o.y, o.x - e.y);   // conj(E) + i conj(O)
}

// Overlap-add geometry.  The istft signal before trimming has (F - 1) * 256 + 1024 samples; position p is
// covered by frames f_lo .. f_hi (at most four), frame f contributing its sample p - 256 f.
MTTS_GL_HD void cover(int p, int F, int &f_lo, int &f_hi) {
    f_lo = p >= kNfft ? (p - (kNfft - kHop)) >> 8 : 0;
    f_hi = (p >> 8) < F - 1 ? (p >> 8) : F - 1;
}

// Sample q of the reflect-padded (512 each side) trimmed signal of length L = (F - 1) * 256 -> position in the
// untrimmed overlap-add signal.  Needs L > 512, i.e. F >= 4.
MTTS_GL_HD int reflect_pos(int q, int F) {
    const int L = (F - 1) * kHop;
    int t = q - kHalf;
    t = t < 0 ? -t : t;
    t = t >= L ? 2 * (L - 1) - t : t;
    return t + kHalf;
}

}  // namespace gl
}  // namespace mtts
