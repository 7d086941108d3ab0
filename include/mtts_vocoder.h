/*
 * mtts_vocoder.h -- C ABI of the HiFi-GAN generator operators in libmtts_hip.so (gfx950), inference only.
 *
 * Same conventions as mtts.h (caller-owned buffers, negative mtts_status on error, thread-local
 * mtts_last_error(), stream-ordered, no host synchronisation, never aborts).  Activations are TOKEN-MAJOR:
 * [rows = B*L, channels], channels contiguous, fp32, 16-byte aligned; L is the frame count at that stage,
 * channels % 8 == 0 and B*L < 2^31.  Every product is an exact fp32 MFMA (v_mfma_f32_32x32x2_f32): the
 * reference's own numerics.  No atomics: two calls give bitwise-equal results.
 *
 * Reference operators replaced (hifi_gan/models.py, relative to the reference root):
 *   mtts_voc_pre       <- Generator.conv_pre (models.py:81, 101): Conv1d(80, C0, 7, padding=3) on the [B, 80, T] mel
 *   mtts_voc_upsample  <- F.leaky_relu(x, 0.1) + Generator.ups[i] (models.py:85-88, 103-104): ConvTranspose1d
 *   mtts_voc_conv      <- every dilated Conv1d of ResBlock1 / ResBlock2 with the leaky ReLU before it, the residual
 *                         add after it (models.py:35-42, 63-68) and the sum / mean over a stage's resblocks
 *                         (models.py:105-111)
 *   mtts_voc_post      <- F.leaky_relu(x) + conv_post + tanh (models.py:112-114)
 */
#ifndef MTTS_VOCODER_H_
#define MTTS_VOCODER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTTS_VOC_MAX_TAPS 11

/* mtts_voc_conv_args.acc_mode: what the epilogue does with the stage's running sum `acc` */
#define MTTS_VOC_ACC_NONE 0 /* acc untouched (may be NULL)                                            */
#define MTTS_VOC_ACC_INIT 1 /* acc[row, n] = v                       (first resblock of a stage)      */
#define MTTS_VOC_ACC_ADD 2  /* acc[row, n] = acc[row, n] + v                                          */
#define MTTS_VOC_ACC_MEAN 3 /* acc[row, n] = (acc[row, n] + v) / acc_div  (last resblock: a division, */
                            /*                                            as models.py:111 divides)   */

/*
 * Dilated Conv1d, "same" padding:  for b < B, u < L, n < N
 *   v = sum_{j<k} sum_{c<cin} f(A[b*L + u + (j - (k-1)/2)*d, c]) * W[n, j*cin + c]  + bias[n]  (+ residual[row, n])
 *   C[row, n] = v (when C != NULL), then acc per acc_mode;   row = b*L + u.
 * Input rows outside [0, L) of the SAME utterance read as zero (a tile never sees its neighbour utterance).
 * f = identity (leaky == 0) or leaky_relu(., slope), applied to A on its way into LDS (no separate pass).
 * k odd, k <= MTTS_VOC_MAX_TAPS; 1 <= d < 2^24 (the halo (k-1)/2*d may exceed L); cin % 8 == 0; N % 8 == 0;
 * W packed [N][k*cin] fp32 (a Conv1d weight [N, cin, k] permuted to [N, k, cin]).  All row strides equal the
 * channel count (A: cin; C, residual, acc: N).
 * ALIASING: C may alias residual (each element is read, then written, by the same thread).  C and acc must
 * never overlap A (other workgroups still read A's halo rows): MTTS_ERR_INVALID_ARG before any launch.
 * Anything outside these shapes is MTTS_ERR_SHAPE before any launch.
 */
typedef struct mtts_voc_conv_args {
    const float *A;
    const float *W;
    const float *bias;     /* [N] or NULL */
    const float *residual; /* [B*L, N] or NULL */
    float *C;              /* [B*L, N] or NULL (only acc is wanted) */
    float *acc;            /* [B*L, N]; required unless acc_mode == MTTS_VOC_ACC_NONE */
    int32_t B, L, cin, N, k, d;
    int32_t leaky;         /* 0 / 1 */
    float slope;
    int32_t acc_mode;
    float acc_div;         /* MTTS_VOC_ACC_MEAN: the divisor (num_kernels) */
} mtts_voc_conv_args;

int mtts_voc_conv(const mtts_voc_conv_args *args, void *hip_stream);

/*
 * leaky_relu(., slope) + ConvTranspose1d(cin, cout, k, stride = u, padding = (k - u)/2) by phase decomposition:
 * with k == 2u every output sample t*u + p is a two-tap conv of input frames (t-1, t) (phases p < u/2) or
 * (t, t+1) (p >= u/2), so the op is two implicit GEMMs of the conv kernel, each writing u/2 * cout columns
 * of C viewed as [B*L, u*cout] -- which IS token-major [B*L*u, cout].  Two launches.
 * Required: k == 2u and u even (every published HiFi-GAN config); else MTTS_ERR_SHAPE before any launch.
 * Wp: the phase-packed weight [u*cout][2*cin] fp32; with w the module's [cin, cout, k] weight and
 * q = p + u/2, row p*cout + n holds
 *     p <  u/2:  [ w[:, n, q + u] | w[:, n, q]     ]   (taps on frames t-1, t)
 *     p >= u/2:  [ w[:, n, q]     | w[:, n, q - u] ]   (taps on frames t, t+1)
 * bias [cout] or NULL.  A [B*L, cin], C [B*L*u, cout]; C must not overlap A.  cin % 8 == 0, cout % 8 == 0.
 */
int mtts_voc_upsample(const float *A, const float *Wp, const float *bias, float *C, int32_t B, int32_t L,
                      int32_t cin, int32_t cout, int32_t k, int32_t u, float slope, void *hip_stream);

/*
 * conv_pre: Conv1d(cin, N, 7, padding = 3) on the caller's CHANNEL-MAJOR mel [B, cin, T], written token-major
 * C [B*T, N].  One transposing launch into the workspace (mtts_voc_pre_workspace_size bytes: the token-major mel),
 * then the conv kernel.  W packed [N][7*cin]; cin % 8 == 0 (80 mel bins), N % 8 == 0.
 */
size_t mtts_voc_pre_workspace_size(int32_t B, int32_t T, int32_t cin);
int mtts_voc_pre(const float *mel, const float *W, const float *bias, float *C, int32_t B, int32_t T, int32_t cin,
                 int32_t N, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * out[b, 0, u] = tanh( sum_{j<7} sum_{c<C} leaky_relu(A[b*L + u + j - 3, c], slope) * w[j*C + c] + bias[0] )
 * A token-major [B*L, C], w [7*C] (conv_post's [1, C, 7] weight permuted to [7, C]), bias [1] or NULL,
 * out [B, 1, L].  The generator passes slope = 0.01: models.py:112 calls F.leaky_relu(x) without a slope,
 * i.e. torch's default 0.01, not LRELU_SLOPE.  A plain VALU kernel (N = 1).  C % 4 == 0, C <= 512.
 */
int mtts_voc_post(const float *A, const float *w, const float *bias, float *out, int32_t B, int32_t L, int32_t C,
                  float slope, void *hip_stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* MTTS_VOCODER_H_ */
