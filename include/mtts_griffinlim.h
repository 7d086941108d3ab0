/*
 * mtts_griffinlim.h -- C ABI of the checkpoint-free mel -> waveform path in libmtts_hip.so (gfx950): the inverse
 * mel projection and Griffin-Lim phase reconstruction, inference only.
 *
 * Same conventions as mtts.h (caller-owned buffers, negative mtts_status on error, thread-local
 * mtts_last_error(), stream-ordered, no host synchronisation, never aborts).  Everything is fp32.  No atomics and a
 * fixed summation order: two calls give bitwise-equal results.
 *
 * Operators restated (torchaudio is not a dependency; the reference's generate.py:73-109 configures them):
 *   mtts_gl_inverse_mel <- torchaudio.transforms.InverseMelScale (the minimum-norm least-squares solution, as a
 *                          product with the pseudo-inverse of the mel basis) and griffinlim's specgram ** (1/power)
 *   mtts_gl_synthesis   <- the phase update of torchaudio.functional.griffinlim and the per-frame half of
 *                          torch.istft (inverse real FFT, window)
 *   mtts_gl_analysis    <- the other half of torch.istft (overlap-add, division by the window envelope, trim) and
 *                          torch.stft (center=True, reflect, onesided, not normalized); or the final waveform
 *
 * The STFT geometry is fixed: n_fft = win_length = 1024, hop = 256 (MTTS_GL_NFFT, MTTS_GL_HOP); anything else is
 * MTTS_ERR_SHAPE before any launch, and so is F < 4 (fewer frames cannot be reflect-padded by 512 samples).
 *
 * Spectra that only these kernels exchange (lin of the synthesis, reb, tprev) are FRAME-MAJOR: [B, F, 513] floats
 * (lin) or [B, F, 513, 2] (re, im).  Windowed frames are [B, F, 1024].
 *
 * twiddle: [1024, 2] fp32, entry k = (cos, -sin)(2 pi k / 1024) = exp(-2 pi i k / 1024), computed in float64.
 * window:  [1024] fp32, the periodic Hann window (or any window whose hop-256 squared overlap-add is nonzero).
 *
 * One Griffin-Lim run of n iterations on (B, F):
 *   synthesis(lin, ang0, NULL, 0, normalize = 0)                      frames of istft(lin * ang0)
 *   for i < n:  analysis(frames -> S[i % 2]);                          reb
 *               synthesis(lin, S[i % 2], i ? S[(i+1) % 2] : NULL, m, normalize = 1)
 *   analysis(frames -> wav)
 * i.e. 2 n + 1 launches after the inverse mel, plus the final gather.
 */
#ifndef MTTS_GRIFFINLIM_H_
#define MTTS_GRIFFINLIM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTTS_GL_NFFT 1024
#define MTTS_GL_HOP 256

/*
 * lin[b, k, f] = max(0, sum_{m < n_mels} pinv[k, m] * g(mel[b, m, f])) ** inv_power   for k < n_rows,
 * lin[b, k, f] = 0                                                                     for n_rows <= k < n_stft,
 * g = exp when log_input != 0, else the identity.  mel [B, n_mels, F]; pinv [n_stft, n_mels] row-major (rows from
 * n_rows on are not read); inv_power = 1 / power > 0.  One launch.
 * lin is [B, n_stft, F] (frame_major == 0, the layout of torchaudio) or [B, F, n_stft] (frame_major != 0, what
 * mtts_gl_synthesis reads).  B <= 65535, B*F < 2^20, n_mels <= 96 (a tile's operands are staged in LDS); beyond:
 * MTTS_ERR_SHAPE.
 */
int mtts_gl_inverse_mel(const float *mel, const float *pinv, float *lin, int32_t B, int32_t n_mels, int32_t n_stft,
                        int32_t n_rows, int32_t F, int32_t log_input, float inv_power, int32_t frame_major,
                        void *hip_stream);

/*
 * frames[b, f, :] = window * irfft_1024(lin[b, f, :] * ang[b, f, :])   with
 *   ang = reb - m * tprev            (tprev may be NULL: ang = reb)
 *   ang = ang / (|ang| + 1e-16)      (when normalize != 0)
 * The imaginary parts of bins 0 and 512 are ignored, as a complex-to-real transform ignores them.  One launch.
 * frames must not alias an input.
 */
int mtts_gl_synthesis(const float *lin, const float *reb, const float *tprev, float m, int32_t normalize,
                      const float *twiddle, const float *window, float *frames, int32_t B, int32_t F, int32_t n_fft,
                      int32_t hop, void *hip_stream);

/*
 * y = overlap-add of frames / overlap-add of window^2, trimmed by 512 at each end: (F - 1) * 256 samples per
 * utterance, each the sum of the at most four frames that cover it, in ascending frame order.
 *   reb != NULL: reb[b, f, :] = rfft_1024(window * reflect_pad_512(y)[256 f : 256 f + 1024])     (one launch)
 *   wav != NULL: wav[b, :] = y, [B, (F - 1) * 256]                                              (one launch)
 * At least one of the two; twiddle may be NULL when reb is.  Outputs must not alias frames.
 */
int mtts_gl_analysis(const float *frames, const float *twiddle, const float *window, float *reb, float *wav, int32_t B,
                     int32_t F, int32_t n_fft, int32_t hop, void *hip_stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* MTTS_GRIFFINLIM_H_ */
