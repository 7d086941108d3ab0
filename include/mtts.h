/*
 * mtts.h -- C ABI of libmtts_hip.so, the MI355X (gfx950) hot path of the Matcha-TTS training step.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t passed as void*.
 * No torch types cross this boundary.  Conventions:
 *   - Ownership: the caller allocates every input, output and workspace buffer
 *     (query sizes with the *_workspace_size functions).  The library keeps no global state
 *     beyond the lazily loaded code objects.
 *   - Errors: 0 (MTTS_OK) on success, a negative mtts_status otherwise; mtts_last_error() returns a
 *     thread-local message describing the last failure on the calling thread.  Never aborts.
 *   - Threading: calls are stream-ordered and asynchronous (no host synchronisation), re-entrant
 *     across streams and threads; the device is the current device of the calling thread.
 *
 * Reference interfaces replaced (paths relative to the reference repository root):
 *   mtts_maximum_path_f32          <- matcha/utils/monotonic_align/__init__.py:40-55  maximum_path(value, mask)
 *   mtts_prior_maximum_path        <- matcha/models/matcha_tts.py:276-288 (log-prior lattice + maximum_path +
 *                                     the duration target), fused
 *   mtts_duration_path             <- matcha/models/matcha_tts.py:273-274 + utils/model.py:77-114 (the alignment
 *                                     from precomputed durations, use_precomputed_durations=True)
 *   mtts_expand_rows_fwd / _bwd    <- matcha/models/matcha_tts.py:314-315  mu_y = attn^T @ mu_x
 *   mtts_segment_crop_fwd / _bwd   <- matcha/models/matcha_tts.py:290-315  forward(out_size=...): random mel segment
 *   mtts_compute_batch_alignments  <- matcha/utils/monotonic_align/core.pyx:101-128   compute_batch_alignments(...)
 *                                     (bound as maximum_path_c, __init__.py:4-8)
 *   mtts_losses_fwd / _bwd         <- flow_matching.py:145-149 (CFM loss) + matcha_tts.py:319-323 (prior loss)
 *   mtts_mel_log_fwd               <- matcha/utils/audio_process.py:62-72  MelSpectrogram.__call__ (after the STFT)
 *   mtts_mel_from_wav              <- matcha/utils/audio_process.py:45-72 per utterance + ljspeech_datamodule.py:84-109
 *                                     (the padded mel batch and y_lengths), from the waveforms in one launch
 *   mtts_mel_stats                 <- the sums of upstream's data-statistics script (mel_mean, mel_std)
 *   mtts_sequence_mask_f32         <- matcha/utils/model.py:13-34 sequence_mask(...).to(float) (matcha_tts.py:259,
 *                                     text_encoder.py:398) and text_encoder.py:300-303 masked_fill(-1e4) as a key bias
 *   mtts_duration_loss_fwd / _bwd  <- matcha_tts.py:287-288 + utils/model.py:117-135 duration_loss
 *   mtts_loss_sum                  <- baselightningmodule.py:121-128 (dur + prior + diff, the logged values)
 * Decoder / CFM operators (matcha/models/components/{decoder,transformer,flow_matching}.py) are
 * declared in mtts_decoder.h.
 */
#ifndef MTTS_H_
#define MTTS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTTS_ABI_VERSION 1

typedef enum mtts_status {
    MTTS_OK = 0,
    MTTS_ERR_INVALID_ARG = -1, /* null pointer, negative size, bad flag */
    MTTS_ERR_SHAPE = -2,       /* shape outside what the kernels support (e.g. Tx > 8192) */
    MTTS_ERR_WORKSPACE = -3,   /* workspace too small */
    MTTS_ERR_HIP = -4,         /* a HIP runtime call failed (launch, attribute) */
    MTTS_ERR_UNSUPPORTED = -5  /* feature not built into this library */
} mtts_status;

/* Library identity / diagnostics. */
int mtts_abi_version(void);
const char *mtts_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Monotonic Alignment Search (Viterbi max-path over the [T_text x T_mel] log-likelihood lattice)
 * ------------------------------------------------------------------------------------------- */

/* flags for mtts_maximum_path_f32 */
#define MTTS_MAS_VALUE_PREMASKED 0x1 /* value already holds value*mask: skip the multiply      */
#define MTTS_MAS_NO_DENSE_PATH 0x2   /* only row_start_out/lengths_out: do not write `path`    */

/* Maximum text length (Tx) the kernels accept. */
#define MTTS_MAS_MAX_TX 8192 /* maximum_path / the fused prior path (transposed lattice): 8 waves x 16 text rows per lane of
                                the multi-wave DP (round 6; 4096 in rounds 4-5) */
#define MTTS_MAS_MAX_TX_ROW_MAJOR 4096 /* mtts_compute_batch_alignments (the row-major lattice it mutates): 8 x 8 rows */

/* Bytes of device workspace mtts_maximum_path_f32 / mtts_compute_batch_alignments need. */
size_t mtts_maximum_path_workspace_size(int32_t B, int32_t Tx, int32_t Ty);

/*
 * maximum_path(value, mask)                         (reference: monotonic_align/__init__.py:40-55)
 *   value, mask : float32 [B, Tx, Ty], C-contiguous, device memory.
 *   path        : float32 [B, Tx, Ty] output, fully written: exactly one 1.0 per column y < t_y[b],
 *                 zeros elsewhere (unless MTTS_MAS_NO_DENSE_PATH).
 *   t_x[b] = (int)sum_x mask[b, x, 0],  t_y[b] = (int)sum_y mask[b, 0, y]   (__init__.py:52-53)
 *   The DP runs on value*mask (one fp32 multiply per cell, __init__.py:45) with the Cython's tie rule
 *   (`from_prev >= from_same` -> diagonal, core.pyx:73) and `best + score` as one fp32 add (:80):
 *   the path is bit-identical to the compiled Cython for 1 <= t_x <= t_y.
 *   Defined behaviour where the reference is undefined: t_x == 0, t_y == 0 or t_x > t_y produce an
 *   all-zero path for that utterance (its row starts are -1).
 *   lengths_out   : optional int32 [B, 2] = (t_x, t_y) per utterance.
 *   row_start_out : optional int32 [B, Tx]; row x of utterance b covers columns
 *                   [row_start[b,x], row_start[b,x+1]-1] (the last row ends at t_y-1); -1 = no path.
 *   The caller's value and mask are not modified.
 */
int mtts_maximum_path_f32(const float *value, const float *mask, float *path, int32_t B, int32_t Tx,
                          int32_t Ty, int32_t flags, int32_t *lengths_out, int32_t *row_start_out,
                          void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * compute_batch_alignments(paths, values, t_xs, t_ys, max_neg_val)   (reference: core.pyx:101-128)
 *   paths  : int32 [B, Tx, Ty]; ones are SET on the path, other entries are left untouched (:88).
 *   values : float32 [B, Tx, Ty]; MUTATED exactly like the Cython (:83-85): for y < t_y, x < t_x the
 *            cell receives the DP value (in-band: cumulative best + score; out-of-band: max_neg_val);
 *            cells outside the [t_x, t_y] rectangle are untouched.
 *   t_xs, t_ys : int32 [B] device arrays.
 */
int mtts_compute_batch_alignments(int32_t *paths, float *values, const int32_t *t_xs,
                                  const int32_t *t_ys, int32_t B, int32_t Tx, int32_t Ty,
                                  float max_neg_val, void *workspace, size_t workspace_bytes,
                                  void *hip_stream);

/*
 * Fused alignment of the training forward (matcha_tts.py:276-288):
 *   lattice[b,i,j] = (log N(y[b,:,j]; mu_x[b,:,i], I)) * x_mask[b,i] * y_mask[b,j]   (matcha_tts.py:277-282,
 *                    maximum_path's value*mask) with the masks from x_lengths / y_lengths (int64 [B]),
 *   then the DP and backtrack of mtts_maximum_path_f32 on it (t_x = x_lengths, t_y = y_lengths).
 *   mu_x : float32 [B, C, Tx], y : float32 [B, C, Ty] (channel-major, C-contiguous, device memory).
 *   Outputs (each optional): path float32 [B,Tx,Ty] (dense hard attention), lengths_out int32 [B,2],
 *   row_start_out int32 [B,Tx] (as mtts_maximum_path_f32), dur_out float32 [B,Tx] = sum_j path[b,i,j],
 *   col_row_out int32 [B,Ty] = the text row of frame j (-1 past t_y), lattice_out float32 [B,Tx,Ty]
 *   (the masked lattice; otherwise it lives in the workspace).
 *   The lattice sums run in ascending channel order, one fp32 operation each (bit-reproducible on the
 *   host); the reference's torch matmuls use an implementation-defined order.
 */
size_t mtts_prior_maximum_path_workspace_size(int32_t B, int32_t Tx, int32_t Ty);
int mtts_prior_maximum_path(const float *mu_x, const float *y, const int64_t *x_lengths, const int64_t *y_lengths,
                            int32_t B, int32_t C, int32_t Tx, int32_t Ty, float *path, int32_t *lengths_out,
                            int32_t *row_start_out, float *dur_out, int32_t *col_row_out, float *lattice_out,
                            void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * Alignment from precomputed durations (matcha_tts.py:273-274: generate_path(durations, x_mask * y_mask) and its
 * sum(-1); utils/model.py:77-114), as the run-length alignment the consumers below read.  Per utterance b:
 *   t_x = clamp(x_lengths[b], 0, Tx), t_y = clamp(y_lengths[b], 0, Ty)            (int64 [B], device)
 *   c_0 = 0, c_{x+1} = c_x + max(durations[b,x], 0)   in float64 (exact on fp32 terms; NaN counts as 0)
 *   e_x = (int)min(ceil(c_x), t_y)
 *   row_start[b,x] = e_x, dur[b,x] = e_{x+1} - e_x    for x < t_x; -1 and 0 past t_x
 *   t_cov = e_{t_x}: the frames the durations cover (<= t_y; they need not add up to t_y)
 *   col_row[b,y] = the x < t_x with e_x <= y < e_{x+1} for y < t_cov, else -1
 *   path[b,x,y] = (col_row[b,y] == x)                 float32 [B,Tx,Ty], optional, fully written
 *   lengths_out = (t_x, t_y), run_lengths_out = (t_x, t_cov)                      int32 [B,2]
 * durations float32 [B,Tx]; every output is optional, but `path` needs row_start_out and run_lengths_out (it is
 * written from them).  Give run_lengths to mtts_expand_rows_bwd / mtts_segment_crop_bwd as their `lengths` (the
 * last row's run ends at t_cov, and a row of length 0 has row_start[x] == row_start[x+1]) and lengths to
 * mtts_segment_crop_fwd (the window is drawn on t_y, as the reference crops on y_lengths).  No workspace, no
 * atomics, fixed order.  MTTS_ERR_SHAPE for Tx > MTTS_MAS_MAX_TX or B > 65535.
 */
int mtts_duration_path(const float *durations, const int64_t *x_lengths, const int64_t *y_lengths, int32_t B,
                       int32_t Tx, int32_t Ty, float *path, int32_t *lengths_out, int32_t *run_lengths_out,
                       int32_t *row_start_out, float *dur_out, int32_t *col_row_out, void *hip_stream);

/*
 * mu_y = attn^T @ mu_x for a hard alignment (matcha_tts.py:314-315) as a gather, and its backward:
 *   fwd: dst[b,c,j] = src[b,c,col_row[b,j]] (0 where col_row < 0); src [B,C,Tx], dst [B,C,Ty] float32.
 *   bwd: dx[b,c,i] = sum over the frames j of row i (row_start / lengths of mtts_maximum_path_f32) of
 *        dy[b,c,j]: 16 strided partial sums (j = start + l + 16k, ascending k) combined by a fixed
 *        xor tree (deterministic, no atomics).
 */
int mtts_expand_rows_fwd(const float *src, const int32_t *col_row, int32_t B, int32_t C, int32_t Tx, int32_t Ty,
                         float *dst, void *hip_stream);
int mtts_expand_rows_bwd(const float *dy, const int32_t *row_start, const int32_t *lengths, int32_t B, int32_t C,
                         int32_t Tx, int32_t Ty, float *dx, void *hip_stream);

/*
 * Random mel segment of the training forward (matcha_tts.py:290-315, forward(out_size=S)), fused with the
 * alignment's consumers: per utterance b, with (t_x, t_y) = lengths[b],
 *   cut_len = min(t_y, S), max_off = max(t_y - S, 0)   (cut_len = 0, off = 0 when t_x == 0 or t_y == 0)
 *   off = clamp(offsets_in[b], 0, max_off)              with offsets_in (int32 [B]; clamped on the device),
 *       = (uint64(rand_words[b]) * max_off) >> 31       otherwise (rand_words int32 [B] in [0, 2^31)): uniform on
 *         [0, max_off) -- max_off itself is never drawn and max_off <= 1 gives 0, as the reference's
 *         random.choice(range(0, max_offset)) (:292-295).  Integer arithmetic only: exact on the host.
 *   y_cut[b,c,j]    = y[b,c,off+j]                    j < cut_len, else 0       float32 [B,C,S]
 *   mu_y_cut[b,c,j] = mu_x[b,c,col_row[b,off+j]]      j < cut_len, else 0       float32 [B,C,S]
 *   attn_cut[b,i,j] = (j < cut_len && col_row[b,off+j] == i)                    float32 [B,Tx,S], optional
 *   mask_cut[b,j]   = j < cut_len                                               float32 [B,S]
 *   seg[b]          = (off, cut_len)                                            int32 [B,2]
 * y [B,C,Ty], mu_x [B,C,Tx] float32; col_row [B,Ty], lengths [B,2] as mtts_prior_maximum_path wrote them.  One of
 * rand_words / offsets_in must be given (offsets_in wins).  One launch; 1 <= S <= Ty.
 *
 * bwd: d_mu_x[b,c,i] = sum of d_mu_y_cut[b,c,j] over the frames of row i inside the window.  Bit for bit what
 * mtts_expand_rows_bwd returns for a full-length dy that holds d_mu_y_cut in [off, off+cut_len) and zeros
 * elsewhere: lane l of 16 takes the frames row_start + l + 16k that fall in the window, then the same xor tree,
 * per 4096-frame slab of the full-length frame axis.  Deterministic, no atomics.
 */
int mtts_segment_crop_fwd(const float *y, const float *mu_x, const int32_t *col_row, const int32_t *lengths,
                          const int32_t *rand_words, const int32_t *offsets_in, int32_t B, int32_t C, int32_t Tx,
                          int32_t Ty, int32_t S, float *y_cut, float *mu_y_cut, float *attn_cut, float *mask_cut,
                          int32_t *seg, void *hip_stream);
int mtts_segment_crop_bwd(const float *d_mu_y_cut, const int32_t *row_start, const int32_t *lengths,
                          const int32_t *seg, int32_t B, int32_t C, int32_t Tx, int32_t S, float *d_mu_x,
                          void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Log-mel features of the data path (matcha/utils/audio_process.py:32-81, MelSpectrogram.__call__)
 * ------------------------------------------------------------------------------------------- */
/*
 * out[b,m,f] = log(max(sum_{k in [band_lo[m], band_hi[m])} mel_w[m,k] * sqrt(re^2 + im^2 + 1e-9), clip))
 *   spec : float32 [B, n_freq, F, 2] (torch.stft's complex output viewed as real, C-contiguous)
 *   mel_w: float32 [n_mels, n_freq] (the librosa slaney basis); band_lo/hi int32 [n_mels]: the nonzero
 *          bins of each filter (zero weights outside are skipped -- exact, they add +0).
 *   out  : float32 [B, n_mels, F].  Bins are summed in ascending k (fixed order, deterministic).
 */
int mtts_mel_log_fwd(const float *spec, const float *mel_w, const int32_t *band_lo, const int32_t *band_hi,
                     int32_t B, int32_t n_freq, int32_t F, int32_t n_mels, float clip_val, float *out,
                     void *hip_stream);

/*
 * The whole front end in one launch: a ragged waveform batch -> padded log-mel and frame counts, each utterance
 * computed on its own waveform (the reference runs MelSpectrogram per utterance and collate zero-pads the mels).
 *   wav        : [B, L] float32 in [-1, 1], or int16 when wav_is_int16 != 0 (converted as float(s) / 32768, exact)
 *   lengths    : int32 [B] on the device, samples per row; NULL: every row has L.  Clamped to [0, L] by the kernel:
 *                it may hold anything, and no sample outside [0, len) of a row is read.
 *   mel_w, band_lo, band_hi : as for mtts_mel_log_fwd, mel_w [n_mels, 513]
 *   twiddle    : float32 [1024, 2], exp(-2 pi i k / 1024); window: float32 [1024] (periodic Hann); both 8-byte aligned
 *   n_fft = win_size = 1024, hop = 256 is the one geometry served (center=False with the reference's manual reflect
 *   pad of 384 per side); anything else returns MTTS_ERR_SHAPE before any launch.  B <= 65535, n_mels <= 96, L <= 2^30.
 *   out        : float32 [B, n_mels, F_out], F_out = L / 256, fully written.  With len = clamp(lengths[b], 0, L) and
 *                F_b = len / 256 if len >= 385 (the shortest waveform a reflect pad by 384 accepts) else 0:
 *                  f <  F_b: (log(max(sum_k mel_w[m,k] * sqrt(re^2 + im^2 + 1e-9), clip_val)) - mean) / std of the
 *                            spectrum of window * x_pad[256 f : 256 f + 1024], x_pad the utterance's own reflect-padded
 *                            signal; the division is a true division (mean = 0, std = 1 change no bit)
 *                  f >= F_b: pad_value exactly
 *   mel_lengths: int32 [B] output, F_b.  Written also when F_out == 0.
 * Deterministic (no atomics, fixed summation order); a row's result does not depend on the other rows.
 */
int mtts_mel_from_wav(const void *wav, int32_t wav_is_int16, const int32_t *lengths, const float *mel_w,
                      const int32_t *band_lo, const int32_t *band_hi, const float *twiddle, const float *window,
                      int32_t B, int32_t L, int32_t n_fft, int32_t win_size, int32_t hop, int32_t n_mels,
                      float clip_val, float mean, float std, float pad_value, float *out, int32_t *mel_lengths,
                      void *hip_stream);

/*
 * stats[b] = (sum v, sum v^2) in float64 over mel[b, :, :mel_lengths[b]]  (the sums behind data_statistics).
 *   mel: float32 [B, n_mels, F]; mel_lengths: int32 [B] on the device, clamped to [0, F]; stats: float64 [B, 2].
 *   One launch, no atomics, a fixed summation order.
 */
int mtts_mel_stats(const float *mel, const int32_t *mel_lengths, int32_t B, int32_t n_mels, int32_t F, double *stats,
                   void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Training losses (flow_matching.py:145-149 CFM loss, matcha_tts.py:319-323 prior loss), fused
 * ------------------------------------------------------------------------------------------- */
/*
 * out[0] = sum((u_pred - (x1 - (1 - sigma_min) z))^2) / D         (unmasked numerator, reference quirk)
 * out[1] = sum(0.5 ((y - mu_y)^2 + log 2pi) * y_mask) / D,  D = out[2] = sum(y_mask) * C
 *   u_pred token-major [B,T,C]; x1, z, y, mu_y channel-major [B,C,T]; y_mask float [B,T] (float32, device).  u_pred = NULL
 *   skips the CFM term (out[0] = 0); mu_y = NULL skips the prior term.  C <= 128.  Deterministic.
 * Backward: du_pred = 2 g_diff / D (u_pred - u) (token-major), dmu_y = -g_prior / D (y - mu_y) * y_mask
 *   (channel-major); either output may be NULL.  fwd_out is the forward's out (D read from out[2]).
 */
size_t mtts_losses_workspace_size(int32_t B, int32_t T);
int mtts_losses_fwd(const float *u_pred, const float *x1, const float *z, const float *y, const float *mu_y,
                    const float *y_mask, int32_t B, int32_t C, int32_t T, float sigma_min, float *out,
                    void *workspace, size_t workspace_bytes, void *hip_stream);
int mtts_losses_bwd(const float *g_diff, const float *g_prior, const float *fwd_out, const float *u_pred, const float *x1, const float *z,
                    const float *y, const float *mu_y, const float *y_mask, int32_t B, int32_t C, int32_t T,
                    float sigma_min, float *du_pred, float *dmu_y, void *hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Step glue: sequence masks, the duration loss, the loss sum (csrc/losses.hip)
 * ------------------------------------------------------------------------------------------- */
/* mask[b, t] = t < lengths[b] ? 1 : 0 (fp32 [B, T]); key_bias[b, t] = (mask - 1) * 1e4 when non-NULL
 * (either output may be NULL, not both).  lengths int64 [B]. */
int mtts_sequence_mask_f32(const int64_t *lengths, int32_t B, int32_t T, float *mask, float *key_bias,
                           void *hip_stream);
/* logw_ = log(1e-8 + dur) * x_mask (x_mask from lengths);  out[0] = sum((logw - logw_)^2) / sum(lengths),
 * out[1] = sum(lengths) as fp32.  logw, dur fp32 [B, T] (dur: the MAS durations); fixed-order sum.
 * Backward: dlogw = (g / out[1]) * (2 (logw - logw_)). */
int mtts_duration_loss_fwd(const float *logw, const float *dur, const int64_t *lengths, int32_t B, int32_t T,
                           float *out, void *hip_stream);
int mtts_duration_loss_bwd(const float *g, const float *fwd_out, const float *logw, const float *dur,
                           const int64_t *lengths, int32_t B, int32_t T, float *dlogw, void *hip_stream);
/* total = (dur + prior) + diff; logged (optional, 4 floats) = [dur, prior, diff, total].  prior may be NULL (0). */
int mtts_loss_sum(const float *dur, const float *prior, const float *diff, float *total, float *logged,
                  void *hip_stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* MTTS_H_ */
