/* C ABI of libb2s_f0.so: batched YIN pitch tracking (de Cheveigne & Kawahara 2002, steps 1 to 5) and the F0 error along a DTW path
 * for gfx950 (DESIGN.md section l).  Three calls: b2s_f0_quantize (waveform -> the int16 PCM that save_wav writes), b2s_f0_yin (PCM ->
 * one F0 per frame) and b2s_f0_score (two F0 tracks and a path over kept frames -> RMSE, voicing and gross pitch errors).
 *
 * Every integer quantity of the estimator (difference function, its running sum) is exact, and the only roundings are the single
 * fp64 division of the cumulative-mean normalisation and the fp64 operations of the parabolic refinement, none contracted.  So the
 * results do not depend on how the kernel tiles the sums: they are the bits of the NumPy restatement (tests/f0_ref.py), the same from
 * run to run and for an utterance alone or inside a batch.
 *
 * Every call launches on the caller's stream, creates no stream or graph and does not synchronise.  Return codes: 0 = ok, otherwise
 * b2s_f0_last_error() holds the message (argument checks need no GPU; nothing aborts).  No atomics anywhere.
 */
#ifndef B2S_F0_H
#define B2S_F0_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status values (those of b2s_metrics.h and b2s_mcd.h) */
#define B2S_F0_OK 0
#define B2S_F0_EMPTY 1        /* score: an empty path, or the DTW's EMPTY handed on */
#define B2S_F0_FAILED 2       /* a non-finite sample, a length or offsets outside their bounds, a path index or frame number out of range */

#define B2S_F0_MAX_WIN 2048   /* with |pcm| <= 32768 every d[tau] stays below 2^43 */
#define B2S_F0_MAX_TAU 512    /* ... and the running sum of d and d[tau] * tau below 2^53: exact in fp64 */

int b2s_f0_version(void);
const char *b2s_f0_last_error(void);

/* Waveform to 16-bit PCM by the rule of save_wav.
 *   wav [B, Lmax] f32, lengths [B] int32 (0 <= L <= Lmax; L = 0 is allowed), B > 0, Lmax >= 0
 *   peak = max |wav[0:L)|;  pcm = rint(clip(fp64(wav) / max(0.01, fp64(peak)), -1, 1) * 32767), halves to even
 * Outputs:
 *   pcm [B, Lmax] int16, zero past L
 *   peak_out [B] f32, nullable
 *   status [B] int32: B2S_F0_OK, or B2S_F0_FAILED for a length outside 0..Lmax (nothing is read) or a NaN / Inf among the L
 *       samples; a FAILED utterance gets a row of zeros and peak 0 */
int b2s_f0_quantize(const float *wav, const int32_t *lengths, int B, int Lmax, int16_t *pcm, float *peak_out, int32_t *status,
                    void *stream);

/* YIN on PCM.
 *   pcm [B, Lmax] int16, lengths [B] int32
 *   frame_offsets [B + 1] int32: exclusive prefix sum of the frame counts F_b = 1 + L_b / hop; total_frames = frame_offsets[B], on the
 *       host: the rows every output holds
 *   win (2..B2S_F0_MAX_WIN) samples per integration window, hop >= 1, 2 <= tau_min < tau_max <= B2S_F0_MAX_TAU
 *   threshold > 0 (fp64): the absolute threshold of step 4
 *   min_energy >= 0 (int64): a frame whose sum of seg[j]^2 over j < win is below it is unvoiced
 *   sr > 0 (fp64): sampling rate in Hz
 * Frame t of an utterance is centred at sample t * hop: seg[i] = pcm[t * hop - (win + tau_max) / 2 + i], i < win + tau_max, zero
 * outside [0, L).  d[tau] = sum_{j < win} (seg[j] - seg[j + tau])^2 for tau = 0..tau_max, S[tau] = d[1] + .. + d[tau] (exact
 * integers), c[0] = 1, c[tau] = S[tau] == 0 ? 1 : fp64(d[tau] * tau) / fp64(S[tau]).  The pick: the first k in tau_min..tau_max with
 * c[k] < threshold, advanced while k + 1 <= tau_max and c[k + 1] < c[k]; none, or too little energy: unvoiced.  Refinement with
 * a = c[tau - 1], b = c[tau], cc = c[tau + 1] when 1 <= tau - 1 and tau + 1 <= tau_max: den = (a - b) + (cc - b); den > 0:
 * shift = 0.5 * (a - cc) / den, kept when |shift| <= 1.  f0 = sr / (tau + shift).
 * Outputs, row frame_offsets[b] + t for frame t of utterance b:
 *   f0_out [total_frames] f64 (0 = unvoiced), tau_out [total_frames] int32 (0 = unvoiced)
 *   aper_out [total_frames] f64, nullable: min of c[tau_min..tau_max], also for unvoiced frames
 *   cmnd_out [total_frames, tau_max + 1] f64, nullable: c
 *   status [B] int32: B2S_F0_OK, or B2S_F0_FAILED when L is outside 0..Lmax, frame_offsets[b] < 0, frame_offsets[b + 1] >
 *       total_frames or frame_offsets[b + 1] - frame_offsets[b] != 1 + L / hop; nothing is read or written for that utterance.
 *       Offsets that pass are inside the buffers; that they are disjoint is what the prefix sum gives and is not checked. */
int b2s_f0_yin(const int16_t *pcm, const int32_t *lengths, const int32_t *frame_offsets, int total_frames, int B, int Lmax, int win,
               int hop, int tau_min, int tau_max, double threshold, int64_t min_energy, double sr, double *f0_out, int32_t *tau_out,
               double *aper_out, double *cmnd_out, int32_t *status, void *stream);

/* F0 error of x (prediction) against y (target) along a DTW path over kept frames.
 *   f0_x [total_fx] f64, tau_x [total_fx] int32 with fx_offsets [B + 1] as b2s_f0_yin wrote them; the same for y
 *   kept_x [total_kx] int32 with kx_offsets [B + 1]: kept frame i of pair b is frame kept_x[kx_offsets[b] + i] of utterance b (the
 *       offsets are those of the cepstra the path was found on); the same for y
 *   path (int32 (i, j) pairs), path_offsets [B + 1], path_len [B], dtw_status [B] as b2s_met_dtw wrote them; total_path = pairs held
 *   gross_ratio >= 0: a step where both sides are voiced (tau > 0) is a gross error when |fx - fy| > gross_ratio * fy
 * Outputs:
 *   scores [B, 5] f64: rmse_hz, rmse_cents (1200 * log2(fx / fy)) over the steps where both sides are voiced, vde = vuv / steps,
 *       gpe = gross / both, ffe = (vuv + gross) / steps; both == 0 gives NaN in rmse_hz, rmse_cents and gpe.  Thread t of 256 sums
 *       steps t, t + 256, ... in order, then a fixed tree over the threads
 *   counts [B, 4] int32: steps, vuv (exactly one side voiced), both, gross
 *   status [B] int32: B2S_F0_EMPTY (scores NaN, counts 0) for an EMPTY dtw_status, or an OK one with path_len == 0; B2S_F0_FAILED
 *       (scores NaN, counts 0) for any other dtw_status that is not OK, offsets or a path slot outside the totals, a path_len
 *       outside the slot, a path index outside the kept count or a frame number outside the F0 track (never followed);
 *       B2S_F0_OK otherwise */
int b2s_f0_score(const double *f0_x, const int32_t *tau_x, const int32_t *fx_offsets, int total_fx, const double *f0_y,
                 const int32_t *tau_y, const int32_t *fy_offsets, int total_fy, const int32_t *kept_x, const int32_t *kx_offsets,
                 int total_kx, const int32_t *kept_y, const int32_t *ky_offsets, int total_ky, int B, const int32_t *path,
                 const int32_t *path_offsets, int total_path, const int32_t *path_len, const int32_t *dtw_status, double gross_ratio,
                 double *scores, int32_t *counts, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
