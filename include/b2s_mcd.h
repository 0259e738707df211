/* C ABI of libb2s_mcd.so: mel-cepstral distortion after DTW (MCD-DTW, in dB) for gfx950, the two steps around the batched DTW of
 * libb2s_metrics.so (b2s_met_dtw): b2s_mcd_cepstra in front of it, b2s_mcd_score behind it (DESIGN.md section k).
 *
 * Utterances are packed ragged as in b2s_metrics.h: frame f of utterance b is row offsets[b] + f (offsets = exclusive prefix sum of
 * the lengths, B + 1 int32 entries on the device), fp32 rows.  Every call launches on the caller's stream, creates no stream or
 * graph and does not synchronise.  Return codes: 0 = ok, otherwise b2s_mcd_last_error() holds the message (argument checks need no
 * GPU; nothing aborts).  No floating-point atomics anywhere: every result is bit-reproducible, and the same for an utterance alone
 * or inside a larger batch.
 */
#ifndef B2S_MCD_H
#define B2S_MCD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status_out values (those of b2s_metrics.h) */
#define B2S_MCD_OK 0
#define B2S_MCD_EMPTY 1       /* no voiced frame (cepstra), or the DTW's EMPTY handed on (score): MCD = NaN */
#define B2S_MCD_FAILED 2      /* offsets that decrease, run outside 0..total or exceed max_len; a path index outside the voiced count */

#define B2S_MCD_MAX_MELS 512
#define B2S_MCD_MAX_ORDER 256
/* B x ceil(max_len / 64) of one b2s_mcd_cepstra call: 64 utterances of a million frames, or 16 384 of 4096.  The compaction scan is
 * one workgroup over the per-chunk counts, so larger batches are split by the caller. */
#define B2S_MCD_MAX_CHUNKS (1 << 20)

int b2s_mcd_version(void);
const char *b2s_mcd_last_error(void);

/* Workspace bytes of one b2s_mcd_cepstra call (per-chunk voiced counts and output rows); 0 on an argument error (message set).
 * max_len bounds every utterance's length (the launch is sized by it). */
size_t b2s_mcd_ws_bytes(int B, int max_len);

/* Voiced-frame selection, de-normalisation and cepstral transform of one side.
 *   mel [total, n_mels] f32 in the project's normalised mel scale, offsets [B + 1]; 2 <= n_mels <= B2S_MCD_MAX_MELS
 *   a frame is voiced when the maximum over its bins is > 0 and it holds no NaN (np.max(x, -1) > 0); voiced frames keep their order
 *   per bin, in fp64, each operation rounded on its own (no fused multiply-add):
 *       a = symmetric ? (x + max_abs_value) / (2 * max_abs_value) : x;  a = min(max(a, 0), 1)
 *       ln = ((a * max_db - max_db) + ref_db) * ln_scale
 *   dct [order, n_mels] f64 on the device: rows 1..order of the orthonormal DCT-II, 1 <= order <= min(n_mels - 1, B2S_MCD_MAX_ORDER)
 *   c_k = sum_m ln_m * dct[k, m], accumulated from 0 in ascending m, product and sum rounded separately, then rounded once to f32
 * Outputs:
 *   cep_out [>= total, order] f32: rows 0 .. cep_offsets_out[B] - 1 are the voiced frames of the whole batch, gap-free, in order
 *   cep_offsets_out [B + 1] int32: exclusive prefix sum of voiced_out (what b2s_met_dtw takes as x_offsets)
 *   voiced_out [B] int32, status_out [B] int32: B2S_MCD_OK, B2S_MCD_EMPTY (no voiced frame) or B2S_MCD_FAILED: offsets that decrease,
 *       run outside 0..total, a length above max_len (the utterance's rows are never read), or a start below the end of an earlier
 *       well-formed utterance (rows already claimed, e.g. offsets [0, T, 0, T]).  A FAILED utterance counts 0 voiced frames and
 *       writes nothing, so the accepted ones are disjoint and never fill more than `total` rows of cep_out */
int b2s_mcd_cepstra(const float *mel, const int32_t *offsets, int total, int max_len, int B, int n_mels, int order, const double *dct,
                    int symmetric, double max_abs_value, double max_db, double ref_db, double ln_scale, float *cep_out,
                    int32_t *cep_offsets_out, int32_t *voiced_out, int32_t *status_out, void *ws, size_t ws_bytes, void *stream);

/* MCD along the DTW path.  cx [total_cx, order] / cy [total_cy, order] with their B + 1 offsets as b2s_mcd_cepstra wrote them; path
 * (int32 (i, j) pairs), path_offsets [B + 1], path_len [B] and dtw_status [B] as b2s_met_dtw wrote them; total_path = pairs that
 * path (and dist_out) hold.
 *   per step: d = db_scale * sqrt(2 * sum_k (cx[i, k] - cy[j, k])^2) in fp64, k ascending
 *   mcd_out[B] f64 = mean of d over the path: thread t of 256 sums steps t, t + 256, ... in order, then a fixed tree over the threads
 *   dist_out (nullable) f64 [total_path]: d of step q of pair b at path_offsets[b] + q
 *   status_out[B] int32: dtw_status[b] handed on when it is not OK (mcd = NaN); B2S_MCD_FAILED (mcd = NaN) for offsets or a path
 *       slot outside the totals, a path_len outside 1..slot, or a path index outside the pair's voiced counts (never followed) */
int b2s_mcd_score(const float *cx, const int32_t *cx_offsets, int total_cx, const float *cy, const int32_t *cy_offsets, int total_cy,
                  int B, int order, const int32_t *path, const int32_t *path_offsets, int total_path, const int32_t *path_len,
                  const int32_t *dtw_status, double db_scale, double *mcd_out, int32_t *status_out, double *dist_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
