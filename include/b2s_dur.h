/* C ABI of libb2s_dur.so: batched monotonic alignment search over an encoder-decoder attention map and the duration error of two
 * duration vectors for gfx950 (DESIGN.md section m).  Two calls: b2s_dur_mas (map -> the monotonic path of the largest summed
 * weight, and from it one frame count per encoder position) and b2s_dur_score (two duration vectors -> twelve integer sums).
 *
 * Every cell of the search is one fp64 add of an fp32 value and one fp64 compare, in an order the recurrence fixes, so the results
 * do not depend on how the kernel tiles the map: they are the bits of the NumPy restatement (tests/dur_ref.py), the same from run to
 * run and for an utterance alone or inside a batch.  The score call computes integers only.
 *
 * Every call launches on the caller's stream, creates no stream or graph and does not synchronise.  Return codes: 0 = ok, otherwise
 * b2s_dur_last_error() holds the message (argument checks need no GPU; nothing aborts).  No atomics anywhere.
 */
#ifndef B2S_DUR_H
#define B2S_DUR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status values (the first three are those of the other satellite libraries) */
#define B2S_DUR_OK 0
#define B2S_DUR_EMPTY 1       /* mas: enc_len == 0 or dec_len == 0; score: no unit */
#define B2S_DUR_FAILED 2      /* a length out of range, a non-finite weight among the valid cells; score: see there */
#define B2S_DUR_SHORT 3       /* mas: dec_len < enc_len, no monotonic path covers the text (a decoder that stopped early) */

#define B2S_DUR_MAX_S 1024    /* encoder positions: one lane each in one workgroup */
#define B2S_DUR_COUNTS 12     /* int64 values per pair of b2s_dur_score */

int b2s_dur_version(void);
const char *b2s_dur_last_error(void);

/* Bytes of workspace b2s_dur_mas needs: the decision bits, B x T x ceil(S / 64) 64-bit words (one wave ballot per frame and
 * wave).  0 = refused (B <= 0, S outside 1..B2S_DUR_MAX_S, T < 1, or sizes past one call), with the message in last_error. */
size_t b2s_dur_ws_bytes(int B, int S, int T);

/* Monotonic alignment search.
 *   maps [B, S, T] f32 contiguous, T innermost (the `maps` of b2s_met_align_select); enc_len [B], dec_len [B] int32
 * For utterance b with p[s][t] = maps[b][s][t], Sb = enc_len[b], Tb = dec_len[b], in fp64 (an fp32 weight converts exactly):
 *   Q[0][0] = p[0][0], Q[0][s > 0] = -inf;  Q[t][s] = p[s][t] + max(Q[t-1][s], Q[t-1][s-1]) with Q[t-1][-1] = -inf
 *   move[t][s] = Q[t-1][s-1] > Q[t-1][s]  (strict: a tie stays)
 *   a[Tb-1] = Sb-1, and from t to t-1 the position decreases by one if and only if move[t][a[t]]
 * which is the path with a[0] = 0, a[Tb-1] = Sb-1 and steps in {0, 1} that maximises sum_t p[a[t]][t] (a sum of weights, the
 * quantity of b2s_met_align_select's scores; zeros need no special case).
 * Outputs:
 *   path [B, T] int32: a[t], -1 from dec_len on
 *   durations [B, S] int32: frames per position, 0 from enc_len on; over the valid positions they sum to Tb and each is >= 1
 *   score [B] f64: Q[Tb-1][Sb-1]
 *   status [B] int32: B2S_DUR_OK; B2S_DUR_EMPTY (Sb == 0 or Tb == 0: path -1, durations 0, score 0); B2S_DUR_FAILED (a length
 *       outside 0..S or 0..T: nothing of that utterance is read; or a NaN / Inf among the Sb x Tb valid cells) and B2S_DUR_SHORT
 *       (Tb < Sb): path -1, durations 0, score NaN
 * No row from enc_len on is read, and no value from dec_len on reaches a result (the 16-byte load that holds frame Tb - 1 may
 * cover up to three later frames of the same row; they are dropped).
 *   ws: b2s_dur_ws_bytes(B, S, T) bytes, 8-byte aligned */
int b2s_dur_mas(const float *maps, const int32_t *enc_len, const int32_t *dec_len, int B, int S, int T, int32_t *path,
                int32_t *durations, double *score, int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* Duration error of x (prediction) against y (target).
 *   dur_x, dur_y [B, S] int32 (1 <= S <= B2S_DUR_MAX_S), enc_len [B] int32
 *   groups [B, S] int32, nullable: a non-decreasing unit id per position that starts at 0 and skips no value; the durations of
 *       one unit are summed first.  NULL: every position is its own unit
 * Outputs:
 *   counts [B, 12] int64 over the units (dx, dy = a unit's frames on either side): n, sum dx, sum dy, sum |dx - dy|,
 *       sum (dx - dy)^2, sum dx^2, sum dy^2, sum dx dy, max dx, max dy, units with dx == 0, units with dy == 0
 *   status [B] int32: B2S_DUR_OK; B2S_DUR_EMPTY for enc_len == 0; B2S_DUR_FAILED for a length outside 0..S, a negative duration,
 *       a side whose durations sum past 2^31 - 1 (the squares would leave int64), or groups that decrease, start above 0 or skip a
 *       value.  EMPTY and FAILED rows hold zeros */
int b2s_dur_score(const int32_t *dur_x, const int32_t *dur_y, const int32_t *enc_len, const int32_t *groups, int B, int S,
                  int64_t *counts, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
