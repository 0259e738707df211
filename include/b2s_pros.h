/* C ABI of libb2s_pros.so: batched prosody targets for gfx950 (DESIGN.md section n).  Three calls: b2s_pros_energy (int16 PCM -> one
 * exact window energy per frame), b2s_pros_track (YIN's CMND matrix -> the pitch track of the least summed cost, a Viterbi search
 * over the states "unvoiced" and "lag k") and b2s_pros_units (frame-level F0, voicing and energy -> sums per input unit of a
 * duration vector, and the continuous F0 contour in between).
 *
 * Every operation is specified: integers are exact, and every fp64 product, sum, quotient and comparison is written out below in
 * the order it is made, with no fused multiply-add.  The results are the bits of the NumPy restatement (tests/pros_ref.py), the same
 * from run to run and for an utterance alone or inside a batch.
 *
 * Frames are packed per utterance by frame_offsets [B + 1] int32, as b2s_f0_yin takes and b2s_hip.f0.yin_batch returns them.  Every
 * call launches on the caller's stream (NULL: the default stream), creates no stream or graph, reads nothing back and does not
 * synchronise.  Return codes: 0 = ok, otherwise b2s_pros_last_error() holds the message (argument checks need no GPU; nothing
 * aborts).  What is wrong with one utterance is its word in status [B] and leaves the other utterances' outputs alone.  No atomics.
 */
#ifndef B2S_PROS_H
#define B2S_PROS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status values (the first three are those of the other satellite libraries) */
#define B2S_PROS_OK 0
#define B2S_PROS_EMPTY 1      /* track: no frame; units: input_lengths == 0 */
#define B2S_PROS_FAILED 2     /* offsets or a length that do not fit the sizes; track: a NaN or Inf among the lags; units: see there */
#define B2S_PROS_SHORT 3      /* units: the durations sum to more frames than the utterance has */
#define B2S_PROS_NOVOICE 4    /* units: no voiced frame among the frames the durations cover */

#define B2S_PROS_MAX_WIN 2048 /* samples per energy window */
#define B2S_PROS_MAX_LAGS 512 /* lag states tau_min..tau_max of the search: one lane each in one workgroup */
#define B2S_PROS_MAX_W 64     /* half width of the transition band */
#define B2S_PROS_MAX_S 1024   /* input positions of b2s_pros_units */

int b2s_pros_version(void);
const char *b2s_pros_last_error(void);

/* Bytes of workspace b2s_pros_track needs for total_frames frames and the lags tau_min..tau_max: one back-pointer byte per frame
 * and lag (rows of 64 * ceil(lags / 64) bytes) and one int32 per frame for the unvoiced state.  0 = refused (total_frames < 0,
 * tau_min < 1, tau_max < tau_min, more than B2S_PROS_MAX_LAGS lags, or sizes past one call), with the message in last_error.
 * b2s_pros_units needs 4 * total_frames bytes, which is never more. */
size_t b2s_pros_ws_bytes(int total_frames, int tau_min, int tau_max);

/* Window energy per frame.
 *   pcm [B, Lmax] int16, lengths [B] int32, frame_offsets [B + 1] int32 with F_b = 1 + L_b / hop frames per utterance (YIN's count)
 *   win in 1..B2S_PROS_MAX_WIN, hop >= 1
 * E[frame_offsets[b] + t] = sum_{i < win} p[t * hop - win / 2 + i]^2 with p = 0 outside [0, L_b): an exact int64 (below 2^41).
 *   status [B] int32: B2S_PROS_OK, or B2S_PROS_FAILED when L_b is outside 0..Lmax, frame_offsets[b] < 0, frame_offsets[b + 1] >
 *       total_frames or frame_offsets[b + 1] - frame_offsets[b] != 1 + L_b / hop; nothing is read or written for that utterance */
int b2s_pros_energy(const int16_t *pcm, const int32_t *lengths, const int32_t *frame_offsets, int total_frames, int B, int Lmax,
                    int win, int hop, int64_t *energy, int32_t *status, void *stream);

/* Viterbi pitch track over the CMND matrix.
 *   cmnd [total_frames, K] f64, K > tau_max: row t holds c[0..K) of frame t (b2s_f0_yin's cmnd_out, K = tau_max + 1)
 *   energy [total_frames] int64 and floor (int64): frame t is gated off when energy[t] < floor
 *   1 <= tau_min <= tau_max, at most B2S_PROS_MAX_LAGS lags; sr, u, v, lam, mu finite (fp64); 0 <= W <= B2S_PROS_MAX_W
 * States: 0 (unvoiced) and the lags k = tau_min..tau_max.  With t counted inside the utterance:
 *   loc[t][0] = u;  loc[t][k] = +inf for a gated frame, else c[t][k] + fl(mu * (double)k)
 *   Q[0][s] = loc[0][s]
 *   state 0, t >= 1: best = Q[t-1][0], arg = 0; for k' = tau_min..tau_max ascending: cand = Q[t-1][k'] + v, taken when cand < best
 *   state k, t >= 1: best = Q[t-1][0] + v, arg = 0; for k' = max(tau_min, k - W)..min(tau_max, k + W) ascending:
 *       cand = Q[t-1][k'] + fl(lam * (double)|k - k'|), taken when cand < best
 *   Q[t][s] = loc[t][s] + best
 *   end: best = Q[F-1][0], state 0; for k ascending: Q[F-1][k] taken when < best; then the back-pointers are walked
 * Every comparison is strict, so a tie goes to state 0 first and then to the smallest lag.
 * Outputs:
 *   tau [total_frames] int32: the state per frame, 0 = unvoiced
 *   f0 [total_frames] f64: 0 for unvoiced, else sr / (tau + shift) with b2s_f0_yin's parabola on c (without the mu term):
 *       a = c[tau - 1], b = c[tau], cc = c[tau + 1] when 1 <= tau - 1 and tau + 1 <= tau_max: den = (a - b) + (cc - b); den > 0:
 *       shift = 0.5 * (a - cc) / den, kept when |shift| <= 1
 *   score [B] f64: the final Q; 0 for EMPTY, NaN for FAILED
 *   status [B] int32: B2S_PROS_OK; B2S_PROS_EMPTY (no frame); B2S_PROS_FAILED for offsets that decrease or leave 0..total_frames
 *       (nothing is read or written for that utterance) and for a NaN or Inf among c[t][tau_min..tau_max] of any of its frames,
 *       gated ones included (tau and f0 zero)
 *   ws: b2s_pros_ws_bytes(total_frames, tau_min, tau_max) bytes, 4-byte aligned */
int b2s_pros_track(const double *cmnd, const int64_t *energy, int64_t floor, const int32_t *frame_offsets, int total_frames, int B,
                   int K, int tau_min, int tau_max, double sr, double u, double v, double lam, double mu, int W, int32_t *tau,
                   double *f0, double *score, int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* Sums per input unit, and the continuous contour.
 *   f0 [total_frames] f64, tau [total_frames] int32 (voiced: tau > 0), energy [total_frames] int64, frame_offsets [B + 1]
 *   durations [B, S] int32 (1 <= S <= B2S_PROS_MAX_S), input_lengths [B] int32
 *   groups [B, S] int32, nullable: a non-decreasing unit id per position that starts at 0 and skips no value (b2s_hip.durations.
 *       code_point_groups); NULL: every position is its own unit
 * With n = sum of durations[b][:input_lengths[b]] the call uses the first n of the utterance's F frames; unit j covers the frames
 * of its positions, in order.
 *   cont [total_frames] f64: a voiced frame keeps its f0; an unvoiced frame t between its nearest voiced neighbours a < t < b gets
 *       f0[a] + (f0[b] - f0[a]) * ((double)(t - a) / (double)(b - a)) (difference, quotient, product, sum, each rounded); before the
 *       first voiced frame the first voiced value, after the last the last; 0 from frame n on
 *   frames, voiced [B, S] int32, f0_voiced_sum, f0_cont_sum [B, S] f64 (over the unit's voiced frames / all its frames, in frame
 *       order, left to right), energy_sum [B, S] int64; zero from the unit count on, and a unit of 0 frames is all zeros
 *   units [B] int32: the unit count
 *   status [B] int32: B2S_PROS_OK; B2S_PROS_EMPTY (input_lengths == 0); B2S_PROS_FAILED (offsets that decrease or leave
 *       0..total_frames: only status and units are written for that utterance; input_lengths outside 0..S, a negative duration, or groups that
 *       decrease, start above 0 or skip a value); B2S_PROS_SHORT (n > F).  These rows hold zeros, cont over the F frames
 *       included, and units 0.  B2S_PROS_NOVOICE (no voiced frame among the n): cont 0, the counts and energy sums as for OK
 *   ws: 4 * total_frames bytes, 4-byte aligned */
int b2s_pros_units(const double *f0, const int32_t *tau, const int64_t *energy, const int32_t *frame_offsets, int total_frames,
                   const int32_t *durations, const int32_t *input_lengths, const int32_t *groups, int B, int S, double *cont,
                   int32_t *frames, int32_t *voiced, double *f0_voiced_sum, double *f0_cont_sum, int64_t *energy_sum, int32_t *units,
                   int32_t *status, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
