/* C ABI of libb2s_va.so: the variance adaptor of a FastSpeech-2-style student for gfx950, forward and backward (DESIGN.md section
 * o).  Five calls: b2s_va_quantise (pitch or energy per position -> a bin), b2s_va_frames (durations -> frames per utterance),
 * b2s_va_forward (encoder rows plus one embedding row per bin, each repeated for as many frames as its duration: the length
 * regulator), b2s_va_backward (the transposed operation: a sum over each position's frames, and a sum of the position gradients
 * into the embedding tables) and b2s_va_pad (the packed frames as one padded block per utterance for the decoder, and back).
 *
 * Every output bit is decided by the definition: integers and comparisons are exact, and every fp32 sum is written out below in
 * the order it is made, one rounded addition at a time.  The results are the bits of the NumPy restatement (tests/va_ref.py), the
 * same from run to run and for an utterance alone or inside a batch.
 *
 * Positions are padded per utterance ([B, S] with input_lengths [B]); frames are packed by frame_offsets [B + 1] int32.  Every call
 * launches on the caller's stream (NULL: the default stream), creates no stream or graph, reads nothing back and does not
 * synchronise.  Return codes: 0 = ok, otherwise b2s_va_last_error() holds the message (argument checks need no GPU; nothing
 * aborts).  What is wrong with one utterance is its word in status [B] and leaves the other utterances alone.  No atomics.
 */
#ifndef B2S_VA_H
#define B2S_VA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status values (those of the other satellite libraries) */
#define B2S_VA_OK 0
#define B2S_VA_EMPTY 1        /* input_lengths == 0 */
#define B2S_VA_FAILED 2       /* see each call */

#define B2S_VA_MAX_S 1024     /* input positions per utterance */
#define B2S_VA_MAX_D 1024     /* columns; D is a multiple of 4 in 4..B2S_VA_MAX_D */
#define B2S_VA_MAX_BINS 256   /* rows of an embedding table */
#define B2S_VA_MAX_FRAMES (1 << 20) /* frames of one utterance */

/* Common to every call: 1 <= B <= 65535 (more: "split the batch"), 1 <= S <= B2S_VA_MAX_S, and no array of more than 2^31
 * elements ("sizes past one call").  The fp32 arrays x, h, y, dy, dx and the tables are 16-byte aligned. */

int b2s_va_version(void);
const char *b2s_va_last_error(void);

/* Bytes of workspace b2s_va_backward needs:
 *     16 + 2 * (align256(B * S * D * 4) + align256(B * n_bins * 4))
 * with align256(v) = v rounded up to a multiple of 256: 16 bytes to bring a 4-byte aligned workspace to the rows' 16, and per table
 * one partial-sum row per (utterance, position) -- the row of a bin sits at the first position of the utterance that uses the bin
 * -- and one int32 per (utterance, bin) that names that position.
 * 0 = refused (B, S, D or n_bins outside its range, or sizes past one call), with the message in last_error. */
size_t b2s_va_ws_bytes(int B, int S, int D, int n_bins);

/* Bins of a value per position.
 *   values [B, S] f64, input_lengths [B] int32, boundaries [n_bins - 1] f64 (1 <= n_bins <= B2S_VA_MAX_BINS; NULL allowed for 1)
 * bins[b][s] = the number of j with boundaries[j] < values[b][s] (strict, in fp64: torch.bucketize(right=False),
 * np.searchsorted(side="left")) for s < input_lengths[b], and 0 from there on.
 *   status [B] int32: B2S_VA_OK; B2S_VA_EMPTY (input_lengths == 0); B2S_VA_FAILED when input_lengths is outside 0..S or a NaN sits
 *       among the first input_lengths values (bins all 0), and for EVERY utterance when the boundaries are not finite and strictly
 *       ascending (checked on the device; bins all 0) */
int b2s_va_quantise(const double *values, const int32_t *input_lengths, const double *boundaries, int n_bins, int B, int S,
                    int32_t *bins, int32_t *status, void *stream);

/* Frames per utterance.
 *   durations [B, S] int32, input_lengths [B] int32
 * frames[b] = the int64 sum of durations[b][:input_lengths[b]].
 *   status [B] int32: B2S_VA_OK; B2S_VA_EMPTY (input_lengths == 0); B2S_VA_FAILED when input_lengths is outside 0..S, a duration
 *       among the first input_lengths is negative or the sum passes B2S_VA_MAX_FRAMES (frames[b] = 0) */
int b2s_va_frames(const int32_t *durations, const int32_t *input_lengths, int B, int S, int32_t *frames, int32_t *status,
                  void *stream);

/* Embed and expand.
 *   x [B, S, D] f32; pitch_bins, energy_bins [B, S] int32 with pitch_table, energy_table [n_bins, D] f32: a table and its bins are
 *       NULL together, and that term is then not added at all (which is not the same as adding zero: a -0.0 of x stays)
 *   durations [B, S] int32, input_lengths [B] int32, frame_offsets [B + 1] int32, total_frames >= 0
 * With n = input_lengths[b], for s < n:
 *   h[b][s][:] = (x[b][s][:] + pitch_table[pitch_bins[b][s]][:]) + energy_table[energy_bins[b][s]][:]     two fp32 additions
 *   rows s >= n of h are +0.0
 * With c[s] = the sum of the durations before position s, frame t of utterance b belongs to the position s with c[s] <= t < c[s+1]:
 *   y[frame_offsets[b] + t][:] = h[b][s][:]        unit_of_frame[frame_offsets[b] + t] = s
 * Outputs: h [B, S, D] f32 (nullable), y [total_frames, D] f32, unit_of_frame [total_frames] int32 (nullable),
 *   status [B] int32: B2S_VA_OK; B2S_VA_EMPTY (n == 0 and no frame; its h rows are zeros); B2S_VA_FAILED when n is outside 0..S, a
 *       duration among the first n is negative, their sum passes B2S_VA_MAX_FRAMES, a bin among the first n is outside
 *       0..n_bins-1, the offsets decrease or leave 0..total_frames, or frame_offsets[b+1] - frame_offsets[b] differs from the sum
 *       of the durations: nothing but the status is written for that utterance
 * total_frames == 0 is legal (y and unit_of_frame may be NULL): the statuses and h are written and nothing else. */
int b2s_va_forward(const float *x, const int32_t *pitch_bins, const int32_t *energy_bins, const float *pitch_table,
                   const float *energy_table, int n_bins, const int32_t *durations, const int32_t *input_lengths,
                   const int32_t *frame_offsets, int total_frames, int B, int S, int D, float *h, float *y, int32_t *unit_of_frame,
                   int32_t *status, void *stream);

/* The transposed operation.  The index arguments, their validation and the statuses are those of b2s_va_forward.
 *   dy [total_frames, D] f32
 *   dx [B, S, D] f32: dx[b][s][:] starts from +0.0f and gets dy[frame_offsets[b] + t][:] of the position's frames added in frame
 *       order, one rounded fp32 addition each; a position of 0 frames, a position s >= n and every row of an utterance that is not
 *       OK are +0.0
 *   d_pitch_table, d_energy_table [n_bins, D] f32, each nullable with its bins (the forward's table pointers are not needed):
 *       part[b][k][:] starts from +0.0f and gets dx[b][s][:] added for s ascending over the positions s < n whose bin is k (all
 *       +0.0 for an utterance that is not OK); d_table[k][:] starts from +0.0f and gets part[b][k][:] added for b = 0..B-1
 *       ascending.  The tables are written, not accumulated into.
 *   ws: b2s_va_ws_bytes(B, S, D, n_bins) bytes, 4-byte aligned
 * A sum that started at +0.0 is never -0.0 and adding +0.0 leaves it as it is, so the utterances and bins that contribute nothing
 * are skipped; the order of the other additions is the one above. */
int b2s_va_backward(const float *dy, const int32_t *pitch_bins, const int32_t *energy_bins, int n_bins, const int32_t *durations,
                    const int32_t *input_lengths, const int32_t *frame_offsets, int total_frames, int B, int S, int D, float *dx,
                    float *d_pitch_table, float *d_energy_table, int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* Packed frames to one padded block per utterance, and back.
 *   frames [total_frames, D] f32 packed by frame_offsets [B + 1] int32, padded [B, T, D] f32 (1 <= T <= B2S_VA_MAX_FRAMES)
 * to_frames == 0: padded[b][t][:] = frames[frame_offsets[b] + t][:] for t below the utterance's frame count and +0.0 behind it.
 * to_frames != 0: frames[frame_offsets[b] + t][:] = padded[b][t][:] (the transposed copy; what lies behind is not read).
 *   status [B] int32: B2S_VA_OK; B2S_VA_EMPTY (no frame; to_frames == 0 writes its T rows of zeros); B2S_VA_FAILED for offsets that
 *       decrease or leave 0..total_frames and for more than T frames: nothing but the status is written for that utterance */
int b2s_va_pad(float *frames, const int32_t *frame_offsets, int total_frames, int B, int T, int D, float *padded, int to_frames,
               int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
