/* C ABI of libb2s_metrics.so: batched FastDTW (fastdtw 0.3.4 semantics, euclidean distance) and the MSE-after-DTW eval metric
 * for gfx950, the selection of the alignment head that the eval plots (b2s_met_align_*) and the batched edit distance behind the
 * eval's CER (b2s_met_edit_*, at the end).
 *
 * Utterances are packed ragged: frame f of pair b is row x_offsets[b] + f of x (x_offsets = exclusive prefix sum of the lengths,
 * B + 1 int32 entries on the device), fp32 rows of `dim` features, 1 <= dim <= 256; the same for y.  Distances, the pyramid and the
 * cumulative costs are fp64.  radius >= 1 is fastdtw(x, y, radius); radius == -1 is the exact dtw(x, y) (full matrix); radius 0 is
 * refused (fastdtw 0.3.4 cannot backtrack through its window for odd lengths).  Every call launches on the caller's stream, creates
 * no stream or graph and does not synchronise.  Return codes: 0 = ok, otherwise b2s_met_last_error() holds the message (argument
 * checks need no GPU; nothing aborts).
 */
#ifndef B2S_METRICS_H
#define B2S_METRICS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* keep only the voiced frames (rows whose maximum over the features is > 0) of each side before the DTW, as the reference's
 * calculate_mse_dtw does; path indices then refer to the voiced frames */
#define B2S_MET_VOICED_ONLY 1

/* status_out values */
#define B2S_MET_OK 0
#define B2S_MET_EMPTY 1       /* one side has no (voiced) frame: cost, mse = NaN, path_len = 0 (the reference's None) */
#define B2S_MET_FAILED 2      /* offsets inconsistent with total / max arguments, or a path longer than its path_offsets slot */

int b2s_met_version(void);
const char *b2s_met_last_error(void);

/* Workspace bytes for one b2s_met_dtw call with these sizes; 0 on an argument error (message set).  max_x / max_y bound every
 * pair's length (the on-chip plan is sized by them). */
size_t b2s_met_dtw_ws_bytes(int B, int total_x, int total_y, int max_x, int max_y, int dim, int radius, int flags);

/* cost_out[B] f64 = D[len_x, len_y]; mse_out[B] f64 = mean((x[path_x] - y[path_y])^2) over path length x dim (fp64 over the fp32
 * inputs); path_len_out[B] int32; status_out[B] int32 (B2S_MET_*).  path_out (nullable): int32 (i, j) pairs, pair b's path written
 * in order from pair index path_offsets[b]; path_offsets (B + 1 int32 on the device, required with path_out) gives each pair a slot
 * of path_offsets[b + 1] - path_offsets[b] >= len_x + len_y - 1 pairs. */
int b2s_met_dtw(const float *x, const int32_t *x_offsets, int total_x, int max_x, const float *y, const int32_t *y_offsets,
                int total_y, int max_y, int B, int dim, int radius, int flags, double *cost_out, double *mse_out,
                int32_t *path_len_out, int32_t *status_out, int32_t *path_out, const int32_t *path_offsets, void *ws,
                size_t ws_bytes, void *stream);

/* ---- alignment-head selection (csrc/metrics/align.hip) ----
 * The reference's plot_attn picks, per utterance, the encoder-decoder attention head with the largest sum over decoder frames of the
 * per-frame maximum over encoder positions, and draws that one map.  b2s_met_align_select does the selection on the device, so that
 * one [S, T] map per utterance leaves it instead of n_layers * H, and summarises the chosen head's argmax path.
 *
 * layers: HOST array of n_layers (1..16) device pointers, each [B, H, S, T] contiguous fp32 with T innermost (what
 * b2s_decode_alignment writes); they travel in the kernel arguments.  enc_len / dec_len: device int32 [B], clamped to [0, S] and
 * [0, T]; rows s >= enc_len and frames t >= dec_len are never read.
 *   scores_out[B, n_layers, H] f64 = sum_{t < dec_len} max_{s < enc_len} A_l[b, h, s, t]: the maximum exact in fp32, the sum fp64 in
 *       a fixed order (per chunk of b2s_met_align_chunk() frames, then over the chunks), bit-reproducible from run to run
 *   best_out[B] int32 = l * H + h of the largest score: strict > against a running best that starts at 0, layers then heads in order
 *       (the first wins a tie); -1 when no score is > 0
 *   map_out[B, S, T] f32 (nullable) = the chosen head's slab unchanged; zeros for best -1
 *   path_out[B, T] int32 (nullable) = first index of the maximum over s < enc_len of the chosen head at frame t; -1 for t >= dec_len
 *       and for best -1
 *   stats_out[B, 4] int32 (nullable), over that path p: #{t >= 1: p[t] < p[t-1]}, max(p[t] - p[t-1], 0), the number of distinct
 *       positions, p[dec_len - 1]; zeros when there is no path */
int b2s_met_align_chunk(void);
size_t b2s_met_align_ws_bytes(int B, int n_layers, int H, int S, int T);
int b2s_met_align_select(const float *const *layers, int n_layers, int B, int H, int S, int T, const int32_t *enc_len,
                         const int32_t *dec_len, double *scores_out, int32_t *best_out, float *map_out, int32_t *path_out,
                         int32_t *stats_out, void *ws, size_t ws_bytes, void *stream);

/* ---- batched edit distance (csrc/metrics/edit.hip) ----
 * Levenshtein distance with unit costs over ragged pairs of int32 symbol sequences (code points, bytes, word ids: only equality is
 * used): symbol i of side a of pair p is a[a_offsets[p] + i], offsets as above (exclusive prefix sums, B + 1 int32 on the device).
 * a is the truth, b the prediction; each side holds at most b2s_met_edit_max_len() = 4096 symbols, and max_a / max_b (0..4096) bound
 * every pair's lengths (the launch is sized by max_b).  Per pair the result is the lexicographically smallest (cost, substitutions)
 * over all alignments, which fixes the breakdown: del - ins = len_a - len_b and cost = sub + del + ins.  A deletion is a truth symbol
 * missing from the prediction, an insertion the reverse.  An empty side is no error: cost = the other side's length.
 *   dist_out[B] int32 = cost; -1 where status is FAILED
 *   ops_out[B, 3] int32 (nullable) = sub, del, ins; -1, -1, -1 where status is FAILED
 *   status_out[B] int32 = B2S_MET_OK, or B2S_MET_FAILED for a pair whose offsets decrease or run outside 0..total_*, or whose length
 *       exceeds max_*: its symbols are not read
 * One launch on the caller's stream, no workspace; B <= 0, negative totals, max_* outside 0..4096 and NULL required pointers are
 * refused on the host. */
int b2s_met_edit_max_len(void);
int b2s_met_edit_distance(const int32_t *a, const int32_t *a_offsets, int total_a, int max_a, const int32_t *b,
                          const int32_t *b_offsets, int total_b, int max_b, int B, int32_t *dist_out, int32_t *ops_out,
                          int32_t *status_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
