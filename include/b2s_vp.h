/* C ABI of libb2s_vp.so: a variance predictor of a FastSpeech-2-style student for gfx950, forward and backward (DESIGN.md section
 * p).  The predictor is Conv1d(k=3) -> ReLU -> LayerNorm -> Dropout, the same again, then Linear to one scalar per position; the
 * student has one each for duration, pitch and energy.  Everything is fp32 and every operation is rounded on its own: the
 * definition below places every rounding, the results are the bits of the NumPy restatement (tests/vp_ref.py), the same from run to
 * run and for an utterance alone or inside a batch.
 *
 * Positions are padded per utterance ([B, S] with input_lengths [B]).  Every call launches on the caller's stream (NULL: the default
 * stream), creates no stream or graph, reads nothing back and does not synchronise.  Return codes: 0 = ok, otherwise
 * b2s_vp_last_error() holds the message (argument checks need no GPU; nothing aborts).  What is wrong with one utterance is its word
 * in status [B] and leaves the other utterances alone.  No atomics.
 *
 * Parameters, in torch's own layouts (a state_dict of nn.Conv1d / nn.LayerNorm / nn.Linear passes straight through):
 *   W1 [F, D, 3], b1 [F], g1, be1 [F]      conv1.weight, conv1.bias, norm1.weight, norm1.bias
 *   W2 [F, F, 3], b2 [F], g2, be2 [F]      conv2.weight, conv2.bias, norm2.weight, norm2.bias
 *   wl [F], bl [1]                         linear.weight, linear.bias
 *
 * Definition.  n = input_lengths[b].  Rows s >= n, and every row of an utterance that is not OK, read as +0.0 wherever a neighbour
 * tap looks at them.  tree(v) for v of length F: while the length is above 1, v = v[:len/2] + v[len/2:]; the result is v[0].
 *   conv (layer 1: in = x, C = D; layer 2: in = h1, C = F):
 *     a[s][f]: acc = bias[f]; then for j = 0, 1, 2, and c = 0..C-1 inside each j: acc = fmaf(in[s + j - 1][c], W[f][c][j], acc)
 *   r = a > 0 ? a : +0.0;  mu = tree(r) / F;  d = r - mu;  var = tree(d * d) / F;  rstd = 1.0f / sqrtf(var + eps)  (an add, a
 *     correctly rounded square root, a correctly rounded division);  xh = d * rstd;  nrm = (xh * g) + be
 *   h = nrm for p == 0, otherwise h = keep ? nrm * scale : +0.0
 *   dropout: idx = (b * S + s) * F + f as uint32;  keep = lowbias32(idx * 0x9E3779B1 + key) >= thresh;
 *     lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     key = lowbias32(seed_lo + 0x9E3779B9 * site) ^ lowbias32(seed_hi ^ 0x85EBCA6B), site = 1 or 2 for the layer
 *     thresh = (uint32) floor(p * 2^32) in fp64, scale = (float)(1 / (1 - p)), both made on the host; 0 <= p < 1
 *   linear: t[f] = h2[s][f] * wl[f];  pred[b][s] = tree(t) + bl;  pred is +0.0 for s >= n
 * Backward: dh2[s][f] = d_pred[s] * wl[f]; per layer (2, then 1):
 *   dn = dh for p == 0, otherwise keep ? dh * scale : +0.0;  dxh = dn * g;  m1 = tree(dxh) / F;  m2 = tree(dxh * xh) / F
 *   dr = ((dxh - m1) - (xh * m2)) * rstd;  da = a > 0 ? dr : +0.0
 *   din[s][c]: acc = +0.0; then for j = 0, 1, 2, and f = 0..F-1 inside each j: acc = fmaf(da[s + 1 - j][f], W[f][c][j], acc)
 *     (dh1 for layer 2, dx for layer 1)
 *   dW[f][c][j]: acc = +0.0; then over the OK utterances in ascending b, and s = 0..n-1 inside each:
 *     acc = fmaf(da[b][s][f], in[b][s + j - 1][c], acc);  db[f]: the same chain with plain additions of da[b][s][f]
 *   column sums in two levels: per utterance a chain over ascending s from +0.0, then a chain of additions over the OK b in
 *     ascending order from +0.0:  dbe[f] and dbl add dn[s][f] and d_pred[s];  dg[f]: acc = fmaf(dn[s][f], xh[s][f], acc);
 *     dwl[f]: acc = fmaf(d_pred[s], h2[s][f], acc)
 * Out of contract: non-finite inputs, NaN payloads, subnormal intermediates.
 */
#ifndef B2S_VP_H
#define B2S_VP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status values (those of the other satellite libraries) */
#define B2S_VP_OK 0
#define B2S_VP_EMPTY 1        /* input_lengths == 0: its pred row is zeros and it contributes nothing */
#define B2S_VP_FAILED 2       /* input_lengths outside 0..S: forward writes nothing but the status, it contributes nothing to any
                                 sum and its dx rows are +0.0 */

#define B2S_VP_MAX_S 1024     /* input positions per utterance */
#define B2S_VP_MAX_D 1024     /* input columns; D is a multiple of 4 in 4..B2S_VP_MAX_D */

/* Common to every call: 1 <= B <= 65535 (more: "split the batch"), 1 <= S <= B2S_VP_MAX_S, F (the filter size) in {64, 128, 256,
 * 512}, and no array of more than 2^31 elements ("sizes past one call").  Kernel width 3 and two conv layers are fixed.  The fp32
 * arrays are 16-byte aligned. */

int b2s_vp_version(void);
const char *b2s_vp_last_error(void);

/* Bytes of workspace forward and backward need (the same figure for both):
 *     256 + 2 * align256(3 * D * F * 4) + 2 * align256(3 * F * F * 4) + 3 * align256(B * S * F * 4) + align256((5 * F + 1) * B * 4)
 * with align256(v) = v rounded up to a multiple of 256: 256 bytes to bring any pointer to a region boundary; each conv weight
 * repacked twice, [3][C][F] for the forward and [3][F][C] for the input gradient; three [B, S, F] blocks (forward without a tape:
 * h1; backward: da2, dh1, da1); and the per-utterance partial column sums (dbe2, dg2, dwl, dbe1, dg1 [B, F] and dbl [B]).
 * 0 = refused (B, S, D or F outside its range, or sizes past one call), with the message in last_error. */
size_t b2s_vp_ws_bytes(int B, int S, int D, int F);

/* Bytes of the tape that forward writes for backward:
 *     5 * align256(B * S * F * 4) + 2 * align256(B * S * 4)
 * (a1, xh1, h1, a2, xh2 and the two rstd; the content is the implementation's).  0 = refused. */
size_t b2s_vp_tape_bytes(int B, int S, int F);

/* pred [B, S] f32 and status [B] int32 from x [B, S, D] f32, input_lengths [B] int32 and the parameters.  tape: NULL (inference) or
 * b2s_vp_tape_bytes bytes, 16-byte aligned.  ws: b2s_vp_ws_bytes bytes.  p in [0, 1) with seed: the dropout of both layers. */
int b2s_vp_forward(const float *x, const int32_t *input_lengths, const float *W1, const float *b1, const float *g1, const float *be1,
                   const float *W2, const float *b2, const float *g2, const float *be2, const float *wl, const float *bl, float eps,
                   double p, uint64_t seed, int B, int S, int D, int F, float *pred, int32_t *status, void *tape, void *ws,
                   size_t ws_bytes, void *stream);

/* The gradients of d_pred [B, S] f32 (rows s >= n are not read), from x, the parameters and the tape of the forward call with the
 * same p and seed.  Written, not accumulated: dx [B, S, D] (nullable) and the ten parameter gradients in the parameters' shapes,
 * which are NULL together (only dx is wanted, which must then be there) or not at all. */
int b2s_vp_backward(const float *x, const int32_t *input_lengths, const float *W1, const float *b1, const float *g1, const float *be1,
                    const float *W2, const float *b2, const float *g2, const float *be2, const float *wl, const float *bl,
                    const void *tape, const float *d_pred, double p, uint64_t seed, int B, int S, int D, int F, float *dx, float *dW1,
                    float *db1, float *dg1, float *dbe1, float *dW2, float *db2, float *dg2, float *dbe2, float *dwl, float *dbl,
                    void *ws, size_t ws_bytes, void *stream);

/* out_bytes [B, S, F] uint8: 1 where the dropout rule keeps the element at `site` (1 or 2), else 0.  For the tests. */
int b2s_vp_dropout_mask(double p, uint64_t seed, int site, int B, int S, int F, uint8_t *out_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
