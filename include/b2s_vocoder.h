/* C ABI of libb2s_vocoder.so: batched Griffin-Lim vocoder (mel -> wav), mel front end (wav -> mel), silence splitting / trimming
 * (the b2s_voc_silence_* calls, which take their own parameters instead of B2SVocParams), corpus preparation (the b2s_voc_prep_*
 * calls) and down-mixing / resampling to 16 kHz (the b2s_voc_resample* calls at the end) for gfx950.  Thirteen entry points.
 *
 * The reference's utils/audio.py (librosa 0.6.0 semantics) on the GPU, fp32 throughout.  Only n_fft 2048, win 800, hop 200 and
 * 80 mels are compiled in; any other value is refused with an error naming the supported set.  Utterances are packed ragged:
 * frame f is (b, t) with t < T_b and f = frame_offsets[b] + t (frame_offsets = exclusive prefix sum of the lengths, B + 1 int32
 * entries on the device).  Every call launches on the caller's stream, creates no stream or graph and does not synchronise.
 * Return codes: 0 = ok, otherwise b2s_voc_last_error() holds the message (argument checks need no GPU; nothing aborts).
 */
#ifndef B2S_VOCODER_H
#define B2S_VOCODER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t sr, n_fft, hop, win, n_mels;
    float preemphasis, ref_db, max_db, max_abs_value, power;
    int32_t symmetric_mel;
} B2SVocParams;

#define B2S_VOC_WS_MEL2WAV 0
#define B2S_VOC_WS_WAV2MEL 1

int b2s_voc_version(void);
const char *b2s_voc_last_error(void);

/* Workspace bytes for `which` (B2S_VOC_WS_MEL2WAV or B2S_VOC_WS_WAV2MEL); 0 on an argument error (message set). */
size_t b2s_voc_ws_bytes(const B2SVocParams *p, int B, int total_frames, int max_frames, int which);

/* mels [B, Tmax, n_mels] fp32 (normalised, padded) -> wav_out [B, hop * (Tmax - 1)] fp32, zero past hop * (T_b - 1).
 * Every T_b >= 2.  inv_basis = pinv(mel basis) transposed: [n_mels, 1 + n_fft / 2] fp32.  n_iter >= 0 Griffin-Lim iterations. */
int b2s_voc_mel2wav(const B2SVocParams *p, const float *mels, const int32_t *frame_offsets, int B, int Tmax, int total_frames,
                    int n_iter, const float *inv_basis, float *wav_out, void *ws, size_t ws_bytes, void *stream);

/* wav [B, Lmax] fp32 (padded), lengths [B] int32 samples (>= 2) -> mels_out [B, 1 + Lmax / hop, n_mels] fp32 (rows t < 1 + L_b / hop
 * written, the rest left untouched).  basis = mel basis [n_mels, 1 + n_fft / 2] fp32. */
int b2s_voc_wav2mel(const B2SVocParams *p, const float *wav, const int32_t *lengths, const int32_t *frame_offsets, int B, int Lmax,
                    int total_frames, const float *basis, float *mels_out, void *ws, size_t ws_bytes, void *stream);

/* Silence splitting / trimming (librosa 0.6.0 effects.split / effects.trim semantics; csrc/vocoder/silence.hip).  Ragged batch:
 * wav [B, Lmax] fp32, lengths [B] int32 samples on the device, every L_b in 2..Lmax (a length outside is clamped, never read past).
 * frame_length in 2..8192, 1 <= hop_length <= frame_length, top_db > 0.  With Fmax = 1 + (Lmax + 2 * (frame_length / 2) -
 * frame_length) / hop_length frames at most and NI = (Fmax + 1) / 2 intervals at most:
 *   intervals [B, NI, 2] int32   [start, end) in samples, rows i < n_intervals[b] written
 *   n_intervals [B], trim_index [B, 2] (effects.trim's start, end), out_lengths [B] = kept samples
 *   prefix [B, NI]               exclusive prefix sum of the interval lengths (where interval i starts in the gathered output)
 *   flags [B, Fmax] uint8        the non-silent flag of every frame f < F_b; may be NULL */
size_t b2s_voc_silence_ws_bytes(int B, int Lmax, int frame_length, int hop_length);   /* 0 on an argument error (message set) */

int b2s_voc_silence_split(const float *wav, const int32_t *lengths, int B, int Lmax, double top_db, int frame_length, int hop_length,
                          int32_t *intervals, int32_t *n_intervals, int32_t *trim_index, int32_t *prefix, int32_t *out_lengths,
                          uint8_t *flags, void *ws, size_t ws_bytes, void *stream);

/* wav_out [B, Lmax] fp32 = the samples of the intervals of b2s_voc_silence_split (same B, Lmax, frame_length, hop_length), concatenated,
 * zero from out_lengths[b] on.  A pure copy: kept samples are bit-equal to the input's. */
int b2s_voc_silence_gather(const float *wav, int B, int Lmax, int frame_length, int hop_length, const int32_t *intervals,
                           const int32_t *n_intervals, const int32_t *prefix, const int32_t *out_lengths, float *wav_out, void *stream);

/* Corpus preparation: the body of the reference's corpora/process_corpus.py trim_audios on a ragged batch (csrc/vocoder/prep.hip).
 * wav [B, Lmax] fp32, lengths [B] int32 on the device, every L_b in 2..Lmax (a length outside is clamped, never read past).  Per utterance:
 *   1. intervals = split at (top_db 40, frame_length 2048, hop 512); ref = max |y|, mv_i = max |y| over interval i
 *   2. from the front, then from the back, while more than one interval is left: drop a zero-length interval; drop one with
 *      (mv < ref / 10 or (len <= gap / 2 and mv < ref / 4)) and gap >= 4096, gap = the distance to its neighbour; stop at the first kept.
 *      ref / 10 and ref / 4 are fp32 quotients of the fp32 maxima.  n_removed = intervals dropped.
 *   3. status GAP if two neighbouring kept intervals are >= gap_threshold samples apart (the reference: 12288, or 16000 for some corpora)
 *   4. v95 = the k-th smallest (0-based) |y| over the N samples of the kept intervals, k = (int)((double)N * 0.95): exactly
 *      np.sort(np.abs(voiced))[int(len(voiced) * 0.95)], bit for bit, by a radix select on the bit patterns
 *   5. scale = (float)(0.244 / (double)v95); y2 = y * scale in fp32, cropped to [first kept start, last kept end).  This is the
 *      reference's arithmetic under the NumPy 1.x it was written for: a Python float divided by an fp32 scalar is fp64 there, and an
 *      fp32 array times that scalar stays fp32 (NumPy 2 would do the division in fp32).
 *   6. (l, r) = trim index of y2 at (40, 256, 64)
 *   7. out = 1600 samples before l, y2[l:r], 2400 samples after r, taken from y2 where it has them and zero where not:
 *      out_len = r - l + 4000.  status LENGTH unless 16000 <= out_len <= 320000.
 * status SILENT: ref == 0 or v95 == 0.  The reference divides by zero there and writes a file of NaNs; skipping such a file under a
 * name of its own is a deliberate deviation.  Precedence: GAP, then SILENT, then LENGTH.
 *   out [B, Lmax + 4000] fp32, zero from out_lengths[b] on; out_lengths, status, n_removed [B] int32; v95 [B] fp32
 * Of an utterance whose status is not OK only status and n_removed are specified; nothing is read or written out of bounds for it. */
#define B2S_VOC_PREP_OK 0
#define B2S_VOC_PREP_GAP 1
#define B2S_VOC_PREP_LENGTH 2
#define B2S_VOC_PREP_SILENT 3

#define B2S_VOC_WS_PREP_TRIM 0
#define B2S_VOC_WS_PREP_QUANTILE 1

size_t b2s_voc_prep_ws_bytes(int B, int Lmax, int which);   /* 0 on an argument error (message set) */

int b2s_voc_prep_trim(const float *wav, const int32_t *lengths, int B, int Lmax, int gap_threshold, float *out, int32_t *out_lengths,
                      int32_t *status, int32_t *n_removed, float *v95, void *ws, size_t ws_bytes, void *stream);

/* Step 4 alone.  intervals [B, NI, 2] int32: [start, end) sample ranges, ascending and disjoint (values outside 0..L_b are clamped),
 * the first n_intervals[b] <= NI of every row used.  out[b] = the k-th smallest |y| over the N samples the intervals cover,
 * k = min((int)((double)N * fraction), N - 1), 0 <= fraction < 1; 0.0f if N == 0.  Bit-equal to sorting, whatever the ties. */
int b2s_voc_prep_abs_quantile(const float *wav, const int32_t *lengths, int B, int Lmax, const int32_t *intervals,
                              const int32_t *n_intervals, int NI, double fraction, float *out, void *ws, size_t ws_bytes, void *stream);

/* Down-mix and resampling to 16 kHz: the arithmetic of librosa 0.6.0's load(path, sr=16000) on a ragged batch (csrc/vocoder/resample.hip).
 * wav [B, Lmax_in, channels] fp32 (interleaved, padded), lengths [B] int32 frames on the device (clamped into 0..Lmax_in; the padding past
 * a length may hold anything and is never read).  One sample rate and one channel count per call.  Per utterance:
 *   1. mono = np.mean over the channels: a left-to-right fp32 sum, one fp32 division by `channels` (1..8; 1 is used as it is)
 *   2. orig_sr == 16000: out = mono, bit for bit.  Otherwise resampy's 'kaiser_best' filter: 64 zero crossings, 512 table steps per
 *      crossing, rolloff 0.9475937167399596, Kaiser beta 14.769656459379492, the table scaled by ratio = 16000 / orig_sr when that
 *      is < 1, index_step = (int)(min(1, ratio) * 512).  For t < n_valid[b]: time = t * (1 / ratio), n = (int)time,
 *      frac = min(1, ratio) * (time - n) in fp64; out[t] = sum over the left wing (x[n - i]) then the right wing (x[n + 1 + k]) of
 *      (win[o] + eta * (win[o + 1] - win[o])) * x, o = off + i * index_step, off = (int)(frac * 512), eta = frac * 512 - off,
 *      the right wing with frac' = min(1, ratio) - frac.  The table is fp32 (computed in fp64), the sum is fp32.
 *   3. out [B, Lmax_out] fp32 is zero from n_valid[b] to Lmax_out (librosa's fix_length to n_out[b] pads with zeros).
 * n_valid [B] = int(N * ratio) and n_out [B] = int(ceil(N * ratio)), int32 on the device, are the caller's: computed in Python floats
 * exactly as written and never recomputed here (n_out only documents the row's length; nothing past n_valid is non-zero).
 * The filter table is rebuilt into the workspace on every call (32 770 entries); nothing is kept between calls.  A workgroup
 * interpolates a tile of 4096 consecutive outputs of one utterance, halved (down to 256) until the input span of the tile,
 * ceil(tile / ratio) + 2 * (32769 / index_step) + 4 samples rounded up to a multiple of 4, is at most 8064 floats: it is staged
 * in LDS beside the table.  b2s_hip.prep.resample_tile(orig_sr) restates that rule.  orig_sr in 4000..192000. */
size_t b2s_voc_resample_ws_bytes(int B, int Lmax_in, int channels, int orig_sr);   /* 0 on an argument error (message set) */

int b2s_voc_resample(const float *wav, const int32_t *lengths, int B, int Lmax_in, int channels, int orig_sr, const int32_t *n_valid,
                     const int32_t *n_out, int Lmax_out, float *out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
