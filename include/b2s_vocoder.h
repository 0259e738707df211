/* C ABI of libb2s_vocoder.so: batched Griffin-Lim vocoder (mel -> wav), mel front end (wav -> mel) and silence splitting / trimming
 * (the b2s_voc_silence_* calls at the end, which take their own parameters instead of B2SVocParams) for gfx950.
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

#ifdef __cplusplus
}
#endif
#endif
