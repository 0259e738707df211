// Batched silence splitting / trimming for gfx950 (C ABI: include/b2s_vocoder.h, the b2s_voc_silence_* entry points): librosa 0.6.0's
// effects.split / effects.trim and the reference's utils.audio.trim_silence_intervals on a ragged batch wav [B, Lmax] + lengths [B].
//
// Three steps, all on the caller's stream:
//   k_sil_energy     one block per (utterance, tile of frames): the tile's sample span is staged in LDS as squares through the reflect
//                    index; frame_length % hop == 0: per-hop partial sums (one wave per partial, butterfly reduction), then every frame
//                    adds its frame_length / hop partials in order -- a sample is squared and added once, not frame_length / hop times;
//                    otherwise every frame is summed directly.  fp32, fixed order: a frame's energy does not depend on the batch.  The
//                    utterance's maximum is an atomic max on the float's bit pattern (energies are >= 0, so bit order = value order).
//   k_sil_intervals  one block per utterance: level in double from the fp32 energies, flags, edges, block scan -> intervals, trim index,
//                    exclusive prefix of the interval lengths, output length.
//   k_sil_gather     pure copy of the kept samples into wav_out [B, Lmax], zero past out_lengths[b].
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../../include/b2s_vocoder.h"
#include "../side_common.h"

using b2s_side::align_up;
using b2s_side::fail;
using b2s_side::launch_status;

namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int SPAN_MAX = 12288;       // staged samples per block (48 KB of LDS): >= the largest frame_length
constexpr int TILE_MAX = 128;         // frames per block at most
constexpr int MIN_SLIDE_HOP = 16;     // below this a partial per wave wastes the wave: direct sums
constexpr int PART_MAX = TILE_MAX - 1 + 8192 / MIN_SLIDE_HOP;
constexpr int FL_MIN = 2, FL_MAX = 8192;
constexpr int GATHER_PER_BLOCK = NT * 16;

// NumPy 'reflect' index (no edge repeat), with the repeated reflection of a pad longer than the signal; n >= 2
__device__ __forceinline__ int reflect(int i, int n) {
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i >= n ? period - i : i;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__host__ __device__ __forceinline__ int n_frames(int L, int fl, int hop) { return 1 + (L + 2 * (fl / 2) - fl) / hop; }
__host__ __device__ __forceinline__ int tile_frames(int fl, int hop) {
    const int t = (SPAN_MAX - fl) / hop + 1;
    return t < TILE_MAX ? t : TILE_MAX;
}
__device__ __forceinline__ int clamp_len(int L, int Lmax) { return L < 2 ? 2 : (L > Lmax ? Lmax : L); }

__global__ __launch_bounds__(NT) void k_sil_energy(const float *__restrict__ wav, const int32_t *__restrict__ lens, int Lmax, int fl, int hop,
                                                   int tile, int Fmax, float *__restrict__ mse, unsigned int *__restrict__ maxbits) {
    __shared__ float s[SPAN_MAX];
    __shared__ float part[PART_MAX];
    __shared__ float e[TILE_MAX];
    __shared__ float wmax[NW];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = clamp_len(lens[b], Lmax), F = n_frames(L, fl, hop);
    const int f0 = blockIdx.x * tile;
    if (f0 >= F) return;
    const int nf = min(tile, F - f0);
    const int span = (nf - 1) * hop + fl;                        // <= SPAN_MAX by the choice of `tile`
    const int g0 = f0 * hop - fl / 2;                            // sample index of the span's first element (before reflection)
    const float *y = wav + (size_t)b * Lmax;
    // 16-byte loads where four consecutive samples are inside the signal and the address is aligned; the reflected ends are scalar
    const int mis = (int)((((intptr_t)y >> 2) + g0) & 3);
    const int head = (4 - mis) & 3;
    for (int i = tid; i < min(head, span); i += NT) {
        const float v = y[reflect(g0 + i, L)];
        s[i] = v * v;
    }
    for (int i = head + 4 * tid; i < span; i += 4 * NT) {
        const int g = g0 + i;
        if (g >= 0 && g + 3 < L && i + 3 < span) {
            const float4 v = *reinterpret_cast<const float4 *>(y + g);
            s[i] = v.x * v.x; s[i + 1] = v.y * v.y; s[i + 2] = v.z * v.z; s[i + 3] = v.w * v.w;
        } else {
            for (int k = 0; k < 4 && i + k < span; ++k) {
                const float v = y[reflect(g + k, L)];
                s[i + k] = v * v;
            }
        }
    }
    __syncthreads();
    if (fl % hop == 0 && hop >= MIN_SLIDE_HOP) {
        const int R = fl / hop, np = nf - 1 + R;                 // np * hop == span
        for (int h = wv; h < np; h += NW) {
            float acc = 0.f;
            for (int i = lane; i < hop; i += 64) acc += s[h * hop + i];
            acc = wave_sum(acc);
            if (lane == 0) part[h] = acc;
        }
        __syncthreads();
        if (tid < nf) {
            float acc = 0.f;
            for (int r = 0; r < R; ++r) acc += part[tid + r];
            e[tid] = acc;
        }
    } else {
        for (int f = wv; f < nf; f += NW) {
            float acc = 0.f;
            for (int i = lane; i < fl; i += 64) acc += s[f * hop + i];
            acc = wave_sum(acc);
            if (lane == 0) e[f] = acc;
        }
    }
    __syncthreads();
    float m = 0.f;
    if (tid < nf) {
        m = e[tid] / (float)fl;
        mse[(size_t)b * Fmax + f0 + tid] = m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) wmax[wv] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) m = fmaxf(m, wmax[w]);
        atomicMax(maxbits + b, __float_as_uint(m));
    }
}

// exclusive prefix sum of v over the block (NT threads); total = the block's sum.  Ends with a barrier, safe to call in a loop.
__device__ __forceinline__ int block_excl_scan(int v, int *wsum, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int w = 0; w < NW; ++w) {
        if (w < wv) base += wsum[w];
        total += wsum[w];
    }
    __syncthreads();
    return base + inc - v;
}

__device__ __forceinline__ bool nonsilent(const float *__restrict__ m, int f, int F, double ref, double top_db) {
    if (f < 0 || f >= F) return false;
    return 10.0 * log10(fmax(1e-10, (double)m[f])) - ref > -top_db;
}

__global__ __launch_bounds__(NT) void k_sil_intervals(const float *__restrict__ mse, const unsigned int *__restrict__ maxbits,
                                                      const int32_t *__restrict__ lens, int Lmax, int fl, int hop, int Fmax, int NI, double top_db,
                                                      int32_t *__restrict__ intervals, int32_t *__restrict__ n_intervals,
                                                      int32_t *__restrict__ trim_index, int32_t *__restrict__ prefix,
                                                      int32_t *__restrict__ out_lengths, uint8_t *__restrict__ flags) {
    __shared__ int wsum[NW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = clamp_len(lens[b], Lmax), F = n_frames(L, fl, hop);
    const float *m = mse + (size_t)b * Fmax;
    const double ref = 10.0 * log10(fmax(1e-10, (double)__uint_as_float(maxbits[b])));
    int32_t *iv = intervals + (size_t)b * NI * 2;
    // edge at position k in 0..F where the flag changes between frame k - 1 and frame k (frames -1 and F count as silent)
    int n_edges = 0;
    for (int k0 = 0; k0 <= F; k0 += NT) {
        const int k = k0 + tid;
        const bool cur = nonsilent(m, k, F, ref, top_db);
        const bool edge = k <= F && cur != nonsilent(m, k - 1, F, ref, top_db);
        if (flags && k < F) flags[(size_t)b * Fmax + k] = cur;
        int total;
        const int at = n_edges + block_excl_scan(edge, wsum, total);
        if (edge) iv[at] = min((long long)k * hop, (long long)L);      // at < 2 * ceil(F / 2): the edges come in pairs
        n_edges += total;
    }
    const int n = n_edges / 2;
    __syncthreads();                                             // the block's own interval writes are visible to it from here
    int32_t *pre = prefix + (size_t)b * NI;
    int kept = 0;
    for (int i0 = 0; i0 < n; i0 += NT) {
        const int i = i0 + tid;
        const int len = i < n ? iv[2 * i + 1] - iv[2 * i] : 0;
        int total;
        const int at = kept + block_excl_scan(len, wsum, total);
        if (i < n) pre[i] = at;
        kept += total;
    }
    if (tid == 0) {
        n_intervals[b] = n;
        out_lengths[b] = kept;
        trim_index[2 * b] = n ? iv[0] : 0;
        trim_index[2 * b + 1] = n ? iv[2 * n - 1] : 0;
    }
}

__global__ __launch_bounds__(NT) void k_sil_gather(const float *__restrict__ wav, int Lmax, int NI, const int32_t *__restrict__ intervals,
                                                   const int32_t *__restrict__ n_intervals, const int32_t *__restrict__ prefix,
                                                   const int32_t *__restrict__ out_lengths, float *__restrict__ wav_out) {
    const int b = blockIdx.y;
    const int n = min(n_intervals[b], NI), kept = min(out_lengths[b], Lmax);
    const int32_t *iv = intervals + (size_t)b * NI * 2, *pre = prefix + (size_t)b * NI;
    const float *y = wav + (size_t)b * Lmax;
    float *out = wav_out + (size_t)b * Lmax;
    const int o0 = blockIdx.x * GATHER_PER_BLOCK, o1 = min(o0 + GATHER_PER_BLOCK, Lmax);
    for (int o = o0 + threadIdx.x; o < o1; o += NT) {
        float v = 0.f;
        if (o < kept) {
            int lo = 0, hi = n - 1;                              // largest i with pre[i] <= o
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= o) lo = mid; else hi = mid - 1;
            }
            const int src = iv[2 * lo] + (o - pre[lo]);
            if (src >= 0 && src < Lmax) v = y[src];
        }
        out[o] = v;
    }
}

int check_shape(const char *what, int B, int Lmax, int fl, int hop) {
    if (B <= 0) return fail("%s: B must be > 0 (got %d)", what, B);
    if (Lmax < 2) return fail("%s: Lmax must be >= 2 samples (got %d); every utterance needs at least 2", what, Lmax);
    if (fl < FL_MIN || fl > FL_MAX) return fail("%s: frame_length must be in %d..%d (got %d)", what, FL_MIN, FL_MAX, fl);
    if (hop < 1 || hop > fl) return fail("%s: hop_length must be in 1..frame_length=%d (got %d)", what, fl, hop);
    if ((long long)Lmax + fl >= (1LL << 30)) return fail("%s: Lmax %d is too long", what, Lmax);
    return 0;
}

}  // namespace

extern "C" {

size_t b2s_voc_silence_ws_bytes(int B, int Lmax, int frame_length, int hop_length) {
    if (check_shape("silence_ws_bytes", B, Lmax, frame_length, hop_length)) return 0;
    const int Fmax = n_frames(Lmax, frame_length, hop_length);
    return align_up(sizeof(float) * (size_t)B * Fmax) + align_up(sizeof(unsigned int) * (size_t)B);
}

int b2s_voc_silence_split(const float *wav, const int32_t *lengths, int B, int Lmax, double top_db, int frame_length, int hop_length,
                          int32_t *intervals, int32_t *n_intervals, int32_t *trim_index, int32_t *prefix, int32_t *out_lengths,
                          uint8_t *flags, void *ws, size_t ws_bytes, void *stream) {
    if (check_shape("silence_split", B, Lmax, frame_length, hop_length)) return 1;
    if (!(top_db > 0.0)) return fail("silence_split: top_db must be > 0 (got %g)", top_db);
    if (!wav || !lengths || !intervals || !n_intervals || !trim_index || !prefix || !out_lengths || !ws)
        return fail("silence_split: a pointer argument is NULL");
    const size_t need = b2s_voc_silence_ws_bytes(B, Lmax, frame_length, hop_length);
    if (ws_bytes < need) return fail("silence_split: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int Fmax = n_frames(Lmax, frame_length, hop_length), NI = (Fmax + 1) / 2;
    const int tile = tile_frames(frame_length, hop_length);
    hipStream_t st = (hipStream_t)stream;
    float *mse = (float *)ws;
    unsigned int *maxbits = (unsigned int *)((char *)ws + align_up(sizeof(float) * (size_t)B * Fmax));
    const hipError_t me = hipMemsetAsync(maxbits, 0, sizeof(unsigned int) * (size_t)B, st);
    if (me != hipSuccess) return fail("silence_split: clearing the maxima failed: %s", hipGetErrorString(me));
    hipLaunchKernelGGL(k_sil_energy, dim3((Fmax + tile - 1) / tile, B), dim3(NT), 0, st, wav, lengths, Lmax, frame_length, hop_length, tile,
                       Fmax, mse, maxbits);
    hipLaunchKernelGGL(k_sil_intervals, dim3(B), dim3(NT), 0, st, mse, maxbits, lengths, Lmax, frame_length, hop_length, Fmax, NI, top_db,
                       intervals, n_intervals, trim_index, prefix, out_lengths, flags);
    return launch_status("silence_split");
}

int b2s_voc_silence_gather(const float *wav, int B, int Lmax, int frame_length, int hop_length, const int32_t *intervals,
                           const int32_t *n_intervals, const int32_t *prefix, const int32_t *out_lengths, float *wav_out, void *stream) {
    if (check_shape("silence_gather", B, Lmax, frame_length, hop_length)) return 1;
    if (!wav || !intervals || !n_intervals || !prefix || !out_lengths || !wav_out) return fail("silence_gather: a pointer argument is NULL");
    const int NI = (n_frames(Lmax, frame_length, hop_length) + 1) / 2;
    hipLaunchKernelGGL(k_sil_gather, dim3((Lmax + GATHER_PER_BLOCK - 1) / GATHER_PER_BLOCK, B), dim3(NT), 0, (hipStream_t)stream, wav, Lmax, NI,
                       intervals, n_intervals, prefix, out_lengths, wav_out);
    return launch_status("silence_gather");
}

}  // extern "C"
