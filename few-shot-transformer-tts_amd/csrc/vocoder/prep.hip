// Batched corpus preparation for gfx950 (C ABI: include/b2s_vocoder.h, the b2s_voc_prep_* entry points): the body of the reference's
// corpora/process_corpus.py trim_audios on a ragged batch wav [B, Lmax] + lengths [B].  Everything is launched on the caller's stream;
// no stream or graph is created and nothing synchronises with the host.
//
//   split (40, 2048, 512)     b2s_voc_silence_split (silence.hip)
//   k_prep_peaks              one block per (utterance, tile): |y| bit patterns staged in LDS; the tile's maximum goes into ref[b] and the
//                             maximum over every interval's part of the tile into mv[b, i], both by an atomic max on the bit pattern
//                             (non-negative floats order like their bits, so the result does not depend on the order)
//   k_prep_select             one block per utterance: the reference's two `while` loops over the intervals, the gap test, status
//   k_prep_hist<P> / k_prep_scan<P>, P = 0, 1, 2
//                             exact order statistic of |y| over the kept intervals: radix select over bits 31..21, 20..10, 9..0.  A hist
//                             block owns a tile of 16 384 samples, decides once which intervals touch the tile (a tile inside one
//                             interval takes every sample without a test), counts into an LDS histogram and flushes the non-empty bins
//                             with integer atomics; a scan block per utterance picks the bin that holds the rank, keeps the residual
//                             rank and clears the histogram for the next pass.  Integer counts: independent of scheduling.
//   k_prep_plan, k_prep_scale scale = (float)(0.244 / (double)v95); y2 = y * scale (fp32), cropped to the kept range, zero after
//   split (40, 256, 64)       b2s_voc_silence_split on y2 -> trim index (l, r)
//   k_prep_margins            out = y2[l - 1600, r + 2400) with zeros where y2 has no sample; out_len, final status
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../../include/b2s_vocoder.h"
#include "../side_common.h"

using b2s_side::align_up;
using b2s_side::fail;
using b2s_side::launch_status;

namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int BINS = 2048;
constexpr int HIST_TILE = NT * 4 * 16;        // samples per histogram block
constexpr int PEAK_TILE = NT * 4 * 4;         // samples per peak block (their bit patterns fit 16 KB of LDS)
constexpr int COPY_TILE = NT * 16;
constexpr int FL1 = 2048, HOP1 = 512, FL2 = 256, HOP2 = 64;
constexpr double TOP_DB = 40.0;
constexpr int LEAD = 1600, TAIL = 2400, MIN_OUT = 16000, MAX_OUT = 320000, SPIKE_GAP = 4096;
constexpr unsigned ABS_MASK = 0x7fffffffu;

struct SelState { unsigned prefix, rank, n, pad; };

__host__ __device__ __forceinline__ int n_frames(int L, int fl, int hop) { return 1 + (L + 2 * (fl / 2) - fl) / hop; }
__host__ __device__ __forceinline__ int max_intervals(int Lmax, int fl, int hop) { return (n_frames(Lmax, fl, hop) + 1) / 2; }
__device__ __forceinline__ int clamp_len(int L, int Lmax) { return L < 2 ? 2 : (L > Lmax ? Lmax : L); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// interval j of a list, clamped into [0, L] with end >= start: nothing a caller passes can send a read out of the row
__device__ __forceinline__ void interval(const int32_t *__restrict__ iv, int j, int L, int &s, int &e) {
    s = clampi(iv[2 * j], 0, L);
    e = clampi(iv[2 * j + 1], s, L);
}

// first j in [k0, k1] whose end is > pos (k1 + 1 if none); the intervals are ascending and disjoint
__device__ __forceinline__ int first_ending_after(const int32_t *__restrict__ iv, int k0, int k1, int L, int pos) {
    int lo = k0, hi = k1 + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int s, e;
        interval(iv, mid, L, s, e);
        if (e > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the four samples at row index g .. g + 3 (16-byte aligned by the caller's choice of tile origin) as |y| bit patterns; 0 outside [0, L)
__device__ __forceinline__ void load4_abs(const float *__restrict__ y, int g, int L, unsigned (&u)[4]) {
    if (g >= 0 && g + 3 < L) {
        const uint4 v = *reinterpret_cast<const uint4 *>(y + g);
        u[0] = v.x & ABS_MASK; u[1] = v.y & ABS_MASK; u[2] = v.z & ABS_MASK; u[3] = v.w & ABS_MASK;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = (g + k >= 0 && g + k < L) ? (__float_as_uint(y[g + k]) & ABS_MASK) : 0u;
    }
}

__device__ __forceinline__ unsigned block_max(unsigned v, unsigned *wred) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned m = wred[0];
    for (int w = 1; w < NW; ++w) m = max(m, wred[w]);
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(NT) void k_prep_peaks(const float *__restrict__ wav, const int32_t *__restrict__ lens, int Lmax,
                                                   const int32_t *__restrict__ intervals, const int32_t *__restrict__ n_intervals, int NI,
                                                   unsigned *__restrict__ refbits, unsigned *__restrict__ mvbits) {
    __shared__ unsigned s[PEAK_TILE];
    __shared__ unsigned wred[NW];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int L = clamp_len(lens[b], Lmax);
    const float *y = wav + (size_t)b * Lmax;
    const int mis = (int)(((uintptr_t)y >> 2) & 3);
    const int t0 = blockIdx.x * PEAK_TILE - mis;
    const int lo = max(t0, 0), hi = min(t0 + PEAK_TILE, L);
    if (lo >= hi) return;
    unsigned m = 0;
    for (int i = 4 * tid; i < PEAK_TILE; i += 4 * NT) {
        unsigned u[4];
        load4_abs(y, t0 + i, L, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[i + k] = u[k];
            m = max(m, u[k]);
        }
    }
    m = block_max(m, wred);                                      // its barriers also publish s[]
    if (tid == 0) atomicMax(refbits + b, m);
    const int32_t *iv = intervals + (size_t)b * NI * 2;
    const int n = clampi(n_intervals[b], 0, NI);
    for (int j = first_ending_after(iv, 0, n - 1, L, lo); j < n; ++j) {
        int a, e;
        interval(iv, j, L, a, e);
        if (a >= hi) break;
        a = max(a, lo);
        e = min(e, hi);
        unsigned mj = 0;
        for (int g = a + tid; g < e; g += NT) mj = max(mj, s[g - t0]);
        mj = block_max(mj, wred);
        if (tid == 0 && e > a) atomicMax(mvbits + (size_t)b * NI + j, mj);
    }
}

// The reference's noise-spike removal and gap test (process_corpus.py:50-93).  ref and mv are fp32 maxima; ref / 10 and ref / 4 are fp32.
__global__ void k_prep_select(const int32_t *__restrict__ lens, int Lmax, const int32_t *__restrict__ intervals,
                              const int32_t *__restrict__ n_intervals, int NI, const unsigned *__restrict__ refbits,
                              const unsigned *__restrict__ mvbits, int gap_threshold, int32_t *__restrict__ kept,
                              int32_t *__restrict__ status, int32_t *__restrict__ n_removed) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int L = clamp_len(lens[b], Lmax);
    const int32_t *iv = intervals + (size_t)b * NI * 2;
    const unsigned *mvb = mvbits + (size_t)b * NI;
    const int n = clampi(n_intervals[b], 0, NI);
    const float ref = __uint_as_float(refbits[b]);
    const float tenth = ref / 10.0f, quarter = ref / 4.0f;
    int lo = 0, hi = n - 1, removed = 0;
    while (hi > lo) {
        int s, e, s1, e1;
        interval(iv, lo, L, s, e);
        if (s == e) { ++lo; ++removed; continue; }
        interval(iv, lo + 1, L, s1, e1);
        const int gap = s1 - e;
        const float mv = __uint_as_float(mvb[lo]);
        if ((mv < tenth || (e - s <= gap / 2 && mv < quarter)) && gap >= SPIKE_GAP) { ++lo; ++removed; } else break;
    }
    while (hi > lo) {
        int s, e, s1, e1;
        interval(iv, hi, L, s, e);
        if (s == e) { --hi; ++removed; continue; }
        interval(iv, hi - 1, L, s1, e1);
        const int gap = s - e1;
        const float mv = __uint_as_float(mvb[hi]);
        if ((mv < tenth || (e - s <= gap / 2 && mv < quarter)) && gap >= SPIKE_GAP) { --hi; ++removed; } else break;
    }
    int st = n <= 0 ? B2S_VOC_PREP_SILENT : B2S_VOC_PREP_OK;
    for (int k = lo; k < hi; ++k) {
        int s, e, s1, e1;
        interval(iv, k, L, s, e);
        interval(iv, k + 1, L, s1, e1);
        if (s1 - e >= gap_threshold) { st = B2S_VOC_PREP_GAP; break; }
    }
    if (st == B2S_VOC_PREP_OK && ref == 0.0f) st = B2S_VOC_PREP_SILENT;
    kept[2 * b] = lo;
    kept[2 * b + 1] = hi;
    status[b] = st;
    n_removed[b] = removed;
}

template <int PASS>
__device__ __forceinline__ void count(unsigned bits, unsigned prefix, unsigned *h) {
    if (PASS == 0) atomicAdd(h + (bits >> 21), 1u);
    else if (PASS == 1) { if ((bits >> 21) == (prefix >> 21)) atomicAdd(h + ((bits >> 10) & 2047u), 1u); }
    else { if ((bits >> 10) == (prefix >> 10)) atomicAdd(h + (bits & 1023u), 1u); }
}

// kept == NULL: all n_intervals[b] intervals of the list; otherwise the inclusive index range kept[b] = (first, last)
template <int PASS>
__global__ __launch_bounds__(NT) void k_prep_hist(const float *__restrict__ wav, const int32_t *__restrict__ lens, int Lmax,
                                                  const int32_t *__restrict__ intervals, const int32_t *__restrict__ n_intervals,
                                                  const int32_t *__restrict__ kept, int NI, const SelState *__restrict__ state,
                                                  unsigned *__restrict__ hist) {
    __shared__ unsigned h[BINS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int L = clamp_len(lens[b], Lmax);
    const float *y = wav + (size_t)b * Lmax;
    const int mis = (int)(((uintptr_t)y >> 2) & 3);
    const int t0 = blockIdx.x * HIST_TILE - mis;
    const int lo = max(t0, 0), hi = min(t0 + HIST_TILE, L);
    if (lo >= hi) return;
    const int n = clampi(n_intervals[b], 0, NI);
    const int k0 = kept ? clampi(kept[2 * b], 0, n) : 0, k1 = kept ? clampi(kept[2 * b + 1], -1, n - 1) : n - 1;
    if (k1 < k0) return;
    const int32_t *iv = intervals + (size_t)b * NI * 2;
    const int j0 = first_ending_after(iv, k0, k1, L, lo);
    if (j0 > k1) return;
    int s0, e0;
    interval(iv, j0, L, s0, e0);
    if (s0 >= hi) return;                                        // the tile lies in a gap
    const unsigned prefix = PASS ? state[b].prefix : 0u;
    if (PASS && state[b].n == 0) return;
    for (int i = tid; i < BINS; i += NT) h[i] = 0;
    __syncthreads();
    if (s0 <= lo && e0 >= hi) {                                  // the tile lies inside one interval: every sample of [lo, hi) counts
        for (int i = 4 * tid; i < HIST_TILE; i += 4 * NT) {
            const int g = t0 + i;
            if (g >= hi) break;
            unsigned u[4];
            load4_abs(y, g, L, u);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (g + k >= lo && g + k < hi) count<PASS>(u[k], prefix, h);
        }
    } else {                                                     // a thread's samples ascend, so its interval cursor only moves forward
        int j = j0, s = s0, e = e0;
        for (int i = 4 * tid; i < HIST_TILE; i += 4 * NT) {
            const int g = t0 + i;
            if (g >= hi || j > k1) break;
            unsigned u[4];
            load4_abs(y, g, L, u);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = g + k;
                while (j <= k1 && e <= p) {
                    ++j;
                    if (j <= k1) interval(iv, j, L, s, e);
                }
                if (j <= k1 && p >= s && p >= lo && p < hi) count<PASS>(u[k], prefix, h);
            }
        }
    }
    __syncthreads();
    unsigned *gh = hist + (size_t)b * BINS;
    for (int i = tid; i < BINS; i += NT)
        if (h[i]) atomicAdd(gh + i, h[i]);
}

// One block per utterance: the bin that holds the rank.  PASS 0 also fixes the rank: n = the number of counted samples,
// rank = min((int)((double)n * fraction), n - 1).  The last pass writes the value; n == 0 gives 0.0f.
template <int PASS>
__global__ __launch_bounds__(NT) void k_prep_scan(unsigned *__restrict__ hist, SelState *__restrict__ state, double fraction,
                                                  float *__restrict__ out) {
    __shared__ unsigned wsum[NW];
    constexpr int PER = BINS / NT;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned *gh = hist + (size_t)b * BINS + tid * PER;
    const SelState st = state[b];
    unsigned c[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        c[k] = gh[k];
        gh[k] = 0;
        sum += c[k];
    }
    unsigned inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned base = 0, total = 0;
    for (int w = 0; w < NW; ++w) {
        if (w < wv) base += wsum[w];
        total += wsum[w];
    }
    base += inc - sum;
    unsigned n = st.n, rank = st.rank, prefix = st.prefix;
    if (PASS == 0) {
        n = total;
        prefix = 0;
        rank = 0;
        if (n) {
            const unsigned k = (unsigned)(int)((double)n * fraction);
            rank = k < n ? k : n - 1;
        }
    }
    if (n == 0) {
        if (tid == 0) {
            state[b] = SelState{0u, 0u, 0u, 0u};
            if (PASS == 2) out[b] = 0.0f;
        }
        return;
    }
    if (sum && rank >= base && rank < base + sum) {              // exactly one thread
        unsigned cum = base;
        int k = 0;
        while (k < PER - 1 && rank >= cum + c[k]) cum += c[k++];
        const unsigned bin = (unsigned)(tid * PER + k);
        prefix |= PASS == 0 ? bin << 21 : (PASS == 1 ? bin << 10 : bin);
        state[b] = SelState{prefix, rank - cum, n, 0u};
        if (PASS == 2) out[b] = __uint_as_float(prefix);
    }
}

// scale, crop range and the `silent` status of every utterance; plan[b] = (crop start, len2)
__global__ void k_prep_plan(const int32_t *__restrict__ lens, int Lmax, const int32_t *__restrict__ intervals, int NI,
                            const int32_t *__restrict__ n_intervals, const int32_t *__restrict__ kept, const float *__restrict__ v95,
                            int32_t *__restrict__ status, float *__restrict__ scale, int32_t *__restrict__ plan, int32_t *__restrict__ len2,
                            int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int L = clamp_len(lens[b], Lmax);
    const int n = clampi(n_intervals[b], 0, NI);
    int st = status[b];
    if (st == B2S_VOC_PREP_OK && !(v95[b] > 0.0f)) st = B2S_VOC_PREP_SILENT;
    int c0 = 0, c1 = 0;
    float sc = 0.0f;
    if (st == B2S_VOC_PREP_OK && n > 0) {
        const int32_t *iv = intervals + (size_t)b * NI * 2;
        int s, e;
        interval(iv, clampi(kept[2 * b], 0, n - 1), L, c0, e);
        interval(iv, clampi(kept[2 * b + 1], 0, n - 1), L, s, c1);
        c1 = max(c1, c0);
        sc = (float)(0.244 / (double)v95[b]);
    }
    status[b] = st;
    scale[b] = sc;
    plan[2 * b] = c0;
    plan[2 * b + 1] = c1 - c0;
    len2[b] = c1 - c0;                                           // the second split clamps it into 2..Lmax; the row is zero past it
}

__global__ __launch_bounds__(NT) void k_prep_scale(const float *__restrict__ wav, int Lmax, const float *__restrict__ scale,
                                                   const int32_t *__restrict__ plan, float *__restrict__ y2) {
    const int b = blockIdx.y;
    const int c0 = plan[2 * b], n2 = plan[2 * b + 1];
    const float sc = scale[b];
    const float *y = wav + (size_t)b * Lmax;
    float *o = y2 + (size_t)b * Lmax;
    const int o0 = blockIdx.x * COPY_TILE, o1 = min(o0 + COPY_TILE, Lmax);
    for (int i = o0 + threadIdx.x; i < o1; i += NT) o[i] = i < n2 ? y[c0 + i] * sc : 0.0f;      // c0 + n2 <= L
}

__global__ __launch_bounds__(NT) void k_prep_margins(const float *__restrict__ y2, int Lmax, const int32_t *__restrict__ plan,
                                                     const int32_t *__restrict__ trim2, float *__restrict__ out,
                                                     int32_t *__restrict__ out_lengths, int32_t *__restrict__ status) {
    const int b = blockIdx.y, W = Lmax + LEAD + TAIL;
    const int n2 = plan[2 * b + 1];
    const int st = status[b];
    const bool live = st == B2S_VOC_PREP_OK || st == B2S_VOC_PREP_LENGTH;
    const int l = clampi(trim2[2 * b], 0, n2), r = clampi(trim2[2 * b + 1], l, n2);
    const int out_len = live ? r - l + LEAD + TAIL : 0;
    const float *y = y2 + (size_t)b * Lmax;
    float *o = out + (size_t)b * W;
    const int o0 = blockIdx.x * COPY_TILE, o1 = min(o0 + COPY_TILE, W);
    for (int i = o0 + threadIdx.x; i < o1; i += NT) {
        const int src = l - LEAD + i;
        o[i] = (i < out_len && src >= 0 && src < n2) ? y[src] : 0.0f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out_lengths[b] = out_len;
        if (st == B2S_VOC_PREP_OK && (out_len < MIN_OUT || out_len > MAX_OUT)) status[b] = B2S_VOC_PREP_LENGTH;
    }
}

int check_shape(const char *what, int B, int Lmax) {
    if (B <= 0) return fail("%s: B must be > 0 (got %d)", what, B);
    if (B > 65535) return fail("%s: B must be <= 65535 (got %d)", what, B);
    if (Lmax < 2) return fail("%s: Lmax must be >= 2 samples (got %d); every utterance needs at least 2", what, Lmax);
    if ((long long)Lmax + LEAD + TAIL + FL1 >= (1LL << 30)) return fail("%s: Lmax %d is too long", what, Lmax);
    return 0;
}

struct Layout {
    size_t hist, state, total_quantile;
    size_t sil, iv1, n1, trim1, pre1, ol1, ref, mv, kept, scale, plan, len2, y2, iv2, n2, trim2, pre2, ol2, total;
    int NI1, NI2;
};

Layout layout(int B, int Lmax) {
    Layout l;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align_up(bytes); return o; };
    const size_t i32 = sizeof(int32_t);
    l.NI1 = max_intervals(Lmax, FL1, HOP1);
    l.NI2 = max_intervals(Lmax, FL2, HOP2);
    l.hist = take(sizeof(unsigned) * (size_t)B * BINS);
    l.state = take(sizeof(SelState) * (size_t)B);
    l.total_quantile = at;
    const size_t s1 = b2s_voc_silence_ws_bytes(B, Lmax, FL1, HOP1), s2 = b2s_voc_silence_ws_bytes(B, Lmax, FL2, HOP2);
    l.sil = take(s1 > s2 ? s1 : s2);
    l.iv1 = take(i32 * (size_t)B * l.NI1 * 2);
    l.n1 = take(i32 * B);
    l.trim1 = take(i32 * B * 2);
    l.pre1 = take(i32 * (size_t)B * l.NI1);
    l.ol1 = take(i32 * B);
    l.ref = take(sizeof(unsigned) * (size_t)B);                  // ref and mv are adjacent: one memset clears both
    l.mv = take(sizeof(unsigned) * (size_t)B * l.NI1);
    l.kept = take(i32 * B * 2);
    l.scale = take(sizeof(float) * (size_t)B);
    l.plan = take(i32 * B * 2);
    l.len2 = take(i32 * B);
    l.y2 = take(sizeof(float) * (size_t)B * Lmax);
    l.iv2 = take(i32 * (size_t)B * l.NI2 * 2);
    l.n2 = take(i32 * B);
    l.trim2 = take(i32 * B * 2);
    l.pre2 = take(i32 * (size_t)B * l.NI2);
    l.ol2 = take(i32 * B);
    l.total = at;
    return l;
}

// the three histogram / scan passes; hist must be zero on entry and is zero again on exit
void select_passes(const float *wav, const int32_t *lengths, int B, int Lmax, const int32_t *intervals, const int32_t *n_intervals,
                   const int32_t *kept, int NI, double fraction, unsigned *hist, SelState *state, float *out, hipStream_t st) {
    const dim3 grid((Lmax + 3 + HIST_TILE - 1) / HIST_TILE, B);
    hipLaunchKernelGGL(k_prep_hist<0>, grid, dim3(NT), 0, st, wav, lengths, Lmax, intervals, n_intervals, kept, NI, state, hist);
    hipLaunchKernelGGL(k_prep_scan<0>, dim3(B), dim3(NT), 0, st, hist, state, fraction, out);
    hipLaunchKernelGGL(k_prep_hist<1>, grid, dim3(NT), 0, st, wav, lengths, Lmax, intervals, n_intervals, kept, NI, state, hist);
    hipLaunchKernelGGL(k_prep_scan<1>, dim3(B), dim3(NT), 0, st, hist, state, fraction, out);
    hipLaunchKernelGGL(k_prep_hist<2>, grid, dim3(NT), 0, st, wav, lengths, Lmax, intervals, n_intervals, kept, NI, state, hist);
    hipLaunchKernelGGL(k_prep_scan<2>, dim3(B), dim3(NT), 0, st, hist, state, fraction, out);
}

}  // namespace

extern "C" {

size_t b2s_voc_prep_ws_bytes(int B, int Lmax, int which) {
    if (check_shape("prep_ws_bytes", B, Lmax)) return 0;
    if (which != B2S_VOC_WS_PREP_TRIM && which != B2S_VOC_WS_PREP_QUANTILE) { fail("prep_ws_bytes: unknown workspace kind %d", which); return 0; }
    const Layout l = layout(B, Lmax);
    return which == B2S_VOC_WS_PREP_TRIM ? l.total : l.total_quantile;
}

int b2s_voc_prep_abs_quantile(const float *wav, const int32_t *lengths, int B, int Lmax, const int32_t *intervals,
                              const int32_t *n_intervals, int NI, double fraction, float *out, void *ws, size_t ws_bytes, void *stream) {
    if (check_shape("prep_abs_quantile", B, Lmax)) return 1;
    if (NI <= 0) return fail("prep_abs_quantile: NI must be > 0 (got %d)", NI);
    if (!(fraction >= 0.0 && fraction < 1.0)) return fail("prep_abs_quantile: fraction must be in [0, 1) (got %g)", fraction);
    if (!wav || !lengths || !intervals || !n_intervals || !out || !ws) return fail("prep_abs_quantile: a pointer argument is NULL");
    const Layout l = layout(B, Lmax);
    if (ws_bytes < l.total_quantile) return fail("prep_abs_quantile: workspace of %zu bytes, %zu needed", ws_bytes, l.total_quantile);
    hipStream_t st = (hipStream_t)stream;
    unsigned *hist = (unsigned *)((char *)ws + l.hist);
    const hipError_t me = hipMemsetAsync(hist, 0, l.total_quantile, st);
    if (me != hipSuccess) return fail("prep_abs_quantile: clearing the histograms failed: %s", hipGetErrorString(me));
    select_passes(wav, lengths, B, Lmax, intervals, n_intervals, nullptr, NI, fraction, hist, (SelState *)((char *)ws + l.state), out, st);
    return launch_status("prep_abs_quantile");
}

int b2s_voc_prep_trim(const float *wav, const int32_t *lengths, int B, int Lmax, int gap_threshold, float *out, int32_t *out_lengths,
                      int32_t *status, int32_t *n_removed, float *v95, void *ws, size_t ws_bytes, void *stream) {
    if (check_shape("prep_trim", B, Lmax)) return 1;
    if (gap_threshold <= 0) return fail("prep_trim: gap_threshold must be > 0 samples (got %d)", gap_threshold);
    if (!wav || !lengths || !out || !out_lengths || !status || !n_removed || !v95 || !ws) return fail("prep_trim: a pointer argument is NULL");
    const Layout l = layout(B, Lmax);
    if (ws_bytes < l.total) return fail("prep_trim: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    auto i32 = [&](size_t off) { return (int32_t *)(w + off); };
    unsigned *hist = (unsigned *)(w + l.hist), *ref = (unsigned *)(w + l.ref), *mv = (unsigned *)(w + l.mv);
    SelState *state = (SelState *)(w + l.state);
    float *scale = (float *)(w + l.scale), *y2 = (float *)(w + l.y2);
    hipError_t me = hipMemsetAsync(hist, 0, l.total_quantile, st);
    if (me == hipSuccess) me = hipMemsetAsync(ref, 0, l.kept - l.ref, st);
    if (me != hipSuccess) return fail("prep_trim: clearing the workspace failed: %s", hipGetErrorString(me));
    const size_t sil_bytes = l.iv1 - l.sil;
    if (b2s_voc_silence_split(wav, lengths, B, Lmax, TOP_DB, FL1, HOP1, i32(l.iv1), i32(l.n1), i32(l.trim1), i32(l.pre1), i32(l.ol1), nullptr,
                              w + l.sil, sil_bytes, stream))
        return 1;
    hipLaunchKernelGGL(k_prep_peaks, dim3((Lmax + 3 + PEAK_TILE - 1) / PEAK_TILE, B), dim3(NT), 0, st, wav, lengths, Lmax, i32(l.iv1), i32(l.n1),
                       l.NI1, ref, mv);
    hipLaunchKernelGGL(k_prep_select, dim3(B), dim3(64), 0, st, lengths, Lmax, i32(l.iv1), i32(l.n1), l.NI1, ref, mv, gap_threshold, i32(l.kept),
                       status, n_removed);
    select_passes(wav, lengths, B, Lmax, i32(l.iv1), i32(l.n1), i32(l.kept), l.NI1, 0.95, hist, state, v95, st);
    hipLaunchKernelGGL(k_prep_plan, dim3((B + NT - 1) / NT), dim3(NT), 0, st, lengths, Lmax, i32(l.iv1), l.NI1, i32(l.n1), i32(l.kept), v95,
                       status, scale, i32(l.plan), i32(l.len2), B);
    hipLaunchKernelGGL(k_prep_scale, dim3((Lmax + COPY_TILE - 1) / COPY_TILE, B), dim3(NT), 0, st, wav, Lmax, scale, i32(l.plan), y2);
    if (b2s_voc_silence_split(y2, i32(l.len2), B, Lmax, TOP_DB, FL2, HOP2, i32(l.iv2), i32(l.n2), i32(l.trim2), i32(l.pre2), i32(l.ol2), nullptr,
                              w + l.sil, sil_bytes, stream))
        return 1;
    const int W = Lmax + LEAD + TAIL;
    hipLaunchKernelGGL(k_prep_margins, dim3((W + COPY_TILE - 1) / COPY_TILE, B), dim3(NT), 0, st, y2, Lmax, i32(l.plan), i32(l.trim2), out,
                       out_lengths, status);
    return launch_status("prep_trim");
}

}  // extern "C"
