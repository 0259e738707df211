// The variance adaptor for gfx950: quantise, embed and expand, and the transposed operation (C ABI: include/b2s_va.h, definition:
// DESIGN.md section o).
//
// plan()         what every kernel of forward and backward starts with, per workgroup of 256 threads: the checks of one utterance
//                and the inclusive scan of its durations into LDS (four positions per thread, a shuffle scan per wave, the four
//                wave totals through LDS).  Integers only, so every workgroup of an utterance comes to the same words.
// k_va_quantise  one workgroup per utterance: the boundaries in LDS (checked by every workgroup), a lower-bound search per value.
// k_va_frames    one workgroup per utterance: the int64 sum of its durations.
// k_va_forward   grid (chunks, B).  A wave takes FW consecutive frames: it finds the position of the first one by a search in the
//                scan, holds that position's row (x + table rows, 16 bytes per lane and load) in registers and stores it once per
//                frame, then steps to the next position that has frames.  A row is read once per wave that covers it and written
//                once per frame.  The h rows are one wave each, in the same launch.
// k_va_dx        grid (chunks, B), one wave per position, one lane per four columns: the position's dy rows are asked for several
//                at a time (depth()) and added in frame order.  Nothing is reduced across lanes.
// k_va_part      grid (chunks, B), one wave per (table, position): the first position of an utterance that uses a bin adds the dx
//                rows of all positions of that bin, in position order, and stores the sum at its own row of the workspace; its
//                position is the (utterance, bin) word of the index.  The others have nothing to do.
// k_va_table     one wave per (bin, 256 columns, table): walks the utterances in order through the index and adds their rows.
// k_va_pad       grid (chunks, B), one wave per row: packed frames to padded [B, T, D] with zeros behind, or back.
// The split by utterance keeps a bin that thousands of positions share (the unvoiced pitch bin) from being one serial chain: the
// chains are at most S and then at most B long.
// Contraction is off for the whole file (there is no product in it; the flag is the siblings').
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include "../../../include/b2s_va.h"
#include "../side_common.h"

using b2s_side::align_up;
using b2s_side::fail;

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, NW = NT / 64;                    // threads and waves of every workgroup
constexpr int MAX_S = B2S_VA_MAX_S, PER_THREAD = MAX_S / NT;
constexpr int MAX_BINS = B2S_VA_MAX_BINS;
constexpr int MAX_D4 = B2S_VA_MAX_D / 4, ROW_REGS = MAX_D4 / 64;   // float4 per row, and per lane
constexpr int FW = 8;                                    // frames per wave and step of k_va_forward
// rows asked for before the first is added (k_va_dx, k_va_part, k_va_table), by the float4 a lane holds per row: 64 to 96 registers
constexpr int depth(int rr) { return rr == 1 ? 16 : rr == 2 ? 12 : rr == 3 ? 8 : 6; }

struct Index {                                           // the index arguments of forward and backward
    const int32_t *pb, *eb, *dur, *in_len, *off;
    int n_bins, total, S, D4;
    int32_t *status;
};

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// The status of utterance b, the same in every thread; for B2S_VA_OK incl[s] = durations[0] + .. + durations[s] for s < n and *n_out,
// *o0_out, *frames_out are set.  `wsum` is LDS for NW words.  All NT threads call it; it ends with a barrier.
__device__ int plan(const Index &a, int b, int *incl, long long *wsum, int *n_out, long long *o0_out, int *frames_out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, S = a.S;
    const int n = a.in_len[b];
    const long long o0 = a.off[b], o1 = a.off[b + 1];
    if (n < 0 || n > S || o0 < 0 || o1 < o0 || o1 > a.total) return B2S_VA_FAILED;
    const size_t row = (size_t)b * S;
    int bad = 0;
    long long mine[PER_THREAD], sum = 0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = tid * PER_THREAD + j;
        int d = 0;
        if (i < n) {
            d = a.dur[row + i];
            if (a.pb) { const int k = a.pb[row + i]; bad |= k < 0 || k >= a.n_bins; }
            if (a.eb) { const int k = a.eb[row + i]; bad |= k < 0 || k >= a.n_bins; }
        }
        bad |= d < 0;
        sum += d;
        mine[j] = sum;
    }
    long long scan = sum;                                  // inclusive over the wave's threads
#pragma unroll
    for (int h = 1; h < 64; h <<= 1) {
        const long long up = __shfl_up(scan, h);
        if (lane >= h) scan += up;
    }
    if (lane == 63) wsum[w] = scan;
    bad = __syncthreads_or(bad);
    long long before = scan - sum, all = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        if (i < w) before += wsum[i];
        all += wsum[i];
    }
    if (bad || all > B2S_VA_MAX_FRAMES || o1 - o0 != all) {
        __syncthreads();
        return B2S_VA_FAILED;
    }
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = tid * PER_THREAD + j;
        if (i < n) incl[i] = (int)(before + mine[j]);
    }
    *n_out = n, *o0_out = o0, *frames_out = (int)all;
    __syncthreads();
    return n == 0 ? B2S_VA_EMPTY : B2S_VA_OK;
}

// ----------------------------------------------------------------------------------------------------------------- quantise

__global__ __launch_bounds__(NT) void k_va_quantise(const double *__restrict__ values, const int32_t *__restrict__ in_len,
                                                   const double *__restrict__ bounds, int n_bins, int S, int32_t *__restrict__ bins,
                                                   int32_t *__restrict__ status) {
    __shared__ double bd[MAX_BINS];
    const int b = blockIdx.x, tid = threadIdx.x, nb = n_bins - 1;
    int bad = 0;
    if (tid < nb) {
        const double v = bounds[tid];
        bd[tid] = v;
        bad |= !(fabs(v) <= 1.7976931348623157e308);
        if (tid + 1 < nb) bad |= !(v < bounds[tid + 1]);
    }
    bad = __syncthreads_or(bad);
    const int n = in_len[b];
    const size_t row = (size_t)b * S;
    const bool range = n >= 0 && n <= S;
    int nan = 0;
    if (range && !bad)
        for (int i = tid; i < n; i += NT) nan |= values[row + i] != values[row + i];
    nan = __syncthreads_or(nan);
    const bool ok = range && !bad && !nan;
    for (int i = tid; i < S; i += NT) {
        int lo = 0;
        if (ok && i < n) {
            const double v = values[row + i];
            int hi = nb;                                   // the first j in [0, nb] with !(bd[j] < v)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (bd[mid] < v) lo = mid + 1;
                else hi = mid;
            }
        }
        bins[row + i] = lo;
    }
    if (tid == 0) status[b] = !ok ? B2S_VA_FAILED : n == 0 ? B2S_VA_EMPTY : B2S_VA_OK;
}

// ------------------------------------------------------------------------------------------------------------------- frames

__global__ __launch_bounds__(NT) void k_va_frames(const int32_t *__restrict__ dur, const int32_t *__restrict__ in_len, int S,
                                                 int32_t *__restrict__ frames, int32_t *__restrict__ status) {
    __shared__ long long wsum[NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = in_len[b];
    if (n < 0 || n > S) {                                  // the whole workgroup
        if (tid == 0) frames[b] = 0, status[b] = B2S_VA_FAILED;
        return;
    }
    const size_t row = (size_t)b * S;
    int bad = 0;
    long long sum = 0;
    for (int i = tid; i < n; i += NT) {
        const int d = dur[row + i];
        bad |= d < 0;
        sum += d;
    }
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) sum += __shfl_xor(sum, h);
    if (lane == 0) wsum[w] = sum;
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        long long all = 0;
        for (int i = 0; i < NW; ++i) all += wsum[i];
        const bool ok = !bad && all <= B2S_VA_MAX_FRAMES;
        frames[b] = ok ? (int)all : 0;
        status[b] = !ok ? B2S_VA_FAILED : n == 0 ? B2S_VA_EMPTY : B2S_VA_OK;
    }
}

// ------------------------------------------------------------------------------------------------------------------ forward

struct FwdArgs {
    Index ix;
    const float4 *x, *pt, *et;
    float4 *h, *y;
    int32_t *uof;
};

// The kernels that hold rows in registers are compiled for RR = 1..ROW_REGS float4 per lane (D <= 256 RR); the launch picks the
// smallest that fits D, so that narrow rows leave the registers to more rows in flight.

// row s of h: this lane's float4 columns lane, lane + 64, ..
template <int RR>
__device__ __forceinline__ void h_row(const FwdArgs &a, size_t pos, int lane, float4 (&r)[RR]) {
    const int D4 = a.ix.D4;
    const float4 *xr = a.x + pos * D4;
    const float4 *pr = a.pt ? a.pt + (size_t)a.ix.pb[pos] * D4 : nullptr;
    const float4 *er = a.et ? a.et + (size_t)a.ix.eb[pos] * D4 : nullptr;
#pragma unroll
    for (int j = 0; j < RR; ++j) {
        const int c = lane + 64 * j;
        if (c < D4) {
            float4 v = xr[c];
            if (pr) v = add4(v, pr[c]);
            if (er) v = add4(v, er[c]);
            r[j] = v;
        }
    }
}

template <int RR>
__device__ __forceinline__ void store_row(float4 *dst, int D4, int lane, const float4 (&r)[RR]) {
#pragma unroll
    for (int j = 0; j < RR; ++j) {
        const int c = lane + 64 * j;
        if (c < D4) dst[c] = r[j];
    }
}

template <int RR>
__device__ __forceinline__ void zero_row(float4 (&r)[RR]) {
#pragma unroll
    for (int j = 0; j < RR; ++j) r[j] = make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int RR>
__global__ __launch_bounds__(NT) void k_va_forward(FwdArgs a) {
    __shared__ int incl[MAX_S];
    __shared__ long long wsum[NW];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, S = a.ix.S, D4 = a.ix.D4;
    int n = 0, F = 0;
    long long o0 = 0;
    const int st = plan(a.ix, b, incl, wsum, &n, &o0, &F);
    if (blockIdx.x == 0 && tid == 0) a.ix.status[b] = st;
    if (st == B2S_VA_FAILED) return;                               // the whole workgroup
    const size_t row = (size_t)b * S;
    float4 r[RR];
    if (a.h) {
        for (int s = blockIdx.x * NW + w; s < S; s += gridDim.x * NW) {
            if (s < n) h_row(a, row + s, lane, r);
            else zero_row(r);
            store_row(a.h + (row + s) * D4, D4, lane, r);
        }
    }
    // F > 0 implies n > 0 and incl[n - 1] == F
    for (long long t0 = ((long long)blockIdx.x * NW + w) * FW; t0 < F; t0 += (long long)gridDim.x * NW * FW) {
        const int t1 = min((int)t0 + FW, F);
        int t = (int)t0, lo = 0, hi = n - 1;                       // s = the first position with incl[s] > t; incl[n - 1] = F > t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (incl[mid] <= t) lo = mid + 1;
            else hi = mid;
        }
        int s = lo;
        while (t < t1) {
            const int end = min(incl[s], t1);                      // > t
            h_row(a, row + s, lane, r);
            if (a.uof && lane < end - t) a.uof[o0 + t + lane] = s; // end - t <= FW <= 64
            for (; t < end; ++t) store_row(a.y + (size_t)(o0 + t) * D4, D4, lane, r);
            if (t < t1) {
                ++s;
                while (incl[s] <= t) ++s;                          // positions of 0 frames; stops at the latest at n - 1
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- backward

struct BwdArgs {
    Index ix;
    const float4 *dy;
    float4 *dx;
    float4 *part[2];                                     // [B, S, D4] per table (pitch, energy), NULL without the table
    int32_t *slot[2];                                    // [B, n_bins] per table: the position that holds the bin's row, or -1
    float4 *dtab[2];
    int B;
};

// acc = (..((acc + rows[0]) + rows[1]) ..) over `count` consecutive rows of D4 float4: this lane's columns, DEPTH rows asked for at
// a time
template <int RR>
__device__ __forceinline__ void add_rows(const float4 *rows, int count, int D4, int lane, float4 (&acc)[RR]) {
    constexpr int DEPTH = depth(RR);
    for (int i0 = 0; i0 < count; i0 += DEPTH) {
        float4 v[DEPTH][RR];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i)
#pragma unroll
            for (int j = 0; j < RR; ++j) {
                const int c = lane + 64 * j;
                if (i0 + i < count && c < D4) v[i][j] = rows[(size_t)(i0 + i) * D4 + c];
            }
#pragma unroll
        for (int i = 0; i < DEPTH; ++i)
#pragma unroll
            for (int j = 0; j < RR; ++j)
                if (i0 + i < count && lane + 64 * j < D4) acc[j] = add4(acc[j], v[i][j]);
    }
}

template <int RR>
__global__ __launch_bounds__(NT) void k_va_dx(BwdArgs a) {
    __shared__ int incl[MAX_S];
    __shared__ long long wsum[NW];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, S = a.ix.S, D4 = a.ix.D4;
    int n = 0, F = 0;
    long long o0 = 0;
    const int st = plan(a.ix, b, incl, wsum, &n, &o0, &F);
    if (blockIdx.x == 0) {
        if (tid == 0) a.ix.status[b] = st;
        for (int tb = 0; tb < 2; ++tb)
            if (a.slot[tb])
                for (int k = tid; k < a.ix.n_bins; k += NT) a.slot[tb][(size_t)b * a.ix.n_bins + k] = -1;
    }
    if (st != B2S_VA_OK) n = 0;
    const size_t row = (size_t)b * S;
    for (int s = blockIdx.x * NW + w; s < S; s += gridDim.x * NW) {
        float4 acc[RR];
        zero_row(acc);
        if (s < n) {
            const int first = s ? incl[s - 1] : 0;
            add_rows(a.dy + (size_t)(o0 + first) * D4, incl[s] - first, D4, lane, acc);
        }
        store_row(a.dx + (row + s) * D4, D4, lane, acc);
    }
}

// after k_va_dx on the same stream: status, dx and the -1 of the index are there
template <int RR>
__global__ __launch_bounds__(NT) void k_va_part(BwdArgs a) {
    constexpr int DEPTH = depth(RR);
    __shared__ int bins[2][MAX_S];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, S = a.ix.S, D4 = a.ix.D4;
    if (a.ix.status[b] != B2S_VA_OK) return;                       // the whole workgroup; n is in 1..S and the bins are in range
    const int n = a.ix.in_len[b];
    const size_t row = (size_t)b * S;
    const int32_t *src[2] = {a.ix.pb, a.ix.eb};
    for (int tb = 0; tb < 2; ++tb)
        if (a.part[tb])
            for (int i = tid; i < n; i += NT) bins[tb][i] = src[tb][row + i];
    __syncthreads();
    for (int item = blockIdx.x * NW + w; item < 2 * n; item += gridDim.x * NW) {
        const int tb = item >= n, s = item - tb * n;
        if (!a.part[tb]) continue;
        const int *bn = bins[tb];
        const int k = bn[s];
        int earlier = 0;
        for (int i = lane; i < s; i += 64) earlier |= bn[i] == k;
        if (__any(earlier)) continue;                              // not the first position of its bin
        float4 acc[RR];
        zero_row(acc);
        for (int i0 = s & ~63; i0 < n; i0 += 64) {                 // the positions of the bin from s on, ascending, DEPTH at a time
            const int i = i0 + lane;
            unsigned long long live = __ballot(i >= s && i < n && bn[i] == k);
            while (live) {
                float4 v[DEPTH][RR];
                int got = 0;
#pragma unroll
                for (int q = 0; q < DEPTH; ++q) {
                    if (live) {
                        const float4 *from = a.dx + (row + i0 + __ffsll((long long)live) - 1) * D4;
                        live &= live - 1;
#pragma unroll
                        for (int j = 0; j < RR; ++j)
                            if (lane + 64 * j < D4) v[q][j] = from[lane + 64 * j];
                        got = q + 1;
                    }
                }
#pragma unroll
                for (int q = 0; q < DEPTH; ++q)
#pragma unroll
                    for (int j = 0; j < RR; ++j)
                        if (q < got && lane + 64 * j < D4) acc[j] = add4(acc[j], v[q][j]);
            }
        }
        store_row(a.part[tb] + (row + s) * D4, D4, lane, acc);
        if (lane == 0) a.slot[tb][(size_t)b * a.ix.n_bins + k] = s;
    }
}

// grid (n_bins, ceil(D4 / 64), 2), one wave: d_table[k][this wave's 256 columns]
__global__ __launch_bounds__(64) void k_va_table(BwdArgs a) {
    const int k = blockIdx.x, tb = blockIdx.z, lane = threadIdx.x, c = blockIdx.y * 64 + lane, S = a.ix.S, D4 = a.ix.D4;
    if (!a.dtab[tb]) return;
    const int32_t *slot = a.slot[tb];
    const float4 *part = a.part[tb];
    constexpr int DEPTH = depth(1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b0 = 0; b0 < a.B; b0 += 64) {
        const int b = b0 + lane;
        const int mine = b < a.B ? slot[(size_t)b * a.ix.n_bins + k] : -1;
        unsigned long long live = __ballot(mine >= 0);
        while (live) {                                             // the utterances that hold the bin, ascending, DEPTH at a time
            float4 v[DEPTH];
            int got = 0;
#pragma unroll
            for (int i = 0; i < DEPTH; ++i) {
                if (live) {
                    const int src = __ffsll((long long)live) - 1;
                    live &= live - 1;
                    const int s = __shfl(mine, src);
                    if (c < D4) v[i] = part[((size_t)(b0 + src) * S + s) * D4 + c];
                    got = i + 1;
                }
            }
#pragma unroll
            for (int i = 0; i < DEPTH; ++i)
                if (i < got && c < D4) acc = add4(acc, v[i]);
        }
    }
    if (c < D4) a.dtab[tb][(size_t)k * D4 + c] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------- pad

// grid (chunks, B), one wave per row of the padded utterance
__global__ __launch_bounds__(NT) void k_va_pad(float4 *__restrict__ frames, const int32_t *__restrict__ off, int total, int T, int D4,
                                              float4 *__restrict__ padded, int to_frames, int32_t *__restrict__ status) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long o0 = off[b], o1 = off[b + 1];
    const bool ok = o0 >= 0 && o1 >= o0 && o1 <= total && o1 - o0 <= T;
    if (blockIdx.x == 0 && threadIdx.x == 0) status[b] = !ok ? B2S_VA_FAILED : o1 == o0 ? B2S_VA_EMPTY : B2S_VA_OK;
    if (!ok) return;
    const int F = (int)(o1 - o0), rows = to_frames ? F : T;
    for (int t = blockIdx.x * NW + w; t < rows; t += gridDim.x * NW) {
        float4 *pr = padded + ((size_t)b * T + t) * D4, *fr = frames + (size_t)(o0 + t) * D4;
        for (int c = lane; c < D4; c += 64) {
            if (to_frames) fr[c] = pr[c];
            else pr[c] = t < F ? fr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the checks

bool misaligned(const void *p) { return (uintptr_t)p % 16 != 0; }

int check_batch(int B, int S) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (B > 65535) return fail("at most 65535 utterances per call (got %d); split the batch", B);
    if (S < 1 || S > MAX_S) return fail("S must be in 1..%d (got %d)", MAX_S, S);
    return 0;
}

int check_sizes(int B, int S, int D, int n_bins) {
    if (check_batch(B, S)) return 1;
    if (D < 4 || D > B2S_VA_MAX_D || D % 4) return fail("D must be a multiple of 4 in 4..%d (got %d)", B2S_VA_MAX_D, D);
    if (n_bins < 1 || n_bins > MAX_BINS) return fail("n_bins must be in 1..%d (got %d)", MAX_BINS, n_bins);
    if ((long long)B * S * D > (1LL << 31)) return fail("B * S * D = %lld elements: sizes past one call", (long long)B * S * D);
    return 0;
}

int check_index(const char *what, const void *pb, const void *eb, const void *ptab, const void *etab, bool tables_needed,
                const void *dur, const void *in_len, const void *off, int total, int B, int S, int D, int n_bins, const void *status) {
    if (check_sizes(B, S, D, n_bins)) return 1;
    if (total < 0) return fail("total_frames must be >= 0 (got %d)", total);
    if ((long long)total * D > (1LL << 31)) return fail("total_frames * D = %lld elements: sizes past one call", (long long)total * D);
    if (!dur || !in_len || !off || !status) return fail("%s: durations, input_lengths, frame_offsets or status is NULL", what);
    if ((pb != nullptr) != (ptab != nullptr) && (tables_needed || ptab))
        return fail("%s: the pitch table and pitch_bins are NULL together", what);
    if ((eb != nullptr) != (etab != nullptr) && (tables_needed || etab))
        return fail("%s: the energy table and energy_bins are NULL together", what);
    if (misaligned(ptab) || misaligned(etab)) return fail("%s: the tables must be 16-byte aligned", what);
    return 0;
}

size_t ws_need(int B, int S, int D, int n_bins) {
    return 16 + 2 * (align_up((size_t)B * S * D * sizeof(float)) + align_up((size_t)B * n_bins * sizeof(int32_t)));
}

// workgroups per utterance for `per_utt` pieces of work of NW each: all of them for a small batch, fewer as B grows
int chunks(long long per_utt, int B) {
    const long long want = (per_utt + NW - 1) / NW, cap = std::max(1, 8192 / B);
    return (int)std::max(1LL, std::min(want, cap));
}

// launches KERNEL<RR> with NT threads for the smallest RR whose 64 * RR float4 hold a row of d4
#define BY_ROW_REGS(d4, KERNEL, grid, st, args)                                              \
    do {                                                                                     \
        if ((d4) <= 64) hipLaunchKernelGGL((KERNEL<1>), grid, dim3(NT), 0, st, args);        \
        else if ((d4) <= 128) hipLaunchKernelGGL((KERNEL<2>), grid, dim3(NT), 0, st, args);  \
        else if ((d4) <= 192) hipLaunchKernelGGL((KERNEL<3>), grid, dim3(NT), 0, st, args);  \
        else hipLaunchKernelGGL((KERNEL<ROW_REGS>), grid, dim3(NT), 0, st, args);            \
    } while (0)

}  // namespace

extern "C" {

int b2s_va_version(void) { return 100; }

const char *b2s_va_last_error(void) { return b2s_side::last_error(); }

size_t b2s_va_ws_bytes(int B, int S, int D, int n_bins) { return check_sizes(B, S, D, n_bins) ? 0 : ws_need(B, S, D, n_bins); }

int b2s_va_quantise(const double *values, const int32_t *input_lengths, const double *boundaries, int n_bins, int B, int S,
                    int32_t *bins, int32_t *status, void *stream) {
    if (check_batch(B, S)) return 1;
    if (n_bins < 1 || n_bins > MAX_BINS) return fail("n_bins must be in 1..%d (got %d)", MAX_BINS, n_bins);
    if (!values || !input_lengths || !bins || !status) return fail("quantise: values, input_lengths, bins or status is NULL");
    if (n_bins > 1 && !boundaries) return fail("quantise: boundaries is NULL");
    hipLaunchKernelGGL(k_va_quantise, dim3(B), dim3(NT), 0, (hipStream_t)stream, values, input_lengths, boundaries, n_bins, S, bins,
                       status);
    return b2s_side::launch_status("quantise");
}

int b2s_va_frames(const int32_t *durations, const int32_t *input_lengths, int B, int S, int32_t *frames, int32_t *status,
                  void *stream) {
    if (check_batch(B, S)) return 1;
    if (!durations || !input_lengths || !frames || !status) return fail("frames: durations, input_lengths, frames or status is NULL");
    hipLaunchKernelGGL(k_va_frames, dim3(B), dim3(NT), 0, (hipStream_t)stream, durations, input_lengths, S, frames, status);
    return b2s_side::launch_status("frames");
}

int b2s_va_pad(float *frames, const int32_t *frame_offsets, int total_frames, int B, int T, int D, float *padded, int to_frames,
               int32_t *status, void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (B > 65535) return fail("at most 65535 utterances per call (got %d); split the batch", B);
    if (T < 1 || T > B2S_VA_MAX_FRAMES) return fail("T must be in 1..%d (got %d)", B2S_VA_MAX_FRAMES, T);
    if (D < 4 || D > B2S_VA_MAX_D || D % 4) return fail("D must be a multiple of 4 in 4..%d (got %d)", B2S_VA_MAX_D, D);
    if (total_frames < 0) return fail("total_frames must be >= 0 (got %d)", total_frames);
    if ((long long)B * T * D > (1LL << 31)) return fail("B * T * D = %lld elements: sizes past one call", (long long)B * T * D);
    if ((long long)total_frames * D > (1LL << 31))
        return fail("total_frames * D = %lld elements: sizes past one call", (long long)total_frames * D);
    if (!frame_offsets || !status || !padded || (total_frames > 0 && !frames))
        return fail("pad: frames, frame_offsets, padded or status is NULL");
    if (misaligned(frames) || misaligned(padded)) return fail("pad: frames and padded must be 16-byte aligned");
    hipLaunchKernelGGL(k_va_pad, dim3(chunks(T, B), B), dim3(NT), 0, (hipStream_t)stream, (float4 *)frames, frame_offsets, total_frames,
                       T, D / 4, (float4 *)padded, to_frames ? 1 : 0, status);
    return b2s_side::launch_status("pad");
}

int b2s_va_forward(const float *x, const int32_t *pitch_bins, const int32_t *energy_bins, const float *pitch_table,
                   const float *energy_table, int n_bins, const int32_t *durations, const int32_t *input_lengths,
                   const int32_t *frame_offsets, int total_frames, int B, int S, int D, float *h, float *y, int32_t *unit_of_frame,
                   int32_t *status, void *stream) {
    if (check_index("forward", pitch_bins, energy_bins, pitch_table, energy_table, true, durations, input_lengths, frame_offsets,
                    total_frames, B, S, D, n_bins, status))
        return 1;
    if (!x || (total_frames > 0 && !y)) return fail("forward: x or y is NULL");
    if (misaligned(x) || misaligned(y) || misaligned(h)) return fail("forward: x, h and y must be 16-byte aligned");
    FwdArgs a;
    a.ix = Index{pitch_bins, energy_bins, durations, input_lengths, frame_offsets, n_bins, total_frames, S, D / 4, status};
    a.x = (const float4 *)x, a.pt = (const float4 *)pitch_table, a.et = (const float4 *)energy_table;
    a.h = (float4 *)h, a.y = (float4 *)y, a.uof = unit_of_frame;
    const long long frames = std::min((long long)total_frames, (long long)B2S_VA_MAX_FRAMES);
    const int gx = chunks(std::max((frames + FW - 1) / FW, h ? (long long)S : 0LL), B);
    BY_ROW_REGS(a.ix.D4, k_va_forward, dim3(gx, B), (hipStream_t)stream, a);
    return b2s_side::launch_status("forward");
}

int b2s_va_backward(const float *dy, const int32_t *pitch_bins, const int32_t *energy_bins, int n_bins, const int32_t *durations,
                    const int32_t *input_lengths, const int32_t *frame_offsets, int total_frames, int B, int S, int D, float *dx,
                    float *d_pitch_table, float *d_energy_table, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    if (check_index("backward", pitch_bins, energy_bins, d_pitch_table, d_energy_table, false, durations, input_lengths,
                    frame_offsets, total_frames, B, S, D, n_bins, status))
        return 1;
    if (!dx || (total_frames > 0 && !dy)) return fail("backward: dy or dx is NULL");
    if (misaligned(dy) || misaligned(dx)) return fail("backward: dy and dx must be 16-byte aligned");
    const size_t need = ws_need(B, S, D, n_bins);
    if (!ws || ws_bytes < need) return fail("backward: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    if ((uintptr_t)ws % sizeof(int32_t)) return fail("backward: the workspace must be 4-byte aligned");
    BwdArgs a;
    a.ix = Index{pitch_bins, energy_bins, durations, input_lengths, frame_offsets, n_bins, total_frames, S, D / 4, status};
    a.dy = (const float4 *)dy, a.dx = (float4 *)dx, a.B = B;
    float *dtab[2] = {d_pitch_table, d_energy_table};
    const size_t part_bytes = align_up((size_t)B * S * D * sizeof(float)), slot_bytes = align_up((size_t)B * n_bins * sizeof(int32_t));
    for (int tb = 0; tb < 2; ++tb) {
        unsigned char *base = (unsigned char *)(((uintptr_t)ws + 15) & ~(uintptr_t)15) + tb * (part_bytes + slot_bytes);   // rows of float4
        a.dtab[tb] = (float4 *)dtab[tb];
        a.part[tb] = dtab[tb] ? (float4 *)base : nullptr;
        a.slot[tb] = dtab[tb] ? (int32_t *)(base + part_bytes) : nullptr;
    }
    const hipStream_t st = (hipStream_t)stream;
    BY_ROW_REGS(a.ix.D4, k_va_dx, dim3(chunks(S, B), B), st, a);
    if (d_pitch_table || d_energy_table) {
        BY_ROW_REGS(a.ix.D4, k_va_part, dim3(chunks(2LL * S, B), B), st, a);
        hipLaunchKernelGGL(k_va_table, dim3(n_bins, (D / 4 + 63) / 64, 2), dim3(64), 0, st, a);
    }
    return b2s_side::launch_status("backward");
}

}  // extern "C"
