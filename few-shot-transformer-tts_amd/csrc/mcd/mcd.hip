// Mel-cepstral distortion after DTW for gfx950 (C ABI: include/b2s_mcd.h, definition: DESIGN.md section k): the cepstral front end
// and the scoring along the path, around the batched DTW of libb2s_metrics.so.
//
// b2s_mcd_cepstra is three launches.  Every utterance is cut into chunks of 64 frames, one 256-thread workgroup per (utterance,
// chunk):
//   k_mcd_count    voiced flag of each frame of the chunk (a wave reads the row, two ballots), the chunk's voiced count
//   k_mcd_scan     one workgroup: which utterances are accepted (well formed and not overlapping an earlier one), their counts, the
//                  exclusive scan over the WHOLE batch (the DTW needs gap-free offsets), the first output row of every chunk
//                  (-1 for a refused utterance), the status
//   k_mcd_cepstra  the flags again (same function, same bits), ranks from the ballot, then FB voiced frames at a time: log-magnitudes
//                  in fp64 into LDS, the DCT rows in LDS (KC rows at a time, loaded once when all `order` rows fit), one thread per
//                  (frame, coefficient) with the sum over the bins in ascending order, one rounding to fp32
// The whole file is compiled with contraction off, so that every product and sum rounds on its own as the definition asks: the fp32
// cepstra equal the NumPy restatement bit for bit.  b2s_mcd_score is one launch, one workgroup per pair: a gather along the path, a
// per-thread sum in step order and a fixed tree over the threads.  Integer ballots only, no atomics.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../../include/b2s_mcd.h"
#include "../side_common.h"

using b2s_side::align_up;
using b2s_side::fail;

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;               // threads per block
constexpr int CHUNK = 64;             // frames per workgroup: one ballot ranks them
constexpr int FB_MAX = 16;            // voiced frames whose log-magnitudes are in LDS at once
constexpr int LN_BYTES = 16 * 1024;   // LDS for them
constexpr int TAB_BYTES = 32 * 1024;  // LDS for the DCT rows

inline int chunks_of(int max_len) { return max_len > 0 ? (max_len + CHUNK - 1) / CHUNK : 1; }

int check_ws_args(int B, int max_len) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (max_len < 0) return fail("max_len must be >= 0 (got %d)", max_len);
    // the scan is one workgroup that walks every chunk count twice: a call is capped where that stays a small part of it
    if ((long long)B * chunks_of(max_len) > B2S_MCD_MAX_CHUNKS)
        return fail("B %d x %d chunks of %d frames exceed the %d chunks of one call; split the batch", B, chunks_of(max_len), CHUNK,
                    B2S_MCD_MAX_CHUNKS);
    return 0;
}

// first row and length of utterance b; false when the offsets decrease, run outside 0..total or the length exceeds max_len (in this
// order nothing overflows)
__device__ __forceinline__ bool utt_range(const int32_t *__restrict__ off, int b, int total, int max_len, int &o, int &len) {
    const int o0 = off[b], o1 = off[b + 1];
    if (o0 < 0 || o1 < o0 || o1 > total || o1 - o0 > max_len) return false;
    o = o0, len = o1 - o0;
    return true;
}

// bit f = frame start + f is voiced (f < nf <= 64): the maximum over the bins is > 0 and no bin is a NaN.  Whole block; every
// thread returns the same mask.  Wave w reads frames 16 w .. 16 w + 15, the lanes along the bins.
__device__ unsigned long long chunk_mask(const float *__restrict__ mel, int start, int nf, int n_mels, int *sflag) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int f = wave * (CHUNK / 4); f < (wave + 1) * (CHUNK / 4); ++f) {
        int keep = 0;
        if (f < nf) {
            const float *row = mel + (size_t)(start + f) * n_mels;
            bool pos = false, nan = false;
            for (int m = lane; m < n_mels; m += 64) {
                const float v = row[m];
                pos |= v > 0.f;
                nan |= v != v;
            }
            const unsigned long long any_pos = __ballot(pos), any_nan = __ballot(nan);
            keep = any_pos != 0 && any_nan == 0;
        }
        if (lane == 0) sflag[f] = keep;
    }
    __syncthreads();
    return __ballot(sflag[lane] != 0);
}

__global__ __launch_bounds__(NT) void k_mcd_count(const float *__restrict__ mel, const int32_t *__restrict__ off, int total,
                                                  int max_len, int n_mels, int S, int32_t *__restrict__ counts) {
    __shared__ int sflag[CHUNK];
    const int b = blockIdx.x / S, c = blockIdx.x - b * S;
    int o = 0, len = 0, n = 0;
    if (utt_range(off, b, total, max_len, o, len)) {
        const int nf = min(CHUNK, len - c * CHUNK);
        if (nf > 0) n = __popcll(chunk_mask(mel, o + c * CHUNK, nf, n_mels, sflag));
    }
    if (threadIdx.x == 0) counts[(size_t)b * S + c] = n;
}

__global__ __launch_bounds__(NT) void k_mcd_scan(const int32_t *__restrict__ off, int total, int max_len, int B, int S,
                                                 const int32_t *__restrict__ counts, int32_t *__restrict__ bases,
                                                 int32_t *__restrict__ cep_off, int32_t *__restrict__ voiced,
                                                 int32_t *__restrict__ status) {
    __shared__ int sh[NT];
    const int tid = threadIdx.x;
    int carry = 0, claimed = 0;                   // voiced rows so far; the largest end of a well-formed utterance so far
    for (int b0 = 0; b0 < B; b0 += NT) {
        const int b = b0 + tid;
        int o = 0, len = 0;
        bool ok = b < B && utt_range(off, b, total, max_len, o, len);
        // An utterance is accepted when its own range is well formed AND it starts at or after the end of every well-formed
        // utterance before it (an exclusive prefix maximum of their ends).  Accepted utterances are then pairwise disjoint inside
        // 0..total, so their voiced rows sum to at most total, the rows cep_out holds -- offsets like [0, T, 0, T] cannot make the
        // compaction run past the buffer.  Prefix sums, which is what the contract asks for, always pass.
        sh[tid] = ok ? o + len : 0;
        __syncthreads();
        for (int d = 1; d < NT; d <<= 1) {
            const int v = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] = max(sh[tid], v);
            __syncthreads();
        }
        const int before = max(claimed, tid > 0 ? sh[tid - 1] : 0);
        claimed = max(claimed, sh[NT - 1]);
        __syncthreads();
        ok = ok && o >= before;
        int n = 0;
        if (ok)
            for (int c = 0; c < S; ++c) n += counts[(size_t)b * S + c];
        sh[tid] = n;
        __syncthreads();
        for (int d = 1; d < NT; d <<= 1) {
            const int v = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += v;
            __syncthreads();
        }
        if (b < B) {
            int run = carry + sh[tid] - n;
            cep_off[b] = run;
            voiced[b] = n;
            status[b] = !ok ? B2S_MCD_FAILED : n == 0 ? B2S_MCD_EMPTY : B2S_MCD_OK;
            for (int c = 0; c < S; ++c) {
                bases[(size_t)b * S + c] = ok ? run : -1;
                run += ok ? counts[(size_t)b * S + c] : 0;
            }
        }
        carry += sh[NT - 1];
        __syncthreads();
    }
    if (tid == 0) cep_off[B] = carry;
}

struct MelScale {
    double max_abs_value, two_a, max_db, ref_db, ln_scale;
    int symmetric;
};

// normalised mel value -> natural-log magnitude; contraction is off, every operation rounds on its own
__device__ __forceinline__ double log_mag(float x, const MelScale &s) {
    double a = (double)x;
    if (s.symmetric) a = (a + s.max_abs_value) / s.two_a;
    a = fmin(fmax(a, 0.0), 1.0);
    const double db = (a * s.max_db - s.max_db) + s.ref_db;
    return db * s.ln_scale;
}

__global__ __launch_bounds__(NT) void k_mcd_cepstra(const float *__restrict__ mel, const int32_t *__restrict__ off, int total,
                                                    int max_len, int n_mels, int order, int S, const double *__restrict__ dct,
                                                    MelScale sc, int FB, int KC, const int32_t *__restrict__ bases,
                                                    float *__restrict__ cep_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int sflag[CHUNK], vidx[CHUNK];
    const int ld = n_mels | 1;                    // odd row stride in doubles: the rows of the table start in different banks
    double *sln = (double *)smem, *stab = sln + (size_t)FB * ld;
    const int b = blockIdx.x / S, c = blockIdx.x - b * S, tid = threadIdx.x;
    int o, len;
    if (!utt_range(off, b, total, max_len, o, len)) return;
    const int base = bases[(size_t)b * S + c];    // -1: the scan refused the utterance (it overlaps an earlier one)
    if (base < 0) return;
    const int start = o + c * CHUNK, nf = min(CHUNK, len - c * CHUNK);
    if (nf <= 0) return;
    const unsigned long long mask = chunk_mask(mel, start, nf, n_mels, sflag);
    const int nv = __popcll(mask);
    // accepted utterances are disjoint, so base + nv <= total, the rows cep_out holds; the test costs nothing and keeps the store
    // inside the buffer whatever the offsets are
    if (nv == 0 || base + nv > total) return;
    if (tid < CHUNK && ((mask >> tid) & 1)) vidx[__popcll(mask & ((1ull << tid) - 1))] = tid;
    __syncthreads();
    bool table_in_lds = false;
    for (int j0 = 0; j0 < nv; j0 += FB) {
        const int nb = min(FB, nv - j0);
        for (int e = tid; e < nb * n_mels; e += NT) {
            const int f = e / n_mels, m = e - f * n_mels;
            sln[f * ld + m] = log_mag(mel[(size_t)(start + vidx[j0 + f]) * n_mels + m], sc);
        }
        for (int k0 = 0; k0 < order; k0 += KC) {
            const int kc = min(KC, order - k0);
            if (!table_in_lds || KC < order) {
                for (int e = tid; e < kc * n_mels; e += NT) {
                    const int kk = e / n_mels, m = e - kk * n_mels;
                    stab[kk * ld + m] = dct[(size_t)(k0 + kk) * n_mels + m];
                }
                table_in_lds = true;
            }
            __syncthreads();
            for (int it = tid; it < nb * kc; it += NT) {
                const int f = it / kc, kk = it - f * kc;
                const double *l = sln + f * ld, *d = stab + kk * ld;
                double acc = 0.0;
                for (int m = 0; m < n_mels; ++m) {
                    const double p = l[m] * d[m];
                    acc = acc + p;
                }
                cep_out[(size_t)(base + j0 + f) * order + k0 + kk] = (float)acc;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(NT) void k_mcd_score(const float *__restrict__ cx, const int32_t *__restrict__ cx_off, int total_cx,
                                                  const float *__restrict__ cy, const int32_t *__restrict__ cy_off, int total_cy,
                                                  int order, const int32_t *__restrict__ path, const int32_t *__restrict__ path_off,
                                                  int total_path, const int32_t *__restrict__ path_len,
                                                  const int32_t *__restrict__ dtw_status, double db_scale,
                                                  double *__restrict__ mcd_out, int32_t *__restrict__ status_out,
                                                  double *__restrict__ dist_out) {
    __shared__ double red[NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double QNAN = __builtin_nan("");
    auto finish = [&](int status, double mcd) {
        if (tid == 0) {
            status_out[b] = status;
            mcd_out[b] = mcd;
        }
    };
    const int st = dtw_status[b];
    if (st != B2S_MCD_OK) {
        finish(st == B2S_MCD_EMPTY ? B2S_MCD_EMPTY : B2S_MCD_FAILED, QNAN);
        return;
    }
    const int x0 = cx_off[b], x1 = cx_off[b + 1], y0 = cy_off[b], y1 = cy_off[b + 1], p0 = path_off[b], p1 = path_off[b + 1];
    const int n = path_len[b];
    if (x0 < 0 || x1 < x0 || x1 > total_cx || y0 < 0 || y1 < y0 || y1 > total_cy || p0 < 0 || p1 < p0 || p1 > total_path || n < 1 ||
        n > p1 - p0) {
        finish(B2S_MCD_FAILED, QNAN);
        return;
    }
    const int nx = x1 - x0, ny = y1 - y0;
    double acc = 0.0;
    int outside = 0;
    for (int q = tid; q < n; q += NT) {
        const int i = path[2 * ((size_t)p0 + q)], j = path[2 * ((size_t)p0 + q) + 1];
        double d = QNAN;
        if ((unsigned)i >= (unsigned)nx || (unsigned)j >= (unsigned)ny) {
            outside = 1;
        } else {
            const float *a = cx + (size_t)(x0 + i) * order, *c = cy + (size_t)(y0 + j) * order;
            double s = 0.0;
            for (int k = 0; k < order; ++k) {
                const double e = (double)a[k] - (double)c[k];
                s = s + e * e;
            }
            d = db_scale * sqrt(2.0 * s);
            acc = acc + d;
        }
        if (dist_out) dist_out[(size_t)p0 + q] = d;
    }
    red[tid] = acc;
    const int any_outside = __syncthreads_or(outside);
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if (any_outside) finish(B2S_MCD_FAILED, QNAN);
    else finish(B2S_MCD_OK, red[0] / (double)n);
}

}  // namespace

extern "C" {

int b2s_mcd_version(void) { return 100; }

const char *b2s_mcd_last_error(void) { return b2s_side::last_error(); }

size_t b2s_mcd_ws_bytes(int B, int max_len) {
    if (check_ws_args(B, max_len)) return 0;
    return 2 * align_up((size_t)B * chunks_of(max_len) * sizeof(int32_t));
}

int b2s_mcd_cepstra(const float *mel, const int32_t *offsets, int total, int max_len, int B, int n_mels, int order, const double *dct,
                    int symmetric, double max_abs_value, double max_db, double ref_db, double ln_scale, float *cep_out,
                    int32_t *cep_offsets_out, int32_t *voiced_out, int32_t *status_out, void *ws, size_t ws_bytes, void *stream) {
    if (check_ws_args(B, max_len)) return 1;
    if (total < 0) return fail("cepstra: total must be >= 0 (got %d)", total);
    if (n_mels < 2 || n_mels > B2S_MCD_MAX_MELS) return fail("cepstra: n_mels must be in 2..%d (got %d)", B2S_MCD_MAX_MELS, n_mels);
    const int max_order = n_mels - 1 < B2S_MCD_MAX_ORDER ? n_mels - 1 : B2S_MCD_MAX_ORDER;
    if (order < 1 || order > max_order)
        return fail("cepstra: order must be in 1..%d for %d mel bins (got %d)", max_order, n_mels, order);
    if (symmetric && !(max_abs_value > 0.0)) return fail("cepstra: max_abs_value must be > 0 for symmetric mels (got %g)", max_abs_value);
    if (!offsets || !dct) return fail("cepstra: offsets or dct is NULL");
    if (total > 0 && (!mel || !cep_out)) return fail("cepstra: mel or cep_out is NULL with frames to read");
    if (!cep_offsets_out || !voiced_out || !status_out) return fail("cepstra: cep_offsets_out, voiced_out or status_out is NULL");
    const size_t half = align_up((size_t)B * chunks_of(max_len) * sizeof(int32_t));
    if (!ws || ws_bytes < 2 * half) return fail("cepstra: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, 2 * half);
    const hipStream_t s = (hipStream_t)stream;
    const int S = chunks_of(max_len);
    int32_t *counts = (int32_t *)ws, *bases = (int32_t *)((char *)ws + half);
    const size_t row_bytes = (size_t)(n_mels | 1) * sizeof(double);
    int FB = (int)(LN_BYTES / row_bytes), KC = (int)(TAB_BYTES / row_bytes);
    FB = FB > FB_MAX ? FB_MAX : FB;
    KC = KC > order ? order : KC;
    MelScale sc;
    sc.max_abs_value = max_abs_value, sc.two_a = 2.0 * max_abs_value, sc.max_db = max_db, sc.ref_db = ref_db, sc.ln_scale = ln_scale;
    sc.symmetric = symmetric != 0;
    hipLaunchKernelGGL(k_mcd_count, dim3(B * S), dim3(NT), 0, s, mel, offsets, total, max_len, n_mels, S, counts);
    hipLaunchKernelGGL(k_mcd_scan, dim3(1), dim3(NT), 0, s, offsets, total, max_len, B, S, counts, bases, cep_offsets_out, voiced_out,
                       status_out);
    hipLaunchKernelGGL(k_mcd_cepstra, dim3(B * S), dim3(NT), (FB + KC) * row_bytes, s, mel, offsets, total, max_len, n_mels, order, S,
                       dct, sc, FB, KC, bases, cep_out);
    return b2s_side::launch_status("cepstra");
}

int b2s_mcd_score(const float *cx, const int32_t *cx_offsets, int total_cx, const float *cy, const int32_t *cy_offsets, int total_cy,
                  int B, int order, const int32_t *path, const int32_t *path_offsets, int total_path, const int32_t *path_len,
                  const int32_t *dtw_status, double db_scale, double *mcd_out, int32_t *status_out, double *dist_out, void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (order < 1 || order > B2S_MCD_MAX_ORDER) return fail("score: order must be in 1..%d (got %d)", B2S_MCD_MAX_ORDER, order);
    if (total_cx < 0 || total_cy < 0 || total_path < 0)
        return fail("score: totals must be >= 0 (got %d, %d and %d)", total_cx, total_cy, total_path);
    if (!cx_offsets || !cy_offsets || !path_offsets || !path_len || !dtw_status)
        return fail("score: cx_offsets, cy_offsets, path_offsets, path_len or dtw_status is NULL");
    if ((total_cx > 0 && !cx) || (total_cy > 0 && !cy) || (total_path > 0 && !path)) return fail("score: cx, cy or path is NULL");
    if (!mcd_out || !status_out) return fail("score: mcd_out or status_out is NULL");
    hipLaunchKernelGGL(k_mcd_score, dim3(B), dim3(NT), 0, (hipStream_t)stream, cx, cx_offsets, total_cx, cy, cy_offsets, total_cy, order,
                       path, path_offsets, total_path, path_len, dtw_status, db_scale, mcd_out, status_out, dist_out);
    return b2s_side::launch_status("score");
}

}  // extern "C"
