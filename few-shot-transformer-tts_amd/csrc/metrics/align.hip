// Alignment-head selection and path diagnostics for gfx950 (C ABI: include/b2s_metrics.h, b2s_met_align_*).
//
// Input: n_layers device arrays A_l[B, H, S, T] fp32, T (decoder frames) innermost -- what b2s_decode_alignment writes.  For every
// (utterance, layer, head) the score is sum over t < dec_len of max over s < enc_len of A_l[b, h, s, t] (the reference's plot_attn
// rule); the head with the largest score is kept, its [S, T] slab copied out, and its per-frame argmax path summarised.
//
// k_met_align_reduce, the hot path: grid (frame chunk, layer * head, utterance), 256 threads.  A chunk is CHUNK = 256 frames.  The
// four waves of a block take one contiguous quarter of the rows s < enc_len each; inside a wave every lane owns four frames and
// walks its rows with eight loads in flight, keeping the running fp32 maximum and its first row.  With T a multiple of 4 (and
// 16-byte aligned bases) a lane owns four ADJACENT frames and reads them with one 16-byte load per row (1 KiB per wave and row);
// otherwise lane k owns frames k, k + 64, k + 128, k + 192 of the chunk and reads dwords (256 B per wave instruction).  Rows
// s >= enc_len and frames t >= dec_len are never loaded: a chunk wholly past dec_len returns at once, a lane past it issues no load.
// Waves 1-3 hand their (max, row) to wave 0 through LDS, which merges them in wave order with a strict > (so the first row wins a
// tie, as NumPy's argmax), stores the per-frame argmax of this head to the workspace, and sums the chunk's maxima in fp64 in a fixed
// order (per lane, then a shuffle tree) into one partial per (utterance, head, chunk).  No floating-point atomics anywhere.
//
// k_met_align_finish: grid (utterance, FIN_SPLIT), 256 threads.  Every block adds the partials of each head in chunk order (one
// thread per head), scans the heads in order with a strict > against a running best that starts at 0, and copies its share of the
// chosen slab.  Block 0 of an utterance also writes the scores, the choice, the path and its statistics (integer LDS atomics; the
// visited flags of the distinct count live in the workspace, so S is not bounded by LDS).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../../include/b2s_metrics.h"
#include "../side_common.h"

namespace {

using b2s_side::fail;

constexpr int NT = 256;               // threads per block
constexpr int CHUNK = 256;            // frames per workgroup: 64 lanes x 4 frames
constexpr int MAX_LAYERS = 16;
constexpr int FIN_SPLIT = 16;         // blocks per utterance that share the copy of the chosen slab
constexpr int UNROLL = 8;             // rows in flight per lane

struct LayerPtrs {
    const float *p[MAX_LAYERS];
};

struct WsLayout {
    size_t part, amax, visited, total;
    int n_chunks;
};

inline size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

WsLayout layout(int B, int n_layers, int H, int S, int T) {
    WsLayout l;
    const size_t LH = (size_t)n_layers * H;
    l.n_chunks = (T + CHUNK - 1) / CHUNK;
    l.part = 0;                                                            // double [B, LH, n_chunks]
    l.amax = l.part + round16((size_t)B * LH * l.n_chunks * sizeof(double));   // int32 [B, LH, T]
    l.visited = l.amax + round16((size_t)B * LH * T * sizeof(int32_t));        // uint32 [B, S]
    l.total = l.visited + round16((size_t)B * S * sizeof(uint32_t));
    return l;
}

int check_args(int B, int n_layers, int H, int S, int T) {
    if (n_layers < 1 || n_layers > MAX_LAYERS) return fail("align: n_layers must be in 1..%d (got %d)", MAX_LAYERS, n_layers);
    if (B <= 0) return fail("align: B must be > 0 (got %d)", B);
    if (H <= 0) return fail("align: H must be > 0 (got %d)", H);
    if (S <= 0) return fail("align: S must be > 0 (got %d)", S);
    if (T <= 0) return fail("align: T must be > 0 (got %d)", T);
    if (B > 65535) return fail("align: B must be <= 65535 (got %d)", B);
    if ((long long)n_layers * H > 65535) return fail("align: n_layers * H must be <= 65535 (got %lld)", (long long)n_layers * H);
    return 0;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline void upd(float v, int s, float &m, int &ix) {
    if (v > m) {
        m = v;
        ix = s;
    }
}

__global__ __launch_bounds__(NT) void k_met_align_reduce(LayerPtrs layers, int H, int S, int T, int n_chunks,
                                                         const int32_t *__restrict__ enc_len, const int32_t *__restrict__ dec_len,
                                                         double *__restrict__ part, int32_t *__restrict__ amax, int vec) {
    const int chunk = blockIdx.x, lh = blockIdx.y, b = blockIdx.z, LH = gridDim.y;
    const int dec = clampi(dec_len[b], 0, T), enc = clampi(enc_len[b], 0, S);
    const int c0 = chunk * CHUNK;
    if (c0 >= dec || enc == 0) return;            // block-uniform: nothing is read, and the finishing kernel never looks here
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int l = lh / H, h = lh - l * H;
    const float *__restrict__ base = layers.p[l] + ((size_t)b * H + h) * (size_t)S * T;
    const int q = (enc + 3) >> 2;
    const int s_lo = min(wave * q, enc), s_hi = min(s_lo + q, enc);

    float m[4];
    int ix[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = -INFINITY;
        ix[j] = 0;
    }
    // first frame of this lane, the stride between its four frames, and how many of them are < dec_len
    const int t0 = vec ? c0 + lane * 4 : c0 + lane, tstep = vec ? 1 : 64;
    int nv = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) nv += (t0 + j * tstep < dec) ? 1 : 0;

    if (vec && nv == 4) {
        const float *__restrict__ col = base + t0;
        int s = s_lo;
        for (; s + UNROLL <= s_hi; s += UNROLL) {
            float4 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) v[u] = *reinterpret_cast<const float4 *>(col + (size_t)(s + u) * T);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                upd(v[u].x, s + u, m[0], ix[0]);
                upd(v[u].y, s + u, m[1], ix[1]);
                upd(v[u].z, s + u, m[2], ix[2]);
                upd(v[u].w, s + u, m[3], ix[3]);
            }
        }
        for (; s < s_hi; ++s) {
            const float4 v = *reinterpret_cast<const float4 *>(col + (size_t)s * T);
            upd(v.x, s, m[0], ix[0]);
            upd(v.y, s, m[1], ix[1]);
            upd(v.z, s, m[2], ix[2]);
            upd(v.w, s, m[3], ix[3]);
        }
    } else if (nv > 0) {
        // dword loads: every lane of the odd-T layout, and the one lane of the 16-byte layout that straddles dec_len
        const float *__restrict__ col = base + t0;
        int s = s_lo;
        for (; s + 4 <= s_hi; s += 4) {
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[u][j] = j < nv ? col[(size_t)(s + u) * T + j * tstep] : -INFINITY;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) upd(v[u][j], s + u, m[j], ix[j]);
        }
        for (; s < s_hi; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) upd(col[(size_t)s * T + j * tstep], s, m[j], ix[j]);
    }

    __shared__ float sh_m[3][4][64];
    __shared__ int sh_ix[3][4][64];
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sh_m[wave - 1][j][lane] = m[j];
            sh_ix[wave - 1][j][lane] = ix[j];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // wave 0 holds the lowest rows: a later wave replaces its result only with a strictly larger maximum
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int j = 0; j < 4; ++j) upd(sh_m[w][j][lane], sh_ix[w][j][lane], m[j], ix[j]);
    int32_t *__restrict__ arow = amax + ((size_t)b * LH + lh) * T;
    double acc = 0.0;
    if (vec && nv == 4) {
        *reinterpret_cast<int4 *>(arow + t0) = make_int4(ix[0], ix[1], ix[2], ix[3]);
        acc = (((double)m[0] + (double)m[1]) + (double)m[2]) + (double)m[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) {
                arow[t0 + j * tstep] = ix[j];
                acc += (double)m[j];
            }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) part[((size_t)b * LH + lh) * n_chunks + chunk] = acc;
}

__global__ __launch_bounds__(NT) void k_met_align_finish(LayerPtrs layers, int LH, int H, int S, int T, int n_chunks,
                                                         const int32_t *__restrict__ enc_len, const int32_t *__restrict__ dec_len,
                                                         const double *__restrict__ part, const int32_t *__restrict__ amax,
                                                         uint32_t *__restrict__ visited, double *__restrict__ scores_out,
                                                         int32_t *__restrict__ best_out, float *__restrict__ map_out,
                                                         int32_t *__restrict__ path_out, int32_t *__restrict__ stats_out, int vec_map) {
    const int b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const int dec = clampi(dec_len[b], 0, T), enc = clampi(enc_len[b], 0, S);
    const int used = enc > 0 ? (dec + CHUNK - 1) / CHUNK : 0;      // chunks the reduction wrote for this utterance
    __shared__ double sh_score[NT];
    __shared__ double sh_bestv;
    __shared__ int sh_best, sh_back, sh_jump, sh_distinct;
    if (tid == 0) {
        sh_bestv = 0.0;
        sh_best = -1;
        sh_back = sh_jump = sh_distinct = 0;
    }
    __syncthreads();
    for (int lh0 = 0; lh0 < LH; lh0 += NT) {
        const int lh = lh0 + tid;
        if (lh < LH) {
            const double *__restrict__ p = part + ((size_t)b * LH + lh) * n_chunks;
            double sc = 0.0;
            for (int c = 0; c < used; ++c) sc += p[c];
            sh_score[tid] = sc;
            if (y == 0) scores_out[(size_t)b * LH + lh] = sc;
        }
        __syncthreads();
        if (tid == 0) {
            const int n = min(NT, LH - lh0);
            double bv = sh_bestv;
            int bi = sh_best;
            for (int i = 0; i < n; ++i)
                if (sh_score[i] > bv) {
                    bv = sh_score[i];
                    bi = lh0 + i;
                }
            sh_bestv = bv;
            sh_best = bi;
        }
        __syncthreads();
    }
    const int best = sh_best;
    if (y == 0 && tid == 0) best_out[b] = best;

    if (map_out) {
        const size_t n = (size_t)S * T;
        float *__restrict__ dst = map_out + (size_t)b * n;
        const float *__restrict__ src = best >= 0 ? layers.p[best / H] + ((size_t)b * H + best % H) * n : nullptr;
        const size_t n4 = vec_map ? n / 4 : 0, step = (size_t)NT * gridDim.y;
        for (size_t i = (size_t)y * NT + tid; i < n4; i += step)
            reinterpret_cast<float4 *>(dst)[i] = src ? reinterpret_cast<const float4 *>(src)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (size_t i = n4 * 4 + (size_t)y * NT + tid; i < n; i += step) dst[i] = src ? src[i] : 0.f;
    }
    if (y != 0 || (!path_out && !stats_out)) return;

    const int n = best >= 0 ? dec : 0;            // best >= 0 implies dec > 0 and enc > 0, so every p[t < n] was written
    const int32_t *__restrict__ p = amax + ((size_t)b * LH + (best >= 0 ? best : 0)) * T;
    if (path_out)
        for (int t = tid; t < T; t += NT) path_out[(size_t)b * T + t] = t < n ? p[t] : -1;
    if (!stats_out) return;
    uint32_t *vis = visited + (size_t)b * S;
    for (int s = tid; s < S; s += NT) vis[s] = 0u;
    __syncthreads();
    for (int t = tid; t < n; t += NT) {
        const int pt = p[t];
        vis[pt] = 1u;                             // pt < enc <= S
        if (t >= 1) {
            const int d = pt - p[t - 1];
            if (d < 0) atomicAdd(&sh_back, 1);
            else atomicMax(&sh_jump, d);
        }
    }
    __syncthreads();
    int cnt = 0;
    for (int s = tid; s < S; s += NT) cnt += vis[s] ? 1 : 0;
    if (cnt) atomicAdd(&sh_distinct, cnt);
    __syncthreads();
    if (tid == 0) {
        int32_t *o = stats_out + (size_t)b * 4;
        o[0] = sh_back;
        o[1] = sh_jump;
        o[2] = sh_distinct;
        o[3] = n > 0 ? p[n - 1] : 0;
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int b2s_met_align_chunk(void) { return CHUNK; }

size_t b2s_met_align_ws_bytes(int B, int n_layers, int H, int S, int T) {
    if (check_args(B, n_layers, H, S, T)) return 0;
    return layout(B, n_layers, H, S, T).total;
}

int b2s_met_align_select(const float *const *layers, int n_layers, int B, int H, int S, int T, const int32_t *enc_len,
                         const int32_t *dec_len, double *scores_out, int32_t *best_out, float *map_out, int32_t *path_out,
                         int32_t *stats_out, void *ws, size_t ws_bytes, void *stream) {
    if (check_args(B, n_layers, H, S, T)) return 1;
    if (!layers) return fail("align: layers is NULL");
    if (!enc_len || !dec_len) return fail("align: enc_len or dec_len is NULL");
    if (!scores_out || !best_out) return fail("align: scores_out or best_out is NULL");
    if (!ws) return fail("align: ws is NULL");
    const WsLayout l = layout(B, n_layers, H, S, T);
    if (ws_bytes < l.total) return fail("align: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    LayerPtrs lp;
    bool al = aligned16(ws);
    for (int i = 0; i < MAX_LAYERS; ++i) {
        lp.p[i] = i < n_layers ? layers[i] : nullptr;
        if (i < n_layers && !lp.p[i]) return fail("align: layers[%d] is NULL", i);
        al = al && aligned16(lp.p[i]);
    }
    const int LH = n_layers * H;
    const int vec = al && (T % 4 == 0);
    const int vec_map = al && aligned16(map_out) && (((size_t)S * T) % 4 == 0);
    char *w = (char *)ws;
    hipLaunchKernelGGL(k_met_align_reduce, dim3(l.n_chunks, LH, B), dim3(NT), 0, (hipStream_t)stream, lp, H, S, T, l.n_chunks, enc_len,
                       dec_len, (double *)(w + l.part), (int32_t *)(w + l.amax), vec);
    hipLaunchKernelGGL(k_met_align_finish, dim3(B, map_out ? FIN_SPLIT : 1), dim3(NT), 0, (hipStream_t)stream, lp, LH, H, S, T,
                       l.n_chunks, enc_len, dec_len, (const double *)(w + l.part), (const int32_t *)(w + l.amax),
                       (uint32_t *)(w + l.visited), scores_out, best_out, map_out, path_out, stats_out, vec_map);
    return b2s_side::launch_status("align");
}

}  // extern "C"
