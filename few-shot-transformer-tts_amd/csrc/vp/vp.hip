// A variance predictor for gfx950, forward and backward (C ABI: include/b2s_vp.h, definition: DESIGN.md section p).
//
// tap_gemm()    the product every GEMM-shaped kernel shares: a tile of 32 rows by TN columns per workgroup of 256 threads, RM rows by
//               4 columns per thread, operands staged through LDS 16 k at a time with the next stage's global loads in flight while
//               this one is multiplied.  Every accumulator is one fmaf chain in the k order of the definition (tap, then column), on
//               the VALU: fmaf is the definition's own operation, so the bits hold by construction.
// k_vp_repack   a conv weight [F][C][3] -> [3][C][F] (forward) or [3][F][C] (input gradient), so that the GEMM's columns are contiguous.
// k_vp_conv     grid (row tiles, B): conv as three shifted taps, the workgroup owns all F columns of its 32 rows, so ReLU, LayerNorm,
//               dropout and (layer 2) the Linear are its epilogue: the tile goes through LDS, a wave takes a row, a lane the columns
//               lane, lane + 64, ..; tree() is then log2(F / 64) lane-local additions and a six-step butterfly.
// k_vp_rowbwd   one wave per row: dropout, LayerNorm and ReLU backward (two trees).
// k_vp_colpart  one thread per (utterance, column): the chains over s of dbe, dg (and dwl, dbl for layer 2).
// k_vp_colfinal one thread per column and sum: the chain over the OK utterances.
// k_vp_din      tap_gemm with the taps mirrored and the weight transposed: dh1 and dx.
// k_vp_dw       one accumulator tile of dW per workgroup, K = the rows of the OK utterances in order, no split; db rides as a column
//               of ones in the workgroups of the centre tap.
// Contraction is off for the whole file: every product that is not inside an explicit fmaf is rounded before it is added.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "../../../include/b2s_vp.h"
#include "../side_common.h"

using b2s_side::align_up;
using b2s_side::fail;

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, NW = NT / 64;                    // threads and waves of every GEMM workgroup
constexpr int TR = 32, KC = 16;                          // rows of a tile, k per LDS stage
constexpr int DW_TN = 128;                               // columns of a dW tile

struct Drop {                                            // the dropout of one site
    uint32_t key, thresh;
    float scale;
    int on;                                              // p != 0
};

__host__ __device__ inline uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool keeps(const Drop &d, uint32_t idx) { return lowbias32(idx * 0x9E3779B1u + d.key) >= d.thresh; }

__device__ __forceinline__ float dropped(const Drop &d, uint32_t idx, float v) {
    if (!d.on) return v;
    return keeps(d, idx) ? v * d.scale : 0.f;
}

// tree() of the definition over F = 64 * NC values, this lane holding the columns lane + 64 * i; every lane gets the result
template <int NC>
__device__ __forceinline__ float tree(const float (&in)[NC]) {
    float v[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) v[i] = in[i];
#pragma unroll
    for (int h = NC / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int i = 0; i < h; ++i) v[i] = v[i] + v[i + h];
    float s = v[0];
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) s = s + __shfl_xor(s, h);   // lane l < h: s[l] + s[l + h]; the other lanes mirror them
    return s;
}

// ------------------------------------------------------------------------------------------------------------------ the product

template <int TN>
struct Tile {
    static constexpr int TX = TN / 4, TY = NT / TX, RM = TR / TY;   // threads along the columns and rows, rows per thread
    static constexpr int WPT = KC * TN / 4 / NT;                    // float4 of a W stage per thread
    static_assert(RM >= 1 && WPT >= 1 && TY * RM == TR, "tile");
};

// acc[i][c] = fmaf(As[row ty * RM + i][kk], Ws[kk][4 * tx + c], acc[i][c]) for kk = 0..kmax-1 ascending (kmax a multiple of 4)
template <int TN>
__device__ __forceinline__ void mac(const float *As, const float *Ws, int kmax, int tx, int ty, float (&acc)[Tile<TN>::RM][4]) {
    constexpr int RM = Tile<TN>::RM;
    for (int kk = 0; kk < kmax; kk += 4) {
        float4 w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = *(const float4 *)(Ws + (kk + q) * TN + 4 * tx);
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            const float4 a = *(const float4 *)(As + (ty * RM + i) * KC + kk);
            const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[i][0] = fmaf(av[q], w[q].x, acc[i][0]);
                acc[i][1] = fmaf(av[q], w[q].y, acc[i][1]);
                acc[i][2] = fmaf(av[q], w[q].z, acc[i][2]);
                acc[i][3] = fmaf(av[q], w[q].w, acc[i][3]);
            }
        }
    }
}

// For the rows r0..r0+31 of one utterance of n rows and the columns n0..n0+TN-1:
//   acc[r][col] = fmaf(A[r + dir * (j - 1)][k], W[j][k][col], acc[r][col]) for j = 0, 1, 2 and k = 0..K-1 inside each j,
// rows outside 0..n-1 reading as +0.0 (the term is made).  A: the utterance's rows of K floats; W: [3][K][N]; K and N multiples of 4.
// smem: TR * TN floats.  Ends with a barrier, so smem is free afterwards.
template <int TN>
__device__ __forceinline__ void tap_gemm(const float *__restrict__ A, int K, int n, int r0, int dir, const float *__restrict__ W, int N,
                                         int n0, float (&acc)[Tile<TN>::RM][4], float *smem) {
    constexpr int WPT = Tile<TN>::WPT, TX = Tile<TN>::TX;
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    float *Ws = smem, *As = smem + KC * TN;
    const int nk = (K + KC - 1) / KC, steps = 3 * nk;
    float4 wreg[WPT], areg;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int step) {
        const int j = step / nk, k0 = (step - j * nk) * KC;
#pragma unroll
        for (int q = 0; q < WPT; ++q) {
            const int idx = tid + q * NT, kk = idx / TX, col = n0 + 4 * (idx - kk * TX);
            wreg[q] = (k0 + kk < K && col < N) ? *(const float4 *)(W + ((size_t)j * K + k0 + kk) * N + col) : zero;
        }
        if (tid < TR * KC / 4) {
            const int s = r0 + (tid >> 2) + dir * (j - 1), k = k0 + (tid & 3) * 4;
            areg = (s >= 0 && s < n && k < K) ? *(const float4 *)(A + (size_t)s * K + k) : zero;
        }
    };
    fetch(0);
    for (int step = 0; step < steps; ++step) {
#pragma unroll
        for (int q = 0; q < WPT; ++q) ((float4 *)Ws)[tid + q * NT] = wreg[q];
        if (tid < TR * KC / 4) ((float4 *)As)[tid] = areg;
        __syncthreads();
        if (step + 1 < steps) fetch(step + 1);
        const int k0 = (step % nk) * KC;
        mac<TN>(As, Ws, min(KC, K - k0), tx, ty, acc);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------- repack

// W [F][C][3] -> out [3][C][F] (to_cf) or [3][F][C]
__global__ __launch_bounds__(NT) void k_vp_repack(const float *__restrict__ W, float *__restrict__ out, int F, int C, int to_cf) {
    const size_t per = (size_t)F * C, total = 3 * per;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int j = (int)(i / per);
        const size_t rem = i - j * per;
        const int f = to_cf ? (int)(rem % F) : (int)(rem / C), c = to_cf ? (int)(rem / F) : (int)(rem % C);
        out[i] = W[((size_t)f * C + c) * 3 + j];
    }
}

// --------------------------------------------------------------------------------------------------------------------- forward

struct ConvArgs {
    const float *in, *Wt, *bias, *g, *be, *wl, *bl;     // wl, bl: layer 2
    const int32_t *len;
    int S, C;
    float eps;
    Drop drop;
    float *a_out, *xh_out, *rstd_out;                   // the tape, NULL together
    float *h_out;                                       // layer 1
    float *pred;                                        // layer 2
    int32_t *status;                                    // layer 1
};

template <int F>
__global__ __launch_bounds__(NT) void k_vp_conv(ConvArgs a) {
    constexpr int RM = Tile<F>::RM, TX = Tile<F>::TX, NC = F / 64;
    __shared__ float4 smem4[TR * F / 4];
    float *smem = (float *)smem4;
    const int b = blockIdx.y, r0 = blockIdx.x * TR, tid = threadIdx.x, S = a.S;
    const int n = a.len[b];
    const bool failed = n < 0 || n > S;
    if (a.status && blockIdx.x == 0 && tid == 0) a.status[b] = failed ? B2S_VP_FAILED : n == 0 ? B2S_VP_EMPTY : B2S_VP_OK;
    if (failed) return;                                  // the whole workgroup
    const size_t row0 = (size_t)b * S;
    if (a.pred)                                          // behind the length, inside this tile
        for (int i = tid; i < TR; i += NT)
            if (r0 + i >= n && r0 + i < S) a.pred[row0 + r0 + i] = 0.f;
    if (r0 >= n) return;
    const int tx = tid % TX, ty = tid / TX;
    float acc[RM][4];
    {
        const float4 bv = *(const float4 *)(a.bias + 4 * tx);
#pragma unroll
        for (int i = 0; i < RM; ++i) acc[i][0] = bv.x, acc[i][1] = bv.y, acc[i][2] = bv.z, acc[i][3] = bv.w;
    }
    tap_gemm<F>(a.in + row0 * a.C, a.C, n, r0, 1, a.Wt, F, 0, acc, smem);
#pragma unroll
    for (int i = 0; i < RM; ++i)
        *(float4 *)(smem + (ty * RM + i) * F + 4 * tx) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    float g[NC], be[NC], wl[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        g[i] = a.g[lane + 64 * i], be[i] = a.be[lane + 64 * i];
        wl[i] = a.pred ? a.wl[lane + 64 * i] : 0.f;
    }
    for (int r = w; r < TR && r0 + r < n; r += NW) {
        const size_t row = row0 + r0 + r;
        float av[NC], v[NC], d[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            av[i] = smem[r * F + lane + 64 * i];
            v[i] = av[i] > 0.f ? av[i] : 0.f;
        }
        const float mu = tree<NC>(v) / (float)F;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            d[i] = v[i] - mu;
            v[i] = d[i] * d[i];
        }
        const float var = tree<NC>(v) / (float)F;
        const float rstd = 1.0f / sqrtf(var + a.eps);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int f = lane + 64 * i;
            const float xh = d[i] * rstd;
            const float nrm = (xh * g[i]) + be[i];
            const float h = dropped(a.drop, (uint32_t)(row * F + f), nrm);
            if (a.a_out) a.a_out[row * F + f] = av[i], a.xh_out[row * F + f] = xh;
            if (a.h_out) a.h_out[row * F + f] = h;
            v[i] = h * wl[i];
        }
        if (a.rstd_out && lane == 0) a.rstd_out[row] = rstd;
        if (a.pred) {
            const float t = tree<NC>(v) + a.bl[0];
            if (lane == 0) a.pred[row] = t;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- backward

struct RowArgs {                                        // one layer's row and column work
    const float *dh;                                    // layer 1: dh1 [B, S, F]; layer 2: NULL (dh = d_pred * wl)
    const float *d_pred, *wl, *g, *be;                  // d_pred, wl, be: layer 2
    const float *a, *xh, *rstd;                         // the tape
    const int32_t *len;
    int S, B;
    Drop drop;
    float *da;                                          // [B, S, F]
    float *p_dbe, *p_dg, *p_dwl, *p_dbl;                // partials [B, F], [B]; p_dwl, p_dbl: layer 2
};

// grid (chunks, B), one wave per row
template <int F>
__global__ __launch_bounds__(NT) void k_vp_rowbwd(RowArgs a) {
    constexpr int NC = F / 64;
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6, S = a.S;
    const int n = a.len[b];
    if (n < 1 || n > S) return;
    float g[NC], wl[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        g[i] = a.g[lane + 64 * i];
        wl[i] = a.dh ? 0.f : a.wl[lane + 64 * i];
    }
    for (int s = blockIdx.x * NW + w; s < n; s += gridDim.x * NW) {
        const size_t row = (size_t)b * S + s;
        const float dp = a.dh ? 0.f : a.d_pred[row], rstd = a.rstd[row];
        float dxh[NC], xh[NC], v[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int f = lane + 64 * i;
            const float dh = a.dh ? a.dh[row * F + f] : dp * wl[i];
            dxh[i] = dropped(a.drop, (uint32_t)(row * F + f), dh) * g[i];
            xh[i] = a.xh[row * F + f];
            v[i] = dxh[i] * xh[i];
        }
        const float m1 = tree<NC>(dxh) / (float)F;
        const float m2 = tree<NC>(v) / (float)F;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int f = lane + 64 * i;
            const float dr = ((dxh[i] - m1) - (xh[i] * m2)) * rstd;
            a.da[row * F + f] = a.a[row * F + f] > 0.f ? dr : 0.f;
        }
    }
}

// grid (F / 64, B), 64 threads: the chains over s of one utterance and 64 columns
template <int F>
__global__ __launch_bounds__(64) void k_vp_colpart(RowArgs a) {
    const int b = blockIdx.y, f = blockIdx.x * 64 + threadIdx.x, S = a.S;
    const int n = a.len[b];
    if (n < 1 || n > S) return;
    const bool last = a.dh == nullptr;                   // layer 2
    const float g = a.g[f], wl = last ? a.wl[f] : 0.f, be = last ? a.be[f] : 0.f;
    float dbe = 0.f, dg = 0.f, dwl = 0.f, dbl = 0.f;
    for (int s = 0; s < n; ++s) {
        const size_t row = (size_t)b * S + s;
        const uint32_t idx = (uint32_t)(row * F + f);
        const float xh = a.xh[row * F + f];
        const float dp = last ? a.d_pred[row] : 0.f;
        const float dh = last ? dp * wl : a.dh[row * F + f];
        const float dn = dropped(a.drop, idx, dh);
        dbe = dbe + dn;
        dg = fmaf(dn, xh, dg);
        if (last) {
            const float h2 = dropped(a.drop, idx, (xh * g) + be);
            dwl = fmaf(dp, h2, dwl);
            dbl = dbl + dp;
        }
    }
    a.p_dbe[(size_t)b * F + f] = dbe, a.p_dg[(size_t)b * F + f] = dg;
    if (last) {
        a.p_dwl[(size_t)b * F + f] = dwl;
        if (f == 0) a.p_dbl[b] = dbl;
    }
}

struct FinalArgs {
    const float *part[6];                               // dbe2, dg2, dwl, dbe1, dg1 [B, F]; dbl [B]
    float *out[6];
    const int32_t *len;
    int S, B, F;
};

// grid (F / 64, 6), 64 threads: the chain over the OK utterances
__global__ __launch_bounds__(64) void k_vp_colfinal(FinalArgs a) {
    const int which = blockIdx.y, f = blockIdx.x * 64 + threadIdx.x, wide = which < 5;
    if (!wide && f != 0) return;
    const int stride = wide ? a.F : 1;
    const float *part = a.part[which];
    float acc = 0.f;
    for (int b = 0; b < a.B; ++b) {
        const int n = a.len[b];
        if (n >= 1 && n <= a.S) acc = acc + part[(size_t)b * stride + f];
    }
    a.out[which][f] = acc;
}

struct DinArgs {
    const float *da, *Wb;                               // [B, S, F], [3][F][N]
    const int32_t *len;
    int S, F, N;
    float *out;                                         // [B, S, N]: dh1 or dx, every row written
};

// grid (row tiles, B, column tiles)
template <int TN>
__global__ __launch_bounds__(NT) void k_vp_din(DinArgs a) {
    constexpr int RM = Tile<TN>::RM, TX = Tile<TN>::TX;
    __shared__ float4 smem4[TR * TN / 4];
    const int b = blockIdx.y, r0 = blockIdx.x * TR, n0 = blockIdx.z * TN, tid = threadIdx.x, S = a.S, N = a.N;
    const int tx = tid % TX, ty = tid / TX;
    int n = a.len[b];
    if (n < 0 || n > S) n = 0;
    float acc[RM][4];
#pragma unroll
    for (int i = 0; i < RM; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
    if (r0 < n) tap_gemm<TN>(a.da + (size_t)b * S * a.F, a.F, n, r0, -1, a.Wb, N, n0, acc, (float *)smem4);   // the whole workgroup
    const int col = n0 + 4 * tx;
    if (col >= N) return;
#pragma unroll
    for (int i = 0; i < RM; ++i) {
        const int s = r0 + ty * RM + i;
        if (s >= S) continue;
        const float4 v = s < n ? make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        *(float4 *)(a.out + ((size_t)b * S + s) * N + col) = v;
    }
}

struct DwArgs {
    const float *da, *in;                               // [B, S, F], [B, S, C]
    const int32_t *len;
    int S, B, F, C;
    float *dW, *db;                                     // [F][C][3], [F]
};

// grid (F / 32, column tiles of C, 3 taps): dW[f0..f0+31][c0..c0+127][j], one chain over the rows of the OK utterances
__global__ __launch_bounds__(NT) void k_vp_dw(DwArgs a) {
    constexpr int TN = DW_TN, RM = Tile<TN>::RM, TX = Tile<TN>::TX, WPT = Tile<TN>::WPT;
    __shared__ float4 smem4[TR * TN / 4];
    float *Ws = (float *)smem4, *As = Ws + KC * TN;
    const int f0 = blockIdx.x * TR, c0 = blockIdx.y * TN, j = blockIdx.z, tid = threadIdx.x, S = a.S, F = a.F, C = a.C;
    const int tx = tid % TX, ty = tid / TX;
    const bool ones = blockIdx.y == 0 && j == 1 && tx == 0;   // db: the column of ones
    float acc[RM][4], accb[RM];
#pragma unroll
    for (int i = 0; i < RM; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = accb[i] = 0.f;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 wreg[WPT], areg;
    int b = -1, s0 = 0, n = 0;                           // the stage in flight: rows s0..s0+15 of utterance b
    auto next_utt = [&]() {                              // the next OK utterance, or b = B
        for (++b; b < a.B; ++b) {
            n = a.len[b];
            if (n >= 1 && n <= S) break;
        }
        s0 = 0;
    };
    auto fetch = [&]() {
#pragma unroll
        for (int q = 0; q < WPT; ++q) {
            const int idx = tid + q * NT, kk = idx / TX, col = c0 + 4 * (idx - kk * TX), s = s0 + kk + j - 1;
            wreg[q] = (s0 + kk < n && s >= 0 && s < n && col < C) ? *(const float4 *)(a.in + ((size_t)b * S + s) * C + col) : zero;
        }
        if (tid < TR * KC / 4) {
            const int kk = tid >> 3, s = s0 + kk;
            areg = s < n ? *(const float4 *)(a.da + ((size_t)b * S + s) * F + f0 + 4 * (tid & 7)) : zero;
        }
    };
    next_utt();
    if (b < a.B) fetch();
    while (b < a.B) {
#pragma unroll
        for (int q = 0; q < WPT; ++q) ((float4 *)Ws)[tid + q * NT] = wreg[q];
        if (tid < TR * KC / 4) {                         // transposed: As[f][kk]
            const int kk = tid >> 3, fr = 4 * (tid & 7);
            As[(fr + 0) * KC + kk] = areg.x, As[(fr + 1) * KC + kk] = areg.y;
            As[(fr + 2) * KC + kk] = areg.z, As[(fr + 3) * KC + kk] = areg.w;
        }
        __syncthreads();
        s0 += KC;
        if (s0 >= n) next_utt();
        if (b < a.B) fetch();
        mac<TN>(As, Ws, KC, tx, ty, acc);
        if (ones)
#pragma unroll
            for (int i = 0; i < RM; ++i)
                for (int kk = 0; kk < KC; ++kk) accb[i] = accb[i] + As[(ty * RM + i) * KC + kk];
        __syncthreads();
    }
    // a row of the chunk behind the utterance's end adds fmaf(+0, x, acc) or acc + +0.0: the chains start at +0.0, are never -0.0,
    // and stay as they are
#pragma unroll
    for (int i = 0; i < RM; ++i) {
        const int f = f0 + ty * RM + i;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c0 + 4 * tx + c < C) a.dW[((size_t)f * C + c0 + 4 * tx + c) * 3 + j] = acc[i][c];
        if (ones) a.db[f] = accb[i];
    }
}

// ------------------------------------------------------------------------------------------------------------------- the mask

__global__ __launch_bounds__(NT) void k_vp_mask(Drop d, size_t total, uint8_t *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) out[i] = keeps(d, (uint32_t)i);
}

// ---------------------------------------------------------------------------------------------------------------- the checks

bool misaligned(const void *p) { return (uintptr_t)p % 16 != 0; }

int check_bsf(int B, int S, int F) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (B > 65535) return fail("at most 65535 utterances per call (got %d); split the batch", B);
    if (S < 1 || S > B2S_VP_MAX_S) return fail("S must be in 1..%d (got %d)", B2S_VP_MAX_S, S);
    if (F != 64 && F != 128 && F != 256 && F != 512) return fail("F must be 64, 128, 256 or 512 (got %d)", F);
    if ((long long)B * S * F > (1LL << 31)) return fail("B * S * F = %lld elements: sizes past one call", (long long)B * S * F);
    return 0;
}

int check_sizes(int B, int S, int D, int F) {
    if (check_bsf(B, S, F)) return 1;
    if (D < 4 || D > B2S_VP_MAX_D || D % 4) return fail("D must be a multiple of 4 in 4..%d (got %d)", B2S_VP_MAX_D, D);
    if ((long long)B * S * D > (1LL << 31)) return fail("B * S * D = %lld elements: sizes past one call", (long long)B * S * D);
    return 0;
}

int check_p(double p) {
    if (!(p >= 0.0 && p < 1.0)) return fail("p must be in [0, 1) (got %g)", p);
    return 0;
}

Drop drop_of(double p, uint64_t seed, int site) {
    Drop d;
    d.key = lowbias32((uint32_t)seed + 0x9E3779B9u * (uint32_t)site) ^ lowbias32((uint32_t)(seed >> 32) ^ 0x85EBCA6Bu);
    d.thresh = (uint32_t)std::floor(p * 4294967296.0);
    d.scale = (float)(1.0 / (1.0 - p));
    d.on = p != 0.0;
    return d;
}

struct Sizes {                                           // bytes of the regions of the workspace and the tape
    size_t w1, w2, act, part, rows;
};

Sizes sizes_of(int B, int S, int D, int F) {
    Sizes z;
    z.w1 = align_up((size_t)3 * D * F * sizeof(float)), z.w2 = align_up((size_t)3 * F * F * sizeof(float));
    z.act = align_up((size_t)B * S * F * sizeof(float)), z.part = align_up((size_t)(5 * F + 1) * B * sizeof(float));
    z.rows = align_up((size_t)B * S * sizeof(float));
    return z;
}

size_t ws_need(const Sizes &z) { return 256 + 2 * z.w1 + 2 * z.w2 + 3 * z.act + z.part; }

struct Workspace {
    float *Wt1, *Wb1, *Wt2, *Wb2, *act[3], *part;
};

Workspace carve(void *ws, const Sizes &z) {
    unsigned char *p = (unsigned char *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    Workspace w;
    w.Wt1 = (float *)p, p += z.w1;
    w.Wb1 = (float *)p, p += z.w1;
    w.Wt2 = (float *)p, p += z.w2;
    w.Wb2 = (float *)p, p += z.w2;
    for (int i = 0; i < 3; ++i) w.act[i] = (float *)p, p += z.act;
    w.part = (float *)p;
    return w;
}

struct Tape {
    float *a1, *xh1, *h1, *a2, *xh2, *rstd1, *rstd2;
};

Tape tape_of(const void *tape, const Sizes &z) {
    unsigned char *p = (unsigned char *)tape;
    Tape t;
    t.a1 = (float *)p, t.xh1 = (float *)(p + z.act), t.h1 = (float *)(p + 2 * z.act), t.a2 = (float *)(p + 3 * z.act);
    t.xh2 = (float *)(p + 4 * z.act), t.rstd1 = (float *)(p + 5 * z.act), t.rstd2 = (float *)(p + 5 * z.act + z.rows);
    return t;
}

void repack(const float *W, float *out, int F, int C, int to_cf, hipStream_t st) {
    const int blocks = (int)std::min<size_t>(((size_t)3 * F * C + NT - 1) / NT, 1024);
    hipLaunchKernelGGL(k_vp_repack, dim3(blocks), dim3(NT), 0, st, W, out, F, C, to_cf);
}

#define BY_F(F, KERNEL, grid, block, st, args)                                                     \
    do {                                                                                           \
        if ((F) == 64) hipLaunchKernelGGL((KERNEL<64>), grid, block, 0, st, args);                 \
        else if ((F) == 128) hipLaunchKernelGGL((KERNEL<128>), grid, block, 0, st, args);          \
        else if ((F) == 256) hipLaunchKernelGGL((KERNEL<256>), grid, block, 0, st, args);          \
        else hipLaunchKernelGGL((KERNEL<512>), grid, block, 0, st, args);                          \
    } while (0)

void launch_din(const DinArgs &a, int B, hipStream_t st) {
    const int tiles = (a.S + TR - 1) / TR;
    if (a.N <= 64) hipLaunchKernelGGL((k_vp_din<64>), dim3(tiles, B, 1), dim3(NT), 0, st, a);
    else if (a.N <= 128) hipLaunchKernelGGL((k_vp_din<128>), dim3(tiles, B, 1), dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((k_vp_din<256>), dim3(tiles, B, (a.N + 255) / 256), dim3(NT), 0, st, a);
}

// workgroups of NW rows per utterance: all of them for a small batch, fewer as B grows
int row_chunks(int S, int B) { return std::max(1, std::min((S + NW - 1) / NW, std::max(1, 8192 / B))); }

}  // namespace

extern "C" {

int b2s_vp_version(void) { return 100; }

const char *b2s_vp_last_error(void) { return b2s_side::last_error(); }

size_t b2s_vp_ws_bytes(int B, int S, int D, int F) { return check_sizes(B, S, D, F) ? 0 : ws_need(sizes_of(B, S, D, F)); }

size_t b2s_vp_tape_bytes(int B, int S, int F) {
    if (check_bsf(B, S, F)) return 0;
    const Sizes z = sizes_of(B, S, 4, F);
    return 5 * z.act + 2 * z.rows;
}

int b2s_vp_forward(const float *x, const int32_t *input_lengths, const float *W1, const float *b1, const float *g1, const float *be1,
                   const float *W2, const float *b2, const float *g2, const float *be2, const float *wl, const float *bl, float eps,
                   double p, uint64_t seed, int B, int S, int D, int F, float *pred, int32_t *status, void *tape, void *ws,
                   size_t ws_bytes, void *stream) {
    if (check_sizes(B, S, D, F) || check_p(p)) return 1;
    if (!(eps >= 0.f)) return fail("eps must be >= 0 (got %g)", (double)eps);
    if (!x || !input_lengths || !pred || !status) return fail("forward: x, input_lengths, pred or status is NULL");
    if (!W1 || !b1 || !g1 || !be1 || !W2 || !b2 || !g2 || !be2 || !wl || !bl) return fail("forward: a parameter is NULL");
    if (misaligned(x) || misaligned(b1) || misaligned(b2) || misaligned(tape))
        return fail("forward: x, b1, b2 and the tape must be 16-byte aligned");
    const Sizes z = sizes_of(B, S, D, F);
    if (!ws || ws_bytes < ws_need(z)) return fail("forward: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, ws_need(z));
    const Workspace w = carve(ws, z);
    const hipStream_t st = (hipStream_t)stream;
    Tape t = {};
    if (tape) t = tape_of(tape, z);
    float *h1 = tape ? t.h1 : w.act[0];
    repack(W1, w.Wt1, F, D, 1, st);
    repack(W2, w.Wt2, F, F, 1, st);
    const dim3 grid((S + TR - 1) / TR, B);
    ConvArgs c1 = {x, w.Wt1, b1, g1, be1, nullptr, nullptr, input_lengths, S, D, eps, drop_of(p, seed, 1),
                   t.a1, t.xh1, t.rstd1, h1, nullptr, status};
    BY_F(F, k_vp_conv, grid, dim3(NT), st, c1);
    ConvArgs c2 = {h1, w.Wt2, b2, g2, be2, wl, bl, input_lengths, S, F, eps, drop_of(p, seed, 2),
                   t.a2, t.xh2, t.rstd2, nullptr, pred, nullptr};
    BY_F(F, k_vp_conv, grid, dim3(NT), st, c2);
    return b2s_side::launch_status("forward");
}

int b2s_vp_backward(const float *x, const int32_t *input_lengths, const float *W1, const float *b1, const float *g1, const float *be1,
                    const float *W2, const float *b2, const float *g2, const float *be2, const float *wl, const float *bl,
                    const void *tape, const float *d_pred, double p, uint64_t seed, int B, int S, int D, int F, float *dx, float *dW1,
                    float *db1, float *dg1, float *dbe1, float *dW2, float *db2, float *dg2, float *dbe2, float *dwl, float *dbl,
                    void *ws, size_t ws_bytes, void *stream) {
    if (check_sizes(B, S, D, F) || check_p(p)) return 1;
    if (!x || !input_lengths || !tape || !d_pred) return fail("backward: x, input_lengths, the tape or d_pred is NULL");
    if (!W1 || !b1 || !g1 || !be1 || !W2 || !b2 || !g2 || !be2 || !wl || !bl) return fail("backward: a parameter is NULL");
    float *const grads[10] = {dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dwl, dbl};
    int have = 0;
    for (float *gp : grads) have += gp != nullptr;
    if (have != 0 && have != 10) return fail("backward: the ten parameter gradients are NULL together or not at all (%d are there)", have);
    if (!have && !dx) return fail("backward: nothing to compute: dx and the parameter gradients are NULL");
    if (misaligned(x) || misaligned(dx) || misaligned(tape)) return fail("backward: x, dx and the tape must be 16-byte aligned");
    const Sizes z = sizes_of(B, S, D, F);
    if (!ws || ws_bytes < ws_need(z)) return fail("backward: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, ws_need(z));
    const Workspace w = carve(ws, z);
    const Tape t = tape_of(tape, z);
    const hipStream_t st = (hipStream_t)stream;
    float *da2 = w.act[0], *dh1 = w.act[1], *da1 = w.act[2];
    const size_t BF = (size_t)B * F;
    float *part = w.part;                                // dbe2, dg2, dwl, dbe1, dg1 [B, F], dbl [B]
    const dim3 rows(row_chunks(S, B), B), cols(F / 64, B);

    RowArgs r2 = {nullptr, d_pred, wl, g2, be2, t.a2, t.xh2, t.rstd2, input_lengths, S, B, drop_of(p, seed, 2), da2,
                  part, part + BF, part + 2 * BF, part + 5 * BF};
    BY_F(F, k_vp_rowbwd, rows, dim3(NT), st, r2);
    if (have) BY_F(F, k_vp_colpart, cols, dim3(64), st, r2);
    repack(W2, w.Wb2, F, F, 0, st);
    DinArgs d2 = {da2, w.Wb2, input_lengths, S, F, F, dh1};
    launch_din(d2, B, st);
    RowArgs r1 = {dh1, nullptr, nullptr, g1, nullptr, t.a1, t.xh1, t.rstd1, input_lengths, S, B, drop_of(p, seed, 1), da1,
                  part + 3 * BF, part + 4 * BF, nullptr, nullptr};
    BY_F(F, k_vp_rowbwd, rows, dim3(NT), st, r1);
    if (have) BY_F(F, k_vp_colpart, cols, dim3(64), st, r1);
    if (dx) {
        repack(W1, w.Wb1, F, D, 0, st);
        DinArgs d1 = {da1, w.Wb1, input_lengths, S, F, D, dx};
        launch_din(d1, B, st);
    }
    if (have) {
        DwArgs w2 = {da2, t.h1, input_lengths, S, B, F, F, dW2, db2};
        hipLaunchKernelGGL(k_vp_dw, dim3(F / TR, (F + DW_TN - 1) / DW_TN, 3), dim3(NT), 0, st, w2);
        DwArgs w1 = {da1, x, input_lengths, S, B, F, D, dW1, db1};
        hipLaunchKernelGGL(k_vp_dw, dim3(F / TR, (D + DW_TN - 1) / DW_TN, 3), dim3(NT), 0, st, w1);
        FinalArgs fa = {{part, part + BF, part + 2 * BF, part + 3 * BF, part + 4 * BF, part + 5 * BF},
                        {dbe2, dg2, dwl, dbe1, dg1, dbl}, input_lengths, S, B, F};
        hipLaunchKernelGGL(k_vp_colfinal, dim3(F / 64, 6), dim3(64), 0, st, fa);
    }
    return b2s_side::launch_status("backward");
}

int b2s_vp_dropout_mask(double p, uint64_t seed, int site, int B, int S, int F, uint8_t *out_bytes, void *stream) {
    if (check_bsf(B, S, F) || check_p(p)) return 1;
    if (site != 1 && site != 2) return fail("site must be 1 or 2 (got %d)", site);
    if (!out_bytes) return fail("dropout_mask: out_bytes is NULL");
    const size_t total = (size_t)B * S * F;
    const int blocks = (int)std::min<size_t>((total + NT - 1) / NT, 4096);
    hipLaunchKernelGGL(k_vp_mask, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, drop_of(p, seed, site), total, out_bytes);
    return b2s_side::launch_status("dropout_mask");
}

}  // extern "C"
