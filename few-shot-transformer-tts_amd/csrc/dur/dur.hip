// Monotonic alignment search and the duration error for gfx950 (C ABI: include/b2s_dur.h, definition: DESIGN.md section m).
//
// k_dur_mas<VEC, MULTI>  one workgroup per utterance, one lane per encoder position, the row Q[t-1] in registers (fp64).  Lane s
//                reads its own row maps[b][s][:] in blocks of 16 frames (four 16-byte loads with VEC, i.e. T a multiple of 4 and an
//                aligned base; sixteen dword loads otherwise), two blocks ahead of the one it works on, through a ring of three
//                register blocks.  Q[t-1][s-1] arrives by a DPP wave shift inside a wave.  Across waves (MULTI, S > 64) the waves are
//                skewed by one block: in macro-step m wave w works on block m - w, and before each frame its last lane leaves
//                Q[t-1] in LDS, where wave w + 1 picks the sixteen values up one macro-step later.  That is ONE barrier per sixteen
//                frames, nblocks + waves - 1 of them, executed by every wave alike (no spinning, no flags).  S <= 64 is one wave
//                without a barrier.  Each frame's decisions leave as one ballot word per wave: lane j keeps the word of frame j of
//                the block, and the block's words go out in one store.  Then wave 0 walks back over the words, 64 frames per load
//                (lane j holds the word of frame t - j; the serial part reads it with readlane and only collects the steps, the
//                path and the frame where each position starts follow from a popcount per lane); the durations are the differences
//                of those starts.
// k_dur_score    one workgroup per pair: unit sums from LDS, twelve int64 reductions over a fixed tree.  Integers only.
// Contraction is off for the whole file, although no product is formed: every cell is one add and one compare.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include <cstdint>
#include "../../../include/b2s_dur.h"
#include "../side_common.h"

using b2s_side::fail;

#pragma clang fp contract(off)

namespace {

constexpr int K = 16;                      // frames per block
constexpr int RING = 3;                    // register blocks: the one in work and two in flight
constexpr int MAX_WAVES = B2S_DUR_MAX_S / 64;
constexpr int NT = 256;                    // threads of the score kernel
constexpr unsigned long long MAX_CELLS = 1ull << 40;   // B x S x T of one call

// ------------------------------------------------------------------------------------------------------------------- search

struct MasArgs {
    const float *maps;
    const int32_t *enc_len, *dec_len;
    int S, T, W64;
    int32_t *path, *dur;
    double *score;
    int32_t *status;
    unsigned long long *dec;               // [B, T, W64] decision words
};

// v of the lane below; lane 0 of the wave gets `first`.  wave_shr:1 with bound_ctrl off leaves `old` where there is no source lane.
__device__ __forceinline__ double from_lane_below(double v, double first) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double read_lane(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// The barrier of the frame loop orders LDS traffic only: a full __syncthreads() would also wait for the loads in flight, which
// are asked for two blocks ahead exactly so that nobody waits for them.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Frames k K .. k K + 15 of one row, asked for without a branch: a steady stream of loads is what lets the compiler count the ones
// in flight instead of waiting for all of them.  A frame from Tb on is replaced by the last frame (VEC: the last 16-byte group) below
// Tb, and a block index outside 0 .. nblocks - 1 by the nearest inside, so every address is a valid cell of the row; what comes back
// for such a frame is never used.
template <bool VEC>
__device__ __forceinline__ void load_block(const float *row, int k, int nblocks, int Tb, float (&d)[K]) {
    k = min(max(k, 0), nblocks - 1);
#pragma unroll
    for (int g = 0; g < K / 4; ++g) {
        const int t0 = k * K + 4 * g;
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4 *>(row + min(t0, (Tb - 1) & ~3));
            d[4 * g] = v.x, d[4 * g + 1] = v.y, d[4 * g + 2] = v.z, d[4 * g + 3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) d[4 * g + i] = row[min(t0 + i, Tb - 1)];
        }
    }
}

// what a lane carries from frame to frame
struct Lane {
    double q;                              // Q[t-1][s]
    int bad;                               // a NaN or Inf was met
};

// The sixteen frames of block k (FULL: all below Tb) on the weights p.  ev: lane j holds Q[t-1] of the position below this wave
// for frame j of the block.  edge_out: where the last lane leaves this wave's own.  Returns the ballot word of frame `lane`.
template <bool MULTI, bool FULL>
__device__ __forceinline__ unsigned long long run_block(Lane &st, const float (&p)[K], int k, int Tb, int tid, bool mine, double ev,
                                                        double *edge_out) {
    const int lane = tid & 63;
    const double NINF = -__builtin_inf();
    unsigned long long word = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (FULL || k * K + j < Tb) {
            const float pv = p[j];
            st.bad |= mine && !(fabsf(pv) <= FLT_MAX);
            if (MULTI && lane == 63) edge_out[j] = st.q;
            double left = from_lane_below(st.q, MULTI ? read_lane(ev, j) : NINF);
            if (j == 0 && k == 0) {                      // frame 0: Q[0][0] = p[0][0] and -inf above it
                left = NINF;
                st.q = tid == 0 ? -0.0 : NINF;           // -0.0 + p is p, bit for bit
            }
            const bool mv = left > st.q;
            const unsigned long long bal = __ballot(mv);
            if (lane == j) word = bal;
            st.q = (double)pv + (mv ? left : st.q);
        }
    }
    return word;
}

template <bool VEC, bool MULTI>
__global__ __launch_bounds__(B2S_DUR_MAX_S) void k_dur_mas(MasArgs a) {
    __shared__ double edge[MULTI ? MAX_WAVES : 1][2][K];
    __shared__ int start[B2S_DUR_MAX_S + 1];
    __shared__ double score_sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Sb = a.enc_len[b], Tb = a.dec_len[b];
    int32_t *path = a.path + (size_t)b * a.T, *dur = a.dur + (size_t)b * a.S;
    const double QNAN = __builtin_nan(""), NINF = -__builtin_inf();

    auto nothing = [&](int st) {                         // the outputs of every status but OK
        for (int i = tid; i < a.T; i += nthr) path[i] = -1;
        for (int i = tid; i < a.S; i += nthr) dur[i] = 0;
        if (tid == 0) {
            a.status[b] = st;
            a.score[b] = st == B2S_DUR_EMPTY ? 0.0 : QNAN;
        }
    };
    if (Sb < 0 || Sb > a.S || Tb < 0 || Tb > a.T) return nothing(B2S_DUR_FAILED);      // the whole workgroup, here and below
    if (Sb == 0 || Tb == 0) return nothing(B2S_DUR_EMPTY);
    if (Tb < Sb) return nothing(B2S_DUR_SHORT);

    const int nblocks = (Tb + K - 1) / K, nfull = Tb / K, Wb = (Sb + 63) >> 6, M = nblocks + Wb - 1;
    const bool mine = tid < Sb, working = w < Wb;
    const float *row = a.maps + ((size_t)b * a.S + min(tid, Sb - 1)) * a.T;           // a lane without a position rereads the last one
    unsigned long long *dec = a.dec + (size_t)b * a.T * a.W64;
    Lane st = {NINF, 0};
    float buf[RING][K];
    // Macro-step m: this wave works on block m - w, whose weights sit in ring slot (m + 2) % 3, and asks for those of macro-step
    // m + 2.  The count starts at m = -2, so that the first two requests go out before the first frame, and runs in threes: the
    // steps before 0 and from M on find no block and only meet at the barrier.
    for (int m0 = -2; m0 < M; m0 += RING) {
#pragma unroll
        for (int r = 0; r < RING; ++r) {
            const int m = m0 + r, kn = m + 2 - w, k = m - w;
            load_block<VEC>(row, kn, nblocks, Tb, buf[(r + 2) % RING]);
            if (working && k >= 0 && k < nblocks) {
                double ev = NINF;
                if (MULTI && w > 0) ev = edge[w - 1][(m + 1) & 1][lane & (K - 1)];     // left there one macro-step ago
                double *edge_out = edge[MULTI ? w : 0][m & 1];
                const unsigned long long word = k < nfull ? run_block<MULTI, true>(st, buf[r], k, Tb, tid, mine, ev, edge_out)
                                                          : run_block<MULTI, false>(st, buf[r], k, Tb, tid, mine, ev, edge_out);
                const int t = k * K + lane;
                if (lane < K && t < Tb) dec[(size_t)t * a.W64 + w] = word;
            }
            if (MULTI) lds_barrier();
        }
    }
    const double q = st.q;
    const int bad = st.bad;
    if (tid == Sb - 1) score_sh = q;
    for (int i = Tb + tid; i < a.T; i += nthr) path[i] = -1;
    __threadfence_block();
    if (__syncthreads_or(bad)) return nothing(B2S_DUR_FAILED);

    if (w == 0) {
        // The walk back, 64 frames per round inside one column of 64 positions.  Lane j holds the decision word of frame t - j.  The
        // serial part runs on values every lane shares (the scalar unit): it only collects, as bit j of `steps`, whether the path
        // steps down at frame t - j, and stops early when it leaves the column.  Everything else follows in parallel: the position
        // at frame t - j is the round's first position minus the steps before lane j, and where a lane's frame steps down its
        // position starts.  Bit 0 of column 0 is cleared (nothing lies below position 0), so x stays >= 0 there.
        int sp = Sb - 1, t = Tb - 1;
        while (t >= 1) {
            const int c = sp >> 6, tt = t - lane;
            unsigned long long wd = tt >= 1 ? dec[(size_t)tt * a.W64 + c] : 0ull;
            if (c == 0) wd &= ~1ull;
            int x = sp & 63, j = 0;
            unsigned long long steps = 0;
            while (j < 64 && x >= 0) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)wd, j);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(wd >> 32), j);
                const unsigned long long bit = ((((unsigned long long)hi << 32) | lo) >> x) & 1ull;
                steps |= bit << j;
                x -= (int)bit;
                ++j;
            }
            const int p = sp - __popcll(steps & ((1ull << lane) - 1ull));
            if (lane < j && tt >= 1) {
                path[tt] = p;
                if ((steps >> lane) & 1ull) start[p] = tt;
            }
            sp -= __popcll(steps);
            t -= j;
        }
        if (lane == 0) {
            path[0] = sp;
            start[0] = 0;
            start[Sb] = Tb;
        }
    }
    __syncthreads();
    for (int i = tid; i < a.S; i += nthr) dur[i] = i < Sb ? start[i + 1] - start[i] : 0;
    if (tid == 0) {
        a.status[b] = B2S_DUR_OK;
        a.score[b] = score_sh;
    }
}

// -------------------------------------------------------------------------------------------------------------------- score

__global__ __launch_bounds__(NT) void k_dur_score(const int32_t *__restrict__ dur_x, const int32_t *__restrict__ dur_y,
                                                 const int32_t *__restrict__ enc_len, const int32_t *__restrict__ groups, int S,
                                                 long long *__restrict__ counts, int32_t *__restrict__ status) {
    __shared__ int sx[B2S_DUR_MAX_S], sy[B2S_DUR_MAX_S], sg[B2S_DUR_MAX_S];
    __shared__ unsigned long long red[B2S_DUR_COUNTS][NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = enc_len[b];
    long long *out = counts + (size_t)b * B2S_DUR_COUNTS;
    auto nothing = [&](int st) {
        if (tid == 0) status[b] = st;
        if (tid < B2S_DUR_COUNTS) out[tid] = 0;
    };
    if (n < 0 || n > S) return nothing(B2S_DUR_FAILED);                                // the whole workgroup, here and below
    if (n == 0) return nothing(B2S_DUR_EMPTY);
    int bad = 0;
    for (int i = tid; i < n; i += NT) {
        const int x = dur_x[(size_t)b * S + i], y = dur_y[(size_t)b * S + i];
        sx[i] = x, sy[i] = y, sg[i] = groups ? groups[(size_t)b * S + i] : i;
        bad |= x < 0 || y < 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
        const long long step = i == 0 ? (long long)sg[0] : (long long)sg[i] - sg[i - 1];
        bad |= i == 0 ? step != 0 : (step < 0 || step > 1);
    }
    if (__syncthreads_or(bad)) return nothing(B2S_DUR_FAILED);
    // a side's total is checked below; until then the squares are taken modulo 2^64 and never signed
    unsigned long long v[B2S_DUR_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += NT) {
        if (i > 0 && sg[i] == sg[i - 1]) continue;                                     // not the first position of its unit
        unsigned long long dx = 0, dy = 0;
        for (int e = i; e < n && sg[e] == sg[i]; ++e) dx += (unsigned)sx[e], dy += (unsigned)sy[e];
        const unsigned long long ad = dx > dy ? dx - dy : dy - dx;
        v[0] += 1, v[1] += dx, v[2] += dy, v[3] += ad, v[4] += ad * ad, v[5] += dx * dx, v[6] += dy * dy, v[7] += dx * dy;
        v[8] = dx > v[8] ? dx : v[8], v[9] = dy > v[9] ? dy : v[9];
        v[10] += dx == 0, v[11] += dy == 0;
    }
    for (int c = 0; c < B2S_DUR_COUNTS; ++c) red[c][tid] = v[c];
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h)
            for (int c = 0; c < B2S_DUR_COUNTS; ++c) {
                const unsigned long long p = red[c][tid], o = red[c][tid + h];
                red[c][tid] = (c == 8 || c == 9) ? (p > o ? p : o) : p + o;
            }
        __syncthreads();
    }
    if (red[1][0] > (unsigned long long)INT_MAX || red[2][0] > (unsigned long long)INT_MAX) return nothing(B2S_DUR_FAILED);
    if (tid == 0) status[b] = B2S_DUR_OK;
    if (tid < B2S_DUR_COUNTS) out[tid] = (long long)red[tid][0];
}

// sizes of b2s_dur_ws_bytes and b2s_dur_mas: 0 and the workspace bytes, or 1 and a message
int mas_sizes(int B, int S, int T, size_t *bytes) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (S < 1 || S > B2S_DUR_MAX_S) return fail("S must be in 1..%d (got %d)", B2S_DUR_MAX_S, S);
    if (T < 1) return fail("T must be >= 1 (got %d)", T);
    if ((unsigned long long)B * (unsigned long long)T > MAX_CELLS / (unsigned long long)S)
        return fail("%d maps of %d x %d exceed the 2^40 cells of one call; split the batch", B, S, T);
    *bytes = (size_t)B * (size_t)T * (size_t)((S + 63) / 64) * sizeof(unsigned long long);
    return 0;
}

}  // namespace

extern "C" {

int b2s_dur_version(void) { return 100; }

const char *b2s_dur_last_error(void) { return b2s_side::last_error(); }

size_t b2s_dur_ws_bytes(int B, int S, int T) {
    size_t bytes = 0;
    return mas_sizes(B, S, T, &bytes) ? 0 : bytes;
}

int b2s_dur_mas(const float *maps, const int32_t *enc_len, const int32_t *dec_len, int B, int S, int T, int32_t *path,
                int32_t *durations, double *score, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    size_t need = 0;
    if (mas_sizes(B, S, T, &need)) return 1;
    if (!maps || !enc_len || !dec_len) return fail("mas: maps, enc_len or dec_len is NULL");
    if (!path || !durations || !score || !status) return fail("mas: path, durations, score or status is NULL");
    if (!ws || ws_bytes < need) return fail("mas: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    if ((uintptr_t)ws % sizeof(unsigned long long)) return fail("mas: the workspace must be 8-byte aligned");
    MasArgs a;
    a.maps = maps, a.enc_len = enc_len, a.dec_len = dec_len, a.S = S, a.T = T, a.W64 = (S + 63) / 64;
    a.path = path, a.dur = durations, a.score = score, a.status = status, a.dec = (unsigned long long *)ws;
    const bool vec = T % 4 == 0 && (uintptr_t)maps % 16 == 0;
    const dim3 grid(B), block(64 * a.W64);
    const hipStream_t st = (hipStream_t)stream;
    if (a.W64 > 1) {
        if (vec) hipLaunchKernelGGL((k_dur_mas<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_dur_mas<false, true>), grid, block, 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_dur_mas<true, false>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_dur_mas<false, false>), grid, block, 0, st, a);
    }
    return b2s_side::launch_status("mas");
}

int b2s_dur_score(const int32_t *dur_x, const int32_t *dur_y, const int32_t *enc_len, const int32_t *groups, int B, int S,
                  int64_t *counts, int32_t *status, void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (S < 1 || S > B2S_DUR_MAX_S) return fail("S must be in 1..%d (got %d)", B2S_DUR_MAX_S, S);
    if (!dur_x || !dur_y || !enc_len) return fail("score: dur_x, dur_y or enc_len is NULL");
    if (!counts || !status) return fail("score: counts or status is NULL");
    hipLaunchKernelGGL(k_dur_score, dim3(B), dim3(NT), 0, (hipStream_t)stream, dur_x, dur_y, enc_len, groups, S,
                       (long long *)counts, status);
    return b2s_side::launch_status("score");
}

}  // extern "C"
