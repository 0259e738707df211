// Batched Levenshtein distance with the substitution / deletion / insertion breakdown for gfx950 (C ABI: include/b2s_metrics.h,
// b2s_met_edit_*): the edit distance behind the eval's CER, and word-level WER on the same kernel.
//
// Contract: unit costs; per pair the lexicographically smallest (cost, substitutions) over all alignments.  One int32 per cell holds
// cost << 16 | sub: a mismatch on the diagonal adds 0x10001, a match 0, a deletion or an insertion 0x10000, and the plain integer
// minimum of the three candidates is that lexicographic minimum (at <= 4096 symbols per side cost <= 8192 and sub <= 4096, so nothing
// carries between the halves or reaches the sign bit).  del and ins follow from del - ins = la - lb.
//
// k_met_edit: one wave64 per pair, four pairs per 256-thread block, run as a systolic array.  No LDS, no workspace, no barrier.
// The prediction b lies along the lanes: lane l owns the C adjacent columns l * C + 1 .. l * C + C of the DP matrix, their b symbols
// and their current row in registers.  C is the smallest of {1, 2, 4, 8, 16, 32, 64} with 64 * C >= lb, chosen PER PAIR (wave-
// uniform; the launch is templated on the largest C that max_b allows, which bounds the registers), so a short pair of a ragged batch
// does not pay for the longest one.  At step t lane l computes DP row t - l + 1 (truth symbol a[t - l]): it takes lane l - 1's last
// column of that row and the symbol of that row with two wave-shift DPP moves (one VALU instruction each, no LDS crossbar), lane 0
// takes the boundary (t + 1) << 16 and a[t] instead.  The truth is read 64 symbols at a time, one per lane, a block ahead of its
// use, and handed to lane 0 with v_readlane.  la + ceil(lb / C) - 1 steps finish a pair; a lane outside its rows does not update, so
// afterwards every lane holds DP row la of its strip and the answer is read from the lane of column lb.
//
// Cells are kept as x[j] = DP[i][j] - j * 0x10000.  In that form the candidate from the left neighbour is the neighbour's x itself,
// so the chain that runs along a strip is ONE v_min3_i32 per cell; the other four instructions of a cell (compare, select, two adds)
// do not depend on it.  Row 0 is x = 0 everywhere, and the value passed between lanes needs no conversion.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../../include/b2s_metrics.h"
#include "../side_common.h"

namespace {

using b2s_side::fail;

constexpr int MAX_LEN = 4096;         // symbols per side: 64 lanes x 64 columns
constexpr int NT = 256;               // threads per block = 4 pairs
constexpr int D = 0x10000;            // one deletion or insertion

// lane l receives lane l - 1's value (DPP wave_shr:1); lane 0 keeps its own, which the caller replaces
__device__ __forceinline__ int lane_up(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

// One pair on one wave, 1 <= la, 1 <= lb <= 64 * C, every argument but `lane` wave-uniform.  Returns cost << 16 | sub.
template <int C>
__device__ __forceinline__ int edit_wave(const int32_t *__restrict__ a, int la, const int32_t *__restrict__ b, int lb, int lane) {
    int bs[C], x[C];
    const int j0 = lane * C;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        bs[k] = j0 + k < lb ? b[j0 + k] : 0;      // columns past lb compute values that no column <= lb ever reads
        x[k] = 0;
    }
    const int nl = (lb + C - 1) / C;              // lanes that own a column
    const int rows = lane < nl ? la : 0;
    const int steps = la + nl - 1;
    int prev_left = 0;                            // x of this strip's left neighbour column in the previous row
    int out = 0, sym = 0;                         // what lane l + 1 takes next step: the strip's last x and the row's truth symbol
    int cur = lane < la ? a[lane] : 0;            // truth symbols t0 .. t0 + 63, one per lane
    int t0 = 0;
    auto step = [&](int i) __attribute__((always_inline)) {
        const int t = t0 + i;
        int left = lane_up(out), s = lane_up(sym);
        const int a_t = __builtin_amdgcn_readlane(cur, i);
        if (lane == 0) {
            left = (t + 1) << 16;
            s = a_t;
        }
        if ((unsigned)(t - lane) < (unsigned)rows) {
            const int new_left = left;
            int diag = prev_left;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const int up = x[k];
                const int c_up = up + D;
                const int c_diag = diag + (s != bs[k] ? 1 : -D);
                left = min(min(c_up, c_diag), left);
                diag = up;
                x[k] = left;
            }
            prev_left = new_left;
            out = left;
            sym = s;
        }
    };
    for (; t0 < steps; t0 += 64) {
        // The first step of a block stands outside the loop so that the load of the next block is issued after the wait for this
        // block's symbols: the loop itself then waits for no memory, and the load has the rest of the block to land.
        step(0);
        const int ahead = t0 + 64 + lane;
        const int next = ahead < la ? a[ahead] : 0;
        const int n = min(64, steps - t0);
        for (int i = 1; i < n; ++i) step(i);
        cur = next;
    }
    const int lr = (lb - 1) / C, kr = (lb - 1) - lr * C;
    int r = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) r = k == kr ? x[k] : r;
    return __builtin_amdgcn_readlane(r, lr) + (lb << 16);
}

template <int CMAX>
__device__ __forceinline__ int edit_dispatch(int need, const int32_t *a, int la, const int32_t *b, int lb, int lane) {
    if constexpr (CMAX > 1) {
        if (need <= CMAX / 2) return edit_dispatch<CMAX / 2>(need, a, la, b, lb, lane);
    }
    return edit_wave<CMAX>(a, la, b, lb, lane);
}

template <int CMAX>
__global__ __launch_bounds__(NT) void k_met_edit(const int32_t *__restrict__ a, const int32_t *__restrict__ a_offsets, int total_a,
                                                 int max_a, const int32_t *__restrict__ b, const int32_t *__restrict__ b_offsets,
                                                 int total_b, int max_b, int B, int32_t *__restrict__ dist_out,
                                                 int32_t *__restrict__ ops_out, int32_t *__restrict__ status_out) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (NT / 64) + (threadIdx.x >> 6)));
    if (p >= B) return;
    const int oa = __builtin_amdgcn_readfirstlane(a_offsets[p]), oa1 = __builtin_amdgcn_readfirstlane(a_offsets[p + 1]);
    const int ob = __builtin_amdgcn_readfirstlane(b_offsets[p]), ob1 = __builtin_amdgcn_readfirstlane(b_offsets[p + 1]);
    // in this order nothing overflows: 0 <= oa <= oa1 <= total_a, then the length against max_a (<= MAX_LEN <= 64 * CMAX for b)
    const bool bad = oa < 0 || oa1 < oa || oa1 > total_a || oa1 - oa > max_a || ob < 0 || ob1 < ob || ob1 > total_b || ob1 - ob > max_b;
    if (bad) {
        if (lane == 0) {
            dist_out[p] = -1;
            status_out[p] = B2S_MET_FAILED;
        }
        if (ops_out && lane < 3) ops_out[(size_t)p * 3 + lane] = -1;
        return;
    }
    const int la = oa1 - oa, lb = ob1 - ob;
    int packed;
    if (la == 0 || lb == 0) packed = (la + lb) << 16;             // all insertions or all deletions
    else packed = edit_dispatch<CMAX>((lb + 63) >> 6, a + oa, la, b + ob, lb, lane);
    if (lane == 0) {
        const int cost = packed >> 16, sub = packed & 0xffff;
        const int del = (cost - sub + la - lb) / 2;               // a truth symbol with no counterpart in the prediction
        dist_out[p] = cost;
        status_out[p] = B2S_MET_OK;
        if (ops_out) {
            ops_out[(size_t)p * 3 + 0] = sub;
            ops_out[(size_t)p * 3 + 1] = del;
            ops_out[(size_t)p * 3 + 2] = cost - sub - del;
        }
    }
}

template <int CMAX>
void launch(const int32_t *a, const int32_t *a_offsets, int total_a, int max_a, const int32_t *b, const int32_t *b_offsets,
            int total_b, int max_b, int B, int32_t *dist_out, int32_t *ops_out, int32_t *status_out, hipStream_t stream) {
    const int per_block = NT / 64;
    hipLaunchKernelGGL(k_met_edit<CMAX>, dim3((B + per_block - 1) / per_block), dim3(NT), 0, stream, a, a_offsets, total_a, max_a, b,
                       b_offsets, total_b, max_b, B, dist_out, ops_out, status_out);
}

}  // namespace

extern "C" {

int b2s_met_edit_max_len(void) { return MAX_LEN; }

int b2s_met_edit_distance(const int32_t *a, const int32_t *a_offsets, int total_a, int max_a, const int32_t *b,
                          const int32_t *b_offsets, int total_b, int max_b, int B, int32_t *dist_out, int32_t *ops_out,
                          int32_t *status_out, void *stream) {
    if (B <= 0) return fail("edit: B must be > 0 (got %d)", B);
    if (total_a < 0 || total_b < 0) return fail("edit: totals must be >= 0 (got %d and %d)", total_a, total_b);
    if (max_a < 0 || max_a > MAX_LEN) return fail("edit: max_a must be in 0..%d (got %d)", MAX_LEN, max_a);
    if (max_b < 0 || max_b > MAX_LEN) return fail("edit: max_b must be in 0..%d (got %d)", MAX_LEN, max_b);
    if (!a_offsets || !b_offsets) return fail("edit: a_offsets or b_offsets is NULL");
    if ((total_a > 0 && !a) || (total_b > 0 && !b)) return fail("edit: a or b is NULL with symbols to read");
    if (!dist_out || !status_out) return fail("edit: dist_out or status_out is NULL");
    const hipStream_t s = (hipStream_t)stream;
    const int need = (max_b + 63) / 64;           // columns per lane of the longest prediction
#define B2S_EDIT_LAUNCH(CMAX) \
    launch<CMAX>(a, a_offsets, total_a, max_a, b, b_offsets, total_b, max_b, B, dist_out, ops_out, status_out, s)
    if (need <= 1) B2S_EDIT_LAUNCH(1);
    else if (need <= 2) B2S_EDIT_LAUNCH(2);
    else if (need <= 4) B2S_EDIT_LAUNCH(4);
    else if (need <= 8) B2S_EDIT_LAUNCH(8);
    else if (need <= 16) B2S_EDIT_LAUNCH(16);
    else if (need <= 32) B2S_EDIT_LAUNCH(32);
    else B2S_EDIT_LAUNCH(64);
#undef B2S_EDIT_LAUNCH
    return b2s_side::launch_status("edit");
}

}  // extern "C"
