// Batched FastDTW (fastdtw 0.3.4, euclidean distance) and MSE after DTW for gfx950 (C ABI: include/b2s_metrics.h), fp64 throughout.
//
// One 256-thread workgroup per pair, one launch per call.  The block compacts the voiced frames into an fp64 copy (level 0), builds
// the halving pyramid (level l + 1 row i = (row 2i + row 2i+1) / 2, an odd last row dropped) while both sides are >= radius + 2,
// then walks the levels from the coarsest up.  The coarsest level (and the exact mode) runs over the full matrix; every finer level
// runs over the window expanded from the coarser path, which is one column interval [lo_i, hi_i] per row (DESIGN.md section h):
//     c = i / 2,  lo_i = max(0, 2 * (pmin[max(0, c - r)] - r)),  hi_i = min(ny - 1, 2 * (pmax[min(nc - 1, c + r)] + r) + 1)
// where pmin / pmax are the first / last column of the coarse path in each coarse row.
//
// The banded DP goes over strips of 64 rows, one row per lane of wave 0, skewed by one column per lane: at step s lane k updates
// cell (r0 + k, lo[r0] + s - k), so its "up" is lane k - 1's previous result (one shuffle), "diag" is the up it saw one step earlier
// and "left" is its own previous result.  Lane 63 leaves the strip's last row in LDS for lane 0 of the next strip.  Each cell does
// the library's fixed update (candidates up, left, diag in that order, strict < so ties keep the first), so the result does not
// depend on the order.  The euclidean distances of the next 16 steps are computed by waves 1-3 (16 lanes per distance) into an LDS
// tile while wave 0 runs the current 16 (double buffered).  Back-pointers take one byte per window cell, in LDS when the level fits, else in the
// workspace; a single lane backtracks.  Expect the kernel to be latency-bound: the DP is a chain of ~nx + ny steps per level.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../../include/b2s_metrics.h"
#include "../side_common.h"

using b2s_side::align_up;
using b2s_side::fail;

namespace {

constexpr int NT = 256;               // threads per block
constexpr int STEP_TILE = 16;         // DP steps per distance tile
constexpr int GRP = 16;               // lanes per distance (feature dimension split across them)
constexpr int MAX_DIM = 256;
constexpr int MAX_LEVELS = 40;
constexpr int LDS_BYTES = 64 * 1024 - 1024;    // dynamic LDS per block (the static level table and scalars take the rest of 64 KiB)

// LDS plan, sized by the longest sequences: distance tiles, the strip boundary row, per-row window / offsets, the coarse path's
// row extents, then back-pointers in whatever is left.
struct LdsPlan {
    int tile, bnd, lo, hi, roff, pmin, pmax, bp, bp_cap;
};

__host__ __device__ inline LdsPlan lds_plan(int max_x, int max_y) {
    LdsPlan p;
    const int ms = (max_x > max_y ? max_x : max_y) + 1, pc = max_x / 2 + 2;
    p.tile = 0;
    p.bnd = p.tile + 2 * STEP_TILE * 64 * 8;
    p.lo = p.bnd + (max_y + 2) * 8;
    p.hi = p.lo + (max_x + 1) * 4;
    p.roff = p.hi + (max_x + 1) * 4;
    p.pmin = p.roff + (ms + 1) * 4;
    p.pmax = p.pmin + pc * 4;
    p.bp = (p.pmax + pc * 4 + 15) & ~15;
    p.bp_cap = LDS_BYTES - p.bp;
    return p;
}

// back-pointer bytes per pair in the workspace: the exact mode's full matrix, or a bound on a fastdtw level's window
// (rows: 2 (pmax - pmin) + 4r + 2 columns each, summed: (nx + 2)(8r + 2) + (4r + 2) ny; the coarsest level: (r + 1) max(nx, ny))
size_t bp_stride(int max_x, int max_y, int radius) {
    const size_t full = (size_t)max_x * max_y;
    if (radius < 0) return align_up(full);
    const size_t r = radius, band = (max_x + 2) * (8 * r + 2) + (4 * r + 2) * max_y;
    const size_t coarse = (r + 1) * (size_t)(max_x > max_y ? max_x : max_y);
    size_t cap = band > coarse ? band : coarse;
    return align_up((cap < full ? cap : full) + 64);
}

struct WsLayout {
    size_t px, py, path, bp, total, bp_stride;
};

WsLayout layout(int B, int total_x, int total_y, int max_x, int max_y, int dim, int radius) {
    WsLayout l;
    l.px = 0;
    l.py = l.px + align_up((size_t)2 * total_x * dim * sizeof(double));
    l.path = l.py + align_up((size_t)2 * total_y * dim * sizeof(double));
    l.bp = l.path + align_up(((size_t)total_x + total_y) * 2 * sizeof(int32_t));
    l.bp_stride = bp_stride(max_x, max_y, radius);
    l.total = l.bp + (size_t)B * l.bp_stride + 256;
    return l;
}

int check_args(int B, int total_x, int total_y, int max_x, int max_y, int dim, int radius, int flags) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (dim < 1 || dim > MAX_DIM) return fail("dim must be in 1..%d (got %d)", MAX_DIM, dim);
    if (radius == 0)
        return fail("radius 0 is not supported: fastdtw 0.3.4's window is empty in the top row for odd lengths and its backtrack "
                    "fails; use radius >= 1, or -1 for the exact dtw");
    if (radius < -1) return fail("radius must be >= 1, or -1 for the exact dtw (got %d)", radius);
    if (flags & ~B2S_MET_VOICED_ONLY) return fail("unknown flags 0x%x (known: B2S_MET_VOICED_ONLY = 1)", flags);
    if (total_x < 0 || total_y < 0 || max_x < 0 || max_y < 0)
        return fail("lengths must be >= 0 (total_x %d, total_y %d, max_x %d, max_y %d)", total_x, total_y, max_x, max_y);
    if (max_x > total_x || max_y > total_y)
        return fail("max_x %d / max_y %d exceed total_x %d / total_y %d", max_x, max_y, total_x, total_y);
    const LdsPlan p = lds_plan(max_x, max_y);
    if (p.bp_cap < 0)
        return fail("max_x %d / max_y %d do not fit the on-chip plan (%d bytes of LDS needed, %d available); split longer "
                    "sequences", max_x, max_y, p.bp, LDS_BYTES);
    return 0;
}

// exclusive prefix sum of a[0..n) in place, a[n] = total; wave 0 only
__device__ void wave_scan_excl(int *a, int n) {
    const int lane = threadIdx.x & 63;
    const int seg = (n + 63) / 64;
    const int b0 = min(n, lane * seg), b1 = min(n, b0 + seg);
    int s = 0;
    for (int i = b0; i < b1; ++i) s += a[i];
    int inc = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    int run = inc - s;
    for (int i = b0; i < b1; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
    if (lane == 63) a[n] = inc;
}

// flags of the rows of one side (voiced: max over the features > 0, NaN rows are not voiced, as np.max(x, -1) > 0), scanned into
// compacted row indices, then the compacted rows copied to fp64.  Returns the compacted length.
__device__ int compact(const float *__restrict__ src, int n, int dim, int voiced_only, double *__restrict__ dst, int *roff) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += NT) {
        int keep = 1;
        if (voiced_only) {
            bool pos = false, nan = false;
            for (int d = 0; d < dim; ++d) {
                const float v = src[(size_t)i * dim + d];
                pos |= v > 0.f;
                nan |= v != v;
            }
            keep = pos && !nan;
        }
        roff[i] = keep;
    }
    __syncthreads();
    if (tid < 64) wave_scan_excl(roff, n);
    __syncthreads();
    const int m = roff[n];
    for (int e = tid; e < n * dim; e += NT) {
        const int i = e / dim, d = e - i * dim;
        if (roff[i + 1] != roff[i]) dst[(size_t)roff[i] * dim + d] = (double)src[e];
    }
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(NT) void k_met_dtw(const float *__restrict__ x, const int32_t *__restrict__ xoff, int total_x, int max_x,
                                                const float *__restrict__ y, const int32_t *__restrict__ yoff, int total_y, int max_y,
                                                int dim, int radius, int voiced_only, double *cost_out, double *mse_out,
                                                int32_t *plen_out, int32_t *status_out, int32_t *path_out,
                                                const int32_t *__restrict__ path_off, double *px_ws, double *py_ws, int32_t *path_ws,
                                                uint8_t *bp_ws, size_t bp_stride) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int sh_plen, sh_bad;
    __shared__ int lvx[MAX_LEVELS], lvy[MAX_LEVELS], ox[MAX_LEVELS], oy[MAX_LEVELS];     // pyramid: rows and first row per level
    __shared__ double sh_cost;
    const LdsPlan P = lds_plan(max_x, max_y);
    double *tile = (double *)(smem + P.tile);
    double *bnd = (double *)(smem + P.bnd);
    int *lo = (int *)(smem + P.lo), *hi = (int *)(smem + P.hi), *roff = (int *)(smem + P.roff);
    int *pmin = (int *)(smem + P.pmin), *pmax = (int *)(smem + P.pmax);
    uint8_t *bp_lds = smem + P.bp;

    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double INF = __builtin_inf(), QNAN = __builtin_nan("");
    const int x0 = xoff[b], lx = xoff[b + 1] - x0, y0 = yoff[b], ly = yoff[b + 1] - y0;
    auto finish = [&](int status, double cost, double mse, int plen) {
        if (tid == 0) {
            status_out[b] = status;
            cost_out[b] = cost;
            mse_out[b] = mse;
            plen_out[b] = plen;
        }
    };
    if (x0 < 0 || y0 < 0 || lx < 0 || ly < 0 || lx > max_x || ly > max_y || x0 + lx > total_x || y0 + ly > total_y) {
        finish(B2S_MET_FAILED, QNAN, QNAN, 0);
        return;
    }
    double *px = px_ws + (size_t)2 * x0 * dim, *py = py_ws + (size_t)2 * y0 * dim;
    const int nx0 = compact(x + (size_t)x0 * dim, lx, dim, voiced_only, px, roff);
    const int ny0 = compact(y + (size_t)y0 * dim, ly, dim, voiced_only, py, roff);
    if (nx0 == 0 || ny0 == 0) {
        finish(B2S_MET_EMPTY, QNAN, QNAN, 0);
        return;
    }

    // pyramid sizes: halve while both sides are >= radius + 2 (fastdtw's min_time_size)
    int L = 0;
    {
        int nx = nx0, ny = ny0, rx = 0, ry = 0;
        while (radius > 0 && L + 1 < MAX_LEVELS && nx >= radius + 2 && ny >= radius + 2) {
            if (tid == 0) lvx[L] = nx, lvy[L] = ny, ox[L] = rx, oy[L] = ry;
            rx += nx, ry += ny, nx /= 2, ny /= 2;
            ++L;
        }
        if (tid == 0) lvx[L] = nx, lvy[L] = ny, ox[L] = rx, oy[L] = ry;
    }
    __syncthreads();
    for (int l = 1; l <= L; ++l) {
        const double *sx = px + (size_t)ox[l - 1] * dim, *sy = py + (size_t)oy[l - 1] * dim;
        double *dx = px + (size_t)ox[l] * dim, *dy = py + (size_t)oy[l] * dim;
        for (int e = tid; e < lvx[l] * dim; e += NT) {
            const int i = e / dim, d = e - i * dim;
            dx[e] = (sx[(size_t)2 * i * dim + d] + sx[(size_t)(2 * i + 1) * dim + d]) / 2.0;
        }
        for (int e = tid; e < lvy[l] * dim; e += NT) {
            const int i = e / dim, d = e - i * dim;
            dy[e] = (sy[(size_t)2 * i * dim + d] + sy[(size_t)(2 * i + 1) * dim + d]) / 2.0;
        }
        __syncthreads();
    }

    int plen = 0;
    for (int l = L; l >= 0; --l) {
        const int nx = lvx[l], ny = lvy[l];
        const double *X = px + (size_t)ox[l] * dim, *Y = py + (size_t)oy[l] * dim;
        // window of this level: full at the coarsest, else expanded from the coarser path
        for (int i = tid; i < nx; i += NT) {
            int a = 0, c = ny - 1;
            if (l < L) {
                const int nc = lvx[l + 1], cr = i >> 1;
                a = max(0, 2 * (pmin[max(0, cr - radius)] - radius));
                c = min(ny - 1, 2 * (pmax[min(nc - 1, cr + radius)] + radius) + 1);
            }
            lo[i] = a, hi[i] = c, roff[i] = c - a + 1;
        }
        for (int j = tid; j <= ny; j += NT) bnd[j] = j == 0 ? 0.0 : INF;
        __syncthreads();
        if (tid < 64) wave_scan_excl(roff, nx);
        __syncthreads();
        const int cells = roff[nx];
        uint8_t *bp = cells <= P.bp_cap ? bp_lds : bp_ws + (size_t)b * bp_stride;
        if (cells > P.bp_cap && (size_t)cells > bp_stride) {
            finish(B2S_MET_FAILED, QNAN, QNAN, 0);
            return;
        }

        for (int r0 = 0; r0 < nx; r0 += 64) {
            const int rl = min(r0 + 63, nx - 1), base = lo[r0];
            const int steps = hi[rl] - base + 1 + (rl - r0), ntiles = (steps + STEP_TILE - 1) / STEP_TILE;
            // distances of tile t (steps t * 16 ..) for every lane's cell inside the window; waves 1-3 as 12 groups of 16 lanes,
            // one DP row per group at a time: the x row stays in registers, each y row is read coalesced, the 16 partial sums are
            // combined by a fixed butterfly (only the order of the feature sum differs from NumPy's dot)
            auto fill = [&](int t, double *buf) {
                const int g = (tid - 64) / GRP, sl = tid % GRP, s0 = t * STEP_TILE, send = min(STEP_TILE, steps - s0);
                for (int k = g; k < 64 && r0 + k < nx; k += (NT - 64) / GRP) {
                    const int r = r0 + k;
                    const int ua = max(0, lo[r] - base + k - s0), ub = min(send, hi[r] - base + k - s0 + 1);
                    if (ua >= ub) continue;
                    const double *xrow = X + (size_t)r * dim;
                    double xr[MAX_DIM / GRP];
#pragma unroll
                    for (int m = 0; m < MAX_DIM / GRP; ++m) xr[m] = sl + m * GRP < dim ? xrow[sl + m * GRP] : 0.0;
                    for (int u = ua; u < ub; ++u) {
                        const double *yrow = Y + (size_t)(base + s0 + u - k) * dim;
                        double acc = 0.0;
#pragma unroll
                        for (int m = 0; m < MAX_DIM / GRP; ++m) {
                            if (sl + m * GRP < dim) {
                                const double e = xr[m] - yrow[sl + m * GRP];
                                acc += e * e;
                            }
                        }
                        for (int o = 1; o < GRP; o <<= 1) acc += __shfl_xor(acc, o, GRP);
                        if (sl == 0) buf[u * 64 + k] = sqrt(acc);
                    }
                }
            };
            const int r = r0 + lane;
            const bool act = r < nx;
            const int mylo = act ? lo[r] : 0, myhi = act ? hi[r] : -1, myoff = act ? roff[r] : 0;
            double cur = INF, upp = INF;
            if (wave != 0) fill(0, tile);
            __syncthreads();
            for (int t = 0; t < ntiles; ++t) {
                if (wave == 0) {
                    const double *tb = tile + (t & 1) * STEP_TILE * 64;
                    const int s1 = min(STEP_TILE, steps - t * STEP_TILE);
                    for (int u = 0; u < s1; ++u) {
                        const int j = base + t * STEP_TILE + u - lane;
                        double upv = __shfl_up(cur, 1);      // lane k - 1 at the previous step: D[i - 1, j]
                        double dgv = upp;                    // lane k - 1 two steps back: D[i - 1, j - 1]
                        upp = upv;
                        if (act && j >= mylo && j <= myhi) {
                            if (lane == 0) upv = bnd[j + 1], dgv = bnd[j];
                            const double dt = tb[u * 64 + lane];
                            double best = upv + dt;
                            uint8_t dir = 0;
                            const double lf = cur + dt, dg = dgv + dt;
                            if (lf < best) best = lf, dir = 1;
                            if (dg < best) best = dg, dir = 2;
                            cur = best;
                            bp[myoff + (j - mylo)] = dir;
                            if (r == nx - 1 && j == ny - 1) sh_cost = best;
                        } else {
                            cur = INF;
                        }
                        if (lane == 63 && j >= 0 && j < ny) bnd[j + 1] = cur;
                    }
                } else if (t + 1 < ntiles) {
                    fill(t + 1, tile + ((t + 1) & 1) * STEP_TILE * 64);
                }
                __syncthreads();
            }
            if (tid == 0) bnd[0] = INF;                     // D[i, 0] = inf below the first strip
        }

        // backtrack from (nx, ny): the level-0 path into the workspace (reversed), a coarser level's row extents into pmin / pmax
        if (tid == 0) {
            int I = nx, J = ny, n = 0, last = -1, bad = 0;
            int32_t *pw = path_ws + (size_t)2 * (x0 + y0);
            while (I > 0 || J > 0) {
                const int i = I - 1, j = J - 1;
                if (I <= 0 || J <= 0 || n >= nx + ny || j < lo[i] || j > hi[i]) {
                    bad = 1;
                    break;
                }
                if (l == 0) {
                    pw[2 * n] = i, pw[2 * n + 1] = j;
                } else {
                    if (i != last) pmax[i] = j, last = i;
                    pmin[i] = j;
                }
                ++n;
                const uint8_t dir = bp[roff[i] + j - lo[i]];
                if (dir != 1) --I;
                if (dir != 0) --J;
            }
            sh_plen = n;
            sh_bad = bad;
        }
        __syncthreads();
        if (sh_bad) {
            finish(B2S_MET_FAILED, QNAN, QNAN, 0);
            return;
        }
        plen = sh_plen;
    }

    // MSE over the path on the level-0 rows (exact fp64 copies of the fp32 inputs); fixed-order tree reduction
    const int32_t *pw = path_ws + (size_t)2 * (x0 + y0);
    double acc = 0.0;
    for (int q = tid; q < plen; q += NT) {
        const double *a = px + (size_t)pw[2 * q] * dim, *c = py + (size_t)pw[2 * q + 1] * dim;
        for (int d = 0; d < dim; ++d) {
            const double e = a[d] - c[d];
            acc += e * e;
        }
    }
    double *red = tile;
    red[tid] = acc;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    int status = B2S_MET_OK;
    if (path_out) {
        const int p0 = path_off[b];
        if (path_off[b + 1] - p0 < plen) {
            status = B2S_MET_FAILED;
        } else {
            for (int q = tid; q < plen; q += NT) {
                const int m = plen - 1 - q;
                path_out[2 * ((size_t)p0 + m)] = pw[2 * q];
                path_out[2 * ((size_t)p0 + m) + 1] = pw[2 * q + 1];
            }
        }
    }
    finish(status, sh_cost, red[0] / ((double)plen * dim), plen);
}

}  // namespace

extern "C" {

int b2s_met_version(void) { return 100; }

const char *b2s_met_last_error(void) { return b2s_side::last_error(); }

size_t b2s_met_dtw_ws_bytes(int B, int total_x, int total_y, int max_x, int max_y, int dim, int radius, int flags) {
    if (check_args(B, total_x, total_y, max_x, max_y, dim, radius, flags)) return 0;
    return layout(B, total_x, total_y, max_x, max_y, dim, radius).total;
}

int b2s_met_dtw(const float *x, const int32_t *x_offsets, int total_x, int max_x, const float *y, const int32_t *y_offsets,
                int total_y, int max_y, int B, int dim, int radius, int flags, double *cost_out, double *mse_out,
                int32_t *path_len_out, int32_t *status_out, int32_t *path_out, const int32_t *path_offsets, void *ws,
                size_t ws_bytes, void *stream) {
    if (check_args(B, total_x, total_y, max_x, max_y, dim, radius, flags)) return 1;
    if (!x_offsets || !y_offsets || !cost_out || !mse_out || !path_len_out || !status_out || !ws)
        return fail("dtw: a pointer argument is NULL");
    if ((total_x > 0 && !x) || (total_y > 0 && !y)) return fail("dtw: x or y is NULL");
    if (path_out && !path_offsets) return fail("dtw: path_out needs path_offsets");
    const WsLayout l = layout(B, total_x, total_y, max_x, max_y, dim, radius);
    if (ws_bytes < l.total) return fail("dtw: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    char *w = (char *)ws;
    hipLaunchKernelGGL(k_met_dtw, dim3(B), dim3(NT), LDS_BYTES, (hipStream_t)stream, x, x_offsets, total_x, max_x, y, y_offsets,
                       total_y, max_y, dim, radius, flags & B2S_MET_VOICED_ONLY, cost_out, mse_out, path_len_out, status_out,
                       path_out, path_offsets, (double *)(w + l.px), (double *)(w + l.py), (int32_t *)(w + l.path),
                       (uint8_t *)(w + l.bp), l.bp_stride);
    return b2s_side::launch_status("dtw");
}

}  // extern "C"
