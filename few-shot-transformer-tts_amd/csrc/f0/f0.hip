// YIN pitch tracking and the F0 error along a DTW path for gfx950 (C ABI: include/b2s_f0.h, definition: DESIGN.md section l).
//
// k_f0_quantize  one workgroup per utterance: the peak and a non-finite flag (maximum and OR, order free), then the int16 row
// k_f0_yin<R>    one wave per frame, up to 4 frames of one utterance per workgroup.  The frame's segment sits in the wave's own
//                slice of LDS as fp64.  Lane l owns the R consecutive lags R l .. R l + R - 1 and keeps a sliding register window
//                of seg[j + R l ..]: per sample j one broadcast read of seg[j] and one new window element feed R + 1 FMAs (the
//                autocorrelation r[tau] of its lags and the energy of its first lag).  R is odd (5 up to 319 lags, 9 up to 512), so
//                the lanes' window reads, R doubles apart, fall into different banks.  d[tau] = E(0) + E(tau) - 2 r(tau) with
//                E(tau + 1) = E(tau) - seg[tau]^2 + seg[tau + win]^2.  Every operand is an integer below 2^53, so the fp64 FMAs are
//                exact in any order.  The running sum over tau is a serial sum over a lane's lags and a shuffle scan over the
//                lanes; the threshold search, the minimum and the local-minimum walk are wave minimum reductions.
// k_f0_score     one workgroup per pair, as k_mcd_score: a gather along the path, per-thread sums in step order, a fixed tree.
// Contraction is off for the whole file: the FMAs of the autocorrelation are written as fma(), everything else rounds on its own.
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include "../../../include/b2s_f0.h"
#include "../side_common.h"

using b2s_side::fail;

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                // threads per block of the score kernel
constexpr int QNT = 1024;              // ... of the quantiser: one workgroup per utterance, so as many loads in flight as a block can hold
constexpr int YIN_LDS = 64 * 1024;     // LDS of one YIN workgroup at most

// ------------------------------------------------------------------------------------------------------------------ quantise

__global__ __launch_bounds__(QNT) void k_f0_quantize(const float *__restrict__ wav, const int32_t *__restrict__ lengths, int Lmax,
                                                    int16_t *__restrict__ pcm, float *__restrict__ peak_out,
                                                    int32_t *__restrict__ status) {
    __shared__ float red[QNT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = lengths[b];
    const bool ok_len = L >= 0 && L <= Lmax;
    const float *row = wav + (size_t)b * Lmax;
    int16_t *out = pcm + (size_t)b * Lmax;
    float peak = 0.f;
    int bad = 0;
    if (ok_len)
#pragma unroll 4
        for (int i = tid; i < L; i += QNT) {
            const float a = fabsf(row[i]);
            bad |= !(a <= 3.402823466e+38f);              // NaN or Inf
            peak = fmaxf(peak, a);
        }
    red[tid] = peak;
    const int any_bad = __syncthreads_or(bad);
    for (int h = QNT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = fmaxf(red[tid], red[tid + h]);
        __syncthreads();
    }
    peak = red[0];
    const bool ok = ok_len && !any_bad;
    if (tid == 0) {
        status[b] = ok ? B2S_F0_OK : B2S_F0_FAILED;
        if (peak_out) peak_out[b] = ok ? peak : 0.f;
    }
    const double div = fmax(0.01, (double)peak);
#pragma unroll 4
    for (int i = tid; i < Lmax; i += QNT) {
        int16_t v = 0;
        if (ok && i < L) {
            const double scaled = (double)row[i] / div;
            v = (int16_t)rint(fmin(fmax(scaled, -1.0), 1.0) * 32767.0);
        }
        out[i] = v;
    }
}

// ----------------------------------------------------------------------------------------------------------------------- YIN

struct YinArgs {
    const int16_t *pcm;
    const int32_t *lengths, *frame_off;
    int total_frames, Lmax, tiles, win, hop, tau_min, tau_max, NP;
    double threshold, sr;
    long long min_energy;
    double *f0_out;
    int32_t *tau_out;
    double *aper_out, *cmnd_out;
    int32_t *status;
};

__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// LDS per wave: NP doubles.  NP >= win + 65 R covers every window read (j + R lane + k <= win - 1 + 63 R + 2 R - 2) and the energy
// update (tau + win <= win + 64 R - 1); elements from win + tau_max on are zero.
template <int R>
__global__ __launch_bounds__(256) void k_f0_yin(YinArgs a) {
    extern __shared__ __align__(16) double smem[];
    const int wpb = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int L = a.lengths[b];
    const int o0 = a.frame_off[b], o1 = a.frame_off[b + 1];
    const bool ok = L >= 0 && L <= a.Lmax && o0 >= 0 && o1 >= o0 && o1 <= a.total_frames && o1 - o0 == 1 + L / a.hop;
    if (tile == 0 && threadIdx.x == 0) a.status[b] = ok ? B2S_F0_OK : B2S_F0_FAILED;
    if (!ok) return;                                     // the whole block: nothing of this utterance is read
    const int F = o1 - o0;
    if (tile * wpb >= F) return;                         // the whole block
    const int t = tile * wpb + wave;
    const bool active = t < F;                           // an idle wave of the last tile works on zeros and stores nothing
    const int win = a.win, tau_max = a.tau_max, N = win + tau_max;
    double *seg = smem + (size_t)wave * a.NP;
    {
        const int16_t *row = a.pcm + (size_t)b * a.Lmax;
        const long long first = (long long)t * a.hop - N / 2;
        for (int i = lane; i < a.NP; i += 64) {
            const long long s = first + i;
            seg[i] = (active && i < N && s >= 0 && s < L) ? (double)row[s] : 0.0;
        }
    }
    __syncthreads();

    // r[k] = sum_{j < win} seg[j] * seg[j + R lane + k], e = sum_{j < win} seg[j + R lane]^2
    const int base = R * lane;
    const double *sb = seg + base;
    double r[R], w[2 * R - 1], e = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) r[k] = 0.0;
#pragma unroll
    for (int i = 0; i < R - 1; ++i) w[i] = sb[i];
    const int full = win / R * R;
    for (int j0 = 0; j0 < full; j0 += R) {
#pragma unroll
        for (int i = 0; i < R; ++i) w[R - 1 + i] = sb[j0 + R - 1 + i];
#pragma unroll
        for (int jj = 0; jj < R; ++jj) {
            const double x = seg[j0 + jj];
            e = fma(w[jj], w[jj], e);
#pragma unroll
            for (int k = 0; k < R; ++k) r[k] = fma(x, w[jj + k], r[k]);
        }
#pragma unroll
        for (int i = 0; i < R - 1; ++i) w[i] = w[i + R];
    }
    for (int j = full; j < win; ++j) {
        const double x = seg[j];
        e = fma(sb[j], sb[j], e);
#pragma unroll
        for (int k = 0; k < R; ++k) r[k] = fma(x, sb[j + k], r[k]);
    }

    // d of this lane's lags (0 past tau_max), its running sum, c
    const double e0 = __shfl(e, 0);
    double d[R], s[R], c[R], run = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        d[k] = base + k <= tau_max ? (e0 + e) - 2.0 * r[k] : 0.0;
        run = run + d[k];
        s[k] = run;
        const double out = sb[k], in = sb[k + win];
        e = (e - out * out) + in * in;                   // E(tau + 1) from E(tau)
    }
    double incl = run;
    for (int o = 1; o < 64; o <<= 1) {
        const double v = __shfl_up(incl, o);
        if (lane >= o) incl = incl + v;
    }
    const double excl = incl - run;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int tau = base + k;
        const double S = excl + s[k];
        c[k] = (tau == 0 || S == 0.0) ? 1.0 : (d[k] * (double)tau) / S;
    }
    __syncthreads();                                     // every read of seg is done: its head becomes c[0..tau_max]
    double *cb = seg;
#pragma unroll
    for (int k = 0; k < R; ++k)
        if (base + k <= tau_max) cb[base + k] = c[k];
    __syncthreads();
    const size_t frame = (size_t)o0 + t;
    if (active && a.cmnd_out) {
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (base + k <= tau_max) a.cmnd_out[frame * (tau_max + 1) + base + k] = c[k];
    }

    // the pick
    double amin = __builtin_inf();
    int first = INT_MAX;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int tau = base + k;
        if (tau >= a.tau_min && tau <= tau_max) {
            amin = fmin(amin, c[k]);
            if (first == INT_MAX && c[k] < a.threshold) first = tau;
        }
    }
    amin = wave_min(amin);
    first = wave_min(first);
    int tau_pick = 0;
    double f0 = 0.0;
    if (first != INT_MAX && (long long)e0 >= a.min_energy) {
        int stop = INT_MAX;                              // first k >= `first` that is the last lag or has c[k + 1] >= c[k]
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int tau = base + k;
            if (stop == INT_MAX && tau >= first && tau <= tau_max && (tau + 1 > tau_max || !(cb[tau + 1] < c[k]))) stop = tau;
        }
        tau_pick = wave_min(stop);
        double shift = 0.0;
        if (tau_pick - 1 >= 1 && tau_pick + 1 <= tau_max) {
            const double p = cb[tau_pick - 1], q = cb[tau_pick], n = cb[tau_pick + 1];
            const double den = (p - q) + (n - q);
            if (den > 0.0) {
                const double sh = 0.5 * (p - n) / den;
                if (fabs(sh) <= 1.0) shift = sh;
            }
        }
        f0 = a.sr / ((double)tau_pick + shift);
    }
    if (active && lane == 0) {
        a.f0_out[frame] = f0;
        a.tau_out[frame] = tau_pick;
        if (a.aper_out) a.aper_out[frame] = amin;
    }
}

// --------------------------------------------------------------------------------------------------------------------- score

struct ScoreArgs {
    const double *f0_x, *f0_y;
    const int32_t *tau_x, *tau_y, *fx_off, *fy_off, *kept_x, *kept_y, *kx_off, *ky_off, *path, *path_off, *path_len, *dtw_status;
    int total_fx, total_fy, total_kx, total_ky, total_path;
    double gross_ratio;
    double *scores;
    int32_t *counts, *status;
};

__device__ __forceinline__ bool range_ok(const int32_t *off, int b, int total, int &o, int &n) {
    const int o0 = off[b], o1 = off[b + 1];
    if (o0 < 0 || o1 < o0 || o1 > total) return false;
    o = o0, n = o1 - o0;
    return true;
}

__global__ __launch_bounds__(NT) void k_f0_score(ScoreArgs a) {
    __shared__ double red_hz[NT], red_ct[NT];
    __shared__ int red_n[3][NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double QNAN = __builtin_nan("");
    auto finish = [&](int status, int steps, int vuv, int both, int gross, double hz, double ct) {
        if (tid == 0) {
            a.status[b] = status;
            int32_t *cn = a.counts + (size_t)b * 4;
            cn[0] = steps, cn[1] = vuv, cn[2] = both, cn[3] = gross;
            double *sc = a.scores + (size_t)b * 5;
            const bool okay = status == B2S_F0_OK;
            sc[0] = okay && both > 0 ? sqrt(hz / (double)both) : QNAN;
            sc[1] = okay && both > 0 ? sqrt(ct / (double)both) : QNAN;
            sc[2] = okay ? (double)vuv / (double)steps : QNAN;
            sc[3] = okay && both > 0 ? (double)gross / (double)both : QNAN;
            sc[4] = okay ? (double)(vuv + gross) / (double)steps : QNAN;
        }
    };
    const int st = a.dtw_status[b], n = a.path_len[b];
    if (st == B2S_F0_EMPTY || (st == B2S_F0_OK && n == 0)) {
        finish(B2S_F0_EMPTY, 0, 0, 0, 0, 0.0, 0.0);
        return;
    }
    int fx0, Fx, fy0, Fy, kx0, nx, ky0, ny, p0, slot;
    if (st != B2S_F0_OK || !range_ok(a.fx_off, b, a.total_fx, fx0, Fx) || !range_ok(a.fy_off, b, a.total_fy, fy0, Fy) ||
        !range_ok(a.kx_off, b, a.total_kx, kx0, nx) || !range_ok(a.ky_off, b, a.total_ky, ky0, ny) ||
        !range_ok(a.path_off, b, a.total_path, p0, slot) || n < 0 || n > slot) {
        finish(B2S_F0_FAILED, 0, 0, 0, 0, 0.0, 0.0);
        return;
    }
    double hz = 0.0, ct = 0.0;
    int vuv = 0, both = 0, gross = 0, outside = 0;
    for (int q = tid; q < n; q += NT) {
        const int i = a.path[2 * ((size_t)p0 + q)], j = a.path[2 * ((size_t)p0 + q) + 1];
        if ((unsigned)i >= (unsigned)nx || (unsigned)j >= (unsigned)ny) {
            outside = 1;
            continue;
        }
        const int fi = a.kept_x[kx0 + i], fj = a.kept_y[ky0 + j];
        if ((unsigned)fi >= (unsigned)Fx || (unsigned)fj >= (unsigned)Fy) {
            outside = 1;
            continue;
        }
        const bool vx = a.tau_x[fx0 + fi] > 0, vy = a.tau_y[fy0 + fj] > 0;
        if (vx != vy) ++vuv;
        if (vx && vy) {
            const double x = a.f0_x[fx0 + fi], y = a.f0_y[fy0 + fj];
            const double e = x - y, cents = 1200.0 * log2(x / y);
            ++both;
            if (fabs(e) > a.gross_ratio * y) ++gross;
            hz = hz + e * e;
            ct = ct + cents * cents;
        }
    }
    red_hz[tid] = hz, red_ct[tid] = ct;
    red_n[0][tid] = vuv, red_n[1][tid] = both, red_n[2][tid] = gross;
    const int any_outside = __syncthreads_or(outside);
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red_hz[tid] = red_hz[tid] + red_hz[tid + h];
            red_ct[tid] = red_ct[tid] + red_ct[tid + h];
            for (int m = 0; m < 3; ++m) red_n[m][tid] += red_n[m][tid + h];
        }
        __syncthreads();
    }
    if (any_outside) finish(B2S_F0_FAILED, 0, 0, 0, 0, 0.0, 0.0);
    else finish(B2S_F0_OK, n, red_n[0][0], red_n[1][0], red_n[2][0], red_hz[0], red_ct[0]);
}

}  // namespace

extern "C" {

int b2s_f0_version(void) { return 100; }

const char *b2s_f0_last_error(void) { return b2s_side::last_error(); }

int b2s_f0_quantize(const float *wav, const int32_t *lengths, int B, int Lmax, int16_t *pcm, float *peak_out, int32_t *status,
                    void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (Lmax < 0) return fail("quantize: Lmax must be >= 0 (got %d)", Lmax);
    if (!lengths || !status) return fail("quantize: lengths or status is NULL");
    if (Lmax > 0 && (!wav || !pcm)) return fail("quantize: wav or pcm is NULL with samples to read");
    hipLaunchKernelGGL(k_f0_quantize, dim3(B), dim3(QNT), 0, (hipStream_t)stream, wav, lengths, Lmax, pcm, peak_out, status);
    return b2s_side::launch_status("quantize");
}

int b2s_f0_yin(const int16_t *pcm, const int32_t *lengths, const int32_t *frame_offsets, int total_frames, int B, int Lmax, int win,
               int hop, int tau_min, int tau_max, double threshold, int64_t min_energy, double sr, double *f0_out, int32_t *tau_out,
               double *aper_out, double *cmnd_out, int32_t *status, void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (Lmax < 0) return fail("yin: Lmax must be >= 0 (got %d)", Lmax);
    if (total_frames < 0) return fail("yin: total_frames must be >= 0 (got %d)", total_frames);
    if (win < 2 || win > B2S_F0_MAX_WIN) return fail("yin: win must be in 2..%d (got %d)", B2S_F0_MAX_WIN, win);
    if (hop < 1) return fail("yin: hop must be >= 1 (got %d)", hop);
    if (tau_min < 2 || tau_min >= tau_max || tau_max > B2S_F0_MAX_TAU)
        return fail("yin: need 2 <= tau_min < tau_max <= %d (got %d and %d)", B2S_F0_MAX_TAU, tau_min, tau_max);
    if (!(threshold > 0.0)) return fail("yin: threshold must be > 0 (got %g)", threshold);
    if (min_energy < 0) return fail("yin: min_energy must be >= 0 (got %lld)", (long long)min_energy);
    if (!(sr > 0.0)) return fail("yin: sr must be > 0 (got %g)", sr);
    if (!lengths || !frame_offsets || !status) return fail("yin: lengths, frame_offsets or status is NULL");
    if (Lmax > 0 && !pcm) return fail("yin: pcm is NULL with samples to read");
    if (total_frames > 0 && (!f0_out || !tau_out)) return fail("yin: f0_out or tau_out is NULL with frames to write");
    const int R = tau_max + 1 <= 64 * 5 ? 5 : 9;
    const int NP = win + 65 * R;                                   // >= win + tau_max + 1: tau_max < 64 R
    int wpb = YIN_LDS / (NP * (int)sizeof(double));
    wpb = wpb > 4 ? 4 : wpb;                                       // NP <= 2633 doubles: at least 3 waves
    const long long tiles = ((long long)Lmax / hop + 1 + wpb - 1) / wpb;
    if (tiles * B > INT_MAX) return fail("yin: %d utterances of up to %lld frames exceed one launch; split the batch", B, tiles * wpb);
    YinArgs a;
    a.pcm = pcm, a.lengths = lengths, a.frame_off = frame_offsets;
    a.total_frames = total_frames, a.Lmax = Lmax, a.tiles = (int)tiles, a.win = win, a.hop = hop, a.tau_min = tau_min;
    a.tau_max = tau_max, a.NP = NP, a.threshold = threshold, a.sr = sr, a.min_energy = (long long)min_energy;
    a.f0_out = f0_out, a.tau_out = tau_out, a.aper_out = aper_out, a.cmnd_out = cmnd_out, a.status = status;
    const dim3 grid((unsigned)(tiles * B)), block(64 * wpb);
    const size_t lds = (size_t)wpb * NP * sizeof(double);
    if (R == 5) hipLaunchKernelGGL(k_f0_yin<5>, grid, block, lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_f0_yin<9>, grid, block, lds, (hipStream_t)stream, a);
    return b2s_side::launch_status("yin");
}

int b2s_f0_score(const double *f0_x, const int32_t *tau_x, const int32_t *fx_offsets, int total_fx, const double *f0_y,
                 const int32_t *tau_y, const int32_t *fy_offsets, int total_fy, const int32_t *kept_x, const int32_t *kx_offsets,
                 int total_kx, const int32_t *kept_y, const int32_t *ky_offsets, int total_ky, int B, const int32_t *path,
                 const int32_t *path_offsets, int total_path, const int32_t *path_len, const int32_t *dtw_status, double gross_ratio,
                 double *scores, int32_t *counts, int32_t *status, void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (total_fx < 0 || total_fy < 0 || total_kx < 0 || total_ky < 0 || total_path < 0)
        return fail("score: totals must be >= 0 (got %d, %d, %d, %d and %d)", total_fx, total_fy, total_kx, total_ky, total_path);
    if (!(gross_ratio >= 0.0)) return fail("score: gross_ratio must be >= 0 (got %g)", gross_ratio);
    if (!fx_offsets || !fy_offsets || !kx_offsets || !ky_offsets || !path_offsets || !path_len || !dtw_status)
        return fail("score: fx_offsets, fy_offsets, kx_offsets, ky_offsets, path_offsets, path_len or dtw_status is NULL");
    if ((total_fx > 0 && (!f0_x || !tau_x)) || (total_fy > 0 && (!f0_y || !tau_y))) return fail("score: an F0 or tau buffer is NULL");
    if ((total_kx > 0 && !kept_x) || (total_ky > 0 && !kept_y) || (total_path > 0 && !path))
        return fail("score: kept_x, kept_y or path is NULL");
    if (!scores || !counts || !status) return fail("score: scores, counts or status is NULL");
    ScoreArgs a;
    a.f0_x = f0_x, a.f0_y = f0_y, a.tau_x = tau_x, a.tau_y = tau_y, a.fx_off = fx_offsets, a.fy_off = fy_offsets;
    a.kept_x = kept_x, a.kept_y = kept_y, a.kx_off = kx_offsets, a.ky_off = ky_offsets, a.path = path, a.path_off = path_offsets;
    a.path_len = path_len, a.dtw_status = dtw_status, a.total_fx = total_fx, a.total_fy = total_fy, a.total_kx = total_kx;
    a.total_ky = total_ky, a.total_path = total_path, a.gross_ratio = gross_ratio, a.scores = scores, a.counts = counts;
    a.status = status;
    hipLaunchKernelGGL(k_f0_score, dim3(B), dim3(NT), 0, (hipStream_t)stream, a);
    return b2s_side::launch_status("score");
}

}  // extern "C"
