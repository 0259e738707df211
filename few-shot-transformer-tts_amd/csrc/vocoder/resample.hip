// Batched down-mix and resampling to 16 kHz for gfx950 (C ABI: include/b2s_vocoder.h, the b2s_voc_resample* entry points): the
// arithmetic of librosa 0.6.0's load(path, sr=16000) -- np.mean over the channels, then resampy's 'kaiser_best' windowed-sinc
// interpolation (64 zero crossings, 512 table steps per crossing, linear interpolation between table entries) and fix_length -- on a
// ragged batch wav [B, Lmax_in, C] + lengths [B].  Everything is launched on the caller's stream; no stream or graph is created, nothing
// synchronises with the host and nothing is kept between calls: the filter table is rebuilt into the caller's workspace every time.
//
//   k_rs_table      win[k] = rolloff * sinc(rolloff * k / 512) * I0(beta * sqrt(1 - (k / 32768)^2)) / I0(beta), times ratio when
//                   down-sampling; computed in fp64 (I0 by its power series), stored as fp32.  Entry 32769 repeats entry 32768, so the
//                   difference that stands in for resampy's delta table is zero there, as its delta[32768] is.
//   k_rs_downmix    [B, Lmax_in, C] -> [B, Lmax_in], frames below lengths[b] only: a left-to-right fp32 sum over the channels and one
//                   fp32 division, which is what np.mean(y, axis=0) does.  Skipped for C = 1.
//   k_rs_resample   grid (output tiles, B).  A workgroup owns `tile` consecutive outputs of one utterance and stages, next to the whole
//                   table, the input span they touch: [n_first - W, n_last + W] clipped to [0, N), W = 32769 / index_step taps per wing
//                   at most, N = lengths[b] (the padding past it is never read).  Per output, once and in fp64 as resampy does:
//                   time = t * (1 / ratio), n = (int)time, frac = scale * (time - n), then per wing the table offset and the
//                   interpolation weight eta.  The tap loop is fp32: weight = win[o] + eta * (win[o + 1] - win[o]), acc += weight * x,
//                   left wing first, in resampy's order.  Outputs from n_valid[b] to Lmax_out are written as 0.0.
//                   The table sits in LDS (128 KiB of the 160): reading it through L2 instead, with two workgroups per CU, measured
//                   1.5 to 2.2 times slower on the three batches of bench_resample.py (profiles/r11_bench_resample.json has the kept
//                   variant's figures).  The table reads are dword reads at pseudo-random offsets, so they pay bank conflicts.
//   k_rs_copy       orig_sr == 16000: out = the (down-mixed) input, bit for bit, zero from n_valid[b] on.
//
// n_valid = int(N * ratio) and n_out = int(ceil(N * ratio)) are the caller's (Python floats there); they are never recomputed here.
// A row whose n_valid would make an output start at or past sample N writes 0.0 for it instead of reading out of the row.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../../include/b2s_vocoder.h"
#include "../side_common.h"

using b2s_side::fail;
using b2s_side::launch_status;

namespace {

constexpr int SR_OUT = 16000;
constexpr int NUM_ZEROS = 64, STEPS = 512;
constexpr int NWIN = NUM_ZEROS * STEPS + 1;          // 32769
constexpr int TABLE = NWIN + 1;                      // one repeated entry at the end
constexpr int TABLE_PAD = (TABLE + 63) / 64 * 64;    // floats the table takes in the workspace and in LDS
constexpr double ROLLOFF = 0.9475937167399596, BETA = 14.769656459379492;
constexpr int MAX_CHANNELS = 8, MIN_SR = 4000, MAX_SR = 192000;
constexpr int MAX_LEN = 1 << 28;                     // samples per row, in and out
constexpr int NT = 1024;                             // threads of a resampling workgroup
constexpr int NT_SMALL = 256;                        // threads of the table, down-mix and copy workgroups
constexpr int LDS_BYTES = 160 * 1024;
constexpr int MAX_TILE = 4096, MIN_TILE = 256;

// modified Bessel function of the first kind, order 0, by its power series sum ((x / 2)^2k / (k!)^2)
__host__ __device__ inline double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

struct Plan {
    double ratio, inc, scale;      // 16000 / orig_sr, 1 / ratio, min(1, ratio)
    int step, wing;                // int(scale * 512); taps per wing at most = 32769 / step
    int tile, span;                // outputs per workgroup; floats of LDS for the input span
    size_t lds;                    // dynamic LDS bytes of k_rs_resample
};

// The tile is the largest of 4096, 2048, 1024, 512, 256 outputs whose input span fits beside the table in 160 KiB of LDS.
Plan make_plan(int orig_sr) {
    Plan p;
    p.ratio = (double)SR_OUT / (double)orig_sr;
    p.inc = 1.0 / p.ratio;
    p.scale = p.ratio < 1.0 ? p.ratio : 1.0;
    p.step = (int)(p.scale * STEPS);
    p.wing = NWIN / p.step;
    const int room = LDS_BYTES / 4 - TABLE_PAD - 64;
    p.tile = MAX_TILE;
    for (;;) {
        p.span = ((int)std::ceil(p.tile * p.inc) + 2 * p.wing + 4 + 3) / 4 * 4;
        if (p.span <= room || p.tile == MIN_TILE) break;
        p.tile /= 2;
    }
    p.lds = sizeof(float) * ((size_t)p.span + TABLE_PAD);
    return p;
}

__global__ __launch_bounds__(NT_SMALL) void k_rs_table(float *__restrict__ win, double mult, double inv_i0_beta) {
    const int k = blockIdx.x * NT_SMALL + threadIdx.x;
    if (k >= TABLE_PAD) return;
    if (k >= TABLE) { win[k] = 0.0f; return; }                           // the padding the LDS copy carries along
    const int kk = k < NWIN ? k : NWIN - 1;
    const double u = (double)kk / (double)(NWIN - 1);
    const double taper = bessel_i0(BETA * sqrt(1.0 - u * u)) * inv_i0_beta;
    const double a = ROLLOFF * (double)kk / (double)STEPS;
    const double pa = M_PI * a;
    const double sinc = kk == 0 ? 1.0 : sin(pa) / pa;
    win[k] = (float)(ROLLOFF * sinc * taper * mult);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// frames past lengths[b] are neither read nor written: nothing downstream reads the mono row past its length
__global__ __launch_bounds__(NT_SMALL) void k_rs_downmix(const float *__restrict__ wav, const int32_t *__restrict__ lengths, int Lmax_in, int C,
                                                         float *__restrict__ mono) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * NT_SMALL + threadIdx.x;
    if (p >= clampi(lengths[b], 0, Lmax_in)) return;
    const size_t i = (size_t)b * Lmax_in + p;
    const float *x = wav + i * (size_t)C;
    float acc = x[0];
    for (int c = 1; c < C; ++c) acc = acc + x[c];
    mono[i] = acc / (float)C;
}
// (int)v for a non-negative v; a position past any row (only a caller's inconsistent n_valid gets there) saturates
__device__ __forceinline__ int to_index(double v) { return v < 2147483000.0 ? (int)v : 2147483647; }

__global__ __launch_bounds__(NT_SMALL) void k_rs_copy(const float *__restrict__ x, const int32_t *__restrict__ lengths,
                                                      const int32_t *__restrict__ n_valid, int Lmax_in, int Lmax_out, float *__restrict__ out) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * NT_SMALL + threadIdx.x;
    if (t >= Lmax_out) return;
    const int N = clampi(lengths[b], 0, Lmax_in);
    const int nv = clampi(n_valid[b], 0, N < Lmax_out ? N : Lmax_out);
    out[(size_t)b * Lmax_out + t] = t < nv ? x[(size_t)b * Lmax_in + t] : 0.0f;
}

// table offset and interpolation weight of one wing, as resampy computes them
__device__ __forceinline__ void wing_start(double frac, int &off, float &eta) {
#pragma clang fp contract(off)
    const double idx = frac * (double)STEPS;
    off = (int)idx;
    eta = (float)(idx - (double)off);
}

__global__ __launch_bounds__(NT) void k_rs_resample(const float *__restrict__ x, const int32_t *__restrict__ lengths,
                                                    const int32_t *__restrict__ n_valid, int Lmax_in, int Lmax_out,
                                                    const float *__restrict__ win, double inc, double scale, int step, int wing, int tile,
                                                    int span_cap, float *__restrict__ out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *xs = smem;                       // [span_cap]
    float *tab = smem + span_cap;           // [TABLE_PAD]
    const int b = blockIdx.y, tid = threadIdx.x;
    const int t0 = blockIdx.x * tile;
    const int t1 = t0 + tile < Lmax_out ? t0 + tile : Lmax_out;          // outputs [t0, t1) are this workgroup's
    float *orow = out + (size_t)b * Lmax_out;
    const int N = clampi(lengths[b], 0, Lmax_in);
    const int nv = clampi(n_valid[b], 0, Lmax_out);
    const int tv = nv < t1 ? nv : t1;                                    // outputs [t0, tv) are interpolated, [tv, t1) are zero
    if (tv <= t0 || N < 1) {
        for (int t = t0 + tid; t < t1; t += NT) orow[t] = 0.0f;
        return;
    }
    int n_first = to_index((double)t0 * inc), n_last = to_index((double)(tv - 1) * inc);
    n_first = clampi(n_first, 0, N - 1);
    n_last = clampi(n_last, n_first, N - 1);
    const int lo = n_first - wing > 0 ? n_first - wing : 0;
    int hi = n_last + wing + 1 < N ? n_last + wing + 1 : N;             // the span is [lo, hi)
    if (hi - lo > span_cap) hi = lo + span_cap;                          // cannot happen for a tile and span of make_plan
    const float *xrow = x + (size_t)b * Lmax_in;
    for (int i = tid; i < hi - lo; i += NT) xs[i] = xrow[lo + i];
    {
        const float4 *src = reinterpret_cast<const float4 *>(win);      // the workspace's table is 256-byte aligned, TABLE_PAD % 4 == 0
        float4 *dst = reinterpret_cast<float4 *>(tab);
        for (int i = tid; i < TABLE_PAD / 4; i += NT) dst[i] = src[i];
    }
    __syncthreads();
    for (int t = t0 + tid; t < t1; t += NT) {
        float acc = 0.0f;
        if (t < tv) {
            const double time = (double)t * inc;
            const int n = to_index(time);
            if (n >= lo && n < hi) {
                const double frac = scale * (time - (double)n);
                int off;
                float eta;
                wing_start(frac, off, eta);
                int cnt = (NWIN - off) / step;
                cnt = cnt < n - lo + 1 ? cnt : n - lo + 1;               // i < n + 1, and inside the span
                const float *xp = xs + (n - lo);
                const float *wp = tab + off;
#pragma unroll 4
                for (int i = 0; i < cnt; ++i) {
                    const float w0 = wp[i * step], w1 = wp[i * step + 1];
                    acc = fmaf(fmaf(eta, w1 - w0, w0), xp[-i], acc);
                }
                wing_start(scale - frac, off, eta);
                cnt = (NWIN - off) / step;
                cnt = cnt < hi - n - 1 ? cnt : hi - n - 1;               // k < N - n - 1, and inside the span
                xp = xs + (n - lo + 1);
                wp = tab + off;
#pragma unroll 4
                for (int k = 0; k < cnt; ++k) {
                    const float w0 = wp[k * step], w1 = wp[k * step + 1];
                    acc = fmaf(fmaf(eta, w1 - w0, w0), xp[k], acc);
                }
            }
        }
        orow[t] = acc;
    }
}

int check_shape(const char *what, int B, int Lmax_in, int channels, int orig_sr) {
    if (B <= 0) return fail("%s: B must be > 0 (got %d)", what, B);
    if (Lmax_in < 1) return fail("%s: Lmax_in must be >= 1 (got %d)", what, Lmax_in);
    if (Lmax_in > MAX_LEN) return fail("%s: Lmax_in = %d is too long (at most %d samples)", what, Lmax_in, MAX_LEN);
    if (B > 65535) return fail("%s: B = %d is too large (at most 65535)", what, B);
    if (channels < 1 || channels > MAX_CHANNELS) return fail("%s: channels must be in 1..%d (got %d)", what, MAX_CHANNELS, channels);
    if (orig_sr < MIN_SR || orig_sr > MAX_SR) return fail("%s: orig_sr must be in %d..%d Hz (got %d)", what, MIN_SR, MAX_SR, orig_sr);
    return 0;
}

struct Layout { size_t table, mono, total; };

Layout layout(int B, int Lmax_in, int channels) {
    Layout l;
    l.table = 0;
    l.mono = sizeof(float) * (size_t)TABLE_PAD;                          // a multiple of 256 bytes
    l.total = l.mono + (channels > 1 ? sizeof(float) * (size_t)B * Lmax_in : 0);
    return l;
}

}  // namespace

extern "C" {

size_t b2s_voc_resample_ws_bytes(int B, int Lmax_in, int channels, int orig_sr) {
    if (check_shape("resample_ws_bytes", B, Lmax_in, channels, orig_sr)) return 0;
    return layout(B, Lmax_in, channels).total;
}

int b2s_voc_resample(const float *wav, const int32_t *lengths, int B, int Lmax_in, int channels, int orig_sr, const int32_t *n_valid,
                     const int32_t *n_out, int Lmax_out, float *out, void *ws, size_t ws_bytes, void *stream) {
    if (check_shape("resample", B, Lmax_in, channels, orig_sr)) return 1;
    if (Lmax_out < 1) return fail("resample: Lmax_out must be >= 1 (got %d)", Lmax_out);
    if (Lmax_out > MAX_LEN) return fail("resample: Lmax_out = %d is too long (at most %d samples)", Lmax_out, MAX_LEN);
    if (!wav || !lengths || !n_valid || !n_out || !out || !ws) return fail("resample: a pointer argument is NULL");
    const Layout l = layout(B, Lmax_in, channels);
    if (ws_bytes < l.total) return fail("resample: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    if (((uintptr_t)ws & 15) != 0) return fail("resample: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    const float *mono = wav;
    if (channels > 1) {
        float *m = (float *)(w + l.mono);
        hipLaunchKernelGGL(k_rs_downmix, dim3((Lmax_in + NT_SMALL - 1) / NT_SMALL, B), dim3(NT_SMALL), 0, st, wav, lengths, Lmax_in, channels, m);
        mono = m;
    }
    if (orig_sr == SR_OUT) {
        hipLaunchKernelGGL(k_rs_copy, dim3((Lmax_out + NT_SMALL - 1) / NT_SMALL, B), dim3(NT_SMALL), 0, st, mono, lengths, n_valid, Lmax_in,
                           Lmax_out, out);
        return launch_status("resample");
    }
    const Plan p = make_plan(orig_sr);
    float *win = (float *)(w + l.table);
    hipLaunchKernelGGL(k_rs_table, dim3((TABLE_PAD + NT_SMALL - 1) / NT_SMALL), dim3(NT_SMALL), 0, st, win, p.ratio < 1.0 ? p.ratio : 1.0,
                       1.0 / bessel_i0(BETA));
    const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void *>(k_rs_resample), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    if (ae != hipSuccess) return fail("resample: %zu bytes of LDS refused: %s", p.lds, hipGetErrorString(ae));
    hipLaunchKernelGGL(k_rs_resample, dim3((Lmax_out + p.tile - 1) / p.tile, B), dim3(NT), p.lds, st, mono, lengths, n_valid, Lmax_in, Lmax_out,
                       win, p.inc, p.scale, p.step, p.wing, p.tile, p.span, out);
    return launch_status("resample");
}

}  // extern "C"
