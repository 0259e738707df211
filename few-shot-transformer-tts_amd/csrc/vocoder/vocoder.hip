// Batched Griffin-Lim vocoder and mel front end for gfx950 (C ABI: include/b2s_vocoder.h), fp32 throughout.
//
// The 2048-point real FFT is a 1024-point complex Stockham radix-4 FFT in LDS (5 stages, one radix-4 butterfly per thread of a
// 256-thread block) plus the even/odd split pass; the inverse runs the same in reverse.  Twiddles and the window come from tables
// computed in double precision (k_voc_tables) and are staged in LDS once per block; blocks are persistent over frames.
//
// Griffin-Lim never stores the complex spectrum: one iteration of frame t needs only the window-covered samples
// y[tH - 400, tH + 400) of the previous pass's inverse STFT (reflected at the ends), and those come from the windowed 800-sample
// inverse-FFT segments of at most 8 neighbouring frames.  So each iteration is one launch that gathers y from the previous
// segments (divided by the window sum-square inline), windows it, runs rFFT -> phase projection onto S_t -> irFFT and writes the
// frame's new windowed segment.  A gather: no atomics, deterministic, and a frame's result does not depend on its batch.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include "../../../include/b2s_vocoder.h"
#include "../side_common.h"

using b2s_side::align_up;
using b2s_side::fail;
using b2s_side::launch_status;

namespace {

constexpr int NFFT = 2048, NC = 1024, NBIN = 1025, WIN = 800, HOP = 200, WOFF = 624, NMEL = 80;
constexpr int NTW = 1536;             // exp(-2 pi i k / 2048), k < 1536: every twiddle the radix-4 stages and the split pass use
constexpr int NT = 256;               // threads per block: one radix-4 butterfly each per stage
constexpr int HALF = WIN / 2;         // a frame covers y[t * HOP - HALF, t * HOP + HALF)
constexpr int MAX_LOOKBACK = 1024;    // de-emphasis look-back bound (samples)
constexpr int OLA_CHUNK = 32, OLA_SPAN = NT * OLA_CHUNK;
constexpr int MAG_FRAMES = 16;        // frames per block of k_voc_mag (one read of the inverse basis serves all of them)

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// i * a, or -i * a
__device__ __forceinline__ float2 mul_i(float2 a) { return make_float2(-a.y, a.x); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }

// NumPy 'reflect' index (no edge repeat), with the repeated reflection of a pad longer than the signal; n >= 2
__device__ __forceinline__ int reflect(int i, int n) {
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i >= n ? period - i : i;
}

// utterance of packed frame f: largest b with off[b] <= f
__device__ __forceinline__ int find_utt(const int32_t *__restrict__ off, int B, int f) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct Lds {
    float2 a[NC], b[NC];
    float2 tw[NTW];
    float win[WIN];
};

__device__ __forceinline__ void load_tables(Lds &s, const float2 *__restrict__ tw, const float *__restrict__ win) {
    for (int i = threadIdx.x; i < NTW; i += NT) s.tw[i] = tw[i];
    for (int i = threadIdx.x; i < WIN; i += NT) s.win[i] = win[i];
}

// 1024-point complex FFT, natural order in and out: input in s.a, result in s.b.  INV: exp(+2 pi i ...) and no scaling.
// The caller synchronises before; every stage ends with a barrier.
template <bool INV>
__device__ __forceinline__ void fft1024(Lds &s) {
    const int j = threadIdx.x;
    float2 *src = s.a, *dst = s.b;
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int ns = 1 << (2 * st);
        const int k = j & (ns - 1);
        const int step = 512 >> (2 * st);           // 2048 / (4 ns)
        float2 v0 = src[j], v1 = src[j + 256], v2 = src[j + 512], v3 = src[j + 768];
        if (st > 0) {
            float2 w1 = s.tw[k * step], w2 = s.tw[2 * k * step], w3 = s.tw[3 * k * step];
            if (INV) { w1 = cconj(w1); w2 = cconj(w2); w3 = cconj(w3); }
            v1 = cmul(v1, w1); v2 = cmul(v2, w2); v3 = cmul(v3, w3);
        }
        const float2 s02 = cadd(v0, v2), d02 = csub(v0, v2), s13 = cadd(v1, v3), d13 = csub(v1, v3);
        const float2 r = INV ? mul_i(d13) : mul_mi(d13);
        const int idx = ((j - k) << 2) + k;
        dst[idx] = cadd(s02, s13);
        dst[idx + ns] = cadd(d02, r);
        dst[idx + 2 * ns] = csub(s02, s13);
        dst[idx + 3 * ns] = csub(d02, r);
        __syncthreads();
        float2 *t = src; src = dst; dst = t;
    }
}

// rFFT bins k and 1024 - k (0 < k <= 512) from the complex FFT Z of z[n] = x[2n] + i x[2n+1]
__device__ __forceinline__ void split_fwd(const Lds &s, int k, float2 &xk, float2 &xk2) {
    const int k2 = NC - k;
    const float2 zk = s.b[k], zk2 = s.b[k2];
    const float2 e = make_float2(0.5f * (zk.x + zk2.x), 0.5f * (zk.y - zk2.y));          // (Z[k] + conj Z[k2]) / 2
    const float2 o = mul_mi(make_float2(0.5f * (zk.x - zk2.x), 0.5f * (zk.y + zk2.y)));  // -i (Z[k] - conj Z[k2]) / 2
    xk = cadd(e, cmul(s.tw[k], o));
    xk2 = cadd(cconj(e), cmul(s.tw[k2], cconj(o)));
}

// complex input Z'[k] of the inverse FFT from rFFT bins yk = X[k], yk2 = X[1024 - k]; x = (1 / 2048) * interleave(IFFT(Z'))
__device__ __forceinline__ float2 split_inv(const Lds &s, int k, float2 yk, float2 yk2) {
    const float2 c = cconj(yk2);
    return cadd(cadd(yk, c), mul_i(cmul(cconj(s.tw[k]), csub(yk, c))));
}

__device__ __forceinline__ float2 project(float mag, float2 x) {
    const float d = fmaxf(1e-8f, sqrtf(x.x * x.x + x.y * x.y));
    return make_float2(mag * x.x / d, mag * x.y / d);
}

// y[m] of the inverse STFT (0 <= m < L) from the utterance's windowed segments, divided by the window sum-square
__device__ __forceinline__ float ola_sample(const float *__restrict__ seg, const float *win, int m, int T) {
    const int lo = m < HALF ? 0 : (m - HALF) / HOP + 1;
    const int hi = min(T - 1, (m + HALF) / HOP);
    float acc = 0.f, wss = 0.f;
    for (int u = lo; u <= hi; ++u) {
        const int jp = m - HOP * u + HALF;
        const float w = win[jp];
        acc += seg[(size_t)u * WIN + jp];
        wss += w * w;
    }
    return wss > FLT_MIN ? acc / wss : acc;
}

__global__ void k_voc_tables(float2 *__restrict__ tw, float *__restrict__ win) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < NTW) {
        double sn, cs;
        sincospi((double)i / 1024.0, &sn, &cs);
        tw[i] = make_float2((float)cs, (float)-sn);
    }
    if (i < WIN) win[i] = (float)(0.5 - 0.5 * cospi((double)i / 400.0));
}

// S[f, k] = max(1e-10, sum_m invT[m, k] * amp[f, m]) ^ power, amp = 10 ^ (denormalised dB / 20); MAG_FRAMES frames per block
__global__ __launch_bounds__(NT) void k_voc_mag(const float *__restrict__ mels, const int32_t *__restrict__ off, int B, int Tmax, int F,
                                                const float *__restrict__ invT, float *__restrict__ S, float max_abs, int symmetric,
                                                float max_db, float ref_db, float power) {
    __shared__ float amp[MAG_FRAMES][NMEL];
    const int f0 = blockIdx.x * MAG_FRAMES;
    for (int i = threadIdx.x; i < MAG_FRAMES * NMEL; i += NT) {
        const int fi = i / NMEL, m = i % NMEL, f = f0 + fi;
        float a = 0.f;
        if (f < F) {
            const int b = find_utt(off, B, f), t = f - off[b];
            float v = mels[((size_t)b * Tmax + t) * NMEL + m];
            v = symmetric ? (v + max_abs) / (2.f * max_abs) : v / max_abs;
            v = fminf(fmaxf(v, 0.f), 1.f) * max_db - max_db + ref_db;
            a = powf(10.f, v * 0.05f);
        }
        amp[fi][m] = a;
    }
    __syncthreads();
    const int nf = min(MAG_FRAMES, F - f0);
    for (int k = threadIdx.x; k < NBIN; k += NT) {
        float acc[MAG_FRAMES];
#pragma unroll
        for (int i = 0; i < MAG_FRAMES; ++i) acc[i] = 0.f;
        for (int m = 0; m < NMEL; ++m) {
            const float w = invT[m * NBIN + k];
#pragma unroll
            for (int i = 0; i < MAG_FRAMES; ++i) acc[i] = fmaf(w, amp[i][m], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < MAG_FRAMES; ++i)
            if (i < nf) S[(size_t)(f0 + i) * NBIN + k] = powf(fmaxf(1e-10f, acc[i]), power);
    }
}

// one Griffin-Lim pass.  FIRST: segment = window * irfft(S_t).  Otherwise: gather y from seg_in, window, rFFT, project the phase
// onto S_t, irFFT, window -> seg_out.
template <bool FIRST>
__device__ __forceinline__ void gl_body(const float *__restrict__ S, const float *__restrict__ seg_in, float *__restrict__ seg_out,
                                        const int32_t *__restrict__ off, int B, int F, const float2 *__restrict__ tw_g,
                                        const float *__restrict__ win_g) {
    __shared__ Lds s;
    const int tid = threadIdx.x;
    load_tables(s, tw_g, win_g);
    __syncthreads();
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        const int b = find_utt(off, B, f), t = f - off[b], T = off[b + 1] - off[b];
        const float *Sf = S + (size_t)f * NBIN;
        if (FIRST) {
            for (int k = tid; k <= NC / 2; k += NT) {
                const float2 yk = make_float2(Sf[k], 0.f), yk2 = make_float2(Sf[NC - k], 0.f);
                s.a[k] = split_inv(s, k, yk, yk2);
                if (k > 0 && k < NC / 2) s.a[NC - k] = split_inv(s, NC - k, yk2, yk);
            }
        } else {
            const int L = HOP * (T - 1);
            const float *seg = seg_in + (size_t)off[b] * WIN;
            float *xa = reinterpret_cast<float *>(s.a);
            for (int i = tid; i < NC; i += NT)
                if (i < WOFF / 2 || i >= (WOFF + WIN) / 2) s.a[i] = make_float2(0.f, 0.f);
            for (int jj = tid; jj < WIN; jj += NT)
                xa[WOFF + jj] = s.win[jj] * ola_sample(seg, s.win, reflect(HOP * t - HALF + jj, L), T);
            __syncthreads();
            fft1024<false>(s);
            for (int k = tid; k <= NC / 2; k += NT) {
                float2 xk, xk2, yk, yk2;
                if (k == 0) {
                    const float2 z0 = s.b[0];
                    xk = make_float2(z0.x + z0.y, 0.f);
                    xk2 = make_float2(z0.x - z0.y, 0.f);
                } else {
                    split_fwd(s, k, xk, xk2);
                }
                yk = project(Sf[k], xk);
                yk2 = project(Sf[NC - k], xk2);
                if (k == 0) { yk.y = 0.f; yk2.y = 0.f; }        // irfft ignores the imaginary parts of DC and Nyquist
                s.a[k] = split_inv(s, k, yk, yk2);
                if (k > 0 && k < NC / 2) s.a[NC - k] = split_inv(s, NC - k, yk2, yk);
            }
        }
        __syncthreads();
        fft1024<true>(s);
        const float *xb = reinterpret_cast<const float *>(s.b);
        float *out = seg_out + (size_t)f * WIN;
        for (int jj = tid; jj < WIN; jj += NT) out[jj] = s.win[jj] * (xb[WOFF + jj] * (1.f / NFFT));
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void k_voc_gl_first(const float *__restrict__ S, float *__restrict__ seg_out, const int32_t *__restrict__ off,
                                                     int B, int F, const float2 *__restrict__ tw, const float *__restrict__ win) {
    gl_body<true>(S, nullptr, seg_out, off, B, F, tw, win);
}

__global__ __launch_bounds__(NT) void k_voc_gl_iter(const float *__restrict__ S, const float *__restrict__ seg_in, float *__restrict__ seg_out,
                                                    const int32_t *__restrict__ off, int B, int F, const float2 *__restrict__ tw,
                                                    const float *__restrict__ win) {
    gl_body<false>(S, seg_in, seg_out, off, B, F, tw, win);
}

// final overlap-add + window sum-square division + de-emphasis w[n] = y[n] + a w[n-1] (zero initial state) into the padded
// [B, Lmax] output.  Block = OLA_SPAN outputs of one utterance; y of the span and of MAX_LOOKBACK samples before it is staged in
// LDS (one pad float per 32 so the per-thread sequential reads are conflict-free); each thread runs the recurrence over its
// OLA_CHUNK outputs starting from zero state `lookback` samples earlier (a^lookback < 2^-30).
__global__ __launch_bounds__(NT) void k_voc_ola_deemph(const float *__restrict__ seg_all, const int32_t *__restrict__ off, int Lmax,
                                                       const float *__restrict__ win_g, float a, int lookback, float *__restrict__ wav) {
    constexpr int NY = MAX_LOOKBACK + OLA_SPAN;
    __shared__ float y[NY + NY / 32];
    __shared__ float win[WIN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int T = off[b + 1] - off[b], L = HOP * (T - 1);
    const int n0 = blockIdx.x * OLA_SPAN;
    for (int i = tid; i < WIN; i += NT) win[i] = win_g[i];
    __syncthreads();
    const float *seg = seg_all + (size_t)off[b] * WIN;
    for (int p = tid; p < NY; p += NT) {
        const int n = n0 - MAX_LOOKBACK + p;
        y[p + p / 32] = (n >= 0 && n < L) ? ola_sample(seg, win, n, T) : 0.f;
    }
    __syncthreads();
    const int q0 = MAX_LOOKBACK + tid * OLA_CHUNK;
    float w = 0.f;
    for (int p = q0 - lookback; p < q0; ++p) w = fmaf(a, w, y[p + p / 32]);
    float *out = wav + (size_t)b * Lmax;
    for (int i = 0; i < OLA_CHUNK; ++i) {
        const int p = q0 + i, n = n0 + tid * OLA_CHUNK + i;
        w = fmaf(a, w, y[p + p / 32]);
        if (n < Lmax) out[n] = n < L ? w : 0.f;
    }
}

// [lo, hi) of the nonzero bins of every mel filter (the projection skips the zeros)
__global__ void k_voc_mel_bands(const float *__restrict__ basis, int2 *__restrict__ bands) {
    const int m = threadIdx.x;
    if (m >= NMEL) return;
    int lo = NBIN, hi = 0;
    for (int k = 0; k < NBIN; ++k)
        if (basis[m * NBIN + k] != 0.f) { lo = min(lo, k); hi = k + 1; }
    bands[m] = lo < hi ? make_int2(lo, hi) : make_int2(0, 0);
}

// wav -> normalised mel: preemphasis on the fly, reflect-padded framing, window, rFFT, magnitude, mel projection, dB, normalisation
__global__ __launch_bounds__(NT) void k_voc_wav2mel(const float *__restrict__ wav, const int32_t *__restrict__ lens, const int32_t *__restrict__ off,
                                                    int B, int Lmax, int Tout, int F, const float *__restrict__ basis,
                                                    const int2 *__restrict__ bands, const float2 *__restrict__ tw_g, const float *__restrict__ win_g,
                                                    float coef, float ref_db, float max_db, float max_abs, int symmetric, float *__restrict__ mels) {
    __shared__ Lds s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    load_tables(s, tw_g, win_g);
    __syncthreads();
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        const int b = find_utt(off, B, f), t = f - off[b], len = lens[b];
        const float *x = wav + (size_t)b * Lmax;
        float *xa = reinterpret_cast<float *>(s.a);
        for (int i = tid; i < NC; i += NT)
            if (i < WOFF / 2 || i >= (WOFF + WIN) / 2) s.a[i] = make_float2(0.f, 0.f);
        for (int jj = tid; jj < WIN; jj += NT) {
            const int m = reflect(HOP * t - HALF + jj, len);
            const float p = m > 0 ? x[m] - coef * x[m - 1] : x[0];
            xa[WOFF + jj] = s.win[jj] * p;
        }
        __syncthreads();
        fft1024<false>(s);
        float *mag = reinterpret_cast<float *>(s.a);      // s.a is free after the forward FFT
        for (int k = tid; k <= NC / 2; k += NT) {
            float2 xk, xk2;
            if (k == 0) {
                const float2 z0 = s.b[0];
                xk = make_float2(z0.x + z0.y, 0.f);
                xk2 = make_float2(z0.x - z0.y, 0.f);
            } else {
                split_fwd(s, k, xk, xk2);
            }
            mag[k] = sqrtf(xk.x * xk.x + xk.y * xk.y);
            mag[NC - k] = sqrtf(xk2.x * xk2.x + xk2.y * xk2.y);
        }
        __syncthreads();
        for (int m = wv; m < NMEL; m += NT / 64) {
            const int2 bd = bands[m];
            float acc = 0.f;
            for (int k = bd.x + lane; k < bd.y; k += 64) acc = fmaf(basis[m * NBIN + k], mag[k], acc);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (lane == 0) {
                float v = 20.f * log10f(fmaxf(1e-5f, acc));
                v = fminf(fmaxf((v - ref_db + max_db) / max_db, 1e-8f), 1.f);
                v = symmetric ? v * max_abs * 2.f - max_abs : v * max_abs;
                mels[((size_t)b * Tout + t) * NMEL + m] = v;
            }
        }
        __syncthreads();
    }
}

struct WsLayout {
    size_t tw, win, bands, S, seg0, seg1, total;
};

WsLayout layout(int which, int F) {
    WsLayout l{};
    size_t o = 0;
    l.tw = o; o += align_up(sizeof(float2) * NTW);
    l.win = o; o += align_up(sizeof(float) * WIN);
    if (which == B2S_VOC_WS_MEL2WAV) {
        l.S = o; o += align_up(sizeof(float) * (size_t)F * NBIN);
        l.seg0 = o; o += align_up(sizeof(float) * (size_t)F * WIN);
        l.seg1 = o; o += align_up(sizeof(float) * (size_t)F * WIN);
    } else {
        l.bands = o; o += align_up(sizeof(int2) * NMEL);
    }
    l.total = o;
    return l;
}

int check_params(const B2SVocParams *p) {
    if (!p) return fail("params is NULL");
    if (p->n_fft != NFFT || p->win != WIN || p->hop != HOP || p->n_mels != NMEL)
        return fail("unsupported signal parameters n_fft=%d win_length=%d hop_length=%d num_mels=%d: the vocoder is compiled for "
                    "n_fft=2048, win_length=800, hop_length=200, num_mels=80 only", p->n_fft, p->win, p->hop, p->n_mels);
    if (!(p->max_abs_value > 0.f) || !(p->max_db > 0.f)) return fail("max_abs_value and max_db must be > 0");
    if (!(p->power > 0.f)) return fail("power must be > 0 (got %g)", p->power);
    if (!(p->preemphasis >= 0.f && p->preemphasis < 1.f)) return fail("preemphasis must be in [0, 1) (got %g)", p->preemphasis);
    return 0;
}

// de-emphasis look-back with a^lookback < 2^-30; -1 if it exceeds MAX_LOOKBACK
int deemph_lookback(float a) {
    if (a == 0.f) return 0;
    const int k = (int)std::ceil(30.0 * std::log(2.0) / -std::log((double)a));
    return k > MAX_LOOKBACK ? -1 : k;
}

int check_counts(int B, int frames_per_utt_max, int total_frames, int min_frames, const char *what) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (frames_per_utt_max < min_frames) return fail("%s gives %d frames per utterance at most; at least %d needed", what, frames_per_utt_max, min_frames);
    if (total_frames < (long long)min_frames * B || total_frames > (long long)frames_per_utt_max * B)
        return fail("total_frames %d does not match B=%d utterances of %d..%d frames", total_frames, B, min_frames, frames_per_utt_max);
    return 0;
}

int gl_grid(int F) { return F < 256 * 5 ? F : 256 * 5; }      // persistent: 5 blocks of 256 threads per CU fit the LDS

}  // namespace

extern "C" {

int b2s_voc_version(void) { return 100; }

const char *b2s_voc_last_error(void) { return b2s_side::last_error(); }

size_t b2s_voc_ws_bytes(const B2SVocParams *p, int B, int total_frames, int max_frames, int which) {
    if (check_params(p)) return 0;
    if (which != B2S_VOC_WS_MEL2WAV && which != B2S_VOC_WS_WAV2MEL) { fail("unknown workspace kind %d", which); return 0; }
    if (check_counts(B, max_frames, total_frames, which == B2S_VOC_WS_MEL2WAV ? 2 : 1, "max_frames")) return 0;
    return layout(which, total_frames).total;
}

int b2s_voc_mel2wav(const B2SVocParams *p, const float *mels, const int32_t *frame_offsets, int B, int Tmax, int total_frames,
                    int n_iter, const float *inv_basis, float *wav_out, void *ws, size_t ws_bytes, void *stream) {
    if (check_params(p)) return 1;
    if (check_counts(B, Tmax, total_frames, 2, "Tmax")) return 1;
    if (n_iter < 0) return fail("n_iter must be >= 0 (got %d)", n_iter);
    const int lookback = deemph_lookback(p->preemphasis);
    if (lookback < 0) return fail("preemphasis %g needs a de-emphasis look-back above %d samples", p->preemphasis, MAX_LOOKBACK);
    if (!mels || !frame_offsets || !inv_basis || !wav_out || !ws) return fail("mel2wav: a pointer argument is NULL");
    const WsLayout l = layout(B2S_VOC_WS_MEL2WAV, total_frames);
    if (ws_bytes < l.total) return fail("mel2wav: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    float2 *tw = (float2 *)(w + l.tw);
    float *win = (float *)(w + l.win), *S = (float *)(w + l.S);
    float *seg[2] = {(float *)(w + l.seg0), (float *)(w + l.seg1)};
    const int F = total_frames, Lmax = HOP * (Tmax - 1);
    hipLaunchKernelGGL(k_voc_tables, dim3((NTW + NT - 1) / NT), dim3(NT), 0, st, tw, win);
    hipLaunchKernelGGL(k_voc_mag, dim3((F + MAG_FRAMES - 1) / MAG_FRAMES), dim3(NT), 0, st, mels, frame_offsets, B, Tmax, F, inv_basis, S,
                       p->max_abs_value, p->symmetric_mel, p->max_db, p->ref_db, p->power);
    hipLaunchKernelGGL(k_voc_gl_first, dim3(gl_grid(F)), dim3(NT), 0, st, S, seg[0], frame_offsets, B, F, tw, win);
    for (int i = 0; i < n_iter; ++i)
        hipLaunchKernelGGL(k_voc_gl_iter, dim3(gl_grid(F)), dim3(NT), 0, st, S, seg[i & 1], seg[(i + 1) & 1], frame_offsets, B, F, tw, win);
    hipLaunchKernelGGL(k_voc_ola_deemph, dim3((Lmax + OLA_SPAN - 1) / OLA_SPAN, B), dim3(NT), 0, st, seg[n_iter & 1], frame_offsets, Lmax,
                       win, p->preemphasis, lookback, wav_out);
    return launch_status("mel2wav");
}

int b2s_voc_wav2mel(const B2SVocParams *p, const float *wav, const int32_t *lengths, const int32_t *frame_offsets, int B, int Lmax,
                    int total_frames, const float *basis, float *mels_out, void *ws, size_t ws_bytes, void *stream) {
    if (check_params(p)) return 1;
    if (Lmax < 2) return fail("wav2mel: Lmax must be >= 2 samples (got %d)", Lmax);
    const int Tout = 1 + Lmax / HOP;
    if (check_counts(B, Tout, total_frames, 1, "Lmax")) return 1;
    if (!wav || !lengths || !frame_offsets || !basis || !mels_out || !ws) return fail("wav2mel: a pointer argument is NULL");
    const WsLayout l = layout(B2S_VOC_WS_WAV2MEL, total_frames);
    if (ws_bytes < l.total) return fail("wav2mel: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    float2 *tw = (float2 *)(w + l.tw);
    float *win = (float *)(w + l.win);
    int2 *bands = (int2 *)(w + l.bands);
    hipLaunchKernelGGL(k_voc_tables, dim3((NTW + NT - 1) / NT), dim3(NT), 0, st, tw, win);
    hipLaunchKernelGGL(k_voc_mel_bands, dim3(1), dim3(128), 0, st, basis, bands);
    hipLaunchKernelGGL(k_voc_wav2mel, dim3(gl_grid(total_frames)), dim3(NT), 0, st, wav, lengths, frame_offsets, B, Lmax, Tout, total_frames,
                       basis, bands, tw, win, p->preemphasis, p->ref_db, p->max_db, p->max_abs_value, p->symmetric_mel, mels_out);
    return launch_status("wav2mel");
}

}  // extern "C"
