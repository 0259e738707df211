// Prosody targets for gfx950: window energy, the Viterbi pitch track over YIN's CMND matrix, and sums per input unit (C ABI:
// include/b2s_pros.h, definition: DESIGN.md section n).
//
// k_pros_energy  one wave per frame: the lanes stride over the window (int16 loads that the overlapping windows of the next frames
//                find in the cache), squares and sums in 64 bits from the first add on, one shuffle tree per frame.
// k_pros_track<WC>  one workgroup per utterance, one lane per lag; Q[t-1] of the lags sits in LDS (two rows, ping-pong, with W_MAX
//                cells of +inf on either side, so the band needs no clamp: +inf never wins a strict compare against the finite
//                candidate from state 0).  Per frame: every lane walks its band in ascending order (WC = 8: unrolled, the penalties
//                in registers; WC = 0: any W, the penalties from LDS), state 0's minimum over all lags is a DPP minimum per wave
//                (value only; the first lane that holds it is found by a ballot, which is the tie rule) and one LDS slot per wave
//                that every lane combines in wave order.  One LDS-only barrier per frame; the CMND rows are asked for DEPTH frames
//                ahead into a register ring.  Back-pointers leave as one byte per lag (offset code 0..2W, 255 = from state 0) and
//                one int32 per frame for state 0.  Then one lane walks back, and all lanes refine the lags to F0.
// k_pros_units   one workgroup per utterance: a block scan of the durations, the nearest voiced frame after each frame by ballots
//                over chunks of 256 frames going backwards (to the workspace), the one before it going forwards, the contour, then
//                one thread per unit summing in frame order.
// Contraction is off for the whole file: mu * k, lam * d and the contour's product are rounded before they are added.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include "../../../include/b2s_pros.h"
#include "../side_common.h"

using b2s_side::fail;

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                                  // threads of the energy and units kernels
constexpr int MAX_LAGS = B2S_PROS_MAX_LAGS, MAX_W = B2S_PROS_MAX_W, MAX_WAVES = MAX_LAGS / 64;
constexpr int ROW = MAX_W + MAX_LAGS + MAX_W;            // one Q row in LDS with its two margins
constexpr int DEPTH = 4;                                 // frames of cmnd in flight per lane
constexpr int FROM_ZERO = 255;                           // back-pointer code: the predecessor is state 0
constexpr int MAX_S = B2S_PROS_MAX_S, PER_THREAD = MAX_S / NT;

// ------------------------------------------------------------------------------------------------------------------- energy

__global__ __launch_bounds__(NT) void k_pros_energy(const int16_t *__restrict__ pcm, const int32_t *__restrict__ lengths,
                                                   const int32_t *__restrict__ off, int total, int Lmax, int win, int hop,
                                                   long long *__restrict__ energy, int32_t *__restrict__ status) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int L = lengths[b];
    const long long o0 = off[b], o1 = off[b + 1];
    if (L < 0 || L > Lmax || o0 < 0 || o1 > total || o1 - o0 != 1 + L / hop) {
        if (blockIdx.x == 0 && threadIdx.x == 0) status[b] = B2S_PROS_FAILED;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) status[b] = B2S_PROS_OK;
    const int F = 1 + L / hop;
    const int16_t *p = pcm + (size_t)b * Lmax;
    for (long long t = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); t < F; t += (long long)gridDim.x * (NT / 64)) {
        const long long first = t * hop - win / 2;
        long long e = 0;
        for (int i = lane; i < win; i += 64) {
            const long long at = first + i;
            if (at >= 0 && at < L) {
                const long long s = p[at];
                e += s * s;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) e += __shfl_xor(e, d);
        if (lane == 0) energy[o0 + t] = e;
    }
}

// -------------------------------------------------------------------------------------------------------------------- track

struct TrackArgs {
    const double *cmnd;
    const long long *energy;
    long long floor;
    const int32_t *off;
    int total, K, tau_min, tau_max, nlag, W, RS;
    double sr, u, v, lam, mu;
    int32_t *tau;
    double *f0, *score;
    int32_t *status;
    unsigned char *bp;                                   // [total, RS]
    int32_t *bp0;                                        // [total]
};

template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double read_lane(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// The wave's smallest x as the first lane holds it: its value in *val (that lane's own bits) and the lane as the result.  The four
// DPP steps are permutations inside a row of 16 lanes (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror), so
// every lane has a source; the rows meet through four readlanes.  The minimum serves the compare alone: which lane wins is the
// ballot's lowest bit.  A NaN can leave the ballot empty; lane 0 then stands in (such an utterance is FAILED and never walked).
__device__ __forceinline__ int wave_first_min(double x, double *val) {
    double m = fmin(x, dpp<0xB1>(x));
    m = fmin(m, dpp<0x4E>(m));
    m = fmin(m, dpp<0x141>(m));
    m = fmin(m, dpp<0x140>(m));
    m = fmin(fmin(read_lane(m, 0), read_lane(m, 16)), fmin(read_lane(m, 32), read_lane(m, 48)));
    const unsigned long long bal = __ballot(x == m);
    const int lane = __builtin_amdgcn_readfirstlane(bal ? __ffsll((long long)bal) - 1 : 0);
    *val = read_lane(x, lane);
    return lane;
}

// orders LDS traffic only: a __syncthreads() would also wait for the cmnd loads in flight
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int WC>
__global__ __launch_bounds__(MAX_LAGS) void k_pros_track(TrackArgs a) {
    __shared__ double qrow[2][ROW];
    __shared__ double slot_val[2][MAX_WAVES];
    __shared__ int slot_lag[2][MAX_WAVES];
    __shared__ double pen_sh[MAX_W + 1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nthr >> 6;
    const double INF = __builtin_inf(), QNAN = __builtin_nan("");
    const long long o0 = a.off[b], o1 = a.off[b + 1];
    if (o0 < 0 || o1 < o0 || o1 > a.total) {                       // the whole workgroup, here and below
        if (tid == 0) a.status[b] = B2S_PROS_FAILED, a.score[b] = QNAN;
        return;
    }
    const int F = (int)(o1 - o0);
    if (F == 0) {
        if (tid == 0) a.status[b] = B2S_PROS_EMPTY, a.score[b] = 0.0;
        return;
    }
    const int W = WC ? WC : a.W;
    const bool active = tid < a.nlag;
    const int k = a.tau_min + min(tid, a.nlag - 1);                // a lane without a lag rereads the last one
    const double mupk = a.mu * (double)k;
    const double *col = a.cmnd + (size_t)o0 * a.K + k;
    const long long *en = a.energy + o0;
    unsigned char *bp = a.bp + (size_t)o0 * a.RS + tid;
    int32_t *bp0 = a.bp0 + o0;

    for (int i = tid; i < 2 * ROW; i += nthr) (&qrow[0][0])[i] = INF;
    for (int i = tid; i <= MAX_W; i += nthr) pen_sh[i] = a.lam * (double)i;
    for (int i = tid; i < 2 * MAX_WAVES; i += nthr) (&slot_val[0][0])[i] = INF, (&slot_lag[0][0])[i] = 0;
    double pen[WC + 1];
#pragma unroll
    for (int d = 0; d <= WC; ++d) pen[d] = a.lam * (double)d;

    // the ring: slot r holds frame t0 + r while the block of DEPTH frames from t0 is in work; a frame from F on is the last frame
    // again, so every address is a valid cell, and what comes back for it is never used
    double cm[DEPTH];
    long long ev[DEPTH];
#pragma unroll
    for (int r = 0; r < DEPTH; ++r) {
        const int tc = min(r, F - 1);
        cm[r] = col[(size_t)tc * a.K], ev[r] = en[tc];
    }
    __syncthreads();

    double q = INF, q0 = 0.0;                                      // Q[t-1] of this lane's lag and of state 0
    int bad = 0;
    for (int t0 = 0; t0 < F; t0 += DEPTH) {
#pragma unroll
        for (int r = 0; r < DEPTH; ++r) {
            const int t = t0 + r, p = t & 1;
            const double c = cm[r];
            const long long e = ev[r];
            const int tn = min(t + DEPTH, F - 1);
            cm[r] = col[(size_t)tn * a.K], ev[r] = en[tn];
            if (t < F) {                                           // the same for every lane of the workgroup
                bad |= active && !(fabs(c) <= DBL_MAX);
                const double loc = e < a.floor ? INF : c + mupk;
                if (t == 0) {
                    q = active ? loc : INF;
                    q0 = a.u;
                } else {
                    double best0 = q0, sv[MAX_WAVES];
                    int arg0 = 0, sl[MAX_WAVES];
#pragma unroll
                    for (int i = 0; i < MAX_WAVES; ++i) sv[i] = slot_val[p ^ 1][i], sl[i] = slot_lag[p ^ 1][i];   // all asked for at once
#pragma unroll
                    for (int i = 0; i < MAX_WAVES; ++i) {          // the slot of a wave that is not there holds +inf and never wins
                        const bool take = sv[i] < best0;
                        best0 = take ? sv[i] : best0, arg0 = take ? sl[i] : arg0;
                    }
                    const double *prev = &qrow[p ^ 1][MAX_W + tid - W];
                    double best = q0 + a.v;
                    int code = FROM_ZERO;
                    if (WC) {
#pragma unroll
                        for (int j = 0; j <= 2 * WC; ++j) {
                            const double cand = prev[j] + pen[j < WC ? WC - j : j - WC];
                            if (cand < best) best = cand, code = j;
                        }
                    } else {
                        for (int j = 0; j <= 2 * W; ++j) {
                            const double cand = prev[j] + pen_sh[j < W ? W - j : j - W];
                            if (cand < best) best = cand, code = j;
                        }
                    }
                    q = active ? loc + best : INF;
                    q0 = a.u + best0;
                    bp[(size_t)t * a.RS] = (unsigned char)code;
                    if (tid == 0) bp0[t] = arg0;
                }
                qrow[p][MAX_W + tid] = q;
                double sv;
                const int first = wave_first_min(q + a.v, &sv);
                if (lane == 0) slot_val[p][w] = sv, slot_lag[p][w] = a.tau_min + 64 * w + first;
            }
            lds_barrier();
        }
    }
    if (__syncthreads_or(bad)) {
        for (int i = tid; i < F; i += nthr) a.tau[o0 + i] = 0, a.f0[o0 + i] = 0.0;
        if (tid == 0) a.status[b] = B2S_PROS_FAILED, a.score[b] = QNAN;
        return;
    }

    // the end state: state 0 first, then the lags in ascending order, strict
    {
        double sv;
        const int first = wave_first_min(q, &sv);
        __syncthreads();                                           // everyone is past the last frame's slots
        if (lane == 0) slot_val[0][w] = sv, slot_lag[0][w] = a.tau_min + 64 * w + first;
        __threadfence_block();
        __syncthreads();                                           // and the back-pointers are where lane 0 will read them
    }
    if (tid == 0) {
        double best = q0;
        int s = 0;
        for (int i = 0; i < nw; ++i)
            if (slot_val[0][i] < best) best = slot_val[0][i], s = slot_lag[0][i];
        a.score[b] = best;
        a.status[b] = B2S_PROS_OK;
        for (int t = F - 1; t >= 0; --t) {
            a.tau[o0 + t] = s;
            if (t > 0) {
                if (s == 0) {
                    s = bp0[t];
                } else {
                    const int code = a.bp[((size_t)o0 + t) * a.RS + (s - a.tau_min)];
                    s = code == FROM_ZERO ? 0 : s + code - W;
                }
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int t = tid; t < F; t += nthr) {
        const int s = a.tau[o0 + t];
        double f0 = 0.0;
        if (s > 0) {
            const double *c = a.cmnd + ((size_t)o0 + t) * a.K;
            double shift = 0.0;
            if (s - 1 >= 1 && s + 1 <= a.tau_max) {
                const double p = c[s - 1], m = c[s], n = c[s + 1];
                const double den = (p - m) + (n - m);
                if (den > 0.0) {
                    const double sh = 0.5 * (p - n) / den;
                    if (fabs(sh) <= 1.0) shift = sh;
                }
            }
            f0 = a.sr / ((double)s + shift);
        }
        a.f0[o0 + t] = f0;
    }
}

// -------------------------------------------------------------------------------------------------------------------- units

struct UnitArgs {
    const double *f0;
    const int32_t *tau;
    const long long *energy;
    const int32_t *off;
    int total;
    const int32_t *dur, *in_len, *groups;
    int S;
    double *cont;
    int32_t *frames, *voiced;
    double *vsum, *csum;
    long long *esum;
    int32_t *units, *status;
    int32_t *next;                                       // [total] workspace: the first voiced frame at or after each frame
};

__global__ __launch_bounds__(NT) void k_pros_units(UnitArgs a) {
    __shared__ long long start[MAX_S + 1];               // frame where each position starts; start[n_in] = n
    __shared__ long long ustart[MAX_S + 1];              // the same per unit
    __shared__ long long part[NT];
    __shared__ int sg[MAX_S];
    __shared__ int wave_hit[NT / 64];
    __shared__ int carry_sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, S = a.S;
    const long long o0 = a.off[b], o1 = a.off[b + 1];
    if (o0 < 0 || o1 < o0 || o1 > a.total) {                       // the whole workgroup, here and below
        if (tid == 0) a.status[b] = B2S_PROS_FAILED, a.units[b] = 0;
        return;
    }
    const int F = (int)(o1 - o0);
    const size_t row = (size_t)b * S;
    auto zero_units = [&](int from) {
        for (int i = from + tid; i < S; i += NT) {
            a.frames[row + i] = 0, a.voiced[row + i] = 0, a.esum[row + i] = 0;
            a.vsum[row + i] = 0.0, a.csum[row + i] = 0.0;
        }
    };
    auto nothing = [&](int st) {
        zero_units(0);
        for (int i = tid; i < F; i += NT) a.cont[o0 + i] = 0.0;
        if (tid == 0) a.status[b] = st, a.units[b] = 0;
    };
    const int n_in = a.in_len[b];
    if (n_in < 0 || n_in > S) return nothing(B2S_PROS_FAILED);
    if (n_in == 0) return nothing(B2S_PROS_EMPTY);

    // durations -> start[]: PER_THREAD consecutive positions per thread, then a scan over the threads' totals
    int bad = 0;
    long long mine[PER_THREAD], sum = 0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = tid * PER_THREAD + j;
        const int d = i < n_in ? a.dur[row + i] : 0;
        bad |= d < 0;
        mine[j] = sum;
        sum += d;
        if (i < n_in) sg[i] = a.groups ? a.groups[row + i] : i;
    }
    part[tid] = sum;
    __syncthreads();
    for (int h = 1; h < NT; h <<= 1) {
        const long long add = tid >= h ? part[tid - h] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const long long before = tid ? part[tid - 1] : 0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = tid * PER_THREAD + j;
        if (i < n_in) start[i] = before + mine[j];
    }
    const long long n = part[NT - 1];
    if (tid == 0) start[n_in] = n;
    for (int i = tid; i < n_in; i += NT) {
        const long long step = i == 0 ? (long long)sg[0] : (long long)sg[i] - sg[i - 1];
        bad |= i == 0 ? step != 0 : (step < 0 || step > 1);
    }
    if (__syncthreads_or(bad)) return nothing(B2S_PROS_FAILED);
    if (n > F) return nothing(B2S_PROS_SHORT);
    const int nu = sg[n_in - 1] + 1, nf = (int)n;
    for (int i = tid; i < n_in; i += NT)
        if (i == 0 || sg[i] != sg[i - 1]) ustart[sg[i]] = start[i];
    if (tid == 0) ustart[nu] = n;

    const int32_t *tau = a.tau + o0;
    const double *f0 = a.f0 + o0;
    int32_t *next = a.next + o0;
    const int nchunks = (nf + NT - 1) / NT;
    // backwards: the first voiced frame at or after t (nf: none)
    if (tid == 0) carry_sh = nf;
    __syncthreads();
    for (int c = nchunks - 1; c >= 0; --c) {
        const int t = c * NT + tid;
        const bool v = t < nf && tau[t] > 0;
        const unsigned long long bal = __ballot(v);
        if (lane == 0) wave_hit[w] = bal ? c * NT + 64 * w + __ffsll((long long)bal) - 1 : -1;
        __syncthreads();
        const unsigned long long here = bal >> lane;               // bit 0: this lane
        int nx = here ? t + __ffsll((long long)here) - 1 : -1;
        for (int i = w + 1; i < NT / 64 && nx < 0; ++i) nx = wave_hit[i];
        if (nx < 0) nx = carry_sh;
        if (t < nf) next[t] = nx;
        __syncthreads();
        if (tid == 0) carry_sh = nx;                               // thread 0 looks at the whole chunk
        __syncthreads();
    }
    const bool novoice = carry_sh == nf;
    // forwards: the last voiced frame at or before t (-1: none), and the contour
    __syncthreads();
    if (tid == 0) carry_sh = -1;
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int t = c * NT + tid;
        const bool v = t < nf && tau[t] > 0;
        const unsigned long long bal = __ballot(v);
        if (lane == 0) wave_hit[w] = bal ? c * NT + 64 * w + 63 - __clzll((long long)bal) : -1;
        __syncthreads();
        const unsigned long long here = bal << (63 - lane);        // bit 63: this lane
        int pv = here ? t - __clzll((long long)here) : -1;
        for (int i = w - 1; i >= 0 && pv < 0; --i) pv = wave_hit[i];
        if (pv < 0) pv = carry_sh;
        if (t < nf) {
            double y = 0.0;
            if (!novoice) {
                const int nx = next[t];
                if (pv == t) y = f0[t];
                else if (pv < 0) y = f0[nx];
                else if (nx >= nf) y = f0[pv];
                else y = f0[pv] + (f0[nx] - f0[pv]) * ((double)(t - pv) / (double)(nx - pv));
            }
            a.cont[o0 + t] = y;
        }
        __syncthreads();
        if (tid == NT - 1) carry_sh = pv;                          // the last thread looks back over the whole chunk
        __syncthreads();
    }
    for (int t = nf + tid; t < F; t += NT) a.cont[o0 + t] = 0.0;
    __threadfence_block();
    __syncthreads();

    for (int j = tid; j < nu; j += NT) {
        const int lo = (int)ustart[j], hi = (int)ustart[j + 1];
        int nv = 0;
        double vs = 0.0, cs = 0.0;
        long long es = 0;
        for (int t = lo; t < hi; ++t) {
            if (tau[t] > 0) ++nv, vs += f0[t];
            cs += a.cont[o0 + t];
            es += a.energy[o0 + t];
        }
        a.frames[row + j] = hi - lo, a.voiced[row + j] = nv, a.esum[row + j] = es;
        a.vsum[row + j] = vs, a.csum[row + j] = cs;
    }
    zero_units(nu);
    if (tid == 0) a.status[b] = novoice ? B2S_PROS_NOVOICE : B2S_PROS_OK, a.units[b] = nu;
}

// the sizes of b2s_pros_ws_bytes and b2s_pros_track: 0 with the row stride and the bytes, or 1 and a message
int track_sizes(int total, int tau_min, int tau_max, int *rs, size_t *bytes) {
    if (total < 0) return fail("total_frames must be >= 0 (got %d)", total);
    if (tau_min < 1) return fail("tau_min must be >= 1 (got %d)", tau_min);
    if (tau_max < tau_min) return fail("tau_max must be >= tau_min (got %d and %d)", tau_max, tau_min);
    if ((long long)tau_max - tau_min + 1 > MAX_LAGS)
        return fail("at most %d lags (got tau_min %d, tau_max %d)", MAX_LAGS, tau_min, tau_max);
    *rs = 64 * ((tau_max - tau_min + 1 + 63) / 64);
    *bytes = b2s_side::align_up((size_t)total * (size_t)*rs) + b2s_side::align_up(((size_t)total + 1) * sizeof(int32_t));
    return 0;
}

}  // namespace

extern "C" {

int b2s_pros_version(void) { return 100; }

const char *b2s_pros_last_error(void) { return b2s_side::last_error(); }

size_t b2s_pros_ws_bytes(int total_frames, int tau_min, int tau_max) {
    int rs = 0;
    size_t bytes = 0;
    return track_sizes(total_frames, tau_min, tau_max, &rs, &bytes) ? 0 : bytes;
}

int b2s_pros_energy(const int16_t *pcm, const int32_t *lengths, const int32_t *frame_offsets, int total_frames, int B, int Lmax,
                    int win, int hop, int64_t *energy, int32_t *status, void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (B > 65535) return fail("at most 65535 utterances per energy call (got %d); split the batch", B);
    if (Lmax < 0) return fail("Lmax must be >= 0 (got %d)", Lmax);
    if (total_frames < 0) return fail("total_frames must be >= 0 (got %d)", total_frames);
    if (win < 1 || win > B2S_PROS_MAX_WIN) return fail("win must be in 1..%d (got %d)", B2S_PROS_MAX_WIN, win);
    if (hop < 1) return fail("hop must be >= 1 (got %d)", hop);
    if (!lengths || !frame_offsets || !status) return fail("energy: lengths, frame_offsets or status is NULL");
    if ((Lmax > 0 && !pcm) || (total_frames > 0 && !energy)) return fail("energy: pcm or energy is NULL");
    const int per_block = NT / 64, maxF = 1 + Lmax / hop;
    const int gx = min(max((maxF + per_block - 1) / per_block, 1), 4096);
    hipLaunchKernelGGL(k_pros_energy, dim3(gx, B), dim3(NT), 0, (hipStream_t)stream, pcm, lengths, frame_offsets, total_frames, Lmax,
                       win, hop, (long long *)energy, status);
    return b2s_side::launch_status("energy");
}

int b2s_pros_track(const double *cmnd, const int64_t *energy, int64_t floor, const int32_t *frame_offsets, int total_frames, int B,
                   int K, int tau_min, int tau_max, double sr, double u, double v, double lam, double mu, int W, int32_t *tau,
                   double *f0, double *score, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    int rs = 0;
    size_t need = 0;
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (track_sizes(total_frames, tau_min, tau_max, &rs, &need)) return 1;
    if (K <= tau_max) return fail("K must be > tau_max (got %d and %d)", K, tau_max);
    if (W < 0 || W > B2S_PROS_MAX_W) return fail("W must be in 0..%d (got %d)", B2S_PROS_MAX_W, W);
    if (!std::isfinite(sr) || !std::isfinite(u) || !std::isfinite(v) || !std::isfinite(lam) || !std::isfinite(mu))
        return fail("track: sr, u, v, lam and mu must be finite");
    if (!frame_offsets || !score || !status) return fail("track: frame_offsets, score or status is NULL");
    if (total_frames > 0 && (!cmnd || !energy || !tau || !f0)) return fail("track: cmnd, energy, tau or f0 is NULL");
    if (!ws || ws_bytes < need) return fail("track: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    if ((uintptr_t)ws % sizeof(int32_t)) return fail("track: the workspace must be 4-byte aligned");
    TrackArgs a;
    a.cmnd = cmnd, a.energy = (const long long *)energy, a.floor = (long long)floor, a.off = frame_offsets, a.total = total_frames;
    a.K = K, a.tau_min = tau_min, a.tau_max = tau_max, a.nlag = tau_max - tau_min + 1, a.W = W, a.RS = rs;
    a.sr = sr, a.u = u, a.v = v, a.lam = lam, a.mu = mu, a.tau = tau, a.f0 = f0, a.score = score, a.status = status;
    a.bp = (unsigned char *)ws;
    a.bp0 = (int32_t *)((unsigned char *)ws + b2s_side::align_up((size_t)total_frames * (size_t)rs));
    const hipStream_t st = (hipStream_t)stream;
    if (W == 8) hipLaunchKernelGGL((k_pros_track<8>), dim3(B), dim3(rs), 0, st, a);
    else hipLaunchKernelGGL((k_pros_track<0>), dim3(B), dim3(rs), 0, st, a);
    return b2s_side::launch_status("track");
}

int b2s_pros_units(const double *f0, const int32_t *tau, const int64_t *energy, const int32_t *frame_offsets, int total_frames,
                   const int32_t *durations, const int32_t *input_lengths, const int32_t *groups, int B, int S, double *cont,
                   int32_t *frames, int32_t *voiced, double *f0_voiced_sum, double *f0_cont_sum, int64_t *energy_sum, int32_t *units,
                   int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    if (B <= 0) return fail("B must be > 0 (got %d)", B);
    if (S < 1 || S > B2S_PROS_MAX_S) return fail("S must be in 1..%d (got %d)", B2S_PROS_MAX_S, S);
    if (total_frames < 0) return fail("total_frames must be >= 0 (got %d)", total_frames);
    if (!frame_offsets || !durations || !input_lengths) return fail("units: frame_offsets, durations or input_lengths is NULL");
    if (total_frames > 0 && (!f0 || !tau || !energy || !cont)) return fail("units: f0, tau, energy or cont is NULL");
    if (!frames || !voiced || !f0_voiced_sum || !f0_cont_sum || !energy_sum || !units || !status)
        return fail("units: an output is NULL");
    const size_t need = (size_t)total_frames * sizeof(int32_t);
    if (need && (!ws || ws_bytes < need)) return fail("units: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    if ((uintptr_t)ws % sizeof(int32_t)) return fail("units: the workspace must be 4-byte aligned");
    UnitArgs a;
    a.f0 = f0, a.tau = tau, a.energy = (const long long *)energy, a.off = frame_offsets, a.total = total_frames;
    a.dur = durations, a.in_len = input_lengths, a.groups = groups, a.S = S, a.cont = cont, a.frames = frames, a.voiced = voiced;
    a.vsum = f0_voiced_sum, a.csum = f0_cont_sum, a.esum = (long long *)energy_sum, a.units = units, a.status = status;
    a.next = (int32_t *)ws;
    hipLaunchKernelGGL(k_pros_units, dim3(B), dim3(NT), 0, (hipStream_t)stream, a);
    return b2s_side::launch_status("units");
}

}  // extern "C"
