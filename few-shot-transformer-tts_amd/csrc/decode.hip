// Autoregressive mel / stop-token decoding (reference: synthesize.py:17-72 eval_batch) with a per-layer
// self-attention KV cache, encoder-decoder K/V projected once, and the whole per-frame step captured in a
// hipGraph that is replayed once per frame (the step index, stop flags and lengths live in device memory,
// so the same graph serves every frame; the host only polls `all finished` every few frames).
//
// The reference re-runs prenet + all decoder layers over the whole prefix every frame (no cache, O(t) GEMM +
// O(t^2) attention per frame, memory K/V re-projected every frame).  With dropout off the cached step is
// results-equivalent: position t only ever depends on positions <= t, and the
// reference's masking of finished samples (impute by target_lengths) is reproduced per step.
//
// Per-step HBM traffic (the roofline that bounds this path): decoder-stack weights once (49.9 M params) +
// self K/V cache read (Ld*2*B*t*Dd) + cross K/V read (Ld*2*B*S*Dd) + cache append.
#include "engine.h"
#include "decode_fused.h"
#include "drop_sites.h"

struct b2s_decode_state {
    int B = 0, S = 0, maxT = 0, train = 0;
    uint64_t seed = 0;
    char* ws = nullptr;
    size_t ws_bytes = 0;
    const int32_t* in_len = nullptr;
    int* t = nullptr;            // device: current frame index
    int* finished = nullptr;     // device [B]
    int* lengths = nullptr;      // device [B] (target_lengths of the reference loop)
    int* status = nullptr;       // device [2]: {t, all_finished}
    float* mels = nullptr;       // [B, maxT, NM]
    void* memT = nullptr;
    std::vector<void*> crossKV, selfK, selfV;    // crossKV[l]: K then V of the memory, head-major [2][B][H][S][dh] (contiguous rows per (utterance, head))
    void* kv_tmp = nullptr;                      // [B*S][2D] projection output before the re-layout
    std::vector<float*> crossP, selfP;   // attention rows of every step: [B,H,maxT,S] / [B,H,maxT,maxT]
    void *tgt = nullptr, *a1 = nullptr, *a2 = nullptr, *h = nullptr, *qkv = nullptr, *ctx = nullptr, *f = nullptr, *outT = nullptr;
    float *a3 = nullptr, *x = nullptr, *mean = nullptr, *rstd = nullptr, *mel_step = nullptr, *stop_step = nullptr;
    // fused step (decode_fused.hip): residual stream ping-pong [2][B][D], partial output slabs ping-pong [2][NS][B][D], and the
    // arrival counter of the last kernel of a frame
    float* Xpp[2] = {nullptr, nullptr};
    float* Ppp[2] = {nullptr, nullptr};
    int* done_cnt = nullptr;
    int ns_ffn = 0;
    bool fused = false;
    bool fast = false;          // every decoder sublayer has the default widths (b2s_df_fast_model): default-size kernel instantiations
    // fragment-packed copies of the projection weights the fused bf16 kernels read (b2s_df_pack; made by b2s_decode_begin)
    struct Pack { std::string name; int N, K; void* p; };
    std::vector<Pack> packs;
    const void* Wd(const b2s_model* m, const std::string& n) const {
        for (const Pack& k : packs) if (k.name == n) return k.p;
        return m->W(n);
    }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t graph_stream = nullptr;
    bool keep_self = false;
};

int b2s_ensure_pe_export(b2s_model* m, int len);      // engine.hip

namespace {
inline hipStream_t S_(void* s) { return (hipStream_t)s; }

// [B*S][2][H][dh] (projection output: K | V halves of a row, heads interleaved) -> [2][B][H][S][dh]; c16: 16-byte chunks per head row
__global__ void k_kv_headmajor(const uint4* __restrict__ src, uint4* __restrict__ dst, int B, int S, int H, int c16) {
    const long n = (long)B * S * 2 * H * c16;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c16);
        long r = i / c16;
        const int h = (int)(r % H); r /= H;
        const int kv = (int)(r % 2); r /= 2;
        const int sidx = (int)(r % S); const int b = (int)(r / S);
        dst[((((long)kv * B + b) * H + h) * S + sidx) * c16 + c] = src[i];
    }
}
__global__ void k_dec_begin(int* t, int* finished, int* lengths, int* status, int B) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { finished[i] = 0; lengths[i] = 1; }
    if (i == 0) { *t = 0; status[0] = 0; status[1] = 0; }
}
// tgt[b,:] = mels[b, t-1, :] (zero at t = 0)
template <typename T>
__global__ void k_dec_prep(const float* mels, const int* tptr, T* tgt, int maxT, int NM) {
    const int b = blockIdx.x, t = *tptr;
    for (int c = threadIdx.x; c < NM; c += blockDim.x)
        TT<T>::st(tgt + (long)b * NM + c, t > 0 ? mels[((long)b * maxT + (t - 1)) * NM + c] : 0.f);
}
// x[b,:] = (t>0 && t-1 < len[b] ? a3[b,:] : 0) + pe[t,:]*pe_scale ; dropout (modules.py:113-120 at position t)
__global__ void k_dec_x0(const float* a3, const int* lengths, const float* pe, const float* pe_scale, const int* tptr, float* x,
                         int D, DropCfg drop) {
    const int b = blockIdx.x, t = *tptr;
    const bool have = t > 0 && (t - 1) < lengths[b];
    const float sc = *pe_scale;
    DropCfg d = drop;
    d.key ^= b2s_hash32((uint32_t)t + 0x9e3779b9u);
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float v = (have ? a3[(long)b * D + c] : 0.f) + pe[(long)t * D + c] * sc;
        if (d.thresh) v = b2s_keep(d, (uint32_t)(b * D + c)) ? v * d.scale : 0.f;
        x[(long)b * D + c] = v;
    }
}
// append this frame's k, v (from qkv [B,3D]) to the head-major caches [B,H,maxT,dh] at position t (every head's rows are
// contiguous, so the per-head attention below streams whole cache lines instead of 2*dh-byte segments at a 2*D-byte stride)
template <typename T>
__global__ void k_dec_append(const T* qkv, const int* tptr, T* Kc, T* Vc, int maxT, int D, int dh) {
    const int b = blockIdx.x, t = *tptr, H = D / dh;
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        const int h = c / dh, d = c - h * dh;
        const long o = (((long)b * H + h) * maxT + t) * dh + d;
        Kc[o] = qkv[(long)b * 3 * D + D + c];
        Vc[o] = qkv[(long)b * 3 * D + 2 * D + c];
    }
}
// single-query attention for one (b, h) per 256-thread workgroup: keys [0, n), n = t+1 (self) or klen[b] (cross).
// Scores: 4 lanes share one key row (each 16-byte load instruction covers 64 contiguous bytes of a row), softmax
// through LDS, weighted V sum with one 16-byte column chunk per thread and a cross-row LDS reduction.
template <typename T>
__global__ __launch_bounds__(256) void k_dec_attn(const T* q, int ldq, const T* Kc, const T* Vc, int ldkv, long kv_bstride, long kv_hstride, T* out,
                                                  int ldo, float* probs, int probs_rows, int probs_ld, const int* tptr,
                                                  const int* klen, int self, int H, int dh, int nmax, float scale, DropCfg drop) {
    constexpr int VE = TT<T>::VE;
    extern __shared__ float sh[];            // [dh] q | [nmax] p | [R*dh] partial outputs | [8] reductions
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H, t = *tptr;
    const int n = self ? t + 1 : klen[b];
    float* sq = sh;
    float* p = sh + dh;
    const int CH = dh / VE, R = 256 / CH;
    float* part = p + nmax;
    float* red = part + R * dh;
    const T* Kb = Kc + b * kv_bstride + h * kv_hstride;      // head stride: dh (heads interleaved in a row) or maxT*dh (head-major cache)
    const T* Vb = Vc + b * kv_bstride + h * kv_hstride;
    const int part4 = tid & 3, kslot = tid >> 2;      // scores: 64 keys per pass, 4 lanes per key row
    const int nch = CH / 4;                           // 16-byte chunks per lane (dh is a multiple of 4*VE)
    const int tx = tid % CH, ty = tid / CH;           // value sum: one 16-byte column chunk per thread, R rows in parallel
    // The kernel is a chain of dependent phases on 2 workgroups per CU, so memory latency is what it costs: the loads of SU key
    // passes and of VU value rows are issued together, and the first group of both is in flight before the query is even
    // staged (for the 160-key cross attention that is every load of the kernel in one round trip).  Summation order per
    // lane is the plain sequential one.
    constexpr int SU = sizeof(T) == 2 ? 4 : 2, NCH_MAX = sizeof(T) == 2 ? 4 : 8;      // head width <= 128 (checked by the host)
    constexpr int VU = 8;
    const int nlast = max(n - 1, 0);                  // (clamped rows are loaded but never used)
    uint4 u[SU][NCH_MAX], uv[VU];
    auto load_k = [&](int j0) {
#pragma unroll
        for (int uu = 0; uu < SU; ++uu) {
            const T* kr = Kb + (long)min(j0 + uu * 64 + kslot, nlast) * ldkv;
#pragma unroll
            for (int i = 0; i < NCH_MAX; ++i)
                if (i < nch) u[uu][i] = *reinterpret_cast<const uint4*>(kr + (i * 4 + part4) * VE);
        }
    };
    auto load_v = [&](int j) {
#pragma unroll
        for (int v = 0; v < VU; ++v) uv[v] = *reinterpret_cast<const uint4*>(Vb + (long)min(j + v * R, nlast) * ldkv + tx * VE);
    };
    load_k(0);
    if (ty < R) load_v(ty);
    for (int d = tid; d < dh; d += 256) sq[d] = TT<T>::ld(q + (long)b * ldq + h * dh + d);
    __syncthreads();
    // ---- scores
    float mx = -INFINITY;
    for (int j0 = 0; j0 < n; j0 += 64 * SU) {
        if (j0 > 0) load_k(j0);
#pragma unroll
        for (int uu = 0; uu < SU; ++uu) {
            const int j = j0 + uu * 64 + kslot;
            if (j0 + uu * 64 >= n) break;              // (workgroup-uniform)
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < NCH_MAX; ++i) {
                if (i >= nch) continue;
                const int c = (i * 4 + part4) * VE;
                if (sizeof(T) == 2) {
                    const uint32_t w[4] = {u[uu][i].x, u[uu][i].y, u[uu][i].z, u[uu][i].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) { s += sq[c + 2 * e] * bf2f(w[e] & 0xffff) + sq[c + 2 * e + 1] * bf2f(w[e] >> 16); }
                } else {
                    const float* f = reinterpret_cast<const float*>(&u[uu][i]);
                    s += sq[c] * f[0] + sq[c + 1] * f[1] + sq[c + 2] * f[2] + sq[c + 3] * f[3];
                }
            }
            if (j >= n) s = 0.f;
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if (j < n && part4 == 0) { s *= scale; p[j] = s; mx = fmaxf(mx, s); }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int j = tid; j < n; j += 256) { float e = __expf(p[j] - mx); p[j] = e; sum += e; }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.f / (red[4] + red[5] + red[6] + red[7]);
    DropCfg dc = drop;
    dc.key ^= b2s_hash32((uint32_t)t * 2654435761u + 77u);
    float* prow = probs ? probs + (((long)b * H + h) * probs_rows + t) * probs_ld : nullptr;   // alignment row of this frame
    for (int j = tid; j < n; j += 256) {
        float w = p[j] * inv;
        if (prow) prow[j] = w;
        if (dc.thresh) w = b2s_keep(dc, (uint32_t)((b * H + h) * 4096 + j)) ? w * dc.scale : 0.f;
        p[j] = w;
    }
    __syncthreads();
    // ---- weighted sum of V rows
    if (ty < R) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int j = ty; j < n; j += R * VU) {
            if (j > ty) load_v(j);
#pragma unroll
            for (int v = 0; v < VU; ++v) {
                if (j + v * R >= n) break;
                const float w = p[j + v * R];
                if (sizeof(T) == 2) {
                    const uint32_t ww[4] = {uv[v].x, uv[v].y, uv[v].z, uv[v].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) { acc[2 * e] += w * bf2f(ww[e] & 0xffff); acc[2 * e + 1] += w * bf2f(ww[e] >> 16); }
                } else {
                    const float* f = reinterpret_cast<const float*>(&uv[v]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += w * f[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < VE; ++e) part[ty * dh + tx * VE + e] = acc[e];
    }
    __syncthreads();
    for (int d = tid; d < dh; d += 256) {
        float o = 0.f;
        for (int r = 0; r < R; ++r) o += part[r * dh + d];
        TT<T>::st(out + (long)b * ldo + h * dh + d, o);
    }
}
// finish the frame: mask by activity, write mels[:, t], update stop state (synthesize.py:42-45)
__global__ void k_dec_finish(const float* mel_step, const float* stop_step, const int* tptr, int* finished, int* lengths, float* mels,
                             int maxT, int NM) {
    const int b = blockIdx.x, t = *tptr;
    const bool active = t < lengths[b];
    for (int c = threadIdx.x; c < NM; c += blockDim.x) mels[((long)b * maxT + t) * NM + c] = active ? mel_step[(long)b * NM + c] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool stop = active && stop_step[b] > 0.f;
        const int fin = finished[b] | (stop ? 1 : 0);
        finished[b] = fin;
        if (!fin) lengths[b] += 1;
    }
}
__global__ void k_dec_advance(int* t, const int* finished, int* status, int B) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int all = 1;
        for (int b = 0; b < B; ++b) all &= finished[b];
        *t += 1;
        status[0] = *t; status[1] = all;
    }
}

struct DecPlan {
    size_t bytes;
};
std::string nm2(const std::string& p, const char* list, int i, const char* leaf) { return p + list + "." + std::to_string(i) + "." + leaf; }

void plan_decode(const b2s_model* m, b2s_decode_state& s, Arena& a) {
    const b2s_config& cf = m->cfg;
    const int B = s.B, S = s.S, T = s.maxT, D = cf.decoder_hidden, H = cf.n_attention_head, L = cf.n_decoder_layer, esz = m->esz;
    s.t = (int*)a.take(256); s.finished = (int*)a.take((size_t)B * 4); s.lengths = (int*)a.take((size_t)B * 4);
    s.status = (int*)a.take(256);
    s.mels = a.f32((long)B * T * cf.num_mels);
    s.memT = a.T((long)B * S * D, esz);
    s.crossKV.assign(L, nullptr); s.selfK.assign(L, nullptr); s.selfV.assign(L, nullptr); s.crossP.assign(L, nullptr); s.selfP.assign(L, nullptr);
    for (int l = 0; l < L; ++l) {
        s.crossKV[l] = a.T((long)B * S * 2 * D, esz);
        if (l == 0) s.kv_tmp = a.T((long)B * S * 2 * D, esz);
        s.selfK[l] = a.T((long)B * T * D, esz);
        s.selfV[l] = a.T((long)B * T * D, esz);
        s.crossP[l] = a.f32((long)B * H * T * S);
        if (s.keep_self) s.selfP[l] = a.f32((long)B * H * T * T);
    }
    s.tgt = a.T((long)B * cf.num_mels, esz); s.a1 = a.T((long)B * cf.prenet_hidden, esz); s.a2 = a.T((long)B * cf.prenet_hidden, esz);
    s.a3 = a.f32((long)B * D); s.x = a.f32((long)B * D); s.mean = a.f32(B); s.rstd = a.f32(B);
    s.h = a.T((long)B * D, esz); s.qkv = a.T((long)B * 3 * D, esz); s.ctx = a.T((long)B * D, esz); s.f = a.T((long)B * 4 * D, esz);
    s.outT = a.T((long)B * D, esz); s.mel_step = a.f32((long)B * cf.num_mels); s.stop_step = a.f32(B);
    s.ns_ffn = b2s_df_ffn_slices(m->dtype, D, H, 4 * D);
    s.fused = b2s_df_supported(m->dtype, D, H, 4 * D, cf.num_mels, cf.prenet_hidden, std::max(T, S));
    if (s.fused) {
        const int ns = std::max(H, s.ns_ffn);
        for (int i = 0; i < 2; ++i) { s.Xpp[i] = a.f32((long)B * D); s.Ppp[i] = a.f32((long)ns * B * D); }
        s.done_cnt = (int*)a.take(256);
        const int F = 4 * D, HP = cf.prenet_hidden, NM = cf.num_mels;
        const std::string p = "decoder.decoder.";
        s.packs.clear();
        auto add = [&](const std::string& n, int N, int K) { s.packs.push_back({n, N, K, a.T((long)N * K, 2)}); };
        s.fast = b2s_df_fast_model(D, H, F);
        if (b2s_df_attn_packed(m->dtype, D, H, F))
            for (int l = 0; l < L; ++l) {
                add(nm2(p, "self_attentions", l, "qkv_transform.weight"), 3 * D, D); add(nm2(p, "self_attentions", l, "output_transform.weight"), D, D);
                add(nm2(p, "encdec_attentions", l, "q_transform.weight"), D, D); add(nm2(p, "encdec_attentions", l, "output_transform.weight"), D, D);
            }
        if (b2s_df_ffn_packed(m->dtype, D, H, F))
            for (int l = 0; l < L; ++l) { add(nm2(p, "ffn_layers", l, "input_layer.weight"), F, D); add(nm2(p, "ffn_layers", l, "output_layer.weight"), D, F); }
        if (b2s_df_prenet_packed(m->dtype, HP, NM, D)) { add("decoder.prenet.dense1.weight", HP, HP); add("decoder.prenet.dense_final.weight", D, HP); }
        if (b2s_df_final_packed(m->dtype, D, H, F)) add("decoder.mel_net.weight", NM, D);
    }
}

int lin(const b2s_model* m, hipStream_t st, const void* X, int ldx, const void* W, int M, int N, int K, void* out, int out_fp32, int ldo,
        const GemmEpilogue& e) {
    GemmArgs g;
    g.A.p = X; g.A.ld = ldx; g.A.R = M; g.A.C = K;
    g.B.p = W; g.B.ld = K; g.B.R = N; g.B.C = K;
    g.M = M; g.N = N; g.K = K; g.C = out; g.c_fp32 = out_fp32; g.ldc = ldo; g.epi = e;
    if (M <= 64) {                               // the per-frame GEMMs: stream W once with N/16 workgroups
        const int rc = b2s_gemm_skinny_launch(g, m->dtype, st);
        if (rc >= 0) return rc;
    }
    return b2s_gemm_launch(g, m->dtype, false, false, st);
}

// One frame with one kernel per sublayer (decode_fused.hip): prenet + input, 3 kernels per decoder layer, heads + stop logic.
int step_fused(b2s_model* m, b2s_decode_state* s, hipStream_t st) {
    const b2s_config& cf = m->cfg;
    const int B = s->B, S = s->S, maxT = s->maxT, D = cf.decoder_hidden, H = cf.n_attention_head, dh = D / H, L = cf.n_decoder_layer;
    const int NM = cf.num_mels, HP = cf.prenet_hidden, dt = m->dtype;
    const float pt = s->train ? cf.transformer_dropout_rate : 0.f, pd = s->train ? cf.decoder_dropout_rate : 0.f;
    const float scale = 1.f / sqrtf((float)dh);
    const std::string p = "decoder.decoder.";
    DfPrenet pn;
    pn.mels = s->mels; pn.maxT = maxT; pn.NM = NM; pn.HP = HP; pn.D = D; pn.B = B;
    pn.W0 = m->W("decoder.prenet.dense0.weight"); pn.W1 = s->Wd(m, "decoder.prenet.dense1.weight"); pn.Wf = s->Wd(m, "decoder.prenet.dense_final.weight");
    pn.b0 = m->P("decoder.prenet.dense0.bias"); pn.b1 = m->P("decoder.prenet.dense1.bias");
    pn.pe = m->pe_dec; pn.pe_scale = m->P(p + "pe_scale"); pn.lengths = s->lengths; pn.t = s->t; pn.X = s->Xpp[0];
    pn.drop0 = make_drop(pd, s->seed, drop_op_decode(DS_DEC_PRENET0, 0)); pn.drop1 = make_drop(pd, s->seed, drop_op_decode(DS_DEC_PRENET1, 0)); pn.drop_x = make_drop(pt, s->seed, drop_op_decode(DS_DEC_EMBED, 0));
    B2S_TRY(b2s_df_prenet(dt, pn, st));
    int k = 0, np = 0;                           // sublayer index within the frame, slabs written by the previous kernel
    auto common = [&](const std::string& ln, DropCfg dres) {
        DfCommon c;
        c.X_in = s->Xpp[k & 1]; c.X_out = s->Xpp[(k + 1) & 1]; c.P_prev = s->Ppp[(k + 1) & 1]; c.np_prev = np; c.P_out = s->Ppp[k & 1];
        c.B = B; c.D = D; c.ln_g = m->P(ln + ".weight"); c.ln_b = m->P(ln + ".bias"); c.eps = 1e-6f; c.t = s->t; c.drop_res = dres;
        c.fast = s->fast ? 1 : 0;
        return c;
    };
    for (int l = 0; l < L; ++l) {
        const std::string lna = p + "attn_layer_norms." + std::to_string(l), lnx = p + "encdec_layer_norms." + std::to_string(l),
                          lnf = p + "ffn_layer_norms." + std::to_string(l);
        DfAttn sa;
        sa.c = common(lna, make_drop(pt, s->seed, drop_op_decode(DS_DEC_SELF_RES, l)));
        sa.H = H; sa.dh = dh; sa.Wqkv = s->Wd(m, nm2(p, "self_attentions", l, "qkv_transform.weight"));
        sa.Wo = s->Wd(m, nm2(p, "self_attentions", l, "output_transform.weight"));
        sa.Kc = s->selfK[l]; sa.Vc = s->selfV[l]; sa.ldkv = dh; sa.kv_bstride = (long)maxT * D; sa.kv_hstride = (long)maxT * dh; sa.maxT = maxT;
        sa.probs = s->selfP[l]; sa.probs_rows = maxT; sa.probs_ld = maxT; sa.klen = nullptr; sa.nmax = maxT; sa.scale = scale;
        sa.drop_attn = make_drop(pt, s->seed, drop_op_decode(DS_DEC_SELF_ATTN, l));
        B2S_TRY(b2s_df_attn(dt, true, sa, st));
        ++k; np = H;
        DfAttn xa;
        xa.c = common(lnx, make_drop(pt, s->seed, drop_op_decode(DS_DEC_CROSS_RES, l)));
        xa.H = H; xa.dh = dh; xa.Wqkv = s->Wd(m, nm2(p, "encdec_attentions", l, "q_transform.weight"));
        xa.Wo = s->Wd(m, nm2(p, "encdec_attentions", l, "output_transform.weight"));
        xa.Kc = s->crossKV[l]; xa.Vc = (char*)s->crossKV[l] + (size_t)B * S * D * m->esz; xa.ldkv = dh; xa.kv_bstride = (long)S * D; xa.kv_hstride = (long)S * dh;
        xa.maxT = maxT; xa.probs = s->crossP[l]; xa.probs_rows = maxT; xa.probs_ld = S; xa.klen = s->in_len; xa.nmax = S; xa.scale = scale;
        xa.drop_attn = make_drop(pt, s->seed, drop_op_decode(DS_DEC_CROSS_ATTN, l));
        B2S_TRY(b2s_df_attn(dt, false, xa, st));
        ++k; np = H;
        DfFfn ff;
        ff.c = common(lnf, make_drop(pt, s->seed, drop_op_decode(DS_DEC_FFN_RES, l)));
        ff.F = 4 * D; ff.ns = s->ns_ffn; ff.W1 = s->Wd(m, nm2(p, "ffn_layers", l, "input_layer.weight")); ff.W2 = s->Wd(m, nm2(p, "ffn_layers", l, "output_layer.weight"));
        ff.drop_hid = make_drop(pt, s->seed, drop_op_decode(DS_DEC_FFN_HID, l));
        B2S_TRY(b2s_df_ffn(dt, ff, st));
        ++k; np = s->ns_ffn;
    }
    DfFinal fn;
    fn.fast = s->fast ? 1 : 0;
    fn.X_in = s->Xpp[k & 1]; fn.P_prev = s->Ppp[(k + 1) & 1]; fn.np_prev = np; fn.B = B; fn.D = D; fn.NM = NM; fn.maxT = maxT;
    fn.ln_g = m->P(p + "output_layer_norm.weight"); fn.ln_b = m->P(p + "output_layer_norm.bias"); fn.eps = 1e-6f;
    fn.Wmel = s->Wd(m, "decoder.mel_net.weight"); fn.wstop = m->P("decoder.stop_net.weight"); fn.bstop = m->P("decoder.stop_net.bias");
    fn.mels = s->mels; fn.t = s->t; fn.finished = s->finished; fn.lengths = s->lengths; fn.status = s->status; fn.done_cnt = s->done_cnt;
    return b2s_df_final(dt, fn, st);
}

template <typename T>
int step_t(b2s_model* m, b2s_decode_state* s, hipStream_t st) {
    const b2s_config& cf = m->cfg;
    const int B = s->B, S = s->S, maxT = s->maxT, D = cf.decoder_hidden, H = cf.n_attention_head, dh = D / H, L = cf.n_decoder_layer;
    const int NM = cf.num_mels, HP = cf.prenet_hidden, dt = m->dtype;
    const float pt = s->train ? cf.transformer_dropout_rate : 0.f, pd = s->train ? cf.decoder_dropout_rate : 0.f;
    const float scale = 1.f / sqrtf((float)dh);
    const std::string p = "decoder.decoder.";
    hipLaunchKernelGGL((k_dec_prep<T>), dim3(B), dim3(128), 0, st, s->mels, s->t, (T*)s->tgt, maxT, NM);
    GemmEpilogue e0; e0.bias = m->P("decoder.prenet.dense0.bias"); e0.relu = 1; e0.drop = make_drop(pd, s->seed, drop_op_decode(DS_DEC_PRENET0, 0)); e0.drop_salt = s->t;
    B2S_TRY(lin(m, st, s->tgt, NM, m->W("decoder.prenet.dense0.weight"), B, HP, NM, s->a1, 0, HP, e0));
    GemmEpilogue e1; e1.bias = m->P("decoder.prenet.dense1.bias"); e1.relu = 1; e1.drop = make_drop(pd, s->seed, drop_op_decode(DS_DEC_PRENET1, 0)); e1.drop_salt = s->t;
    B2S_TRY(lin(m, st, s->a1, HP, m->W("decoder.prenet.dense1.weight"), B, HP, HP, s->a2, 0, HP, e1));
    B2S_TRY(lin(m, st, s->a2, HP, m->W("decoder.prenet.dense_final.weight"), B, D, HP, s->a3, 1, D, GemmEpilogue()));
    hipLaunchKernelGGL(k_dec_x0, dim3(B), dim3(256), 0, st, s->a3, s->lengths, m->pe_dec, m->P(p + "pe_scale"), s->t, s->x, D,
                       make_drop(pt, s->seed, drop_op_decode(DS_DEC_EMBED, 0)));
    const int ve = dt ? 8 : 4, Rr = 256 / (dh / ve);
    B2S_CHECK(dh <= 128 && dh % (4 * ve) == 0, "decode attention: head width %d (needs a multiple of %d, at most 128)", dh, 4 * ve);
    const size_t sh_self = (size_t)(dh + maxT + Rr * dh + 8) * 4, sh_cross = (size_t)(dh + S + Rr * dh + 8) * 4;
    for (int l = 0; l < L; ++l) {
        const std::string lna = p + "attn_layer_norms." + std::to_string(l), lnx = p + "encdec_layer_norms." + std::to_string(l),
                          lnf = p + "ffn_layer_norms." + std::to_string(l);
        // causal self-attention over the cache
        B2S_TRY(ro_layernorm_fwd(dt, s->x, m->P(lna + ".weight"), m->P(lna + ".bias"), s->h, D, nullptr, 0, s->mean, s->rstd, B, D, 1e-6f,
                                 nullptr, 1, st));
        // (B <= 64: the weight-streaming GEMM also appends this frame's k / v rows to the caches -- one kernel node fewer per
        // layer; every node costs >= ~7 us in the graph.  LayerNorm-on-load was tried too and lost: 6x the operand loads
        // in the streaming loop cost more than the saved node.)
        const bool fuse_kv = B <= 64 && D % 32 == 0;
        GemmEpilogue eq;
        if (fuse_kv) { eq.kv_k = s->selfK[l]; eq.kv_v = s->selfV[l]; eq.kv_t = s->t; eq.kv_maxT = maxT; eq.kv_D = D; eq.kv_dh = dh; }
        B2S_TRY(lin(m, st, s->h, D, m->W(nm2(p, "self_attentions", l, "qkv_transform.weight")), B, 3 * D, D, s->qkv, 0, 3 * D, eq));
        if (!fuse_kv)
            hipLaunchKernelGGL((k_dec_append<T>), dim3(B), dim3(256), 0, st, (const T*)s->qkv, s->t, (T*)s->selfK[l], (T*)s->selfV[l], maxT, D, dh);
        hipLaunchKernelGGL((k_dec_attn<T>), dim3(B * H), dim3(256), sh_self, st, (const T*)s->qkv, 3 * D, (const T*)s->selfK[l],
                           (const T*)s->selfV[l], dh, (long)maxT * D, (long)maxT * dh, (T*)s->ctx, D, s->selfP[l], maxT, maxT, s->t, (const int*)nullptr, 1, H, dh,
                           maxT, scale, make_drop(pt, s->seed, drop_op_decode(DS_DEC_SELF_ATTN, l)));
        GemmEpilogue ea; ea.drop = make_drop(pt, s->seed, drop_op_decode(DS_DEC_SELF_RES, l)); ea.drop_salt = s->t; ea.residual = s->x; ea.ldr = D;
        B2S_TRY(lin(m, st, s->ctx, D, m->W(nm2(p, "self_attentions", l, "output_transform.weight")), B, D, D, s->x, 1, D, ea));
        // encoder-decoder attention over the pre-projected memory K/V
        B2S_TRY(ro_layernorm_fwd(dt, s->x, m->P(lnx + ".weight"), m->P(lnx + ".bias"), s->h, D, nullptr, 0, s->mean, s->rstd, B, D, 1e-6f,
                                 nullptr, 1, st));
        B2S_TRY(lin(m, st, s->h, D, m->W(nm2(p, "encdec_attentions", l, "q_transform.weight")), B, D, D, s->qkv, 0, D, GemmEpilogue()));
        hipLaunchKernelGGL((k_dec_attn<T>), dim3(B * H), dim3(256), sh_cross, st, (const T*)s->qkv, D, (const T*)s->crossKV[l],
                           (const T*)s->crossKV[l] + (long)B * S * D, dh, (long)S * D, (long)S * dh, (T*)s->ctx, D, s->crossP[l], maxT, S, s->t, s->in_len, 0, H, dh,
                           S, scale, make_drop(pt, s->seed, drop_op_decode(DS_DEC_CROSS_ATTN, l)));
        GemmEpilogue ex; ex.drop = make_drop(pt, s->seed, drop_op_decode(DS_DEC_CROSS_RES, l)); ex.drop_salt = s->t; ex.residual = s->x; ex.ldr = D;
        B2S_TRY(lin(m, st, s->ctx, D, m->W(nm2(p, "encdec_attentions", l, "output_transform.weight")), B, D, D, s->x, 1, D, ex));
        // FFN
        B2S_TRY(ro_layernorm_fwd(dt, s->x, m->P(lnf + ".weight"), m->P(lnf + ".bias"), s->h, D, nullptr, 0, s->mean, s->rstd, B, D, 1e-6f,
                                 nullptr, 1, st));
        GemmEpilogue f1; f1.relu = 1; f1.drop = make_drop(pt, s->seed, drop_op_decode(DS_DEC_FFN_HID, l)); f1.drop_salt = s->t;
        B2S_TRY(lin(m, st, s->h, D, m->W(nm2(p, "ffn_layers", l, "input_layer.weight")), B, 4 * D, D, s->f, 0, 4 * D, f1));
        GemmEpilogue f2; f2.drop = make_drop(pt, s->seed, drop_op_decode(DS_DEC_FFN_RES, l)); f2.drop_salt = s->t; f2.residual = s->x; f2.ldr = D;
        B2S_TRY(lin(m, st, s->f, 4 * D, m->W(nm2(p, "ffn_layers", l, "output_layer.weight")), B, D, 4 * D, s->x, 1, D, f2));
    }
    B2S_TRY(ro_layernorm_fwd(dt, s->x, m->P(p + "output_layer_norm.weight"), m->P(p + "output_layer_norm.bias"), s->outT, D, nullptr, 0,
                             s->mean, s->rstd, B, D, 1e-6f, nullptr, 1, st));
    B2S_TRY(lin(m, st, s->outT, D, m->W("decoder.mel_net.weight"), B, NM, D, s->mel_step, 1, NM, GemmEpilogue()));
    B2S_TRY(ro_rowdot_fwd(dt, s->outT, D, m->P("decoder.stop_net.weight"), m->P("decoder.stop_net.bias"), s->stop_step, B, D, nullptr, 1, st));
    hipLaunchKernelGGL(k_dec_finish, dim3(B), dim3(128), 0, st, s->mel_step, s->stop_step, s->t, s->finished, s->lengths, s->mels, maxT, NM);
    hipLaunchKernelGGL(k_dec_advance, dim3(1), dim3(64), 0, st, s->t, s->finished, s->status, B);
    B2S_LAUNCH_CHECK();
    return 0;
}
int step(b2s_model* m, b2s_decode_state* s, hipStream_t st) {
    if (s->fused) return step_fused(m, s, st);
    return m->dtype ? step_t<bf16_t>(m, s, st) : step_t<float>(m, s, st);
}
}  // namespace

extern "C" size_t b2s_decode_ws_bytes(const b2s_model* m, int B, int S, int max_frames, int keep_self_alignments) {
    if (!m || B <= 0 || S <= 0 || max_frames <= 0) return 0;
    b2s_decode_state s; s.B = B; s.S = S; s.maxT = max_frames; s.keep_self = keep_self_alignments != 0;
    Arena a;
    plan_decode(m, s, a);
    return a.off + 4096;
}

extern "C" int b2s_decode_begin(b2s_model* m, const float* memory, const int32_t* input_lengths, int B, int S, int max_frames, int train,
                                uint64_t seed, int keep_self_alignments, void* ws, size_t ws_bytes, void* stream,
                                b2s_decode_state** out) {
    B2S_CHECK(m && m->bound, "model parameters are not bound");
    B2S_CHECK(memory && input_lengths && ws && out && B > 0 && S > 0 && max_frames > 0, "bad argument");
    // dropout op ids of the loop are decode_base + layer with bases 10 apart (drop_sites.h): an 11th layer would share masks with the next site
    B2S_CHECK(!train || m->cfg.n_decoder_layer <= 10, "decode with dropout supports at most 10 decoder layers (got %d)", m->cfg.n_decoder_layer);
    hipStream_t st = S_(stream);
    b2s_decode_state* s = new b2s_decode_state();
    s->B = B; s->S = S; s->maxT = max_frames; s->train = train; s->seed = seed; s->in_len = input_lengths;
    s->keep_self = keep_self_alignments != 0;
    s->ws = (char*)ws; s->ws_bytes = ws_bytes;
    Arena a; a.base = (char*)ws; a.cap = ws_bytes;
    plan_decode(m, *s, a);
    if (a.overflow || a.off > ws_bytes) { delete s; return b2s_fail(__FILE__, __LINE__, "decode workspace too small: need %zu bytes, got %zu", a.off, ws_bytes); }
    const b2s_config& cf = m->cfg;
    const int D = cf.decoder_hidden;
    int rc = b2s_ensure_pe_export(m, max_frames + 1);
    if (rc) { delete s; return rc; }
    hipLaunchKernelGGL(k_dec_begin, dim3(cdiv(B, 64)), dim3(64), 0, st, s->t, s->finished, s->lengths, s->status, B);
    if (s->done_cnt && hipMemsetAsync(s->done_cnt, 0, sizeof(int), st) != hipSuccess) { delete s; return b2s_fail(__FILE__, __LINE__, "memset failed"); }
    if (s->fused) {     // the first sublayer of the first frame loads (and ignores) a partial slab: it must hold finite values
        const size_t pb = (size_t)std::max(m->cfg.n_attention_head, s->ns_ffn) * B * m->cfg.decoder_hidden * 4;
        for (int i = 0; i < 2; ++i)
            if (hipMemsetAsync(s->Ppp[i], 0, pb, st) != hipSuccess) { delete s; return b2s_fail(__FILE__, __LINE__, "memset failed"); }
    }
    for (const b2s_decode_state::Pack& k : s->packs) {          // (per job: the weights may have been trained since the last one)
        rc = b2s_df_pack(m->W(k.name), k.N, k.K, k.p, st);
        if (rc) { delete s; return rc; }
    }
    rc = ro_cast(m->dtype, memory, s->memT, (long)B * S * D, st);
    for (int l = 0; l < cf.n_decoder_layer && !rc; ++l) {
        // memory K / V of the layer, then head-major: a head's rows of an utterance become one contiguous block (read in place
        // from the [B*S][2D] projection a 192-byte head row straddles two 128-byte lines: 1.5x the bytes, every frame)
        rc = lin(m, st, s->memT, D, m->W(nm2("decoder.decoder.", "encdec_attentions", l, "kv_transform.weight")), B * S, 2 * D, D, s->kv_tmp, 0,
                 2 * D, GemmEpilogue());
        if (!rc) {
            const long n16 = (long)B * S * 2 * D * m->esz / 16;
            hipLaunchKernelGGL(k_kv_headmajor, dim3((unsigned)std::min<long>((n16 + 255) / 256, 4096)), dim3(256), 0, st, (const uint4*)s->kv_tmp,
                               (uint4*)s->crossKV[l], B, S, cf.n_attention_head, D / cf.n_attention_head * m->esz / 16);
        }
        if (!rc) rc = hipMemsetAsync(s->crossP[l], 0, (size_t)B * cf.n_attention_head * max_frames * S * 4, st) == hipSuccess ? 0 : 1;
        if (!rc && s->selfP[l]) rc = hipMemsetAsync(s->selfP[l], 0, (size_t)B * cf.n_attention_head * max_frames * max_frames * 4, st) == hipSuccess ? 0 : 1;
    }
    if (rc) { delete s; return rc ? rc : 1; }
    *out = s;
    return 0;
}

// Run n frames.  use_graph: capture the step once into a hipGraph and replay it (stream must not be the NULL stream).
extern "C" int b2s_decode_run(b2s_model* m, b2s_decode_state* s, int n_steps, int use_graph, void* stream) {
    B2S_CHECK(m && s && n_steps >= 0, "bad argument");
    hipStream_t st = S_(stream);
    if (!use_graph) {
        for (int i = 0; i < n_steps; ++i) B2S_TRY(step(m, s, st));
        return 0;
    }
    if (!s->exec) {
        B2S_CHECK(st != nullptr, "graph capture needs a non-default stream");
        B2S_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        int rc = step(m, s, st);
        hipError_t e = hipStreamEndCapture(st, &s->graph);
        if (rc) return rc;
        B2S_HIP(e);
        B2S_HIP(hipGraphInstantiate(&s->exec, s->graph, nullptr, nullptr, 0));
        s->graph_stream = st;
    }
    for (int i = 0; i < n_steps; ++i) B2S_HIP(hipGraphLaunch(s->exec, st));
    return 0;
}

// Blocking read of {frames generated, all finished} (one small D2H copy; the only host sync of the loop).
extern "C" int b2s_decode_status(b2s_decode_state* s, int* frames_host, int* all_finished_host, void* stream) {
    B2S_CHECK(s && frames_host && all_finished_host, "bad argument");
    int h[2] = {0, 0};
    B2S_HIP(hipMemcpyAsync(h, s->status, sizeof(h), hipMemcpyDeviceToHost, S_(stream)));
    B2S_HIP(hipStreamSynchronize(S_(stream)));
    *frames_host = h[0]; *all_finished_host = h[1];
    return 0;
}

// Copy out the first n_frames frames [B, n_frames, NM], the lengths [B] (int32) and optionally the alignment rows
// of the encoder-decoder attention of `layer`: align_out [B, H, S, n_frames] (attention.py:88 layout).
extern "C" int b2s_decode_fetch(b2s_model* m, b2s_decode_state* s, int n_frames, float* mels_out, int32_t* lengths_out, void* stream) {
    B2S_CHECK(m && s && mels_out && lengths_out && n_frames >= 0 && n_frames <= s->maxT, "bad argument");
    hipStream_t st = S_(stream);
    const int NM = m->cfg.num_mels;
    if (n_frames > 0)
        B2S_HIP(hipMemcpy2DAsync(mels_out, (size_t)n_frames * NM * 4, s->mels, (size_t)s->maxT * NM * 4, (size_t)n_frames * NM * 4, s->B,
                                 hipMemcpyDeviceToDevice, st));
    B2S_HIP(hipMemcpyAsync(lengths_out, s->lengths, (size_t)s->B * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

namespace {
__global__ void k_dec_align(const float* P, float* out, int H, int maxT, int ldp, int nk, int n_frames) {
    // P [B*H, maxT(query), ldp(key)] -> out [B*H, nk(key), n_frames(query)]   (attention.py:88 layout)
    const int bh = blockIdx.y;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)nk * n_frames; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i / n_frames), q = (int)(i - (long)k * n_frames);
        out[((long)bh * nk + k) * n_frames + q] = P[((long)bh * maxT + q) * ldp + k];
    }
}
}  // namespace
extern "C" int b2s_decode_alignment(b2s_model* m, b2s_decode_state* s, int which, int layer, int n_frames, float* align_out, void* stream) {
    B2S_CHECK(m && s && align_out && layer >= 0 && layer < m->cfg.n_decoder_layer && n_frames > 0 && n_frames <= s->maxT, "bad argument");
    B2S_CHECK(which == 1 || (which == 0 && s->keep_self), "self-attention rows were not kept (keep_self_alignments = 0)");
    const int H = m->cfg.n_attention_head;
    if (which == 0)     // [B,H,maxT(q),maxT(k)] -> [B,H,n_frames(k),n_frames(q)]
        hipLaunchKernelGGL(k_dec_align, dim3(64, s->B * H), dim3(256), 0, S_(stream), (const float*)s->selfP[layer], align_out, H, s->maxT,
                           s->maxT, n_frames, n_frames);
    else
        hipLaunchKernelGGL(k_dec_align, dim3(64, s->B * H), dim3(256), 0, S_(stream), (const float*)s->crossP[layer], align_out, H, s->maxT,
                           s->S, s->S, n_frames);
    B2S_LAUNCH_CHECK();
    return 0;
}

extern "C" void b2s_decode_end(b2s_decode_state* s) {
    if (!s) return;
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    delete s;
}
