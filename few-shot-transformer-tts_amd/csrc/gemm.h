// GEMM descriptor shared by the engine and the C-ABI (see gemm.hip).
#pragma once
#include "b2s_common.h"

// One operand of C = op(A) * op(B).  "Stored rows" R are the non-contiguous dimension, "stored
// cols" C the contiguous one.  Non-transposed A is [M rows][K cols]; transposed A is [K rows][M cols].
// Non-transposed B is [N rows][K cols] (i.e. the Linear weight layout); transposed B is [K rows][N cols].
struct GemmOperand {
    const void* p = nullptr;
    long bs_o = 0, bs_i = 0;      // batch strides in elements (outer, inner batch index)
    int ld = 0;                   // leading dimension in elements
    int R = 0, C = 0;             // logical bounds of stored rows / cols
    // conv gather: when g_cin > 0 the operand is the virtual matrix Xg[token m][j*cin + ci] =
    // x[m + j - 2][ci] if 0 <= t+j-2 < min(len[b], T) else 0, with x stored [B*T][cin].
    int g_cin = 0, g_T = 0;
    const int* g_len = nullptr;
};

struct GemmEpilogue {
    float alpha = 1.f;
    const float* bias = nullptr;          // per output column
    int relu = 0;
    const void* relu_aux = nullptr;       // T*: out = aux > 0 ? v * aux_scale : 0   (ReLU+dropout backward)
    int ld_aux = 0;
    float aux_scale = 1.f;
    DropCfg drop = {0, 0, 1.f};           // dropout on the result, element index (z*M + m)*N + n
    const int* drop_salt = nullptr;       // optional device int mixed into the dropout key (decode step index under hipGraph replay)
    const float* residual = nullptr;      // fp32, added after dropout
    int ldr = 0;
    const int* row_len = nullptr;         // zero rows with (m % rows_per_batch) >= row_len[m / rows_per_batch]
    int rows_per_batch = 1;
    int conv_dw_cin = 0;                  // >0: output column n = j*cin+ci is stored at ci*5 + j
    int accumulate = 0;                   // fp32 output only: C += v
    float* colstat = nullptr;             // [2 N] fp32, zeroed by the caller: colstat[n] += sum_m v[m][n], colstat[N + n] += sum_m v[m][n]^2 of the
                                          // raw products (before any other epilogue step) -- the BatchNorm batch statistics of a conv layer's output
    // decode-step fusion, honoured by the weight-streaming kernel only (gemm_skinny.hip; the tiled kernels reject it): output
    // columns [kv_D, 2 kv_D) / [2 kv_D, 3 kv_D) are also appended to the head-major caches kv_k / kv_v [M][kv_D/kv_dh][kv_maxT][kv_dh] at position *kv_t
    void *kv_k = nullptr, *kv_v = nullptr;
    const int* kv_t = nullptr;
    int kv_maxT = 0, kv_D = 0, kv_dh = 0;
};

struct GemmArgs {
    GemmOperand A, B;
    int M = 0, N = 0, K = 0;
    int batch = 1, batch_inner = 1;       // z -> (z / batch_inner, z % batch_inner)
    int splitk = 1;                       // >1: K is split over blockIdx.z, partial sums atomically added (fp32 C, accumulate)
    void* C = nullptr;
    int c_fp32 = 0;                       // 1: float*, 0: compute type T*
    int ldc = 0;
    long cs_o = 0, cs_i = 0;
    GemmEpilogue epi;
    // split-K slab workspace ([splitk][M][N] fp32) owned by the CALLER (the model keeps one per stream it launches on; there
    // is no process-wide slab).  Null / too small: the partial tiles are accumulated with fp32 atomics instead.
    float* ws = nullptr;
    size_t ws_floats = 0;
};

// The GEMM entry point (gemm.hip), and the one place that picks the tiled kernel.  dtype: 0 = fp32 (gemm_kernel,
// mfma_f32_16x16x4f32); 1 = bf16 (mfma_f32_16x16x32_bf16, fp32 accumulate): b2s_gemm_glds256_launch for non-batched problems with
// M >= 129 (B2S_GEMM256_MIN_M), b2s_gemm_glds_launch otherwise.  (The decode step's weight-streaming kernel and the grouped
// weight-gradient launch below are called by name.)
int b2s_gemm_launch(const GemmArgs& g, int dtype, bool ta, bool tb, hipStream_t stream);
// bf16 128x128-tile LDS-DMA kernel (gemm_glds.hip)
int b2s_gemm_glds_launch(const GemmArgs& g, bool ta, bool tb, hipStream_t stream);
// decode-step weight-streaming kernel (gemm_skinny.hip); returns -1 when the problem does not fit it
int b2s_gemm_skinny_launch(const GemmArgs& g, int dtype, hipStream_t stream);
// bf16 256-row-tile family (gemm_glds256.hip; tile width, persistent walk and 128-row variant are chosen inside), and the number
// of 256x128 tiles a problem decomposes into
long b2s_gemm_glds256_tiles(const GemmArgs& g);
int b2s_gemm_glds256_launch(const GemmArgs& g, bool ta, bool tb, const bf16_t* zero, hipStream_t stream);
// split-K slab reduction shared by both bf16 families (gemm_glds.hip)
int b2s_splitk_reduce_launch(const float* ws, float* dst, int M, int N, int ldc, int splitk, int conv_dw_cin, hipStream_t stream);
// up to B2S_MAX_GROUP weight-gradient problems (TN form, fp32 accumulate, no split-K) in one launch
#define B2S_MAX_GROUP 8
// K segments (conv weight gradients, seg_n > 0): the K walk of every work item is cut into seg_n segments, one per utterance b, each with its own
// A row base, B row base and K length (derived in the kernel from the row shift of the work item's filter tap, see conv_seg() in gemm_glds256.hip)
struct b2s_gemm_group { int n; int order; int tile0[B2S_MAX_GROUP + 1]; GemmArgs p[B2S_MAX_GROUP];       // order: 1 = XCD-contiguous over the whole list
                        const int* seg_len; int seg_n, seg_T; };
int b2s_gemm_glds256_grouped_launch(const GemmArgs* probs, int n, const bf16_t* zero, hipStream_t stream);
// Weight gradients of up to B2S_MAX_GROUP Conv1d(k = 5, pad = 2) layers over the same [B][T] token rows in one launch, without a gathered operand:
//   C[co][ci*5 + j] (+)= sum_b sum_t dy[b*T + t][co] * x[b*T + t + j - 2][ci]   over 0 <= t < T, 0 <= t + j - 2 < min(len[b], T)   (len = nullptr: T)
// Problem i: A = dy (A.p, A.ld, A.C = M = cout), B = x (B.p, B.ld, B.C = N = cin), C fp32 [cout][ldc >= 5 cin], epi.accumulate; cin, cout and the
// leading dimensions multiples of 8.  len is DEVICE memory (no host copy is needed: a workgroup reads the seg_n lengths itself).
int b2s_gemm_glds256_conv_dw_launch(const GemmArgs* probs, int n, const int* len, int B, int T, const bf16_t* zero, hipStream_t stream);
int b2s_gemm_conv_dw_launch(const GemmArgs* probs, int n, const int* len, int B, int T, hipStream_t stream);      // gemm.hip: + optional timing record
// 256 zero bytes in device memory, written once at first use and immutable afterwards (source of the out-of-bounds chunks of
// the LDS-DMA loads); the only process-wide device object of the GEMM layer
const bf16_t* b2s_gemm_zero_page();
int b2s_gemm_grouped_launch(const GemmArgs* probs, int n, hipStream_t stream);      // gemm.hip: + optional timing record
