// Attention-guided token pruning between blocks (Liang et al. 2022, "Not All Patches Are What You Need": EViT's token reorganisation, placed at a block
// boundary): keep the K rows the cls token attends to most, fold the rest into one row weighted by their normalised attention.
//   token_score      score[b][j] = mean over heads of P[b][h][0][1 + j]: the cls row of attn_probs (attention_maps.hip; mean fusion) without its cls
//                    column - the same launch, the same bits as mfvit_vit_forward_attn's maps; no second softmax here.
//   token_select     rank with mfvit_patch_rank's total order (value, then index; NaN last), keep {j : rank[j] < K}; both index lists ascending;
//                    w[j] = score[j] / (sum over the dropped, ascending j, f32), or 1 / n_dropped when that sum is zero or not finite.  One workgroup
//                    per image, exact integers.
//   token_reorg_fwd  out[b] = (cls row, kept rows in list order: moves, bit-exact; then the fused row acc = w_0 x_0, acc = fma(w_j, x_j, acc) in list
//                    order: column-parallel, one writer per element).
//   token_reorg_bwd  dx[b] in full, every element written once: the cls and kept rows of dout moved back, a dropped row = w_j * dout[fused] (one f32
//                    product), any row no list names: zeros.  No atomics on memory: the same bits on every run.
// An index outside [0, T - 1) sets the error word, its row is zeros (forward) / it is skipped (fused sum, backward) and it never becomes an address;
// an index named twice sets the error word too (the backward then takes the later list entry).  All wave64, 16-byte accesses on the rows.
#include "kernels.h"

namespace mfvit {
namespace {

constexpr int TP_MAXP = 8192;        // the project's token limit (perturb.hip)
constexpr int TP_THREADS = 256;
constexpr int TP_BWD_BLOCKS = 8;     // workgroups per image of the backward: each rebuilds the image's inverse index map in LDS

// perturb.hip's rank_key: a > b <=> key(a) > key(b) for numbers, -0.0 and +0.0 share a key, every NaN has key 1 (below -inf); keys are >= 1
__device__ __forceinline__ unsigned tp_key(float x) {
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 1u;
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) + 1u;
}
// the float of a key (a zero comes back as +0.0, a NaN as a NaN): what the sum of the dropped scores adds
__device__ __forceinline__ float tp_unkey(unsigned key) {
    const unsigned k = key - 1u;
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(TP_THREADS) void tp_strip_cls_kernel(const float* __restrict__ probs, float* __restrict__ score, int B, int Tn) {
    const long total = (long)B * (Tn - 1);
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long b = q / (Tn - 1);
        score[q] = probs[q + b + 1];                            // row b, column 1 + j
    }
}

// dynamic LDS: keys uint[P4] (later the dropped scores, f32) | dlist ushort[P4] | flags uchar[P4]
__global__ __launch_bounds__(1024) void tp_select_kernel(const float* __restrict__ score, long ld, int P, int K, const int* __restrict__ forced,
                                                         int* __restrict__ idx_keep, int* __restrict__ idx_drop, float* __restrict__ w,
                                                         int* __restrict__ err) {
    extern __shared__ uint4 tp_lds[];
    const int P4 = (P + 3) & ~3;
    unsigned* keys = (unsigned*)tp_lds;
    unsigned short* dlist = (unsigned short*)(keys + P4);
    unsigned char* flags = (unsigned char*)(dlist + P4);
    __shared__ float denom_s;
    const int b = blockIdx.x, nd = P - K;
    const float* row = score + (long)b * ld;
    for (int j = threadIdx.x; j < P4; j += blockDim.x) keys[j] = j < P ? tp_key(row[j]) : 0u;
    __syncthreads();
    if (forced) {                                               // a given selection in place of the ranking: the kept set is what `forced` names
        for (int i = threadIdx.x; i < P; i += blockDim.x) flags[i] = 0;
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            const int id = forced[(long)b * K + k];
            idx_keep[(long)b * K + k] = -1;                     // (a list that keeps fewer than K rows leaves its tail at -1; read first: forced may be idx_keep)
            if (id < 0 || id >= P) *err = 1;
            else flags[id] = 1;
        }
    }
    for (int i = threadIdx.x; i < P && !forced; i += blockDim.x) {         // the count of patch_rank_kernel
        const unsigned ki = keys[i];
        int cnt = 0;
        for (int j = 0; j < P4; j += 4) {
            const uint4 k = tp_lds[j >> 2];
            cnt += k.x > (j < i ? ki - 1u : ki);
            cnt += k.y > (j + 1 < i ? ki - 1u : ki);
            cnt += k.z > (j + 2 < i ? ki - 1u : ki);
            cnt += k.w > (j + 3 < i ? ki - 1u : ki);
        }
        flags[i] = cnt < K ? 1 : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += blockDim.x) {         // compaction: the position of i in its list = the number of its kind below i
        int kept = 0;
        for (int j = 0; j < i; ++j) kept += flags[j];
        // (a forced selection that repeats or misplaces an index keeps fewer than K rows: the surplus of the other list is not written, and
        // the error word says so)
        if (flags[i]) {
            idx_keep[(long)b * K + kept] = i;
        } else if (i - kept < nd) {
            idx_drop[(long)b * nd + (i - kept)] = i;
            dlist[i - kept] = (unsigned short)i;
        } else if (err) {
            *err = 1;
        }
    }
    if (nd == 0) return;                                       // (block-uniform)
    __syncthreads();
    // the dropped scores in list order, over the keys (every thread reads its keys before anyone overwrites one)
    float v[(TP_MAXP + 1023) / 1024];
    int n = 0;
    for (int j = threadIdx.x; j < nd; j += blockDim.x) v[n++] = tp_unkey(keys[dlist[j]]);
    __syncthreads();
    float* dsc = (float*)keys;
    n = 0;
    for (int j = threadIdx.x; j < nd; j += blockDim.x) dsc[j] = v[n++];
    __syncthreads();
    if (threadIdx.x == 0) {                                     // ascending j, f32: the order the weights are defined by
        float s = dsc[0];
        for (int j = 1; j < nd; ++j) s += dsc[j];
        denom_s = s;
    }
    __syncthreads();
    const float denom = denom_s;
    const bool uniform = denom == 0.f || !(fabsf(denom) <= 3.402823466e38f);
    const float u = 1.f / (float)nd;
    for (int j = threadIdx.x; j < nd; j += blockDim.x) w[(long)b * nd + j] = uniform ? u : row[dlist[j]] / denom;
}

// idx[r] inside [0, P), or -1 with the error word set
__device__ __forceinline__ int tp_index(const int* __restrict__ idx, long r, int P, int* __restrict__ err) {
    const int id = idx[r];
    if (id < 0 || id >= P) {
        *err = 1;
        return -1;
    }
    return id;
}

// x (B, T, D) f32 -> out (B, 1 + K + f, D).  Image blockIdx.y; workgroups 0 .. gridDim.x - 2 move the cls and kept rows (one float4 per thread and
// step), the last one checks the image's lists for repeats (LDS counters: dynamic LDS int[P]) and forms the fused row, one float4 column per thread.
__global__ __launch_bounds__(TP_THREADS) void tp_reorg_fwd_kernel(const float* __restrict__ x, const int* __restrict__ idx_keep,
                                                                  const int* __restrict__ idx_drop, const float* __restrict__ w,
                                                                  float* __restrict__ out, int Tn, int D, int K, int fuse, int* __restrict__ err) {
    extern __shared__ uint4 tp_lds[];
    const int P = Tn - 1, D4 = D / 4, nd = P - K, To = 1 + K + fuse;
    const long b = blockIdx.y;
    const float4* xb = (const float4*)(x + b * (long)Tn * D);
    float4* ob = (float4*)(out + b * (long)To * D);
    if (blockIdx.x + 1 < gridDim.x) {
        const int total = (1 + K) * D4;
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (gridDim.x - 1) * blockDim.x) {
            const int r = q / D4, c = q - r * D4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r == 0) {
                v = xb[c];
            } else {
                const int id = tp_index(idx_keep, b * K + r - 1, P, err);
                if (id >= 0) v = xb[(long)(1 + id) * D4 + c];
            }
            ob[(long)r * D4 + c] = v;
        }
        return;
    }
    int* seen = (int*)tp_lds;
    for (int j = threadIdx.x; j < P; j += blockDim.x) seen[j] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < K + (idx_drop ? nd : 0); j += blockDim.x) {
        const int id = j < K ? idx_keep[b * K + j] : idx_drop[b * nd + j - K];
        if (id >= 0 && id < P && atomicAdd(&seen[id], 1) != 0) *err = 1;
    }
    if (!fuse) return;
    for (int c = threadIdx.x; c < D4; c += blockDim.x) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        bool first = true;
        for (int j = 0; j < nd; ++j) {
            const int id = tp_index(idx_drop, b * nd + j, P, err);
            if (id < 0) continue;
            const float wj = w[b * nd + j];
            const float4 v = xb[(long)(1 + id) * D4 + c];
            if (first) {                                        // (a product, not 0 + product: one dropped row with weight 1 comes back bit for bit)
                a.x = wj * v.x; a.y = wj * v.y; a.z = wj * v.z; a.w = wj * v.w;
                first = false;
            } else {
                a.x = fmaf(wj, v.x, a.x); a.y = fmaf(wj, v.y, a.y); a.z = fmaf(wj, v.z, a.z); a.w = fmaf(wj, v.w, a.w);
            }
        }
        ob[(long)(1 + K) * D4 + c] = a;
    }
}

// dout (B, 1 + K + f, D) -> dx (B, T, D), all of it.  Every workgroup of image blockIdx.y builds the image's inverse map in LDS (dynamic LDS int[P]:
// src[p] = the position of patch p in keep ++ drop, -1: in no list; atomicMax: a patch named twice takes the later entry, whatever the thread order),
// then walks its share of the T rows.
__global__ __launch_bounds__(TP_THREADS) void tp_reorg_bwd_kernel(const float* __restrict__ dout, const int* __restrict__ idx_keep,
                                                                  const int* __restrict__ idx_drop, const float* __restrict__ w,
                                                                  float* __restrict__ dx, int Tn, int D, int K, int fuse, int* __restrict__ err) {
    extern __shared__ uint4 tp_lds[];
    int* src = (int*)tp_lds;
    const int P = Tn - 1, D4 = D / 4, nd = P - K, To = 1 + K + fuse;
    const long b = blockIdx.y;
    for (int j = threadIdx.x; j < P; j += blockDim.x) src[j] = -1;
    __syncthreads();
    for (int j = threadIdx.x; j < K + (fuse ? nd : 0); j += blockDim.x) {
        const int id = j < K ? tp_index(idx_keep, b * K + j, P, err) : tp_index(idx_drop, b * nd + j - K, P, err);
        if (id >= 0 && atomicMax(&src[id], j) != -1) *err = 1;
    }
    __syncthreads();
    const float4* gb = (const float4*)(dout + b * (long)To * D);
    float4* db = (float4*)(dx + b * (long)Tn * D);
    const int total = Tn * D4;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
        const int r = q / D4, c = q - r * D4;
        const int code = r == 0 ? -2 : src[r - 1];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (code == -2) {
            v = gb[c];
        } else if (code >= 0 && code < K) {
            v = gb[(long)(1 + code) * D4 + c];
        } else if (code >= K) {
            const float wj = w[b * nd + code - K];
            const float4 g = gb[(long)(1 + K) * D4 + c];
            v = make_float4(wj * g.x, wj * g.y, wj * g.z, wj * g.w);
        }
        db[q] = v;
    }
}

bool tp_rows_ok(const void* a, const void* b2, int B, int Tn, int D, int K, int fuse) {
    if (!a || !b2 || ((size_t)a & 15) || ((size_t)b2 & 15)) return false;
    if (B <= 0 || B > 65535 || Tn < 2 || Tn > TP_MAXP + 1 || (D != 384 && D != 768)) return false;
    if (K < 1 || K > Tn - 1 || (fuse != 0 && fuse != 1)) return false;
    return (long)B * Tn * D < (1L << 31);
}

}  // namespace
}  // namespace mfvit

using namespace mfvit;

extern "C" {

int mfvit_token_score(int qkv_dtype, const void* qkv, const float* lse, int B, int T, int H, int HD, float* probs, float* score,
                      mfvit_stream_t stream) {
    if (!qkv || !lse || !probs || !score || B <= 0 || B > 65535 || T < 2 || T > TP_MAXP + 1 || H <= 0) return MFVIT_EINVAL;
    if (qkv_dtype < MFVIT_F32 || qkv_dtype > MFVIT_X3F16 || (HD != 32 && HD != 64 && HD != 96)) return MFVIT_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    MFVIT_TRY(attn_probs(qkv_dtype, qkv, lse, B, T, H, HD, 1, 1, probs, nullptr, st));
    const long total = (long)B * (T - 1);
    const long nb = (total + TP_THREADS - 1) / TP_THREADS;
    MFVIT_LAUNCH(tp_strip_cls_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(TP_THREADS), 0, st, (const float*)probs, score, B, T);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_token_select(const float* score, int64_t ld, int B, int P, int K, const int32_t* forced, int32_t* idx_keep, int32_t* idx_drop, float* w,
                       int32_t* err, mfvit_stream_t stream) {
    if (!score || !idx_keep || B <= 0 || B > 65535 || P <= 0 || P > TP_MAXP || ld < P || K < 1 || K > P || (forced && !err)) return MFVIT_EINVAL;
    if (K < P && (!idx_drop || !w)) return MFVIT_EINVAL;
    const int P4 = (P + 3) & ~3;
    const int threads = P >= 1024 ? 1024 : ((P + 63) / 64) * 64;
    const size_t lds = ((size_t)P4 * 7 + 15) & ~(size_t)15;     // 4 + 2 + 1 bytes per patch: 56 KiB at the token limit
    MFVIT_LAUNCH(tp_select_kernel, dim3(B), dim3(threads), lds, (hipStream_t)stream, score, (long)ld, P, K, (const int*)forced, (int*)idx_keep,
                 (int*)idx_drop, w, (int*)err);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_token_reorg_fwd(const float* x, const int32_t* idx_keep, const int32_t* idx_drop, const float* w, float* out, int B, int T, int D, int K,
                          int fuse, int32_t* err, mfvit_stream_t stream) {
    if (!tp_rows_ok(x, out, B, T, D, K, fuse) || !idx_keep || !err || x == out) return MFVIT_EINVAL;
    if (fuse && (K == T - 1 || !idx_drop || !w)) return MFVIT_EINVAL;            // (nothing dropped: there is no fused row to form)
    const int items = (1 + K) * (D / 4);
    int nb = (items + TP_THREADS - 1) / TP_THREADS;
    nb = nb > 64 ? 64 : nb;
    MFVIT_LAUNCH(tp_reorg_fwd_kernel, dim3(nb + 1, B), dim3(TP_THREADS), (size_t)(T - 1) * 4, (hipStream_t)stream, x, (const int*)idx_keep,
                 (const int*)idx_drop, w, out, T, D, K, fuse, (int*)err);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_token_reorg_bwd(const float* dout, const int32_t* idx_keep, const int32_t* idx_drop, const float* w, float* dx, int B, int T, int D, int K,
                          int fuse, int32_t* err, mfvit_stream_t stream) {
    if (!tp_rows_ok(dout, dx, B, T, D, K, fuse) || !idx_keep || !err || dout == dx) return MFVIT_EINVAL;
    if (fuse && (K == T - 1 || !idx_drop || !w)) return MFVIT_EINVAL;
    const int items = T * (D / 4);
    int nb = (items + TP_THREADS - 1) / TP_THREADS;
    nb = nb > TP_BWD_BLOCKS ? TP_BWD_BLOCKS : nb;
    MFVIT_LAUNCH(tp_reorg_bwd_kernel, dim3(nb, B), dim3(TP_THREADS), (size_t)(T - 1) * 4, (hipStream_t)stream, dout, (const int*)idx_keep,
                 (const int*)idx_drop, w, dx, T, D, K, fuse, (int*)err);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // extern "C"
