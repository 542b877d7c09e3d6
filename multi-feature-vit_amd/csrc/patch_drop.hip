// Patch dropout front end of the image encoder (timm >= 0.9 PatchDropout(prob, num_prefix_tokens = 1); Liu et al. 2022 "PatchDropout"; FLIP): the
// embedding stage on the KEPT patches only, in front of mfvit_vit_forward_x0, and its backward behind mfvit_vit_backward_x0 (include/mfvit.h).
//   forward:  gather im2col of the kept patches (B K rows x 768, the operand type and column order of im2col16) -> patch GEMM + bias ->
//             x0[b, 1 + k] = row + pos_embed[1 + idx[b, k]],  x0[b, 0] = cls_token + pos_embed[0]
//   backward: d cls_token, d pe_b (column sums in a fixed order), d pe_w (the weight-gradient launcher over the kept rows, split partials through
//             scratch), and on request d img: dx0[kept] W_pe gathered back through the inverse index map, dropped patches exact zeros.
// No float atomic anywhere: every sum has one writer and a fixed order.  Every kernel that takes idx checks 0 <= idx < L: a bad index sets the
// error word, its row is zeros, and it never becomes an address.  All wave64, 16-byte accesses on the image and the operand-type rows.
#include "kernels.h"

namespace mfvit {
namespace {

inline size_t pd_align(size_t x) { return (x + 255) & ~(size_t)255; }

// 8 consecutive logical columns n .. n + 7 (n % 8 == 0: inside one 32-group) of an operand-type row <-> f32
template <typename T> __device__ __forceinline__ void pd_store8(T* row, int n, const float (&f)[8]) {
    T* d = row + (is_split<T>::value ? split_col(n) : n);
    if constexpr (sizeof(T) == 2) {
        typedef typename Vec4<T>::elem E;
        typename Vec8<T>::type o, l;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const E h = (E)f[j];
            o[j] = h;
            if constexpr (is_split<T>::value) l[j] = (E)(f[j] - (float)h);
        }
        *(typename Vec8<T>::type*)d = o;
        if constexpr (is_split<T>::value) *(typename Vec8<T>::type*)((E*)d + 32) = l;
    } else {
        *(float4*)d = make_float4(f[0], f[1], f[2], f[3]);
        *(float4*)(d + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
}
template <typename T> __device__ __forceinline__ void pd_load8(const T* row, int n, float (&f)[8]) {
    const T* s = row + (is_split<T>::value ? split_col(n) : n);
    if constexpr (sizeof(T) == 2) {
        typedef typename Vec4<T>::elem E;
        const typename Vec8<T>::type o = *(const typename Vec8<T>::type*)s;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (float)o[j];
        if constexpr (is_split<T>::value) {
            const typename Vec8<T>::type l = *(const typename Vec8<T>::type*)((const E*)s + 32);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] += (float)l[j];
        }
    } else {
        const float4 a = *(const float4*)s, b = *(const float4*)(s + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
}

// the patch index of kept row (b, k), or -1 (and the error word set) when it lies outside the grid
__device__ __forceinline__ int pd_index(const int64_t* __restrict__ idx, long r, int L, int* __restrict__ err) {
    const int64_t id = idx[r];
    if (id < 0 || id >= (int64_t)L) {
        *err = 1;
        return -1;
    }
    return (int)id;
}

// img (B,3,H,W) f32 -> P [B K][768] of T: row (b, k) is patch idx[b, k] of image b, columns k' = c 256 + py 16 + px as im2col16 writes them.
// One thread moves 8 consecutive pixels (32 B in, 16 / 32 B out).
template <typename T>
__global__ __launch_bounds__(256) void pd_gather_kernel(const float* __restrict__ img, const int64_t* __restrict__ idx, T* __restrict__ P, int B, int K,
                                                        int Hh, int Ww, int* __restrict__ err) {
    const int gw = Ww / 16, L = (Hh / 16) * gw;
    const long total = (long)B * K * 96;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int half = q & 1;
        long r = q >> 1;
        const int py = r % 16; r /= 16;
        const int c = r % 3; r /= 3;                            // r: the kept row b K + k
        const int b = (int)(r / K);
        const int id = pd_index(idx, r, L, err);
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (id >= 0) {
            const int ph = id / gw, pw = id - ph * gw;
            const float* s = img + (((long)b * 3 + c) * Hh + ph * 16 + py) * Ww + pw * 16 + half * 8;
            const float4 v0 = *(const float4*)s, v1 = *(const float4*)(s + 4);
            f[0] = v0.x; f[1] = v0.y; f[2] = v0.z; f[3] = v0.w; f[4] = v1.x; f[5] = v1.y; f[6] = v1.z; f[7] = v1.w;
        }
        pd_store8<T>(P + r * 768 * elems_per<T>::value, c * 256 + py * 16 + half * 8, f);
    }
}

// x0 (B, 1 + K, D) f32: row 0 = cls + pos[0]; row 1 + k = E[b K + k] (the patch GEMM's output, bias added) + pos[1 + idx[b, k]]
template <typename T>
__global__ __launch_bounds__(256) void pd_assemble_kernel(const T* __restrict__ E, const int64_t* __restrict__ idx, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, float* __restrict__ x0, int B, int K, int D, int L,
                                                          int* __restrict__ err) {
    const int per = D / 8, T1 = K + 1;
    const long total = (long)B * T1 * per;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int n = (int)(q % per) * 8;
        const long row = q / per;
        const int t = (int)(row % T1);
        const long b = row / T1;
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float* p = nullptr;
        if (t == 0) {
            const float4 a = *(const float4*)(cls + n), c = *(const float4*)(cls + n + 4);
            f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = c.x; f[5] = c.y; f[6] = c.z; f[7] = c.w;
            p = pos + n;
        } else {
            const long r = b * K + t - 1;
            const int id = pd_index(idx, r, L, err);
            if (id >= 0) {
                pd_load8<T>(E + r * D * elems_per<T>::value, n, f);
                p = pos + (long)(1 + id) * D + n;
            }
        }
        if (p) {
            const float4 a = *(const float4*)p, c = *(const float4*)(p + 4);
            f[0] += a.x; f[1] += a.y; f[2] += a.z; f[3] += a.w; f[4] += c.x; f[5] += c.y; f[6] += c.z; f[7] += c.w;
        }
        float* o = x0 + row * D + n;
        *(float4*)o = make_float4(f[0], f[1], f[2], f[3]);
        *(float4*)(o + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
}

// G [B K][D] of T = the kept rows of dx0 (B, 1 + K, D) f32, cls rows left out: the dY operand of the weight gradient and of the data gradient
template <typename T>
__global__ __launch_bounds__(256) void pd_cast_rows_kernel(const float* __restrict__ dx0, T* __restrict__ G, int B, int K, int D) {
    const int per = D / 8;
    const long total = (long)B * K * per;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int n = (int)(q % per) * 8;
        const long r = q / per, b = r / K, k = r - b * K;
        const float* s = dx0 + (b * (K + 1) + 1 + k) * D + n;
        const float4 a = *(const float4*)s, c = *(const float4*)(s + 4);
        const float f[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
        pd_store8<T>(G + r * D * elems_per<T>::value, n, f);
    }
}

// out[n] += sum over the kept rows of dx0, in a fixed order (the scheme of colsum_rows: sixteen interleaved row sequences per 64 columns, combined
// 0 + 1 + .. + 15, one writer per column)
__global__ __launch_bounds__(1024) void pd_colsum_kept_kernel(const float* __restrict__ dx0, float* __restrict__ out, int B, int K, int D) {
    const int n = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    __shared__ float sm[16][64];
    float s = 0.f;
    if (n < D) {
        const long rows = (long)B * K;
#pragma unroll 4
        for (long r = sub; r < rows; r += 16) {
            const long b = r / K;
            s += dx0[(r + b + 1) * D + n];                      // row b (K + 1) + 1 + (r - b K)
        }
    }
    sm[sub][threadIdx.x & 63] = s;
    __syncthreads();
    if (sub == 0 && n < D) {
        s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += sm[i][threadIdx.x];
        out[n] += s;
    }
}

// inv[b][patch] = k where idx[b, k] = patch (inv starts at -1: a dropped patch)
__global__ __launch_bounds__(256) void pd_invert_kernel(const int64_t* __restrict__ idx, int* __restrict__ inv, int B, int K, int L, int* __restrict__ err) {
    const long r = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (r >= (long)B * K) return;
    const int id = pd_index(idx, r, L, err);
    if (id >= 0) inv[(r / K) * L + id] = (int)(r % K);
}

// dimg (B,3,H,W) f32 = the inverse of pd_gather over G [B K][768] of T: every image element is written once, a dropped patch's with 0.0
template <typename T>
__global__ __launch_bounds__(256) void pd_scatter_kernel(const T* __restrict__ G, const int* __restrict__ inv, float* __restrict__ dimg, int B, int K,
                                                         int Hh, int Ww) {
    const int gh = Hh / 16, gw = Ww / 16;
    const long total = (long)B * gh * gw * 96;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int half = q & 1;
        long r = q >> 1;
        const int py = r % 16; r /= 16;
        const int c = r % 3; r /= 3;                            // r: b L + patch
        const int pw = r % gw;
        const int ph = (r / gw) % gh;
        const long b = r / ((long)gw * gh);
        const int k = inv[r];
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (k >= 0 && k < K) pd_load8<T>(G + (b * K + k) * 768 * elems_per<T>::value, c * 256 + py * 16 + half * 8, f);
        float* o = dimg + ((b * 3 + c) * Hh + ph * 16 + py) * Ww + pw * 16 + half * 8;
        *(float4*)o = make_float4(f[0], f[1], f[2], f[3]);
        *(float4*)(o + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
}

inline int pd_blocks(long items) {
    const long b = (items + 255) / 256;
    return (int)(b < 1 ? 1 : (b < 4096 ? b : 4096));
}

struct PdDims { int dtype, B, K, D, H, W, L, es, e; long R; };
bool pd_dims(const mfvit_patch_keep_cfg* c, PdDims& d) {
    if (!c) return false;
    if (c->dtype != MFVIT_F32 && c->dtype != MFVIT_BF16 && c->dtype != MFVIT_BF16X3 && c->dtype != MFVIT_F16) return false;
    if (c->batch <= 0 || c->img_h <= 0 || c->img_w <= 0 || c->img_h % 16 || c->img_w % 16) return false;
    if (c->dim != 384 && c->dim != 768) return false;
    d.dtype = c->dtype; d.B = c->batch; d.K = c->keep; d.D = c->dim; d.H = c->img_h; d.W = c->img_w;
    d.L = (c->img_h / 16) * (c->img_w / 16);
    if (c->keep < 1 || c->keep > d.L) return false;
    d.R = (long)d.B * d.K;
    if (d.R * 768 >= (1L << 31) || (long)d.B * d.L >= (1L << 31)) return false;   // (the GEMM launchers count rows and elements in int)
    d.es = (c->dtype == MFVIT_BF16 || c->dtype == MFVIT_F16) ? 2 : 4;
    d.e = c->dtype == MFVIT_BF16X3 ? 2 : 1;
    return true;
}
// workspace (bytes): what the forward writes, then what only a backward needs
struct PdLayout { size_t patches, emb, w, fwd_total, wT, dpatch, inv, tnpart, total; };
PdLayout pd_layout(const PdDims& d) {
    PdLayout W;
    size_t o = 0;
    W.patches = o; o += pd_align((size_t)d.R * 768 * d.es);     // the kept rows of im2col: the GEMM's A, the weight gradient's X
    W.emb = o; o += pd_align((size_t)d.R * d.D * d.es);         // forward: the GEMM's output; backward: the kept rows of dx0 in the operand type
    W.w = o; o += pd_align((size_t)d.D * 768 * d.es);           // W_pe in the operand type
    W.fwd_total = o;
    W.wT = o; o += pd_align((size_t)768 * d.D * d.es);          // W_pe^T (the image gradient)
    W.dpatch = o; o += pd_align((size_t)d.R * 768 * d.es);      // dx0[kept] W_pe
    W.inv = o; o += pd_align((size_t)d.B * d.L * 4);
    W.tnpart = o; o += pd_align((size_t)384 * 128 * 128 * 4);   // split partials of the weight gradient (the encoder's slot size, vit.hip)
    W.total = o;
    return W;
}

#define PD_BY_DTYPE(dtype, STMT)                            \
    switch (dtype) {                                        \
        case MFVIT_F32: { typedef float TT; STMT; } break;   \
        case MFVIT_BF16: { typedef bf16 TT; STMT; } break;   \
        case MFVIT_BF16X3: { typedef sbf16 TT; STMT; } break; \
        case MFVIT_F16: { typedef f16 TT; STMT; } break;     \
        default: return MFVIT_EINVAL;                       \
    }

}  // namespace
}  // namespace mfvit

using namespace mfvit;

extern "C" {

size_t mfvit_patch_keep_workspace_bytes(const mfvit_patch_keep_cfg* cfg, int backward) {
    PdDims d;
    if (!pd_dims(cfg, d)) return 0;
    const PdLayout W = pd_layout(d);
    return backward ? W.total : W.fwd_total;
}

int mfvit_patch_keep_embed(const mfvit_patch_keep_cfg* cfg, const float* img, const int64_t* idx, const float* cls_token, const float* pos_embed,
                           const float* pe_w, const float* pe_b, void* workspace, int save, float* x0, int32_t* err, mfvit_stream_t stream) {
    PdDims d;
    if (!pd_dims(cfg, d) || !img || !idx || !cls_token || !pos_embed || !pe_w || !pe_b || !workspace || !x0 || !err) return MFVIT_EINVAL;
    const PdLayout W = pd_layout(d);
    char* const ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    MFVIT_TRY(cast_transpose(d.dtype, pe_w, ws + W.w, save ? ws + W.wT : nullptr, d.D, 768, st));
    PD_BY_DTYPE(d.dtype, MFVIT_LAUNCH(pd_gather_kernel<TT>, dim3(pd_blocks(d.R * 96)), dim3(256), 0, st, img, idx, (TT*)(ws + W.patches), d.B, d.K, d.H,
                                      d.W, (int*)err));
    MFVIT_CHECK_LAUNCH();
    GemmP p = nt(ws + W.patches, 768L * d.e, ws + W.w, 768L * d.e, (int)d.R, d.D, 768);
    p.bias = pe_b;
    p.out0 = ws + W.emb; p.ldo0 = (long)d.D * d.e;
    MFVIT_TRY(gemm_nt_tile(d.dtype, EPI_BIAS, p, st));
    PD_BY_DTYPE(d.dtype, MFVIT_LAUNCH(pd_assemble_kernel<TT>, dim3(pd_blocks((long)d.B * (d.K + 1) * (d.D / 8))), dim3(256), 0, st,
                                      (const TT*)(ws + W.emb), idx, cls_token, pos_embed, x0, d.B, d.K, d.D, d.L, (int*)err));
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_patch_keep_embed_bwd(const mfvit_patch_keep_cfg* cfg, const int64_t* idx, void* workspace, const float* dx0, float* dcls, float* dpe_w,
                               float* dpe_b, float* dimg, int32_t* err, mfvit_stream_t stream) {
    PdDims d;
    if (!pd_dims(cfg, d) || !idx || !workspace || !dx0 || !err || (!dcls && !dpe_w && !dpe_b && !dimg)) return MFVIT_EINVAL;
    const PdLayout W = pd_layout(d);
    char* const ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const long De = (long)d.D * d.e;
    if (dcls) MFVIT_TRY(colsum_rows(dx0, d.D, dcls, d.B, d.K + 1, 0, d.D, st));
    if (dpe_b) {
        MFVIT_LAUNCH(pd_colsum_kept_kernel, dim3((d.D + 63) / 64), dim3(1024), 0, st, dx0, dpe_b, d.B, d.K, d.D);
        MFVIT_CHECK_LAUNCH();
    }
    if (!dpe_w && !dimg) return MFVIT_OK;
    PD_BY_DTYPE(d.dtype, MFVIT_LAUNCH(pd_cast_rows_kernel<TT>, dim3(pd_blocks(d.R * (d.D / 8))), dim3(256), 0, st, dx0, (TT*)(ws + W.emb), d.B, d.K, d.D));
    MFVIT_CHECK_LAUNCH();
    if (dpe_w) {   // d pe_w += dx0[kept]^T patches_kept; split partials as plain stores, reduced in a fixed order
        GemmP p = nt(ws + W.emb, De, ws + W.patches, 768L * d.e, (int)d.R, d.D, 768);
        p.out0 = dpe_w; p.ldo0 = 768;
        p.cpart = (float*)(ws + W.tnpart);
        TnPartScope own(true);                                   // (never queued into a caller's batch: the slot is reduced before this call returns)
        MFVIT_TRY(gemm_tn(d.dtype, p, st));
        MFVIT_TRY(tnpart_batch_flush(st));
    }
    if (dimg) {
        GemmP p = nt(ws + W.emb, De, ws + W.wT, De, (int)d.R, 768, d.D);
        p.out0 = ws + W.dpatch; p.ldo0 = 768L * d.e;
        MFVIT_TRY(gemm_nt_tile(d.dtype, EPI_NONE, p, st));
        if (hipMemsetAsync(ws + W.inv, 0xFF, (size_t)d.B * d.L * 4, st) != hipSuccess) return MFVIT_ELAUNCH;
        MFVIT_LAUNCH(pd_invert_kernel, dim3((unsigned)((d.R + 255) / 256)), dim3(256), 0, st, idx, (int*)(ws + W.inv), d.B, d.K, d.L, (int*)err);
        MFVIT_CHECK_LAUNCH();
        PD_BY_DTYPE(d.dtype, MFVIT_LAUNCH(pd_scatter_kernel<TT>, dim3(pd_blocks((long)d.B * d.L * 96)), dim3(256), 0, st, (const TT*)(ws + W.dpatch),
                                          (const int*)(ws + W.inv), dimg, d.B, d.K, d.H, d.W));
        MFVIT_CHECK_LAUNCH();
    }
    return MFVIT_OK;
}

}  // extern "C"
