// Attention maps of the ViT encoder (DINO's get_last_selfattention, per-block maps, attention rollout), formed after a block's attention
// forward from what that forward leaves in the workspace: the qkv tensor and the natural-log log-sum-exp lse [B][H][T].
//
//   P[b][h][i][j] = exp(scale q_i.k_j - lse[b][h][i]),  scale = head_dim^-1/2 (the forward kernels apply it to the scores; q is not
//   stored pre-scaled) - the probabilities exactly as normalised by the forward's softmax.
//
// Probability kernel.  qkv in any of the encoder's storage formats, layout [B][T][3][H][HD]: f32, bf16, fp16, split bf16 (MFVIT_BF16X3)
// and split fp16 (MFVIT_X3F16), I32 layout for the split ones (common.cuh).  Every operand is widened to f32 on load (split: hi + lo) and
// S = q k^T runs on v_mfma_f32_32x32x2_f32 (exact f32 products: for a 16-bit operand the recomputed S differs from the forward's only in
// summation order).  A lane holds 16 consecutive logical columns of every 32-wide group of its row (lanes 0 - 31 the first 16, lanes
// 32 - 63 the last 16): which k a lane half feeds is free as long as both operands agree, and so every lane reads 32 / 64 contiguous bytes.
// Work split: one workgroup (4 waves) per (image, 32-query tile[, head]); wave w takes the key tiles w, w + 4, ...  Fused forms (mean /
// max / min over heads) loop over the heads inside the key tile and fuse in registers: per-head maps never reach memory.  Their row sums
// (optional) are reduced lane butterfly -> LDS -> a fixed wave order.  Query and key positions past T are clamped on load and never stored.
//
// Rollout kernel (Abnar & Zuidema 2020), cls row only: v = row 0 of a_{L-1}, then v <- v a_l for l = L-2 .. 0 with
// a_l = diag(c_l) (F_l / 2 + I / 2), c_l = 1 / (s_l / 2 + 1 / 2): each step w = v o c_l, v <- (w F_l + w) / 2.  One workgroup per image,
// v in LDS, column sums in a fixed order.
//
// Relevance kernels (Chefer, Gur & Wolf 2021, the self-attention rule), behind block l's attention backward in the data-gradient chain, from the
// qkv and lse of the forward and dO = d y_t / d (attention output before proj) (the proj data gradient, [B][T][D] in the activation storage
// type: f32, bf16, fp16 or split bf16, I32 layout):
//   dP_h = dO_h V_h^T,  A_l = (1/H) sum_h max(0, P_h o dP_h),  and the cls row v of R = (I + A_{L-1}) ... (I + A_0): v <- v + v A_l, l = L-1 .. 0.
// Map kernel: one workgroup per (image, 32-query tile), wave w takes the key tiles w, w + 4, ...  Per head, S = q k^T and dP = dO v^T run on
// v_mfma_f32_32x32x2_f32 with the lane layout of the probability kernel (both operands widened to f32 on load); the heads are summed in
// registers in head order, so per-head maps never reach memory.  Outputs: A_l into `map` (optional) and the tile's share of the row product,
// part[b][tile][j] = sum_{i in tile} v[i] A_l[i][j] (optional; rows in register order, then the two lane halves).  Update kernel: v <- v + the
// tiles' parts in tile order; after block 0 it writes v[1:].  With `first` v is e_0 and is not read.
//
// No atomics anywhere: repeated calls return the same bits.
#include "common.cuh"
#include "kernels.h"
#include "prof.h"

namespace mfvit {

namespace {

constexpr int AM_WAVES = 4;

__device__ __forceinline__ int am_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// storage element of the qkv tensor of tag T
template <typename T> struct AmStor { typedef T E; static constexpr int EP = 1; };
template <> struct AmStor<sbf16> { typedef bf16 E; static constexpr int EP = 2; };
template <> struct AmStor<sf16> { typedef f16 E; static constexpr int EP = 2; };

// f[16 g + i] = logical column 32 g + 16 half + i of a head row piece (g < NB), widened to f32; split tensors: hi + lo
template <typename T, int NB> __device__ __forceinline__ void am_load_frag(const typename AmStor<T>::E* row, int half, float (&f)[16 * NB]) {
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        if constexpr (std::is_same<T, float>::value) {
            const float4* p = (const float4*)(row + 32 * g + 16 * half);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 v = p[i];
                f[16 * g + 4 * i] = v.x; f[16 * g + 4 * i + 1] = v.y; f[16 * g + 4 * i + 2] = v.z; f[16 * g + 4 * i + 3] = v.w;
            }
        } else if constexpr (is_split<T>::value) {
            typedef typename Vec8<T>::type V;
            const V* hp = (const V*)(row + 64 * g + 16 * half);
            const V* lp = (const V*)(row + 64 * g + 32 + 16 * half);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const V h = hp[i], l = lp[i];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[16 * g + 8 * i + j] = (float)h[j] + (float)l[j];
            }
        } else {
            typedef typename Vec8<T>::type V;
            const V* p = (const V*)(row + 32 * g + 16 * half);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const V v = p[i];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[16 * g + 8 * i + j] = (float)v[j];
            }
        }
    }
}

// S tile [32 queries][32 keys] of one head: lane (r, half) gives q row r and k row r; result row i = am_acc_row(reg, lane), column = lane & 31
template <int NB> __device__ __forceinline__ f32x16 am_scores(const float (&qf)[16 * NB], const float (&kf)[16 * NB]) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 16 * NB; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i], kf[i], s, 0, 0, 0);
    return s;
}

// FUSED = false: out [B][H][rows][T] (grid B * H * nqt);  FUSED = true: out [B][rows][T] fused over heads by `op` (1 mean, 2 max, 3 min),
// sums [B][rows] (or NULL) = the fused rows' sums over the T keys (grid B * nqt).  rows = T, or 1 (the cls query); nqt = ceil(rows / 32).
template <typename T, int NB, bool FUSED>
__global__ __launch_bounds__(256) void attn_probs_kernel(const typename AmStor<T>::E* __restrict__ qkv, const float* __restrict__ lse,
                                                         float* __restrict__ out, float* __restrict__ sums, int Tn, int H, int rows, int nqt,
                                                         int op, float c) {
    typedef typename AmStor<T>::E E;
    constexpr int HD = 32 * NB, EP = AmStor<T>::EP;
    __shared__ float part[AM_WAVES][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    int bid = blockIdx.x;
    const int qt = bid % nqt;
    bid /= nqt;
    const int h0 = FUSED ? 0 : bid % H, b = FUSED ? bid : bid / H;
    const int q0 = qt * 32;
    const long hs = (long)H * HD * EP, rs = 3 * hs;                 // storage elements of one of q / k / v of a token, and of all three
    const E* base = qkv + (long)b * Tn * rs;
    const int qrow = min(q0 + (lane & 31), Tn - 1);                  // (rows past the end: a valid row is read, nothing is stored)
    const int nkt = (Tn + 31) / 32;
    // -lse of the lane's 16 result rows in log2 units, and the q fragment: loaded once per head
    float qf[16 * NB], nl[16];
    auto load_head = [&](int h) __attribute__((always_inline)) {
        am_load_frag<T, NB>(base + (long)qrow * rs + (long)h * HD * EP, half, qf);
        const float* lrow = lse + ((long)b * H + h) * Tn;
#pragma unroll
        for (int r = 0; r < 16; ++r) nl[r] = -lrow[min(q0 + am_acc_row(r, lane), Tn - 1)] * 1.4426950408889634f;
    };
    if constexpr (!FUSED) load_head(h0);
    float rsum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rsum[r] = 0.f;
    for (int kt = wave; kt < nkt; kt += AM_WAVES) {
        const int key = kt * 32 + (lane & 31);
        const E* krow = base + (long)min(key, Tn - 1) * rs + hs;
        f32x16 f;
        if constexpr (!FUSED) {
            float kf[16 * NB];
            am_load_frag<T, NB>(krow + (long)h0 * HD * EP, half, kf);
            const f32x16 s = am_scores<NB>(qf, kf);
#pragma unroll
            for (int r = 0; r < 16; ++r) f[r] = exp2f(fmaf(s[r], c, nl[r]));
        } else {
            for (int h = 0; h < H; ++h) {
                load_head(h);
                float kf[16 * NB];
                am_load_frag<T, NB>(krow + (long)h * HD * EP, half, kf);
                const f32x16 s = am_scores<NB>(qf, kf);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = exp2f(fmaf(s[r], c, nl[r]));
                    f[r] = h == 0 ? p : op == 1 ? f[r] + p : op == 2 ? fmaxf(f[r], p) : fminf(f[r], p);
                }
            }
            if (op == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) f[r] = f[r] / (float)H;
            }
        }
        if (key < Tn) {
            float* o = out + (((long)b * (FUSED ? 1 : H) + h0) * rows) * Tn + key;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = q0 + am_acc_row(r, lane);
                if (q < rows) o[(long)q * Tn] = f[r];
                rsum[r] += f[r];
            }
        }
    }
    if (!sums) return;                                                 // (uniform over the grid)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = rsum[r];
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m, 64);   // within the lane half: every lane ends with the same bits
        rsum[r] = v;
    }
    if ((lane & 31) == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) part[wave][am_acc_row(r, lane)] = rsum[r];
    }
    __syncthreads();
    if (threadIdx.x < 32 && q0 + (int)threadIdx.x < rows) {
        float v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < AM_WAVES; ++w) v += part[w][threadIdx.x];
        sums[(long)b * rows + q0 + threadIdx.x] = v;
    }
}

// maps: depth x [B][T][T] fused maps, sums: depth x [B][T] their row sums; out [B][T-1] = R[0, 1:] of the rollout.  LDS: v, w [T] each.
__global__ __launch_bounds__(256) void attn_rollout_kernel(const float* __restrict__ maps, const float* __restrict__ sums, int depth, int B,
                                                           int Tn, float* __restrict__ out) {
    extern __shared__ float am_lds[];
    float* v = am_lds;
    float* w = am_lds + Tn;
    const int b = blockIdx.x;
    const long mstride = (long)B * Tn * Tn, sstride = (long)B * Tn;
    {   // v = row 0 of a_{L-1}
        const float* F = maps + (long)(depth - 1) * mstride + (long)b * Tn * Tn;
        const float c0 = 1.0f / (0.5f * sums[(long)(depth - 1) * sstride + (long)b * Tn] + 0.5f);
        for (int j = threadIdx.x; j < Tn; j += blockDim.x) v[j] = c0 * (0.5f * F[j] + (j == 0 ? 0.5f : 0.f));
    }
    __syncthreads();
    for (int l = depth - 2; l >= 0; --l) {
        const float* F = maps + (long)l * mstride + (long)b * Tn * Tn;
        const float* s = sums + (long)l * sstride + (long)b * Tn;
        for (int i = threadIdx.x; i < Tn; i += blockDim.x) w[i] = v[i] * (1.0f / (0.5f * s[i] + 0.5f));
        __syncthreads();
        for (int j = threadIdx.x; j < Tn; j += blockDim.x) {
            // four partial sums over i = 4 m + t, added in a fixed order
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            int i = 0;
            for (; i + 4 <= Tn; i += 4) {
                a0 = fmaf(w[i], F[(long)i * Tn + j], a0);
                a1 = fmaf(w[i + 1], F[(long)(i + 1) * Tn + j], a1);
                a2 = fmaf(w[i + 2], F[(long)(i + 2) * Tn + j], a2);
                a3 = fmaf(w[i + 3], F[(long)(i + 3) * Tn + j], a3);
            }
            for (; i < Tn; ++i) a0 = fmaf(w[i], F[(long)i * Tn + j], a0);
            v[j] = 0.5f * ((a0 + a1) + (a2 + a3)) + 0.5f * w[j];
        }
        __syncthreads();
    }
    for (int j = 1 + threadIdx.x; j < Tn; j += blockDim.x) out[(long)b * (Tn - 1) + j - 1] = v[j];
}

// Relevance map of one block: map [B][T][T] (or NULL) = A_l; part [B][nqt][T] (or NULL) = per query tile, sum over its rows i of v[i] A_l[i][:],
// with v [B][T] (first: e_0, v not read; part NULL: v must be NULL, it is not read either).  Grid B * nqt, nqt = ceil(T / 32).
template <typename TQ, typename TD, int NB>
__global__ __launch_bounds__(256) void attn_rel_kernel(const typename AmStor<TQ>::E* __restrict__ qkv, const float* __restrict__ lse,
                                                       const typename AmStor<TD>::E* __restrict__ dout, float* __restrict__ map,
                                                       const float* __restrict__ v, float* __restrict__ part, int Tn, int H, int nqt, float c,
                                                       int first) {
    typedef typename AmStor<TQ>::E E;
    typedef typename AmStor<TD>::E ED;
    constexpr int HD = 32 * NB, EP = AmStor<TQ>::EP, EPD = AmStor<TD>::EP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int qt = blockIdx.x % nqt, b = blockIdx.x / nqt;
    const int q0 = qt * 32;
    const long hs = (long)H * HD * EP, rs = 3 * hs;                 // storage elements of one of q / k / v of a token, and of all three
    const long ds = (long)H * HD * EPD;                              // storage elements of a dO row
    const E* base = qkv + (long)b * Tn * rs;
    const int qrow = min(q0 + (lane & 31), Tn - 1);                  // (rows past the end: a valid row is read, nothing is stored)
    const E* qp = base + (long)qrow * rs;
    const ED* dp = dout + ((long)b * Tn + qrow) * ds;
    const float* lb = lse + (long)b * H * Tn;
    const int nkt = (Tn + 31) / 32;
    float vr[16];                                                    // v of the lane's 16 result rows (0 past T; v is read only with part)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = q0 + am_acc_row(r, lane);
        vr[r] = !part || q >= Tn ? 0.f : first ? (q == 0 ? 1.f : 0.f) : v[(long)b * Tn + q];
    }
    for (int kt = wave; kt < nkt; kt += AM_WAVES) {
        const int key = kt * 32 + (lane & 31);
        const E* krow = base + (long)min(key, Tn - 1) * rs + hs;
        const E* vrow = krow + hs;
        f32x16 a;
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = 0.f;
        for (int h = 0; h < H; ++h) {
            f32x16 s, g;
            {
                float qf[16 * NB], kf[16 * NB];
                am_load_frag<TQ, NB>(qp + (long)h * HD * EP, half, qf);
                am_load_frag<TQ, NB>(krow + (long)h * HD * EP, half, kf);
                s = am_scores<NB>(qf, kf);
            }
            {
                float df[16 * NB], vf[16 * NB];
                am_load_frag<TD, NB>(dp + (long)h * HD * EPD, half, df);
                am_load_frag<TQ, NB>(vrow + (long)h * HD * EP, half, vf);
                g = am_scores<NB>(df, vf);
            }
            const float* lrow = lb + (long)h * Tn;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = exp2f(fmaf(s[r], c, -lrow[min(q0 + am_acc_row(r, lane), Tn - 1)] * 1.4426950408889634f));
                a[r] += fmaxf(0.f, p * g[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = a[r] / (float)H;
        if (map && key < Tn) {
            float* o = map + (long)b * Tn * Tn + key;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = q0 + am_acc_row(r, lane);
                if (q < Tn) o[(long)q * Tn] = a[r];
            }
        }
        if (part) {                                                  // (uniform over the grid)
            float pr = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) pr = fmaf(vr[r], a[r], pr);
            pr += __shfl_xor(pr, 32, 64);                            // both halves end with the same bits
            if (half == 0 && key < Tn) part[((long)b * nqt + qt) * Tn + key] = pr;
        }
    }
}

// v [B][T] <- v + sum over the nqt tiles of part [B][nqt][T], tiles in order (first: v = e_0 before the sum); out [B][T-1] (or NULL) = v[:, 1:]
__global__ __launch_bounds__(256) void attn_rel_update_kernel(float* __restrict__ v, const float* __restrict__ part, int B, int Tn, int nqt,
                                                              int first, float* __restrict__ out) {
    const long n = (long)B * Tn;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / Tn), j = (int)(i % Tn);
        float acc = first ? (j == 0 ? 1.f : 0.f) : v[i];
        const float* p = part + (long)b * nqt * Tn + j;
        for (int t = 0; t < nqt; ++t) acc += p[(long)t * Tn];
        v[i] = acc;
        if (out && j > 0) out[(long)b * (Tn - 1) + j - 1] = acc;
    }
}

template <typename TQ, typename TD, int NB>
int launch_rel(const void* qkv, const float* lse, const void* dout, int B, int Tn, int H, float* map, const float* v, float* part, int first,
               hipStream_t st) {
    const int nqt = (Tn + 31) / 32;
    const float c = 1.0f / sqrtf((float)(32 * NB)) * 1.4426950408889634f;   // the forward kernels' scale * log2(e)
    ProfScope ps(PROF_OTHER, 4.0 * B * H * (double)Tn * Tn * 32 * NB, (double)B * Tn * Tn * 4 * (map ? 1 : 0) + (double)B * nqt * Tn * 4, st);
    MFVIT_LAUNCH((attn_rel_kernel<TQ, TD, NB>), dim3(B * nqt), dim3(64 * AM_WAVES), 0, st, (const typename AmStor<TQ>::E*)qkv, lse,
                 (const typename AmStor<TD>::E*)dout, map, v, part, Tn, H, nqt, c, first);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
template <typename TQ, typename TD>
int rel_by_hd(const void* qkv, const float* lse, const void* dout, int B, int Tn, int H, int HD, float* map, const float* v, float* part, int first,
              hipStream_t st) {
    if (HD == 32) return launch_rel<TQ, TD, 1>(qkv, lse, dout, B, Tn, H, map, v, part, first, st);
    if (HD == 64) return launch_rel<TQ, TD, 2>(qkv, lse, dout, B, Tn, H, map, v, part, first, st);
    if (HD == 96) return launch_rel<TQ, TD, 3>(qkv, lse, dout, B, Tn, H, map, v, part, first, st);
    return MFVIT_ENOSYS;
}

template <typename T, int NB>
int launch_probs(const void* qkv, const float* lse, int B, int Tn, int H, int fuse, int rows, float* out, float* sums, hipStream_t st) {
    typedef typename AmStor<T>::E E;
    const int nqt = (rows + 31) / 32;
    const float c = 1.0f / sqrtf((float)(32 * NB)) * 1.4426950408889634f;   // the forward kernels' scale * log2(e)
    ProfScope ps(PROF_OTHER, 2.0 * B * H * (double)rows * Tn * 32 * NB, (double)B * (fuse ? 1 : H) * rows * Tn * 4, st);
    if (fuse)
        MFVIT_LAUNCH((attn_probs_kernel<T, NB, true>), dim3(B * nqt), dim3(64 * AM_WAVES), 0, st, (const E*)qkv, lse, out, sums, Tn, H, rows,
                     nqt, fuse, c);
    else
        MFVIT_LAUNCH((attn_probs_kernel<T, NB, false>), dim3(B * H * nqt), dim3(64 * AM_WAVES), 0, st, (const E*)qkv, lse, out, sums, Tn, H,
                     rows, nqt, 0, c);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
template <typename T>
int probs_by_hd(const void* qkv, const float* lse, int B, int Tn, int H, int HD, int fuse, int rows, float* out, float* sums, hipStream_t st) {
    if (HD == 32) return launch_probs<T, 1>(qkv, lse, B, Tn, H, fuse, rows, out, sums, st);
    if (HD == 64) return launch_probs<T, 2>(qkv, lse, B, Tn, H, fuse, rows, out, sums, st);
    if (HD == 96) return launch_probs<T, 3>(qkv, lse, B, Tn, H, fuse, rows, out, sums, st);
    return MFVIT_ENOSYS;
}

// Per-head statistics of the probabilities (attn_stats in kernels.h has the definitions): attn_probs_kernel<T, NB, false>'s work split and
// its load / score / exp2 sequence, so P has the bits of the per-head maps, but nothing is stored: a lane keeps five f32 sums for each of its
// 16 result rows.  Order of every sum: the lane over its key tiles, ascending -> butterfly over the 32 lanes of a half -> the four waves in
// order (LDS) -> one thread per row (the quotient of distance_renorm) -> double from here on: the rows of the tile in order -> (finish kernel)
// the tiles in order, then the 1 / (T - 1) or 1 / T factor.  Grid nblk * B * H * nqt; block l's tensors lie l * stride bytes behind block 0's.
// part [nblk][B][H][nqt][6] double.  LDS: 4 x 5 x 32 floats + 6 x 32 doubles = 4 KB, and the distance table, (2 gh - 1)(2 gw - 1) floats.
constexpr int AS_NSTAT = 6, AS_NSUM = 5;
// The distances come from an LDS table over (dy, dx), tab[(dy + gh - 1) * (2 gw - 1) + dx + gw - 1] = patch * sqrtf((float)(dy^2 + dx^2)), filled once per
// workgroup: a key's share of the index once per key tile, a row's once per workgroup, one subtraction and one LDS read per element.  TAB = false (a
// grid whose table does not fit): the same expression per element.
constexpr size_t AS_TAB_MAX = 60 * 1024;       // (with the 4 KB above: inside 64 KB)
template <typename T, int NB, bool TAB>
__global__ __launch_bounds__(256) void attn_stats_kernel(const char* __restrict__ qkv0, const char* __restrict__ lse0, long qstride, long lstride,
                                                         double* __restrict__ part, int Tn, int B, int H, int nqt, int gh, int gw, float patch,
                                                         float c) {
    typedef typename AmStor<T>::E E;
    constexpr int HD = 32 * NB, EP = AmStor<T>::EP;
    extern __shared__ float as_tab[];
    __shared__ float wsum[AM_WAVES][AS_NSUM][32];
    __shared__ double rowv[AS_NSTAT][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    int bid = blockIdx.x;
    const int qt = bid % nqt;
    bid /= nqt;
    const int h = bid % H;
    bid /= H;
    const int b = bid % B, l = bid / B;
    const int q0 = qt * 32;
    const long hs = (long)H * HD * EP, rs = 3 * hs;                 // storage elements of one of q / k / v of a token, and of all three
    const E* base = (const E*)(qkv0 + (long)l * qstride) + (long)b * Tn * rs + (long)h * HD * EP;
    const float* lrow = (const float*)(lse0 + (long)l * lstride) + ((long)b * H + h) * Tn;
    const int qrow = min(q0 + (lane & 31), Tn - 1);                  // (rows past the end: a valid row is read, its sums are not counted)
    const int nkt = (Tn + 31) / 32;
    const int W = 2 * gw - 1;
    if constexpr (TAB) {
        for (int i = threadIdx.x; i < (2 * gh - 1) * W; i += blockDim.x) {
            const int dy = i / W - (gh - 1), dx = i - (i / W) * W - (gw - 1);
            as_tab[i] = patch * sqrtf((float)(dy * dy + dx * dx));
        }
        __syncthreads();
    }
    // once per workgroup: the q fragment, -lse of the lane's 16 result rows in log2 units, and the rows' grid coordinates (the cls row and rows
    // past the end take a patch's: their distance sums are not counted)
    float qf[16 * NB], nl[16];
    int qy[TAB ? 1 : 16], qx[16];                                    // TAB: qx = the row's share of the table index
    am_load_frag<T, NB>(base + (long)qrow * rs, half, qf);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = min(q0 + am_acc_row(r, lane), Tn - 1);
        nl[r] = -lrow[q] * 1.4426950408889634f;
        const int qp = max(q, 1) - 1, y = qp / gw, x = qp - y * gw;
        if constexpr (TAB) qx[r] = (y + gh - 1) * W + x + gw - 1;
        else { qy[r] = y; qx[r] = x; }
    }
    float sd[16], sp[16], se[16], s0[16], sq[16];                    // sum P d, sum P (patch keys); sum P (-log2 P); P at key 0; P at key == query
#pragma unroll
    for (int r = 0; r < 16; ++r) sd[r] = sp[r] = se[r] = s0[r] = sq[r] = 0.f;
    for (int kt = wave; kt < nkt; kt += AM_WAVES) {
        const int key = kt * 32 + (lane & 31);
        float kf[16 * NB];
        am_load_frag<T, NB>(base + (long)min(key, Tn - 1) * rs + hs, half, kf);
        const f32x16 s = am_scores<NB>(qf, kf);
        const int kp = max(min(key, Tn - 1), 1) - 1, ky = kp / gw, kx = kp - ky * gw, kidx = ky * W + kx;
        auto dist = [&](int r) __attribute__((always_inline)) {
            if constexpr (TAB) return as_tab[qx[r] - kidx];
            else {
                const int dy = qy[r] - ky, dx = qx[r] - kx;
                return patch * sqrtf((float)(dy * dy + dx * dx));
            }
        };
        if (kt == 0 || kt == qt || kt == nkt - 1) {                  // (uniform) the tile with key 0, the diagonal tile, the tile with keys past T
            const bool kin = key < Tn, kpatch = kin && key >= 1;     // keys at or past T contribute nothing
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = fmaf(s[r], c, nl[r]);                // log2 P
                const float p = exp2f(e);
                const float pk = kin ? p : 0.f, pp = kpatch ? p : 0.f;
                sd[r] += pp * dist(r);
                sp[r] += pp;
                se[r] += pk * (-e);
                s0[r] += key == 0 ? p : 0.f;
                sq[r] += key == q0 + am_acc_row(r, lane) ? pk : 0.f;
            }
        } else {                                                     // patch keys inside T, off the diagonal: three sums
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = fmaf(s[r], c, nl[r]);
                const float p = exp2f(e);
                sd[r] += p * dist(r);
                sp[r] += p;
                se[r] += p * (-e);
            }
        }
    }
    auto reduce = [&](float (&a)[16], int k) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = a[r];
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m, 64);   // within the lane half: every lane ends with the same bits
            if ((lane & 31) == 0) wsum[wave][k][am_acc_row(r, lane)] = v;
        }
    };
    reduce(sd, 0); reduce(sp, 1); reduce(se, 2); reduce(s0, 3); reduce(sq, 4);
    __syncthreads();
    if (threadIdx.x < 32) {
        const int t = threadIdx.x, q = q0 + t;
        float v[AS_NSUM];
#pragma unroll
        for (int k = 0; k < AS_NSUM; ++k) {
            v[k] = wsum[0][k][t];
#pragma unroll
            for (int w = 1; w < AM_WAVES; ++w) v[k] += wsum[w][k][t];
        }
        const bool in = q < Tn, prow = in && q >= 1;                 // rows at or past T are not counted; the distances and cls_mass skip the cls row
        const double ent = (double)v[2] * 0.6931471805599453;        // nats
        rowv[0][t] = prow ? (double)v[0] : 0.0;
        rowv[1][t] = prow && v[1] > 0.f ? (double)v[0] / (double)v[1] : 0.0;
        rowv[2][t] = in ? ent : 0.0;
        rowv[3][t] = q == 0 ? ent : 0.0;
        rowv[4][t] = prow ? (double)v[3] : 0.0;
        rowv[5][t] = in ? (double)v[4] : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < AS_NSTAT) {
        double acc = 0.0;
        for (int i = 0; i < 32; ++i) acc += rowv[threadIdx.x][i];
        part[(long)blockIdx.x * AS_NSTAT + threadIdx.x] = acc;
    }
}

// stats [n][6] = the nqt tile partials of part [n][nqt][6] in tile order, over T - 1 (stats 0, 1, 4), 1 (stat 3) or T (stats 2, 5)
__global__ __launch_bounds__(256) void attn_stats_finish_kernel(const double* __restrict__ part, double* __restrict__ stats, long n, int nqt, int Tn) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n * AS_NSTAT) return;
    const long g = i / AS_NSTAT;
    const int k = (int)(i % AS_NSTAT);
    const double* p = part + g * nqt * AS_NSTAT + k;
    double acc = 0.0;
    for (int t = 0; t < nqt; ++t) acc += p[(long)t * AS_NSTAT];
    stats[i] = acc / (double)(k == 3 ? 1 : (k == 2 || k == 5) ? Tn : Tn - 1);
}

template <typename T, int NB>
int launch_stats(const void* qkv, const float* lse, long qstride, long lstride, int nblk, int B, int Tn, int H, int gh, int gw, float patch,
                 double* stats, double* part, hipStream_t st) {
    const int nqt = (Tn + 31) / 32;
    const long n = (long)nblk * B * H;
    const float c = 1.0f / sqrtf((float)(32 * NB)) * 1.4426950408889634f;   // the forward kernels' scale * log2(e)
    ProfScope ps(PROF_OTHER, 2.0 * n * (double)Tn * Tn * 32 * NB, (double)n * nqt * AS_NSTAT * 16 + (double)n * AS_NSTAT * 8, st);
    const size_t tab = (size_t)(2 * (long)gh - 1) * (2 * (long)gw - 1) * 4;    // (gh * gw < 2^31: no overflow)
    if (tab <= AS_TAB_MAX)
        MFVIT_LAUNCH((attn_stats_kernel<T, NB, true>), dim3((unsigned)(n * nqt)), dim3(64 * AM_WAVES), tab, st, (const char*)qkv, (const char*)lse,
                     qstride, lstride, part, Tn, B, H, nqt, gh, gw, patch, c);
    else
        MFVIT_LAUNCH((attn_stats_kernel<T, NB, false>), dim3((unsigned)(n * nqt)), dim3(64 * AM_WAVES), 0, st, (const char*)qkv, (const char*)lse,
                     qstride, lstride, part, Tn, B, H, nqt, gh, gw, patch, c);
    MFVIT_CHECK_LAUNCH();
    MFVIT_LAUNCH(attn_stats_finish_kernel, dim3((unsigned)((n * AS_NSTAT + 255) / 256)), dim3(256), 0, st, (const double*)part, stats, n, nqt, Tn);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
template <typename T>
int stats_by_hd(const void* qkv, const float* lse, long qstride, long lstride, int nblk, int B, int Tn, int H, int HD, int gh, int gw, float patch,
                double* stats, double* part, hipStream_t st) {
    if (HD == 32) return launch_stats<T, 1>(qkv, lse, qstride, lstride, nblk, B, Tn, H, gh, gw, patch, stats, part, st);
    if (HD == 64) return launch_stats<T, 2>(qkv, lse, qstride, lstride, nblk, B, Tn, H, gh, gw, patch, stats, part, st);
    if (HD == 96) return launch_stats<T, 3>(qkv, lse, qstride, lstride, nblk, B, Tn, H, gh, gw, patch, stats, part, st);
    return MFVIT_ENOSYS;
}

}  // namespace

size_t attn_stats_work_bytes(int nblk, int B, int Tn, int H) {
    if (nblk < 1 || B < 1 || Tn < 2 || H < 1) return 0;
    const double n = (double)nblk * B * H * ((Tn + 31) / 32);
    return n > 2147483647.0 ? 0 : (size_t)n * AS_NSTAT * sizeof(double);
}

int attn_stats(int qdt, const void* qkv, const float* lse, long qstride, long lstride, int nblk, int B, int Tn, int H, int HD, int gh, int gw,
               float patch, double* stats, void* work, size_t work_bytes, hipStream_t st) {
    if (!qkv || !lse || !stats || !work || nblk < 1 || B < 1 || H < 1 || gh < 1 || gw < 1) return MFVIT_EINVAL;
    if ((long)gh * gw + 1 != (long)Tn || (qstride & 15) || (lstride & 15)) return MFVIT_EINVAL;
    if (((size_t)qkv & 15) || ((size_t)lse & 3) || ((size_t)stats & 7) || ((size_t)work & 7)) return MFVIT_EINVAL;
    const size_t need = attn_stats_work_bytes(nblk, B, Tn, H);      // (0: a grid above 2^31 - 1)
    if (!need || work_bytes < need) return MFVIT_EINVAL;
    double* part = (double*)work;
    switch (qdt) {
        case MFVIT_F32: return stats_by_hd<float>(qkv, lse, qstride, lstride, nblk, B, Tn, H, HD, gh, gw, patch, stats, part, st);
        case MFVIT_BF16: return stats_by_hd<bf16>(qkv, lse, qstride, lstride, nblk, B, Tn, H, HD, gh, gw, patch, stats, part, st);
        case MFVIT_F16: return stats_by_hd<f16>(qkv, lse, qstride, lstride, nblk, B, Tn, H, HD, gh, gw, patch, stats, part, st);
        case MFVIT_BF16X3: return stats_by_hd<sbf16>(qkv, lse, qstride, lstride, nblk, B, Tn, H, HD, gh, gw, patch, stats, part, st);
        case MFVIT_X3F16: return stats_by_hd<sf16>(qkv, lse, qstride, lstride, nblk, B, Tn, H, HD, gh, gw, patch, stats, part, st);
        default: return MFVIT_EINVAL;
    }
}

int attn_probs(int qdt, const void* qkv, const float* lse, int B, int Tn, int H, int HD, int fuse, int cls_only, float* out, float* sums,
               hipStream_t st) {
    if (!qkv || !lse || !out || B <= 0 || Tn <= 0 || H <= 0 || fuse < 0 || fuse > 3 || (sums && !fuse)) return MFVIT_EINVAL;
    const int rows = cls_only ? 1 : Tn;
    switch (qdt) {
        case MFVIT_F32: return probs_by_hd<float>(qkv, lse, B, Tn, H, HD, fuse, rows, out, sums, st);
        case MFVIT_BF16: return probs_by_hd<bf16>(qkv, lse, B, Tn, H, HD, fuse, rows, out, sums, st);
        case MFVIT_F16: return probs_by_hd<f16>(qkv, lse, B, Tn, H, HD, fuse, rows, out, sums, st);
        case MFVIT_BF16X3: return probs_by_hd<sbf16>(qkv, lse, B, Tn, H, HD, fuse, rows, out, sums, st);
        case MFVIT_X3F16: return probs_by_hd<sf16>(qkv, lse, B, Tn, H, HD, fuse, rows, out, sums, st);
        default: return MFVIT_EINVAL;
    }
}

int attn_rollout(const float* maps, const float* sums, int depth, int B, int Tn, float* out, hipStream_t st) {
    if (!maps || !sums || !out || depth <= 0 || B <= 0 || Tn < 2) return MFVIT_EINVAL;
    const size_t bytes = 2 * (size_t)Tn * 4;
    if (bytes > 64 * 1024) return MFVIT_ENOSYS;
    ProfScope ps(PROF_OTHER, 2.0 * depth * B * (double)Tn * Tn, 4.0 * depth * B * (double)Tn * Tn, st);
    MFVIT_LAUNCH(attn_rollout_kernel, dim3(B), dim3(256), bytes, st, maps, sums, depth, B, Tn, out);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int attn_rel_map(int qdt, int ddt, const void* qkv, const float* lse, const void* dout, int B, int Tn, int H, int HD, float* map, const float* v,
                 float* part, int first, hipStream_t st) {
    if (!qkv || !lse || !dout || B <= 0 || Tn <= 0 || H <= 0 || (!map && !part) || (part && !first && !v) || (!part && v))
        return MFVIT_EINVAL;
    // (qkv tag, dO tag) pairs of the encoder: the qkv of a split-bf16 encoder may be split fp16 (attn_qkv_dtype), its dO stays split bf16
    if (qdt == MFVIT_F32 && ddt == MFVIT_F32) return rel_by_hd<float, float>(qkv, lse, dout, B, Tn, H, HD, map, v, part, first, st);
    if (qdt == MFVIT_BF16 && ddt == MFVIT_BF16) return rel_by_hd<bf16, bf16>(qkv, lse, dout, B, Tn, H, HD, map, v, part, first, st);
    if (qdt == MFVIT_F16 && ddt == MFVIT_F16) return rel_by_hd<f16, f16>(qkv, lse, dout, B, Tn, H, HD, map, v, part, first, st);
    if (qdt == MFVIT_BF16X3 && ddt == MFVIT_BF16X3) return rel_by_hd<sbf16, sbf16>(qkv, lse, dout, B, Tn, H, HD, map, v, part, first, st);
    if (qdt == MFVIT_X3F16 && ddt == MFVIT_BF16X3) return rel_by_hd<sf16, sbf16>(qkv, lse, dout, B, Tn, H, HD, map, v, part, first, st);
    return MFVIT_EINVAL;
}

int attn_rel_update(float* v, const float* part, int B, int Tn, int first, float* out, hipStream_t st) {
    if (!v || !part || B <= 0 || Tn < 2) return MFVIT_EINVAL;
    const int nqt = (Tn + 31) / 32;
    const long n = (long)B * Tn;
    const int grid = (n + 255) / 256 < 2048 ? (int)((n + 255) / 256) : 2048;
    ProfScope ps(PROF_OTHER, (double)n * nqt, (double)n * (nqt + 2) * 4, st);
    MFVIT_LAUNCH(attn_rel_update_kernel, dim3(grid), dim3(256), 0, st, v, part, B, Tn, nqt, first, out);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // namespace mfvit
