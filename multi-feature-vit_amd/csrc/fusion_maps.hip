// Cross-stream relevance of the Fus_CrossViT exchange (mfvit_bimodal_relevance, include/mfvit.h): Chefer, Gur & Wolf 2021, the self-attention
// rule inside each encoder and the co-attention rule across the exchange, for one exchange layer with cls pooling.
//
// Per image and stream s, from the encoder's relevance maps A^s_l [L_s][B][T][T] (mfvit_vit_backward_rel) and the exchange's gradient-weighted
// maps Abar [2][B][T] (mfvit_fusion_ex_grad_attention; direction d = s is the one whose query is stream s's cls token):
//   R_s = (I + A^s_{L-1}) ... (I + A^s_0),   r_s = R_s[0, :],   n_s = R_s 1 - 1 (the row sums of R_s - I),
//   Rbar_s = the rows of R_s - I normalised to sum 1, plus I (a row with n_s[j] <= 0 is e_j),
//   own     = (1 + Abar^s[0]) r_s[1:]                                    cls of s -> patches of s (self rule on the own-cls key)
//   cross   = Rbar_o[0,0] (what R_s - what + w)[1:]                      cls of o -> patches of s (co-attention rule, = Rbar_o[0,0] w Rbar_s)
//             w = (0, Abar^o[1:]),  what[j] = w[j] / n_s[j]  (0 where n_s[j] <= 0),  o = the other stream.
// One workgroup per (image, stream), three chains over its vectors in LDS, every vector held as its DIFFERENCE from the chain's start so that
// nothing is ever formed as 1 + small - 1:
//   pass 1, blocks 0 .. L-1 (a column chain):  n <- n + A_l (1 + n),  n = 0: a wave per row i, lanes over j
//   pass 2, blocks L-1 .. 0 (two row chains, one read of A_l):  v <- v + (e_0 + v) A_l,  v = 0  (= r_s - e_0)
//                                                               x <- x + (what + x) A_l,  x = 0  (= what R_s - what)
//           a thread per column j (8 columns per thread beyond 1024 tokens); below 1024 tokens the rows are split over 1024 / roundup64(T)
//           thread groups whose partial sums are added in group order.
// Stream s cannot know Rbar_o[0,0]: it leaves its own Rbar_s[0,0] = v[0] / n[0] + 1 in the scratch, and a second, elementwise launch scales
// the two cross rows.  No atomics: repeated calls return the same bits.
#include "common.cuh"
#include "kernels.h"
#include "prof.h"

namespace mfvit {

namespace {

constexpr int BM_THREADS = 1024, BM_JPT = 8, BM_MAX_T = BM_THREADS * BM_JPT;

// out4 [4][B][T-1] = (cc, ce, ec, ee); stream 0 (cxr) writes cc and the unscaled ec, stream 1 (enh) ee and the unscaled ce; s00 [2][B].
// LDS: b0[T] | b1[T] | b2[T] | part[2][G][TJ] (2048 floats)
__global__ __launch_bounds__(BM_THREADS) void bimodal_chain_kernel(const float* __restrict__ maps_c, const float* __restrict__ maps_e, int depth_c,
                                                                   int depth_e, int B, int T, const float* __restrict__ abar,
                                                                   float* __restrict__ out4, float* __restrict__ s00) {
    extern __shared__ float bm_lds[];
    float* b0 = bm_lds;
    float* b1 = b0 + T;
    float* b2 = b1 + T;
    float* part = b2 + T;
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int depth = s == 0 ? depth_c : depth_e;
    const float* maps = s == 0 ? maps_c : maps_e;
    const long tt = (long)T * T;
    const float* a_own = abar + ((long)s * B + b) * T;          // direction s: the query is this stream's cls token
    const float* a_oth = abar + ((long)(1 - s) * B + b) * T;    // direction 1 - s: the other cls token reads this stream's patches
    // ---- pass 1: n = R 1 - 1
    float* cur = b0;
    float* nxt = b1;
    for (int j = tid; j < T; j += BM_THREADS) cur[j] = 0.f;
    __syncthreads();
    for (int l = 0; l < depth; ++l) {
        const float* F = maps + ((long)l * B + b) * tt;
        for (int i = wave; i < T; i += BM_THREADS / 64) {
            const float* row = F + (long)i * T;
            float s0 = 0.f, s1 = 0.f;
            for (int j = lane; j < T; j += 64) { const float a = row[j]; s0 += a; s1 = fmaf(a, cur[j], s1); }
            const float tot = wave_sum(s0 + s1);
            if (lane == 0) nxt[i] = cur[i] + tot;
        }
        __syncthreads();
        float* t = cur; cur = nxt; nxt = t;
    }
    const float n0 = cur[0];
    for (int j = tid; j < T; j += BM_THREADS) {
        const float nj = cur[j];
        b2[j] = j >= 1 && nj > 0.f ? a_oth[j] / nj : 0.f;       // what
    }
    __syncthreads();
    for (int j = tid; j < T; j += BM_THREADS) { b0[j] = 0.f; b1[j] = 0.f; }
    __syncthreads();
    // ---- pass 2: v = r - e_0 (b0), x = what R - what (b1)
    const int TJ = T >= BM_THREADS ? BM_THREADS : (T + 63) & ~63, G = BM_THREADS / TJ;
    const int jj = tid % TJ, g = tid / TJ;
    const int S = (T + G - 1) / G;
    const int i0 = g < G ? g * S : T, i1 = g < G ? (i0 + S < T ? i0 + S : T) : T;
    for (int l = depth - 1; l >= 0; --l) {
        const float* F = maps + ((long)l * B + b) * tt;
        float av[BM_JPT], ax[BM_JPT];
#pragma unroll
        for (int k = 0; k < BM_JPT; ++k) {
            const int j = jj + TJ * k;
            av[k] = g == 0 && j < T ? F[j] : 0.f;               // the e_0 term: row 0 of A_l
            ax[k] = 0.f;
        }
        for (int i = i0; i < i1; ++i) {
            const float vi = b0[i], xi = b1[i] + b2[i];
            const float* row = F + (long)i * T;
#pragma unroll
            for (int k = 0; k < BM_JPT; ++k) {
                const int j = jj + TJ * k;
                if (j < T) { const float a = row[j]; av[k] = fmaf(vi, a, av[k]); ax[k] = fmaf(xi, a, ax[k]); }
            }
        }
        if (G > 1 && g < G) { part[(2 * g) * TJ + jj] = av[0]; part[(2 * g + 1) * TJ + jj] = ax[0]; }    // (T <= TJ: column jj only)
        __syncthreads();
        if (G > 1) {
            if (g == 0 && jj < T) {
                float sv = part[jj], sx = part[TJ + jj];
                for (int g2 = 1; g2 < G; ++g2) { sv += part[(2 * g2) * TJ + jj]; sx += part[(2 * g2 + 1) * TJ + jj]; }
                b0[jj] += sv; b1[jj] += sx;
            }
        } else if (g == 0) {
#pragma unroll
            for (int k = 0; k < BM_JPT; ++k) {
                const int j = jj + TJ * k;
                if (j < T) { b0[j] += av[k]; b1[j] += ax[k]; }
            }
        }
        __syncthreads();
    }
    float* own = out4 + ((long)(s == 0 ? 0 : 3) * B + b) * (T - 1);
    float* cross = out4 + ((long)(s == 0 ? 2 : 1) * B + b) * (T - 1);
    const float c_own = 1.f + a_own[0];
    for (int j = 1 + tid; j < T; j += BM_THREADS) {
        own[j - 1] = c_own * b0[j];
        cross[j - 1] = b1[j] + a_oth[j];
    }
    if (tid == 0) s00[(long)s * B + b] = n0 > 0.f ? b0[0] / n0 + 1.f : 1.f;
}

// ce [B][T-1] *= Rbar_c[0,0] = s00[0][b];  ec [B][T-1] *= Rbar_e[0,0] = s00[1][b]
__global__ __launch_bounds__(256) void bimodal_scale_kernel(float* __restrict__ out4, const float* __restrict__ s00, int B, int T) {
    const long per = (long)B * (T - 1), n = 2 * per;
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const int which = (int)(i / per);                            // 0: ce (slot 1, scaled by stream 0's), 1: ec (slot 2, by stream 1's)
    const long r = i - which * per;
    const int b = (int)(r / (T - 1));
    float* o = out4 + (long)(1 + which) * per + r;
    *o = *o * s00[(long)which * B + b];
}

bool bimodal_ok(int B, int T, int depth_c, int depth_e) { return B > 0 && T >= 2 && T <= BM_MAX_T && depth_c > 0 && depth_e > 0; }

}  // namespace

}  // namespace mfvit

using namespace mfvit;

extern "C" {

size_t mfvit_bimodal_relevance_scratch_bytes(int B, int T) {
    return bimodal_ok(B, T, 1, 1) ? ((size_t)2 * B * 4 + 255) & ~(size_t)255 : 0;
}

int mfvit_bimodal_relevance(int B, int T, int depth_c, int depth_e, const float* maps_c, const float* maps_e, const float* abar, float* out4,
                            void* scratch, mfvit_stream_t stream) {
    if (!bimodal_ok(B, T, depth_c, depth_e) || !maps_c || !maps_e || !abar || !out4 || !scratch) return MFVIT_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)3 * T + 2 * BM_THREADS) * 4;     // at most 104 KB
    static PerDeviceOnce attr;
    if (attr.first()) (void)hipFuncSetAttribute((const void*)bimodal_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const double cells = (double)(depth_c + depth_e) * B * (double)T * T;
    ProfScope ps(PROF_OTHER, 6.0 * cells, 2.0 * 4.0 * cells, st);
    MFVIT_LAUNCH(bimodal_chain_kernel, dim3(B, 2), dim3(BM_THREADS), lds, st, maps_c, maps_e, depth_c, depth_e, B, T, abar, out4, (float*)scratch);
    MFVIT_CHECK_LAUNCH();
    const long n = 2L * B * (T - 1);
    MFVIT_LAUNCH(bimodal_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out4, (const float*)scratch, B, T);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // extern "C"
