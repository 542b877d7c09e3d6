// Low-rank adapters (LoRA, Hu et al. 2021) of the encoder's Linear weights on gfx950: the merge W_eff = W + s B A that the weight shadows are
// built from, and the contraction of the weight gradient dW_eff = dY^T X to the adapters' gradients dA = s B^T dW_eff, dB = s dW_eff A^T.
// f32 throughout, no MFMA: both are memory-bound passes over an [N][K] matrix (r <= 64), and the merge must add in a stated order.
// Batched over (block, target) pairs by a table that rides in the kernel arguments (LoraBatch: at most LORA_MAXP pairs per launch, blockIdx.y = pair):
// a shadow rebuild or an encoder backward issues one launch for the 24 pairs of the default targets, not 24.
// Every sum has a fixed order and nothing is accumulated by atomics: repeated calls return the same bits.
#include "../../include/mfvit.h"
#include "kernels.h"

namespace mfvit {

// ------------------------------------------------------------------ merge: out[n][k] = w[n][k] + scale * sum_j b[n][j] a[j][k]
// One thread per 16-byte piece of a row (k .. k+3): j ascending, one fmaf per term, then ONE multiply by the scale and ONE add to w.  A zero
// update leaves the bits of w (w + 0 would turn -0 into +0).  out == w: every element is read and written by the same thread.
__global__ __launch_bounds__(256) void lora_merge_kernel(LoraBatch bt) {
    const LoraPair& p = bt.pair[blockIdx.y];
    const int r = bt.r, K = p.K, K4 = K >> 2;
    const long total = (long)p.N * K4;
    const float scale = bt.scale;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / K4), k = (int)(i % K4) * 4;
        const float* __restrict__ brow = p.b + (long)n * r;
        const float* __restrict__ acol = p.a + k;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < r; ++j) {
            const float bj = brow[j];
            const float4 a4 = *(const float4*)(acol + (long)j * K);
            acc.x = fmaf(bj, a4.x, acc.x);
            acc.y = fmaf(bj, a4.y, acc.y);
            acc.z = fmaf(bj, a4.z, acc.z);
            acc.w = fmaf(bj, a4.w, acc.w);
        }
        const float4 w4 = *(const float4*)(p.w + (long)n * p.ldw + k);
        const float dx = scale * acc.x, dy = scale * acc.y, dz = scale * acc.z, dw = scale * acc.w;
        float4 o;
        o.x = dx == 0.f ? w4.x : w4.x + dx;
        o.y = dy == 0.f ? w4.y : w4.y + dy;
        o.z = dz == 0.f ? w4.z : w4.z + dz;
        o.w = dw == 0.f ? w4.w : w4.w + dw;
        *(float4*)(p.o0 + (long)n * p.ldo + k) = o;
    }
}

// ------------------------------------------------------------------ gradients: da[j][k] = scale * sum_n b[n][j] dw[n][k],  db[n][j] = scale * sum_k dw[n][k] a[j][k]
// blockIdx.x of a pair: first its ceil(K / 64) column strips of da, then its ceil(N / 32) row groups of db.
//   da: ONE workgroup owns a strip of 64 columns over ALL N rows (the choice between that and a split along n with a second stage: a strip is
//       256 contiguous bytes of every dw row, 6 - 24 strips x 24 - 72 pairs fill the chip, and no partial ever leaves the workgroup).  16 row lanes
//       x 16 column pieces; row lane i adds rows i, i + 16, ... in ascending order for 8 adapter rows j at a time, the 16 row lanes meet in LDS
//       and are added in the order 0 .. 15.
//   db: one wave per row; lane l adds the pieces l, l + 64, ... of the row's K / 4 (ascending), then an xor butterfly (32, 16, .. 1) over the wave.
constexpr int LG_STRIP = 64, LG_ROWS = 32, LG_JC = 8;
__global__ __launch_bounds__(256) void lora_grad_kernel(LoraBatch bt) {
    const LoraPair& p = bt.pair[blockIdx.y];
    const int r = bt.r, N = p.N, K = p.K;
    const float scale = bt.scale;
    const int nstrip = (K + LG_STRIP - 1) / LG_STRIP, ngroup = (N + LG_ROWS - 1) / LG_ROWS;
    const int item = blockIdx.x;
    __shared__ float4 sm[16][LG_JC][16];          // [row lane][j][column piece]: 32 KB
    if (item < nstrip) {
        const int cg = threadIdx.x & 15, rl = threadIdx.x >> 4;
        const int col = item * LG_STRIP + cg * 4;
        const bool ok = col < K;                  // (K % 4 == 0: a piece is whole or absent)
        for (int jc = 0; jc < r; jc += LG_JC) {
            float4 acc[LG_JC];
#pragma unroll
            for (int jj = 0; jj < LG_JC; ++jj) acc[jj] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                for (int n = rl; n < N; n += 16) {
                    const float4 d4 = *(const float4*)(p.w + (long)n * p.ldw + col);
                    const float* __restrict__ brow = p.b + (long)n * r + jc;
#pragma unroll
                    for (int jj = 0; jj < LG_JC; ++jj) {
                        const float bj = jc + jj < r ? brow[jj] : 0.f;
                        acc[jj].x = fmaf(bj, d4.x, acc[jj].x);
                        acc[jj].y = fmaf(bj, d4.y, acc[jj].y);
                        acc[jj].z = fmaf(bj, d4.z, acc[jj].z);
                        acc[jj].w = fmaf(bj, d4.w, acc[jj].w);
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < LG_JC; ++jj) sm[rl][jj][cg] = acc[jj];
            __syncthreads();
            if (threadIdx.x < LG_JC * 16) {
                const int jj = threadIdx.x >> 4, c2 = threadIdx.x & 15;
                const int col2 = item * LG_STRIP + c2 * 4;
                if (jc + jj < r && col2 < K) {
                    float4 s = sm[0][jj][c2];
#pragma unroll
                    for (int i = 1; i < 16; ++i) {
                        const float4 t = sm[i][jj][c2];
                        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
                    }
                    s.x *= scale; s.y *= scale; s.z *= scale; s.w *= scale;
                    *(float4*)(p.o0 + (long)(jc + jj) * K + col2) = s;
                }
            }
            __syncthreads();
        }
        return;
    }
    const int grp = item - nstrip;
    if (grp >= ngroup) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K4 = K >> 2;
    for (int i = 0; i < LG_ROWS / 4; ++i) {
        const int n = grp * LG_ROWS + wave * (LG_ROWS / 4) + i;
        if (n >= N) break;                        // (wave-uniform)
        const float* __restrict__ drow = p.w + (long)n * p.ldw;
        for (int jc = 0; jc < r; jc += LG_JC) {
            float acc[LG_JC];
#pragma unroll
            for (int jj = 0; jj < LG_JC; ++jj) acc[jj] = 0.f;
            for (int m = lane; m < K4; m += 64) {
                const float4 d4 = *(const float4*)(drow + 4 * m);
#pragma unroll
                for (int jj = 0; jj < LG_JC; ++jj) {
                    if (jc + jj < r) {
                        const float4 a4 = *(const float4*)(p.a + (long)(jc + jj) * K + 4 * m);
                        acc[jj] = fmaf(d4.x, a4.x, acc[jj]);
                        acc[jj] = fmaf(d4.y, a4.y, acc[jj]);
                        acc[jj] = fmaf(d4.z, a4.z, acc[jj]);
                        acc[jj] = fmaf(d4.w, a4.w, acc[jj]);
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < LG_JC; ++jj) {
                float s = acc[jj];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
                if (lane == 0 && jc + jj < r) p.o1[(long)n * r + jc + jj] = scale * s;
            }
        }
    }
}

// ------------------------------------------------------------------ launchers
bool lora_pair_ok(const LoraPair& p, int r, bool grad) {
    if (!p.w || !p.a || !p.b || !p.o0 || (grad && !p.o1)) return false;
    if (p.N < 1 || p.K < 4 || p.K % 4 || r < 1 || r > 64) return false;
    if (p.ldw < p.K || p.ldw % 4 || (!grad && (p.ldo < p.K || p.ldo % 4))) return false;
    // 16-byte accesses along k
    if (((size_t)p.w | (size_t)p.a | (size_t)p.o0) % 16) return false;
    return true;
}

int lora_merge_batch(const LoraPair* pairs, int n, int r, float scale, hipStream_t st) {
    for (int i = 0; i < n; ++i)
        if (!lora_pair_ok(pairs[i], r, false)) return MFVIT_EINVAL;
    for (int i0 = 0; i0 < n; i0 += LORA_MAXP) {
        LoraBatch bt;
        bt.n = n - i0 < LORA_MAXP ? n - i0 : LORA_MAXP;
        bt.r = r;
        bt.scale = scale;
        long most = 0;
        for (int i = 0; i < bt.n; ++i) {
            bt.pair[i] = pairs[i0 + i];
            const long t = (long)bt.pair[i].N * (bt.pair[i].K / 4);
            most = t > most ? t : most;
        }
        long gx = (most + 255) / 256;
        gx = gx > 1024 ? 1024 : gx;
        MFVIT_LAUNCH(lora_merge_kernel, dim3((unsigned)gx, (unsigned)bt.n), dim3(256), 0, st, bt);
        MFVIT_CHECK_LAUNCH();
    }
    return MFVIT_OK;
}

int lora_grad_batch(const LoraPair* pairs, int n, int r, float scale, hipStream_t st) {
    for (int i = 0; i < n; ++i)
        if (!lora_pair_ok(pairs[i], r, true)) return MFVIT_EINVAL;
    for (int i0 = 0; i0 < n; i0 += LORA_MAXP) {
        LoraBatch bt;
        bt.n = n - i0 < LORA_MAXP ? n - i0 : LORA_MAXP;
        bt.r = r;
        bt.scale = scale;
        int most = 0;
        for (int i = 0; i < bt.n; ++i) {
            bt.pair[i] = pairs[i0 + i];
            const int t = (bt.pair[i].K + LG_STRIP - 1) / LG_STRIP + (bt.pair[i].N + LG_ROWS - 1) / LG_ROWS;
            most = t > most ? t : most;
        }
        MFVIT_LAUNCH(lora_grad_kernel, dim3((unsigned)most, (unsigned)bt.n), dim3(256), 0, st, bt);
        MFVIT_CHECK_LAUNCH();
    }
    return MFVIT_OK;
}

}  // namespace mfvit

using namespace mfvit;

extern "C" {

int mfvit_lora_merge(const float* w, long ldw, const float* a, const float* b, float scale, float* out, long ldo, int N, int K, int r,
                     mfvit_stream_t stream) {
    if (ldw > INT_MAX || ldo > INT_MAX || ldw < 0 || ldo < 0) return MFVIT_EINVAL;
    LoraPair p = {w, a, b, out, nullptr, N, K, (int)ldw, (int)ldo};
    return lora_merge_batch(&p, 1, r, scale, (hipStream_t)stream);
}

int mfvit_lora_grad(const float* dw, long lddw, const float* a, const float* b, float scale, float* da, float* db, int N, int K, int r,
                    mfvit_stream_t stream) {
    if (lddw > INT_MAX || lddw < 0) return MFVIT_EINVAL;
    LoraPair p = {dw, a, b, da, db, N, K, (int)lddw, K};
    return lora_grad_batch(&p, 1, r, scale, (hipStream_t)stream);
}

}  // extern "C"
