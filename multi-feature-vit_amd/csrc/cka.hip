// Minibatch linear CKA (Kornblith et al. 2019; the minibatch estimator of Nguyen, Raghu & Kornblith 2021; mfvit.similarity drives it): the centred
// Gram matrices of a stack of representations and the HSIC sums between two stacks.
//   gram_kernel         one workgroup per (representation, split of the column range).  A stage of GRAM_STAGE columns of ALL n rows is read once
//                       from memory into LDS, column-major (a column's rows are contiguous: the MFMA operand reads of 32 consecutive rows touch 32
//                       banks), each column's f32 mean over the n rows is taken there in a fixed order and subtracted, and the upper triangle of
//                       32 x 32 tiles is multiplied on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation over the whole split).  Rows >= n
//                       and columns >= k are zero AFTER the centring (they are never centred), so they add exactly nothing.  The partial tiles leave
//                       as plain stores.
//   gram_reduce_kernel  adds the splits' partial tiles in double, in split order, and writes both triangles from the one sum.
//   hsic_kernel         one workgroup per output element: the three sums of the HSIC estimators in double, thread a owns row a (read as column a:
//                       the Gram matrices are symmetric to the bit), a fixed tree over the rows, one read-modify-write of the accumulator.
// Why centre in LDS: residual-stream features carry a large common component; an f32 raw Gram loses the CKA signal to cancellation.  Both
// HSIC estimators are exactly invariant to the per-column shift.  No atomics anywhere; the plan is a function of (n, k) only, so a representation has
// the same bits whatever else is computed in the same call.
#include "gemm.cuh"
#include "kernels.h"

namespace mfvit {

namespace {

constexpr int GRAM_STAGE = 64;         // columns per LDS stage
constexpr int GRAM_MAX_SPLITS = 64;    // splits of the column range (the grid's x extent)
constexpr int GRAM_MIN_STAGES = 4;     // a split is at least this many stages long (but for the last one)
constexpr int GRAM_MAX_REPS = 64;

struct GramPlan { int splits; long cps, last; };
GramPlan gram_plan(long k) {
    const long stages = (k + GRAM_STAGE - 1) / GRAM_STAGE;
    long sps = (stages + GRAM_MAX_SPLITS - 1) / GRAM_MAX_SPLITS;
    if (sps < GRAM_MIN_STAGES) sps = GRAM_MIN_STAGES;
    GramPlan p;
    p.splits = (int)((stages + sps - 1) / sps);
    p.cps = sps * GRAM_STAGE;
    p.last = k - (long)(p.splits - 1) * p.cps;
    return p;
}
bool gram_shape_ok(int reps, int n, long k) { return reps >= 1 && reps <= GRAM_MAX_REPS && n >= 2 && n <= MFVIT_GRAM_MAX_N && k >= 1; }
int gram_tiles(int n) { const int nt = (n + 31) / 32; return nt * (nt + 1) / 2; }

// tile t of the upper triangle, rows of tiles in order: (0,0) (0,1) .. (0,NT-1) (1,1) ..
__device__ __forceinline__ void tile_coords(int t, int nt, int& I, int& J) {
    I = 0;
    while (t >= nt - I) { t -= nt - I; ++I; }
    J = I + t;
}

template <int NT>
__global__ __launch_bounds__(256, 2) void gram_kernel(const float* __restrict__ x, long rep_stride, long ld, int n, long k, long cps,
                                                   float* __restrict__ work) {
    constexpr int NP = NT * 32, NPS = NP + 1, NTILE = NT * (NT + 1) / 2, SLOTS = (NTILE + 3) / 4;
    extern __shared__ float sm[];                       // [GRAM_STAGE][NPS] stage, column-major; [4][GRAM_STAGE] partial column sums
    float* const part = sm + GRAM_STAGE * NPS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, rep = blockIdx.y, splits = gridDim.x;
    const float* const xr = x + (long)rep * rep_stride;
    const long c_begin = (long)s * cps, c_end = c_begin + cps < k ? c_begin + cps : k;
    int ti[SLOTS], tj[SLOTS];
    f32x16 acc[SLOTS];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int t = wave + 4 * sl;
        tile_coords(t < NTILE ? t : 0, NT, ti[sl], tj[sl]);
        ti[sl] *= 32; tj[sl] *= 32;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[sl][i] = 0.f;
    }
    for (long c0 = c_begin; c0 < c_end; c0 += GRAM_STAGE) {
        __syncthreads();                                // the last stage's operand reads are done
        // 16 lanes read the 256 bytes of a row's stage; rows >= n and columns >= k are zero
#pragma unroll 4
        for (int u = 0; u < NP * 16 / 256; ++u) {
            const int idx = u * 256 + tid, row = idx >> 4, q = (idx & 15) * 4;
            const long col = c0 + q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < n) {
                const float* p = xr + (long)row * ld + col;
                if (col + 4 <= c_end) {
                    v = *(const float4*)p;
                } else {                                // the tail of the column range: nothing past column k - 1 is read
                    if (col < c_end) v.x = p[0];
                    if (col + 1 < c_end) v.y = p[1];
                    if (col + 2 < c_end) v.z = p[2];
                }
            }
            float* d = sm + q * NPS + row;
            d[0] = v.x; d[NPS] = v.y; d[2 * NPS] = v.z; d[3 * NPS] = v.w;
        }
        __syncthreads();
        // column means: wave p sums rows p, p + 4, .. of column `lane` in ascending order; the four partials are added as (p0 + p1) + (p2 + p3)
        float* const colp = sm + lane * NPS;
        {
            float a = 0.f;
            for (int row = wave; row < n; row += 4) a = __fadd_rn(a, colp[row]);
            part[wave * GRAM_STAGE + lane] = a;
        }
        __syncthreads();
        {
            const float tot = __fadd_rn(__fadd_rn(part[lane], part[GRAM_STAGE + lane]), __fadd_rn(part[2 * GRAM_STAGE + lane], part[3 * GRAM_STAGE + lane]));
            const float m = __fdiv_rn(tot, (float)n);
            if (c0 + lane < c_end)                      // (a column past the end stays zero: never centred)
                for (int row = wave; row < n; row += 4) colp[row] = __fsub_rn(colp[row], m);
        }
        __syncthreads();
        // lanes 0 - 31 hold column kk of 32 rows, lanes 32 - 63 column kk + 1
        const float* cp = sm + (lane >> 5) * NPS + (lane & 31);
#pragma unroll 4
        for (int kk = 0; kk < GRAM_STAGE; kk += 2, cp += 2 * NPS) {
#pragma unroll
            for (int sl = 0; sl < SLOTS; ++sl)
                if (wave + 4 * sl < NTILE) acc[sl] = __builtin_amdgcn_mfma_f32_32x32x2f32(cp[ti[sl]], cp[tj[sl]], acc[sl], 0, 0, 0);
        }
    }
    float* const w = work + (long)(rep * splits + s) * NTILE * 1024;
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int t = wave + 4 * sl;
        if (t < NTILE) {
#pragma unroll
            for (int i = 0; i < 16; ++i) w[t * 1024 + acc_row(i, lane) * 32 + (lane & 31)] = acc[sl][i];
        }
    }
}

__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ work, double* __restrict__ g, int n, int nt, int splits) {
    const int t = blockIdx.x, rep = blockIdx.y, ntile = nt * (nt + 1) / 2;
    int I, J;
    tile_coords(t, nt, I, J);
    const float* w = work + ((long)rep * splits * ntile + t) * 1024;
    double* gr = g + (long)rep * n * n;
    for (int e = threadIdx.x; e < 1024; e += 256) {
        const int ii = e >> 5, jj = e & 31, i = I * 32 + ii, j = J * 32 + jj;
        if (i >= n || j >= n || (I == J && ii > jj)) continue;     // a diagonal tile: its upper half, mirrored
        double a = 0.0;
        for (int s = 0; s < splits; ++s) a += (double)w[(long)s * ntile * 1024 + e];
        gr[(long)i * n + j] = a;
        gr[(long)j * n + i] = a;
    }
}

// fixed tree over 256 slots of four double arrays; the totals end in slot 0
__device__ __forceinline__ void tree4(double* r, int tid) {
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q * 256 + tid] += r[q * 256 + tid + h];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void hsic_kernel(const double* __restrict__ ga, int ra, const double* __restrict__ gb, int rb, int n, int unbiased,
                                                   double* acc_ab, double* acc_aa, double* acc_bb) {
    __shared__ double red[4 * 256];
    const int tid = threadIdx.x;
    int id = blockIdx.x;
    const double *K, *L;
    double* out;
    if (id < ra * rb) { K = ga + (long)(id / rb) * n * n; L = gb + (long)(id % rb) * n * n; out = acc_ab + id; }
    else if ((id -= ra * rb) < ra) { K = L = ga + (long)id * n * n; out = acc_aa + id; }
    else { id -= ra; K = L = gb + (long)id * n * n; out = acc_bb + id; }
    double s1 = 0.0, rk = 0.0, rl = 0.0;
    if (tid < n) {
        for (int b = 0; b < n; ++b) {                  // row tid, read as column tid (symmetric to the bit): b ascending
            if (unbiased && b == tid) continue;
            const double kv = K[(long)b * n + tid], lv = L[(long)b * n + tid];
            s1 += kv * lv; rk += kv; rl += lv;
        }
    }
    red[tid] = s1; red[256 + tid] = rk; red[512 + tid] = rl; red[768 + tid] = rk * rl;
    tree4(red, tid);
    if (tid == 0) {
        const double S1 = red[0], sK = red[256], sL = red[512], S3 = red[768], N = (double)n;
        const double h = unbiased ? (S1 + sK * sL / ((N - 1.0) * (N - 2.0)) - 2.0 / (N - 2.0) * S3) / (N * (N - 3.0))
                                  : (S1 + sK * sL / (N * N) - 2.0 / N * S3) / ((N - 1.0) * (N - 1.0));
        *out += h;
    }
}

template <int NT> int launch_gram(const float* x, long rep_stride, long ld, int reps, int n, long k, const GramPlan& pl, float* work, hipStream_t st) {
    constexpr int lds = (GRAM_STAGE * (NT * 32 + 1) + 4 * GRAM_STAGE) * 4;
    // (at every launch: a host-side setting of a microsecond, and a call that failed once is not remembered as done)
    if (hipFuncSetAttribute((const void*)gram_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return MFVIT_ELAUNCH;
    MFVIT_LAUNCH(gram_kernel<NT>, dim3(pl.splits, reps), dim3(256), lds, st, x, rep_stride, ld, n, k, pl.cps, work);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // namespace

extern "C" {

int mfvit_gram_plan(int n, int64_t k, int32_t plan[4]) {
    if (!plan || !gram_shape_ok(1, n, k)) return MFVIT_EINVAL;
    const GramPlan p = gram_plan(k);
    if (p.cps > INT32_MAX || k > (int64_t)GRAM_MAX_SPLITS * INT32_MAX) return MFVIT_EINVAL;
    plan[0] = GRAM_STAGE; plan[1] = p.splits; plan[2] = (int32_t)p.cps; plan[3] = (int32_t)p.last;
    return MFVIT_OK;
}

size_t mfvit_gram_work_bytes(int reps, int n, int64_t k) {
    int32_t plan[4];
    if (!gram_shape_ok(reps, n, k) || mfvit_gram_plan(n, k, plan) != MFVIT_OK) return 0;
    return (size_t)reps * plan[1] * gram_tiles(n) * 1024 * sizeof(float);
}

int mfvit_gram_centered(const float* x, int64_t rep_stride, int64_t ld, int reps, int n, int64_t k, double* g, void* work, size_t work_bytes,
                        mfvit_stream_t stream) {
    if (!x || !g || !work || !gram_shape_ok(reps, n, k) || ld < k || (ld & 3) || (rep_stride & 3) || rep_stride < 0 || ((uintptr_t)x & 15) || ((uintptr_t)work & 3))
        return MFVIT_EINVAL;
    const size_t need = mfvit_gram_work_bytes(reps, n, k);
    if (need == 0 || work_bytes < need) return MFVIT_EINVAL;
    const GramPlan pl = gram_plan(k);
    const int nt = (n + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    switch (nt) {
        case 1: rc = launch_gram<1>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
        case 2: rc = launch_gram<2>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
        case 3: rc = launch_gram<3>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
        case 4: rc = launch_gram<4>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
        case 5: rc = launch_gram<5>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
        case 6: rc = launch_gram<6>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
        case 7: rc = launch_gram<7>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
        default: rc = launch_gram<8>(x, rep_stride, ld, reps, n, k, pl, (float*)work, st); break;
    }
    if (rc != MFVIT_OK) return rc;
    MFVIT_LAUNCH(gram_reduce_kernel, dim3(gram_tiles(n), reps), dim3(256), 0, st, (const float*)work, g, n, nt, pl.splits);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_hsic_accumulate(const double* ga, int ra, const double* gb, int rb, int n, int unbiased, double* acc_ab, double* acc_aa, double* acc_bb,
                          mfvit_stream_t stream) {
    if (!ga || !gb || !acc_ab || !acc_aa || !acc_bb || ra < 1 || ra > GRAM_MAX_REPS || rb < 1 || rb > GRAM_MAX_REPS || n > MFVIT_GRAM_MAX_N ||
        n < (unbiased ? 4 : 2))
        return MFVIT_EINVAL;
    MFVIT_LAUNCH(hsic_kernel, dim3(ra * rb + ra + rb), dim3(256), 0, (hipStream_t)stream, ga, ra, gb, rb, n, unbiased ? 1 : 0, acc_ab, acc_aa, acc_bb);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // extern "C"

}  // namespace mfvit
