// The perturbation test for patch-relevance maps (Chefer, Gur & Wolf 2021 section 4: positive / negative perturbation; Petsiuk et al. 2018: deletion /
// insertion): rank the patches of every image by relevance, remove them a fraction at a time, run the model again, score the target class.
//   patch_rank_kernel     rank[b][i] = #{j : rel[j] > rel[i], or rel[j] == rel[i] and j < i}: a total order that depends on the values and the indices only
//                         (one workgroup per image, the row as integer keys in LDS, every thread counts for its own i: no sort network, no atomics).
//   patch_perturb_kernel  out[s][b] = img[b] with the patches whose rank lies in [lo_s, hi_s) replaced by fill[c]: all S masked batches of a test in ONE
//                         launch.  A streaming kernel (moves and fills only: bit-exact), one (image, step) per blockIdx.y / z so that the range is block-uniform,
//                         16-byte accesses with one mask decision each (W % 16 == 0: an aligned group of four lies inside one patch).
//   perturb_score_kernel  per step: images whose first-maximum argmax is the target, sum of the target's softmax probability (double, max-subtracted), sum of
//                         the target's logit.  One workgroup per step, every thread walks its images in index order, then a fixed tree: the same bits on every run.
// The model forwards in between are the encoders' ordinary evaluation forwards (mfvit.perturb).
#include "kernels.h"

namespace mfvit {

namespace {

constexpr int RANK_MAXP = 8192;      // the project's token limit
constexpr int PERT_UNROLL = 4;       // vectors per thread and grid-stride step
constexpr int PERT_BLOCKS = 2048;    // grid target: 256 CUs x 8 workgroups; above it the workgroups stride over their image
constexpr int SCORE_THREADS = 256;

// Monotone integer key of a float: a > b <=> key(a) > key(b) for numbers, -0.0 and +0.0 share a key, every NaN has key 1, below -inf (0x007fffff + 1).
// Keys are >= 1, so that key - 1 never wraps and the padding key 0 is below every threshold.
__device__ __forceinline__ unsigned rank_key(float x) {
    // (integer tests on the bit pattern: subnormals keep their order whatever the denormal mode of the float compares)
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 1u;
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) + 1u;     // (the largest key, +inf, is 0xff800001: no overflow)
}

__global__ __launch_bounds__(1024) void patch_rank_kernel(const float* __restrict__ rel, long ld, int* __restrict__ rank, int P) {
    __shared__ uint4 keys4[RANK_MAXP / 4];
    unsigned* keys = (unsigned*)keys4;
    const int b = blockIdx.x;
    const float* row = rel + (long)b * ld;
    const int P4 = (P + 3) & ~3;
    for (int j = threadIdx.x; j < P4; j += blockDim.x) keys[j] = j < P ? rank_key(row[j]) : 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const unsigned ki = keys[i];
        int cnt = 0;
        // j < i counts when key_j >= key_i, i.e. key_j > key_i - 1; j > i when key_j > key_i; j == i never (every lane of a wave reads the same
        // 16 bytes: an LDS broadcast)
        for (int j = 0; j < P4; j += 4) {
            const uint4 k = keys4[j >> 2];
            cnt += k.x > (j < i ? ki - 1u : ki);
            cnt += k.y > (j + 1 < i ? ki - 1u : ki);
            cnt += k.z > (j + 2 < i ? ki - 1u : ki);
            cnt += k.w > (j + 3 < i ? ki - 1u : ki);
        }
        rank[(long)b * P + i] = cnt;
    }
}

template <int VEC> struct alignas(4 * VEC) PertPack { float v[VEC]; };

// out[s][b] for b = blockIdx.y, s = blockIdx.z; per = C * H * W / VEC packs per image, gw = W / 16, hw = H * W.
template <int VEC>
__global__ __launch_bounds__(256) void patch_perturb_kernel(const float* __restrict__ img, const int* __restrict__ rank, const int* __restrict__ steps,
                                                            const float* __restrict__ fill, float* __restrict__ out, int B, int H, int W, int per) {
    using PK = PertPack<VEC>;
    const int b = blockIdx.y, s = blockIdx.z;
    const int lo = steps[2 * s], hi = steps[2 * s + 1];
    const int gw = W >> 4, hw = H * W;
    const int* rk = rank + (long)b * ((H >> 4) * gw);
    const PK* src = (const PK*)img + (long)b * per;
    PK* dst = (PK*)out + ((long)s * B + b) * per;
    for (int p0 = blockIdx.x * (256 * PERT_UNROLL) + threadIdx.x; p0 < per; p0 += gridDim.x * (256 * PERT_UNROLL)) {
        PK r[PERT_UNROLL] = {};
        int rnk[PERT_UNROLL];
        float f[PERT_UNROLL];
        // every load first ...
#pragma unroll
        for (int u = 0; u < PERT_UNROLL; ++u) {
            const int p = p0 + u * 256;
            rnk[u] = -1;
            f[u] = 0.f;
            if (p < per) {
                const int e = p * VEC, c = e / hw, yx = e - c * hw, y = yx / W, x = yx - y * W;
                rnk[u] = rk[(y >> 4) * gw + (x >> 4)];
                f[u] = fill[c];
                r[u] = src[p];
            }
        }
        // ... then the selects and the stores
#pragma unroll
        for (int u = 0; u < PERT_UNROLL; ++u) {
            const int p = p0 + u * 256;
            if (p >= per) break;
            if (rnk[u] >= lo && rnk[u] < hi) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) r[u].v[k] = f[u];
            }
            dst[p] = r[u];
        }
    }
}

// One workgroup per step s = blockIdx.x.  A row with a non-finite logit or a target outside [0, C) is wrong and adds nothing to the sums (the target
// enters the row by a checked index: nothing outside the row is read).
__global__ __launch_bounds__(SCORE_THREADS) void perturb_score_kernel(const float* __restrict__ logits, long ld, const long* __restrict__ target, int B,
                                                                      int C, unsigned long long* __restrict__ correct, double* __restrict__ sums,
                                                                      unsigned long long* __restrict__ nonfinite) {
    __shared__ double sp[SCORE_THREADS], sl[SCORE_THREADS];
    __shared__ unsigned sc[SCORE_THREADS], sn[SCORE_THREADS];
    const int s = blockIdx.x, tid = threadIdx.x;
    double accp = 0.0, accl = 0.0;
    unsigned nc = 0, nn = 0;
    for (int b = tid; b < B; b += SCORE_THREADS) {
        const float* z = logits + ((long)s * B + b) * ld;
        float m = z[0];
        int am = 0;
        bool finite = isfinite(m);
        for (int c = 1; c < C; ++c) {
            const float v = z[c];
            finite = finite && isfinite(v);
            if (v > m) { m = v; am = c; }
        }
        const long t = target[b];
        if (!finite) { ++nn; continue; }
        if (t < 0 || t >= C) continue;
        double den = 0.0;
        for (int c = 0; c < C; ++c) den += exp((double)z[c] - (double)m);
        accp += exp((double)z[t] - (double)m) / den;
        accl += (double)z[t];
        nc += am == (int)t;
    }
    sp[tid] = accp; sl[tid] = accl; sc[tid] = nc; sn[tid] = nn;
    __syncthreads();
    for (int o = SCORE_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            sp[tid] += sp[tid + o]; sl[tid] += sl[tid + o]; sc[tid] += sc[tid + o]; sn[tid] += sn[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        correct[s] += sc[0];
        nonfinite[s] += sn[0];
        sums[2 * s] += sp[0];
        sums[2 * s + 1] += sl[0];
    }
}

// [p, p + np) and [q, q + nq) share a byte
bool pert_overlap(const void* p, unsigned long long np, const void* q, unsigned long long nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b ? b - a < np : a - b < nq;
}

}  // namespace

extern "C" {

int mfvit_patch_rank(const float* rel, int64_t ld, int32_t* rank, int B, int P, mfvit_stream_t stream) {
    if (!rel || !rank || B <= 0 || B > 65535 || P <= 0 || P > RANK_MAXP || ld < P) return MFVIT_EINVAL;
    const int threads = P <= 256 ? 256 : (P <= 512 ? 512 : 1024);
    MFVIT_LAUNCH(patch_rank_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, rel, (long)ld, rank, P);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_patch_perturb(const float* img, const int32_t* rank, const int32_t* steps, const float* fill, float* out, int B, int C, int H, int W, int S,
                        mfvit_stream_t stream) {
    if (!img || !rank || !steps || !fill || !out) return MFVIT_EINVAL;
    if (H <= 0 || W <= 0 || H % 16 || W % 16 || B <= 0 || C <= 0 || S <= 0 || B > 65535 || S > 65535) return MFVIT_EINVAL;   // B, S: the grid's y and z extents
    if ((long long)(H / 16) * (W / 16) > RANK_MAXP || (long long)C * H * W > (1ll << 30)) return MFVIT_EINVAL;
    const int chw = C * H * W;
    const unsigned long long bytes = (unsigned long long)B * chw * sizeof(float);
    if (pert_overlap(img, bytes, out, bytes * S)) return MFVIT_EINVAL;
    const bool vec = ((uintptr_t)img | (uintptr_t)out) % 16 == 0;      // (W % 16 == 0: an aligned group of four never leaves its patch)
    const int per = vec ? chw / 4 : chw;
    const int chunks = (per + 256 * PERT_UNROLL - 1) / (256 * PERT_UNROLL);
    // as many passes for every workgroup of an (image, step): ceil(chunks * B * S / PERT_BLOCKS) passes over ceil(chunks / passes) workgroups
    const long long passes = ((long long)chunks * B * S + PERT_BLOCKS - 1) / PERT_BLOCKS;
    const dim3 grid((unsigned)((chunks + passes - 1) / passes), B, S);
    if (vec) MFVIT_LAUNCH(patch_perturb_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, img, rank, steps, fill, out, B, H, W, per);
    else MFVIT_LAUNCH(patch_perturb_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, img, rank, steps, fill, out, B, H, W, per);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_perturb_score(const float* logits, int64_t ld, const int64_t* target, int S, int B, int C, uint64_t* correct, double* sums,
                        uint64_t* nonfinite, mfvit_stream_t stream) {
    if (!logits || !target || !correct || !sums || !nonfinite || S <= 0 || B <= 0 || C <= 0 || ld < C) return MFVIT_EINVAL;
    MFVIT_LAUNCH(perturb_score_kernel, dim3(S), dim3(SCORE_THREADS), 0, (hipStream_t)stream, logits, (long)ld, (const long*)target, B, C,
                 (unsigned long long*)correct, sums, (unsigned long long*)nonfinite);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // extern "C"

}  // namespace mfvit
