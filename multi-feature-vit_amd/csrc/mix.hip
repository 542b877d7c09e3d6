// Batch regularisers of the fine-tune recipe that the encoders never see (timm.data.Mixup / RandomErasing, timm.loss.SoftTargetCrossEntropy):
//   batch_mix_kernel  random erasing (mode 'const': fill 0, the dataset mean after Normalize) + Mixup / CutMix of one or two image batches in ONE
//                     launch - the CXR stream and its enhanced twin share partner, coefficient and boxes, so a mixed pair still shows one patient.
//   ce_soft_kernel    soft-target cross entropy (mean) over C <= 64 classes with label smoothing and the mixed target
//                     y_i = lam_i s(t_i) + (1 - lam_i) s(t_partner_i), s(t) = (1 - smoothing) onehot(t) + smoothing / C; the [B][C] target
//                     matrix is never materialised.
// batch_mix is a streaming kernel (3 floats of traffic per element and stream for Mixup, 2 for CutMix / copy): one sample per blockIdx.y, so that the
// descriptor row is block-uniform (scalar loads), 16-byte accesses where W % 4 == 0 (a vector never straddles an image row then), MIX_UNROLL vectors per
// thread with every load of both streams and both sources issued before the first use (up to 16 x 16 bytes in flight per thread).
#include "kernels.h"

namespace mfvit {

namespace {

constexpr int MIX_DESC = 12;     // int32 columns of a descriptor row (include/mfvit.h)
constexpr int MIX_UNROLL = 4;    // vectors per thread and grid-stride step
constexpr int MIX_BLOCKS = 2048; // grid target: 256 CUs x 8 workgroups; above it the workgroups stride over their sample

template <int VEC> struct alignas(4 * VEC) MixPack { float v[VEC]; };

// half-open box [yl, yh) x [xl, xh); off: the empty box
struct MixBox { int yl, yh, xl, xh; };
__device__ __forceinline__ MixBox mix_box(const int* d, bool on) {
    MixBox b = {0, 0, 0, 0};
    if (on) b = {d[0], d[1], d[2], d[3]};
    return b;
}
// bit k: element x0 + k of row y lies inside the box
template <int VEC> __device__ __forceinline__ unsigned mix_inside(const MixBox& b, int y, int x0) {
    unsigned m = 0;
    if (y >= b.yl && y < b.yh) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) m |= (x0 + k >= b.xl && x0 + k < b.xh) ? 1u << k : 0u;
    }
    return m;
}

// out[i] = mix(E(x_i), E(x_j)) for sample i = blockIdx.y of one (b == NULL) or two streams; per = C * H * W / VEC packs per sample.
template <int VEC>
__global__ __launch_bounds__(256) void batch_mix_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ oa,
                                                        float* __restrict__ ob, const int* __restrict__ desc, const float* __restrict__ lam, int n,
                                                        int H, int W, int per) {
    using P = MixPack<VEC>;
    constexpr unsigned FULL = (1u << VEC) - 1u;
    const int i = blockIdx.y;
    const int* di = desc + (long)i * MIX_DESC;
    int j = di[0];
    j = j < 0 ? 0 : (j >= n ? n - 1 : j);      // a bad table must not read outside the batch (boxes only enter comparisons)
    const int* dj = desc + (long)j * MIX_DESC;
    const int mode = di[1];
    const MixBox cut = mix_box(di + 2, mode == 2), ei = mix_box(di + 7, di[6] != 0), ej = mix_box(dj + 7, dj[6] != 0);
    const float l = lam[i];
    const bool two = b != nullptr;
    const P* ai = (const P*)a + (long)i * per;
    const P* aj = (const P*)a + (long)j * per;
    const P* bi = (const P*)b + (long)i * per;
    const P* bj = (const P*)b + (long)j * per;
    P* oai = (P*)oa + (long)i * per;
    P* obi = (P*)ob + (long)i * per;
    for (int p0 = blockIdx.x * (256 * MIX_UNROLL) + threadIdx.x; p0 < per; p0 += gridDim.x * (256 * MIX_UNROLL)) {
        P ri[MIX_UNROLL] = {}, rj[MIX_UNROLL] = {}, si[MIX_UNROLL] = {}, sj[MIX_UNROLL] = {};
        unsigned mc[MIX_UNROLL], mi[MIX_UNROLL], mj[MIX_UNROLL];
        // every load first ...
#pragma unroll
        for (int u = 0; u < MIX_UNROLL; ++u) {
            const int p = p0 + u * 256;
            const int e = p * VEC, x0 = e % W, y = (e / W) % H;
            mc[u] = mix_inside<VEC>(cut, y, x0);
            mi[u] = mix_inside<VEC>(ei, y, x0);
            mj[u] = mix_inside<VEC>(ej, y, x0);
            // a source is read only where one of its elements reaches the output: CutMix moves each element once
            const bool want_i = p < per && mc[u] != FULL && mi[u] != FULL;
            const bool want_j = p < per && (mode == 1 ? mj[u] != FULL : (mc[u] & ~mj[u]) != 0);
            if (want_i) {
                ri[u] = ai[p];
                if (two) si[u] = bi[p];
            }
            if (want_j) {
                rj[u] = aj[p];
                if (two) sj[u] = bj[p];
            }
        }
        // ... then the arithmetic and the stores
#pragma unroll
        for (int u = 0; u < MIX_UNROLL; ++u) {
            const int p = p0 + u * 256;
            if (p >= per) break;
            P qa, qb;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const bool zi = (mi[u] >> k) & 1, zj = (mj[u] >> k) & 1, c = (mc[u] >> k) & 1;
                const float xi = zi ? 0.f : ri[u].v[k], xj = zj ? 0.f : rj[u].v[k];
                const float wi = zi ? 0.f : si[u].v[k], wj = zj ? 0.f : sj[u].v[k];
                // Mixup: lam x_i + (1 - lam) x_j with (1 - lam) x_j = x_j - lam x_j in ONE rounding: two roundings in all, inside the
                // 2^-23 (|lam x_i| + |(1 - lam) x_j|) of two rounded products and a rounded sum, whatever the compiler contracts
                qa.v[k] = mode == 1 ? fmaf(l, xi, fmaf(-l, xj, xj)) : (c ? xj : xi);
                qb.v[k] = mode == 1 ? fmaf(l, wi, fmaf(-l, wj, wj)) : (c ? wj : wi);
            }
            oai[p] = qa;
            if (two) obi[p] = qb;
        }
    }
}

// Soft-target cross entropy (mean), ce_small_kernel's shape (elementwise.hip): one thread per sample, ONE block, the mean a fixed-order sum (per-thread
// sequences, wave sums, the 16 wave totals in order) - the same bits on every run.  y_c = smoothing / C + (1 - smoothing) (lam [c == t] + (1 - lam) [c == tp]).
// The classes enter by comparison only, so an out-of-range label reads nothing; the partner index is clamped.
__global__ __launch_bounds__(1024) void ce_soft_kernel(const float* __restrict__ logits, const long* __restrict__ target, const int* __restrict__ partner,
                                                       const float* __restrict__ lam, float smoothing, float* __restrict__ loss_mean,
                                                       float* __restrict__ dlogits, long* __restrict__ preds, int B, int C) {
    __shared__ float red[16];
    const float off = smoothing / (float)C, on = 1.f - smoothing, invB = 1.f / (float)B;
    float li = 0.f;
    for (int b = threadIdx.x; b < B; b += 1024) {
        const float* z = logits + (long)b * C;
        float m = z[0];
        int am = 0;
        for (int c = 1; c < C; ++c) if (first_max_takes(z[c], m)) { m = z[c]; am = c; }
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(z[c] - m);
        const float ls = logf(s), inv = 1.f / s;
        const int t = (int)target[b];
        int tp = t;
        float l = 1.f;
        if (partner) {
            int pb = partner[b];
            pb = pb < 0 ? 0 : (pb >= B ? B - 1 : pb);
            tp = (int)target[pb];
            l = lam[b];
        }
        const float wt = on * l, wp = on * (1.f - l);
        float acc = 0.f;
        for (int c = 0; c < C; ++c) {
            const float y = off + (c == t ? wt : 0.f) + (c == tp ? wp : 0.f);
            acc = fmaf(y, ls + (m - z[c]), acc);             // - y_c log softmax_c, with lse - z_c = log s + (m - z_c)
            if (dlogits) dlogits[(long)b * C + c] = (expf(z[c] - m) * inv - y) * invB;
        }
        li += acc * invB;
        if (preds) preds[b] = am;
    }
    li = wave_sum(li);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = li;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i];
        *loss_mean = t;
    }
}

// [p, p + bytes) and [q, q + bytes) share a byte
bool mix_overlap(const void* p, const void* q, unsigned long long bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b ? b - a < bytes : a - b < bytes;
}

}  // namespace

extern "C" {

int mfvit_batch_mix(const float* a, const float* b, float* out_a, float* out_b, const int32_t* desc, const float* lam, int n, int C, int H, int W,
                    mfvit_stream_t stream) {
    if (!a || !out_a || !desc || !lam || (b == nullptr) != (out_b == nullptr)) return MFVIT_EINVAL;
    if (n <= 0 || C <= 0 || H <= 0 || W <= 0 || n > 65535 || (long long)C * H * W > (1ll << 30)) return MFVIT_EINVAL;   // n: the grid's y extent
    const int chw = C * H * W;
    const unsigned long long bytes = (unsigned long long)n * chw * sizeof(float);
    // out of place: a sample's partner is read after another workgroup may have written it
    if (mix_overlap(out_a, a, bytes)) return MFVIT_EINVAL;
    if (b && (mix_overlap(out_b, b, bytes) || mix_overlap(out_a, b, bytes) || mix_overlap(out_b, a, bytes) || mix_overlap(out_a, out_b, bytes)))
        return MFVIT_EINVAL;
    const bool vec = W % 4 == 0 && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)out_a | (uintptr_t)out_b) % 16 == 0;
    const int per = vec ? chw / 4 : chw;
    const int chunks = (per + 256 * MIX_UNROLL - 1) / (256 * MIX_UNROLL);
    // as many passes for every workgroup of a sample: ceil(chunks * n / MIX_BLOCKS) passes over ceil(chunks / passes) workgroups
    const int passes = (int)(((long long)chunks * n + MIX_BLOCKS - 1) / MIX_BLOCKS);
    const dim3 grid((chunks + passes - 1) / passes, n);
    if (vec) MFVIT_LAUNCH(batch_mix_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a, b, out_a, out_b, desc, lam, n, H, W, per);
    else MFVIT_LAUNCH(batch_mix_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a, b, out_a, out_b, desc, lam, n, H, W, per);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_cross_entropy_soft(const float* logits, const int64_t* target, const int32_t* partner, const float* lam, float smoothing, float* loss_mean,
                             float* dlogits, int64_t* preds, int B, int C, mfvit_stream_t stream) {
    if (!logits || !target || !loss_mean || (partner == nullptr) != (lam == nullptr)) return MFVIT_EINVAL;
    if (C > 64 || C < 1 || B < 1 || !(smoothing >= 0.f && smoothing < 1.f)) return MFVIT_EINVAL;
    MFVIT_LAUNCH(ce_soft_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, (const long*)target, partner, lam, smoothing, loss_mean, dlogits,
                 (long*)preds, B, C);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // extern "C"

}  // namespace mfvit
