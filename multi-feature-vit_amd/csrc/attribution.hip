// Gradient attribution for the image encoders (integrated gradients: Sundararajan, Taly & Yan 2017; SmoothGrad: Smilkov et al. 2017; saliency:
// Simonyan et al. 2014; mfvit.attribution drives it).  Everything but the model's forward and data-gradient-only backward:
//   attr_inputs_kernel      out[s][b] = base + alpha_s (x - base) (+ sigma_b z): all S inputs of one forward group in ONE launch.  z is a standard
//                           normal from a counter hash of (seed, global sample index, image, element): nothing is stored, and the noise of a sample
//                           does not depend on how the samples are grouped into forwards.
//   attr_accumulate_kernel  acc[b][i] += sum_s w_s g[s][b][i]^power (power 1 or 2), s ascending, one rounding per step.
//   attr_finish_kernel      per pixel a = sum_c f(acc_c (x_c - base_c)) or sum_c f(acc_c), f the identity or |.|; the optional pixel map, the sum of
//                           every 16 x 16 patch and the image's signed total in double.  One workgroup per image: no output has two writers.
// Streaming kernels: 16-byte accesses where the pointer phase allows, a scalar path otherwise; inputs / accumulate run one image per blockIdx.y as
// mix.hip and perturb.hip do.  No atomics; every sum has a fixed order, written next to it.
#include "kernels.h"

namespace mfvit {

namespace {

constexpr int ATTR_BLOCKS = 8192;    // grid target of the two streaming kernels (256 CUs x 8 workgroups x 4 grid-stride steps)
constexpr int FIN_THREADS = 1024;    // attr_finish_kernel: one workgroup per image
constexpr int FIN_QUADS = 256;       // 4-pixel groups of a patch row staged in LDS at a time (64 patches)

template <int VEC> struct alignas(4 * VEC) AttrPack { float v[VEC]; };

// the second word of the noise hash: the same multiply-xorshift form as lowbias32 (common.cuh) with another pair of constants
__device__ __forceinline__ unsigned lowbias32b(unsigned x) {
    x ^= x >> 16; x *= 0x21f0aaadU; x ^= x >> 15; x *= 0x735a2d97U; x ^= x >> 15;
    return x;
}
// key of (seed, global sample index gs, image b); the element index e enters by xor (include/mfvit.h, mfvit_attr_inputs)
__device__ __forceinline__ unsigned attr_key(unsigned long long seed, unsigned gs, unsigned b) {
    const unsigned k = lowbias32((unsigned)seed ^ lowbias32((unsigned)(seed >> 32) + 0x9E3779B9u * (gs + 1u)));
    return lowbias32(k + 0x85EBCA6Bu * (b + 1u));
}
// Box-Muller on two 24-bit uniforms: u1 in (0, 1] (never 0: the logarithm is finite), u2 in [0, 1); the accurate logf / sqrtf / cospif
__device__ __forceinline__ float attr_normal(unsigned key, unsigned e) {
    const unsigned h1 = lowbias32(e ^ key), h2 = lowbias32b(e ^ key);
    const float u1 = __fmul_rn(__fadd_rn((float)(h1 >> 8), 0.5f), 5.9604644775390625e-8f);     // ((h1 >> 8) + 0.5) 2^-24, the sum rounded to f32
    const float u2 = __fmul_rn((float)(h2 >> 8), 5.9604644775390625e-8f);
    return __fmul_rn(sqrtf(__fmul_rn(-2.f, logf(u1))), cospif(__fmul_rn(2.f, u2)));
}

// out[s][b] for b = blockIdx.y, s = blockIdx.z; per = C * hw / VEC packs per image.  v = base (alpha == 0), x (alpha == 1: both moves, bit-exact)
// or fmaf(alpha, x - base, base); with noise out = fmaf(sigma_b, z, v).
template <int VEC>
__global__ __launch_bounds__(256) void attr_inputs_kernel(const float* __restrict__ x, const float* __restrict__ base, int base_full,
                                                          const float* __restrict__ alpha, const float* __restrict__ sigma,
                                                          const unsigned long long* __restrict__ seed, int s0, float* __restrict__ out, int B, int hw,
                                                          int per) {
    using PK = AttrPack<VEC>;
    const int b = blockIdx.y, s = blockIdx.z;
    const float al = alpha[s];
    const bool noisy = sigma != nullptr;
    const float sg = noisy ? sigma[b] : 0.f;
    const unsigned key = noisy ? attr_key(seed[0], (unsigned)(s0 + s), (unsigned)b) : 0u;
    const PK* xs = (const PK*)x + (long)b * per;
    const PK* bs = base_full ? (const PK*)base + (long)b * per : nullptr;
    PK* dst = (PK*)out + ((long)s * B + b) * per;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < per; p += gridDim.x * 256) {
        const PK xv = xs[p];
        PK bv;
        if (base_full) {
            bv = bs[p];
        } else {
            const float f = base[(p * VEC) / hw];      // (the 16-byte path needs hw % 4 == 0: a pack never leaves its channel)
#pragma unroll
            for (int k = 0; k < VEC; ++k) bv.v[k] = f;
        }
        PK o;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float v = al == 0.f ? bv.v[k] : (al == 1.f ? xv.v[k] : fmaf(al, __fsub_rn(xv.v[k], bv.v[k]), bv.v[k]));
            if (noisy) v = fmaf(sg, attr_normal(key, (unsigned)(p * VEC + k)), v);
            o.v[k] = v;
        }
        dst[p] = o;
    }
}

// acc[b] for b = blockIdx.y.  power 1: a = fmaf(w_s, g, a).  power 2: a = (float)fma(w_s g, g, a) in double - w_s g is exact there (48 bits), so the
// square enters unrounded and every step rounds once, as the fmaf of power 1 does.
template <int VEC>
__global__ __launch_bounds__(256) void attr_accumulate_kernel(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ acc, int k,
                                                              int B, int per, int power) {
    using PK = AttrPack<VEC>;
    const int b = blockIdx.y;
    PK* a = (PK*)acc + (long)b * per;
    const PK* gb = (const PK*)g + (long)b * per;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < per; p += gridDim.x * 256) {
        PK av = a[p];
        for (int s = 0; s < k; ++s) {
            const PK gv = gb[(long)s * B * per + p];
            const float ws = w[s];
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                av.v[j] = power == 2 ? (float)fma((double)ws * (double)gv.v[j], (double)gv.v[j], (double)av.v[j]) : fmaf(ws, gv.v[j], av.v[j]);
        }
        a[p] = av;
    }
}

__device__ __forceinline__ void attr_load4(const float* p, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 t = *(const float4*)p;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}

// One workgroup per image b = blockIdx.x.  A work item is a group of four pixels of one image row (inside one patch: 16 % 4 == 0):
//   term   t_c = acc_c * (x_c - base_c) (the difference, then the product, each rounded to f32) or acc_c
//   pixel  a = f(t_0) + f(t_1) + .. in channel order
//   quad   (a_0 + a_1) + (a_2 + a_3)
//   patch  per pixel row of the patch (q_0 + q_1) + (q_2 + q_3) over its four quads, then the 16 rows pairwise in place:
//          ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) + the same of r8 .. r15
//   total  every thread adds its signed terms in double in the order it meets them (patch row, staged chunk, item, channel, pixel), then a
//          fixed tree over the 1024 threads.
__global__ __launch_bounds__(FIN_THREADS) void attr_finish_kernel(const float* __restrict__ acc, const float* __restrict__ x,
                                                                  const float* __restrict__ base, int base_full, int times_input, int absval,
                                                                  float* __restrict__ pixels, float* __restrict__ patches, double* __restrict__ total,
                                                                  int C, int H, int W, int vec) {
    __shared__ float quad[16 * FIN_QUADS];
    __shared__ double tsum[FIN_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hw = H * W, gw = W >> 4, gh = H >> 4, qw = W >> 2;
    const long img = (long)b * C * hw;
    double tot = 0.0;
    for (int py = 0; py < gh; ++py) {
        for (int q0 = 0; q0 < qw; q0 += FIN_QUADS) {
            const int qn = qw - q0 < FIN_QUADS ? qw - q0 : FIN_QUADS;
            for (int i = tid; i < 16 * qn; i += FIN_THREADS) {
                const int r = i / qn, q = i - r * qn;
                const int off = (py * 16 + r) * W + (q0 + q) * 4;
                float a4[4] = {0.f, 0.f, 0.f, 0.f};
                for (int c = 0; c < C; ++c) {
                    float t[4];
                    attr_load4(acc + img + (long)c * hw + off, vec, t);
                    if (times_input) {
                        float xv[4], bv[4];
                        attr_load4(x + img + (long)c * hw + off, vec, xv);
                        if (base_full) attr_load4(base + img + (long)c * hw + off, vec, bv);
                        else bv[0] = bv[1] = bv[2] = bv[3] = base[c];
#pragma unroll
                        for (int j = 0; j < 4; ++j) t[j] = __fmul_rn(t[j], __fsub_rn(xv[j], bv[j]));
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        tot += (double)t[j];
                        const float f = absval ? fabsf(t[j]) : t[j];
                        a4[j] = c == 0 ? f : __fadd_rn(a4[j], f);
                    }
                }
                if (pixels) {
                    float* dst = pixels + (long)b * hw + off;
                    if (vec) *(float4*)dst = make_float4(a4[0], a4[1], a4[2], a4[3]);
                    else { dst[0] = a4[0]; dst[1] = a4[1]; dst[2] = a4[2]; dst[3] = a4[3]; }
                }
                quad[r * FIN_QUADS + q] = __fadd_rn(__fadd_rn(a4[0], a4[1]), __fadd_rn(a4[2], a4[3]));
            }
            __syncthreads();
            for (int p = tid; p < (qn >> 2); p += FIN_THREADS) {       // (W % 16 == 0: qn is a multiple of 4)
                float rs[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* l = quad + r * FIN_QUADS + 4 * p;
                    rs[r] = __fadd_rn(__fadd_rn(l[0], l[1]), __fadd_rn(l[2], l[3]));
                }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
                    for (int r = 0; r < 16; r += 2 * o) rs[r] = __fadd_rn(rs[r], rs[r + o]);
                }
                patches[((long)b * gh + py) * gw + (q0 >> 2) + p] = rs[0];
            }
            __syncthreads();
        }
    }
    tsum[tid] = tot;
    __syncthreads();
    for (int o = FIN_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) tsum[tid] += tsum[tid + o];
        __syncthreads();
    }
    if (tid == 0) total[b] = tsum[0];
}

// [p, p + np) and [q, q + nq) share a byte
bool attr_overlap(const void* p, unsigned long long np, const void* q, unsigned long long nq) {
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b ? b - a < np : a - b < nq;
}

// workgroups along x for B * S images of `per` packs: every thread takes at least four grid-stride steps where the image is long enough
unsigned attr_grid_x(int per, long long images) {
    const long long chunks = ((long long)per + 1023) / 1024;
    const long long cap = (ATTR_BLOCKS + images - 1) / images;
    const long long gx = chunks < cap ? chunks : cap;
    return (unsigned)(gx < 1 ? 1 : gx);
}

}  // namespace

extern "C" {

int mfvit_attr_inputs(const float* x, const float* base, int base_full, const float* alpha, const float* sigma, const uint64_t* seed, int s0,
                      float* out, int S, int B, int C, int64_t hw, mfvit_stream_t stream) {
    if (!x || !base || !alpha || !out || (sigma && !seed)) return MFVIT_EINVAL;
    if (S <= 0 || B <= 0 || C <= 0 || hw <= 0 || S > 65535 || B > 65535 || s0 < 0 || s0 > (1 << 30)) return MFVIT_EINVAL;   // B, S: the grid's y and z extents
    if (hw > (1ll << 30) || (long long)C * hw > (1ll << 30)) return MFVIT_EINVAL;
    const int n = (int)(C * hw);
    const unsigned long long bytes = (unsigned long long)B * n * sizeof(float);
    if (attr_overlap(x, bytes, out, bytes * S) || (base_full && attr_overlap(base, bytes, out, bytes * S))) return MFVIT_EINVAL;
    const bool vec = ((uintptr_t)x | (uintptr_t)out | (base_full ? (uintptr_t)base : 0)) % 16 == 0 && hw % 4 == 0;
    const int per = vec ? n / 4 : n;
    const dim3 grid(attr_grid_x(per, (long long)B * S), B, S);
    if (vec) MFVIT_LAUNCH(attr_inputs_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, base, base_full, alpha, sigma,
                          (const unsigned long long*)seed, s0, out, B, (int)hw, per);
    else MFVIT_LAUNCH(attr_inputs_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, base, base_full, alpha, sigma,
                      (const unsigned long long*)seed, s0, out, B, (int)hw, per);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_attr_accumulate(const float* g, const float* w, float* acc, int k, int B, int64_t n, int power, mfvit_stream_t stream) {
    if (!g || !w || !acc || k <= 0 || k > 65535 || B <= 0 || B > 65535 || n <= 0 || n > (1ll << 30) || (power != 1 && power != 2)) return MFVIT_EINVAL;
    const unsigned long long bytes = (unsigned long long)B * n * sizeof(float);
    if (attr_overlap(acc, bytes, g, bytes * k)) return MFVIT_EINVAL;
    const bool vec = ((uintptr_t)g | (uintptr_t)acc) % 16 == 0 && n % 4 == 0;
    const int per = (int)(vec ? n / 4 : n);
    const dim3 grid(attr_grid_x(per, B), B);
    if (vec) MFVIT_LAUNCH(attr_accumulate_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, g, w, acc, k, B, per, power);
    else MFVIT_LAUNCH(attr_accumulate_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, g, w, acc, k, B, per, power);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_attr_finish(const float* acc, const float* x, const float* base, int base_full, int times_input, int absval, float* pixels,
                      float* patches, double* total, int B, int C, int H, int W, mfvit_stream_t stream) {
    if (!acc || !patches || !total || (times_input && (!x || !base))) return MFVIT_EINVAL;
    if (H <= 0 || W <= 0 || H % 16 || W % 16 || B <= 0 || C <= 0 || (long long)C * H * W > (1ll << 30)) return MFVIT_EINVAL;
    const unsigned long long plane = (unsigned long long)B * H * W * sizeof(float), bytes = plane * C;
    if (attr_overlap(pixels, plane, acc, bytes) || (times_input && (attr_overlap(pixels, plane, x, bytes) ||
                                                                     (base_full && attr_overlap(pixels, plane, base, bytes))))) return MFVIT_EINVAL;
    uintptr_t bits = (uintptr_t)acc | (uintptr_t)pixels;
    if (times_input) bits |= (uintptr_t)x | (base_full ? (uintptr_t)base : 0);
    MFVIT_LAUNCH(attr_finish_kernel, dim3(B), dim3(FIN_THREADS), 0, (hipStream_t)stream, acc, x, base, base_full, times_input, absval, pixels, patches,
                 total, C, H, W, (int)(bits % 16 == 0));
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // extern "C"

}  // namespace mfvit
