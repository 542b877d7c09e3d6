// Photometric half of the MoCo-v3 aug1 / aug2 input chains (main_covid_mocov3based_..._vitsmall.py:388-413) on the device:
//   RandomApply(ColorJitter(0.4, 0.4, 0.2, 0.1)) -> RandomGrayscale -> moco.loader.GaussianBlur -> Solarize -> ToTensor -> Normalize
// bit-exact against Pillow, the backend torchvision's PIL transforms call: ImagingBlend in float32 (ImageEnhance), Convert.c's L and HSV
// conversions (float32 with their double sub-expressions), BoxBlur.c's three extended box passes per axis on uint8 intermediates,
// ImageOps.solarize.  Floating-point contraction is off for this file: Pillow rounds after every product, so no FMA may form.
//   stage 0  input.hip's gather, stopped at the uint8 frame (resized, flipped: a horizontal flip commutes with everything below)
//   stage 1  photo_mean_kernel: the integer sum of L over the frame for the samples whose chain holds contrast, after the pointwise
//            operations that precede contrast in that sample's order (recomputed here; an integer sum has no order)
//   stage 2  photo_finish_kernel: one 32 x 32 output tile per workgroup - jitter and grayscale at the load of the tile and its halo into
//            LDS, six box passes between two LDS images, solarize, (v / 255 - mean) / std, float32 CHW
// A pass reaches r + 1 pixels, so the halo is 3 (r + 1) per side; the LDS images are sized for r <= MAX_R = 1, which is every sigma up to
// 2.4494896 (the reference draws from [0.1, 2]); a larger radius is MFVIT_ENOSYS at the entry point.
#include "common.cuh"
#include "kernels.h"

// hipcc contracts a * b + c into an FMA by default - also through the round-to-nearest add / multiply intrinsics, which are inline
// operators compiled under the header's own contraction mode (measured: the blend at f = 0.6 came out one level off).  So the sums
// and products below are plain operators under this pragma; only the divisions keep their correctly rounded intrinsics.
#pragma clang fp contract(off)

namespace mfvit {

namespace {

constexpr int TILE = 32;
constexpr int MAX_R = 1;
constexpr int MAX_HALO = 3 * (MAX_R + 1);
constexpr int MAX_RW = TILE + 2 * MAX_HALO;
constexpr int PD = 16;    // int32 slots of one sample's photometric descriptor

// photo[s][16]: 0 the jitter operations in order, one nibble each from bit 0 (0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue),
//               1 / 2 / 3 the float32 bits of the brightness / contrast / saturation factor, 4 the hue shift on the 8-bit H (0..255),
//               5 flags (1 grayscale, 2 blur, 4 solarize), 6 / 7 / 8 the box radius r, the weights ww and fw of one pass, 9..15 zero
enum { OP_NONE = 0, OP_BRIGHTNESS = 1, OP_CONTRAST = 2, OP_SATURATION = 3, OP_HUE = 4 };
enum { F_GRAY = 1, F_BLUR = 2, F_SOLARIZE = 4 };

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ImagingBlend(deg, v, f): float32; for 0 <= f <= 1 the value is inside [0, 255] and the clip is the truncation Pillow does there
__device__ __forceinline__ int blend(int deg, int v, float f) {
    const float t = (float)deg + f * (float)(v - deg);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// round(v * a) of hsv2rgb: the double product lands in a float, round() is half away from zero
__device__ __forceinline__ int hsv_term(double v, double a) { return clip255((int)roundf((float)(v * a))); }

// torchvision adjust_hue on PIL: convert('HSV') (rgb2hsv_row), H += shift mod 256, convert('RGB') (hsv2rgb)
__device__ void hue_op(int& r, int& g, int& b, int shift) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int uh = 0, us = 0;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = __fdiv_rn(cr, (float)mx);
        const float rc = __fdiv_rn((float)(mx - r), cr), gc = __fdiv_rn((float)(mx - g), cr), bc = __fdiv_rn((float)(mx - b), cr);
        float h;
        if (r == mx) h = bc - gc;
        else if (g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        double hd = __ddiv_rn((double)h, 6.0) + 1.0;     // in (0.8, 1.9): fmod(hd, 1.0) is an exact subtraction
        if (hd >= 1.0) hd = hd - 1.0;
        uh = clip255((int)((double)(float)hd * 255.0));
        us = clip255((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = mx;
        return;
    }
    const float fs = (float)__ddiv_rn((double)us, 255.0);
    const float h6 = (float)__ddiv_rn((double)uh * 6.0, 255.0);
    const float fi = floorf(h6);
    const double f = (double)(h6 - fi), dfs = (double)fs, dv = (double)mx;
    const int p = hsv_term(dv, 1.0 - dfs);
    const int q = hsv_term(dv, 1.0 - dfs * f);
    const int t = hsv_term(dv, 1.0 - dfs * (1.0 - f));
    switch ((int)fi % 6) {
        case 0: r = mx, g = t, b = p; break;
        case 1: r = q, g = mx, b = p; break;
        case 2: r = p, g = mx, b = t; break;
        case 3: r = p, g = q, b = mx; break;
        case 4: r = t, g = p, b = mx; break;
        default: r = mx, g = p, b = q; break;
    }
}

// the jitter operations of one pixel in the sample's order; UNTIL_CONTRAST stops in front of contrast (the mean pass)
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter(int& r, int& g, int& b, const int* __restrict__ pd, int mean) {
    const int ops = pd[0];
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int op = (ops >> (4 * k)) & 15;
        if (op == OP_BRIGHTNESS) {
            const float f = __int_as_float(pd[1]);
            r = blend(0, r, f), g = blend(0, g, f), b = blend(0, b, f);
        } else if (op == OP_CONTRAST) {
            if (UNTIL_CONTRAST) return;
            const float f = __int_as_float(pd[2]);
            r = blend(mean, r, f), g = blend(mean, g, f), b = blend(mean, b, f);
        } else if (op == OP_SATURATION) {
            const float f = __int_as_float(pd[3]);
            const int l = luma(r, g, b);
            r = blend(l, r, f), g = blend(l, g, f), b = blend(l, b, f);
        } else if (op == OP_HUE) {
            hue_op(r, g, b, pd[4]);
        }
    }
}

__device__ __forceinline__ bool has_contrast(int ops) {
    return (ops & 15) == OP_CONTRAST || ((ops >> 4) & 15) == OP_CONTRAST || ((ops >> 8) & 15) == OP_CONTRAST || ((ops >> 12) & 15) == OP_CONTRAST;
}

// stage 1: sums[s] += L over the frame of sample s in the state contrast finds it in.  Grid (blocks, n); sums zeroed by the caller.
__global__ __launch_bounds__(256) void photo_mean_kernel(const unsigned* __restrict__ frames, const int* __restrict__ photo, int plane,
                                                         unsigned long long* __restrict__ sums) {
    const int smp = blockIdx.y;
    const int* pd = photo + (long)smp * PD;
    if (!has_contrast(pd[0])) return;
    const unsigned* img = frames + (long)smp * plane;
    unsigned acc = 0;                                   // at most 2^30 / 256 pixels of 255 per thread
    for (int i = blockIdx.x * 256 + threadIdx.x; i < plane; i += gridDim.x * 256) {
        const unsigned px = img[i];
        int r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255;
        jitter<true>(r, g, b, pd, 0);
        acc += luma(r, g, b);
    }
    unsigned long long tot = acc;
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_down(tot, o, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = tot;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + smp, part[0] + part[1] + part[2] + part[3]);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one extended box pass (ImagingLineBoxBlur8) over the whole rw x rw LDS image, along x (ALONG_X) or y.  A tap's index clamps to the
// IMAGE edge first, then to the LDS image (those positions are halo that the 3 (r + 1) margin keeps away from the tile).
template <bool ALONG_X>
__device__ __forceinline__ void box_pass(const unsigned* __restrict__ in, unsigned* __restrict__ out, int rw, int org_x, int org_y, int S,
                                         int r, unsigned ww, unsigned fw) {
    for (int p = threadIdx.x; p < rw * rw; p += 256) {
        const int ly = p / rw, lx = p - ly * rw;
        const int pos = ALONG_X ? org_x + lx : org_y + ly, org = ALONG_X ? org_x : org_y;
        unsigned a0 = 0, a1 = 0, a2 = 0, e0 = 0, e1 = 0, e2 = 0;
        for (int d = -r - 1; d <= r + 1; ++d) {
            const int li = clampi(clampi(pos + d, 0, S - 1) - org, 0, rw - 1);
            const unsigned px = in[ALONG_X ? ly * rw + li : li * rw + lx];
            if (d == -r - 1 || d == r + 1) e0 += px & 255, e1 += (px >> 8) & 255, e2 += (px >> 16) & 255;
            else a0 += px & 255, a1 += (px >> 8) & 255, a2 += (px >> 16) & 255;
        }
        // (2 r + 1) ww + 2 fw <= 2^24, so every sum stays under 255 * 2^24 + 2^23 < 2^32 (BoxBlur.c holds it in a UINT32 too)
        out[p] = ((ww * a0 + fw * e0 + (1u << 23)) >> 24) | (((ww * a1 + fw * e1 + (1u << 23)) >> 24) << 8) |
                 (((ww * a2 + fw * e2 + (1u << 23)) >> 24) << 16);
    }
}

// stage 2.  Grid (tiles_x * tiles_y, n).
__global__ __launch_bounds__(256) void photo_finish_kernel(const unsigned* __restrict__ frames, const int* __restrict__ photo,
                                                           const unsigned long long* __restrict__ sums, int S, int tiles_x, float m0, float m1,
                                                           float m2, float s0, float s1, float s2, float* __restrict__ out) {
    __shared__ unsigned buf[2][MAX_RW * MAX_RW];
    const int smp = blockIdx.y;
    const int* pd = photo + (long)smp * PD;
    const int plane = S * S;
    const unsigned* img = frames + (long)smp * plane;
    const int flags = pd[5];
    const bool blur = flags & F_BLUR;
    const int r = clampi(pd[6], 0, MAX_R);
    const int halo = blur ? 3 * (r + 1) : 0, rw = TILE + 2 * halo;
    const int x0 = (blockIdx.x % tiles_x) * TILE, y0 = (blockIdx.x / tiles_x) * TILE;
    const int org_x = x0 - halo, org_y = y0 - halo;
    // Enhance.Contrast's degenerate image: int(mean(L) + 0.5) from the exact sum
    const int mean = has_contrast(pd[0]) ? (int)((2 * sums[smp] + (unsigned long long)plane) / (2 * (unsigned long long)plane)) : 0;
    for (int p = threadIdx.x; p < rw * rw; p += 256) {
        const int ly = p / rw, lx = p - ly * rw;
        const unsigned px = img[(long)clampi(org_y + ly, 0, S - 1) * S + clampi(org_x + lx, 0, S - 1)];
        int cr = px & 255, cg = (px >> 8) & 255, cb = (px >> 16) & 255;
        jitter<false>(cr, cg, cb, pd, mean);
        if (flags & F_GRAY) cr = cg = cb = luma(cr, cg, cb);
        buf[0][p] = (unsigned)cr | ((unsigned)cg << 8) | ((unsigned)cb << 16);
    }
    __syncthreads();
    int cur = 0;
    if (blur) {
        const unsigned ww = (unsigned)pd[7], fw = (unsigned)pd[8];
        for (int k = 0; k < 3; ++k, cur ^= 1) {
            box_pass<true>(buf[cur], buf[cur ^ 1], rw, org_x, org_y, S, r, ww, fw);
            __syncthreads();
        }
        for (int k = 0; k < 3; ++k, cur ^= 1) {
            box_pass<false>(buf[cur], buf[cur ^ 1], rw, org_x, org_y, S, r, ww, fw);
            __syncthreads();
        }
    }
    const bool sol = flags & F_SOLARIZE;
    for (int p = threadIdx.x; p < TILE * TILE; p += 256) {
        const int ty = p / TILE, tx = p % TILE;
        const int x = x0 + tx, y = y0 + ty;
        if (x >= S || y >= S) continue;
        const unsigned px = buf[cur][(ty + halo) * rw + tx + halo];
        int v0 = px & 255, v1 = (px >> 8) & 255, v2 = (px >> 16) & 255;
        if (sol) v0 = v0 < 128 ? v0 : 255 - v0, v1 = v1 < 128 ? v1 : 255 - v1, v2 = v2 < 128 ? v2 : 255 - v2;
        // ToTensor and Normalize exactly as input.hip writes them
        float* o = out + ((long)smp * 3) * plane + (long)y * S + x;
        o[0] = __fdiv_rn(__fdiv_rn((float)v0, 255.0f) - m0, s0);
        o[plane] = __fdiv_rn(__fdiv_rn((float)v1, 255.0f) - m1, s1);
        o[2L * plane] = __fdiv_rn(__fdiv_rn((float)v2, 255.0f) - m2, s2);
    }
}

inline size_t sums_bytes(int n) { return ((size_t)n * 8 + 255) / 256 * 256; }

}  // namespace

size_t input_photometric_workspace_bytes(int n, int S) {
    if (n <= 0 || n > 65535 || S <= 0 || (long long)S * S > (1ll << 30)) return 0;
    return sums_bytes(n) + (size_t)n * S * S * 4;
}

int input_photometric(const unsigned char* src, const long long* desc, const int* tables, const int* photo, int n, int S, int max_radius,
                      void* workspace, const float* mean, const float* stdv, float* out, hipStream_t st) {
    if (n <= 0 || n > 65535 || S <= 0 || (long long)S * S > (1ll << 30) || max_radius < 0) return MFVIT_EINVAL;
    if (max_radius > MAX_R) return MFVIT_ENOSYS;
    unsigned long long* sums = (unsigned long long*)workspace;
    unsigned* frames = (unsigned*)((char*)workspace + sums_bytes(n));
    if (hipMemsetAsync(sums, 0, (size_t)n * 8, st) != hipSuccess) return MFVIT_ELAUNCH;
    const int rc = input_transform_u8(src, desc, tables, n, S, frames, st);
    if (rc != MFVIT_OK) return rc;
    const int plane = S * S;
    MFVIT_LAUNCH(photo_mean_kernel, dim3((plane + 1023) / 1024, n), dim3(256), 0, st, frames, photo, plane, sums);
    MFVIT_CHECK_LAUNCH();
    const int tiles = (S + TILE - 1) / TILE;
    MFVIT_LAUNCH(photo_finish_kernel, dim3(tiles * tiles, n), dim3(256), 0, st, frames, photo, sums, S, tiles, mean[0], mean[1], mean[2], stdv[0],
                 stdv[1], stdv[2], out);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // namespace mfvit
