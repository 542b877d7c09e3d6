// Multi-tensor optimizer steps on gfx950: one (or two) launches over a device-resident chunk table instead of a Python
// loop of per-tensor ATen ops.  HBM-bound: every parameter / gradient / state element is touched once.
//   LARS  - moco_pretraining/moco/moco/optimizer.py:10-43 of the reference (trust ratio only for ndim > 1 tensors)
//   Adam / AdamW - torch.optim.Adam / AdamW semantics (MAIN_CA:455-459, MAIN_MOCO:338-345)
//   SGD   - torch.optim.SGD with momentum and L2 weight decay (MAIN_CA:445-448)
// Chunk table (int64, device): per chunk [tensor_id, p_ptr, g_ptr, s0_ptr, s1_ptr, count, flag]; pointers are to the
// chunk's first element.
#include "common.cuh"

namespace mfvit {

constexpr int CH = 7;

__global__ __launch_bounds__(256) void lars_norms_kernel(const long* __restrict__ tab, float wd, float* __restrict__ norms) {
    const long* e = tab + (long)blockIdx.x * CH;
    if (!e[6]) return;  // ndim <= 1: no trust ratio
    const float* p = (const float*)e[1];
    const float* g = (const float*)e[2];
    const long n = e[5];
    float a = 0.f, b = 0.f;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float pv = p[i], d = fmaf(wd, pv, g[i]);
        a = fmaf(pv, pv, a);
        b = fmaf(d, d, b);
    }
    __shared__ float sc[4];
    a = block_sum<256>(a, sc);
    b = block_sum<256>(b, sc);
    if (threadIdx.x == 0) {
        atomicAdd(norms + 2 * e[0], a);
        atomicAdd(norms + 2 * e[0] + 1, b);
    }
}
__global__ __launch_bounds__(256) void lars_update_kernel(const long* __restrict__ tab, const float* __restrict__ norms, float lr, float wd,
                                                          float momentum, float trust) {
    const long* e = tab + (long)blockIdx.x * CH;
    float* p = (float*)e[1];
    const float* g = (const float*)e[2];
    float* mu = (float*)e[3];
    const long n = e[5];
    const bool big = e[6] != 0;
    float q = 1.f;
    if (big) {
        const float pn = sqrtf(norms[2 * e[0]]), un = sqrtf(norms[2 * e[0] + 1]);
        q = (pn > 0.f && un > 0.f) ? trust * pn / un : 1.f;     // optimizer.py:31-35
    }
    for (long i = threadIdx.x; i < n; i += 256) {
        float d = g[i];
        if (big) d = fmaf(wd, p[i], d) * q;
        const float m = fmaf(mu[i], momentum, d);
        mu[i] = m;
        p[i] = fmaf(-lr, m, p[i]);
    }
}
// flag bit0: decoupled weight decay (AdamW); step-dependent constants are precomputed on the host
__device__ __forceinline__ void adam_elem(float& pv, float gv, float& mv, float& vv, bool decoupled, float lr, float beta1, float beta2, float eps,
                                          float wd, float bc1, float bc2_sqrt) {
    if (decoupled) pv *= 1.f - lr * wd; else gv = fmaf(wd, pv, gv);
    mv = fmaf(beta1, mv, (1.f - beta1) * gv);
    vv = fmaf(beta2, vv, (1.f - beta2) * gv * gv);
    pv = pv - (lr / bc1) * mv / (sqrtf(vv) / bc2_sqrt + eps);
}
// 28 bytes of HBM traffic per element (p, g, m, v in; p, m, v out) and nothing else: 16-byte accesses, two independent groups per thread in
// flight (the 4-byte form ran at 2.2 TB/s: 0.56 ms per step for the 45 M parameters of the two-encoder model).  One table row: what adam_kernel
// and adam_groups_kernel both run, so the two give the same bits for the same hyperparameters.
__device__ __forceinline__ void adam_row(const long* __restrict__ e, bool decoupled, float lr, float beta1, float beta2, float eps, float wd,
                                         float bc1, float bc2_sqrt) {
    float* p = (float*)e[1];
    const float* g = (const float*)e[2];
    float* m = (float*)e[3];
    float* v = (float*)e[4];
    const long n = e[5];
    long done = 0;
    if ((((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) == 0) {
        const long n4 = n >> 2;
        float4* p4 = (float4*)p;
        const float4* g4 = (const float4*)g;
        float4* m4 = (float4*)m;
        float4* v4 = (float4*)v;
        for (long i = threadIdx.x; i < n4; i += 512) {
            const long j = i + 256;
            const bool two = j < n4;
            float4 pa = p4[i], ga = g4[i], ma = m4[i], va = v4[i];
            float4 pb = pa, gb = ga, mb = ma, vb = va;
            if (two) { pb = p4[j]; gb = g4[j]; mb = m4[j]; vb = v4[j]; }
            adam_elem(pa.x, ga.x, ma.x, va.x, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
            adam_elem(pa.y, ga.y, ma.y, va.y, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
            adam_elem(pa.z, ga.z, ma.z, va.z, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
            adam_elem(pa.w, ga.w, ma.w, va.w, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
            p4[i] = pa; m4[i] = ma; v4[i] = va;
            if (two) {
                adam_elem(pb.x, gb.x, mb.x, vb.x, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
                adam_elem(pb.y, gb.y, mb.y, vb.y, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
                adam_elem(pb.z, gb.z, mb.z, vb.z, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
                adam_elem(pb.w, gb.w, mb.w, vb.w, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
                p4[j] = pb; m4[j] = mb; v4[j] = vb;
            }
        }
        done = n4 << 2;
    }
    for (long i = done + threadIdx.x; i < n; i += 256) {
        float pv = p[i], mv = m[i], vv = v[i];
        adam_elem(pv, g[i], mv, vv, decoupled, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
        m[i] = mv;
        v[i] = vv;
        p[i] = pv;
    }
}
__global__ __launch_bounds__(256) void adam_kernel(const long* __restrict__ tab, float lr, float beta1, float beta2, float eps, float wd,
                                                   float bc1, float bc2_sqrt) {
    const long* e = tab + (long)blockIdx.x * CH;
    adam_row(e, e[6] & 1, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
}
__device__ __forceinline__ void sgd_row(const long* __restrict__ e, float lr, float momentum, float wd, int first) {
    float* p = (float*)e[1];
    const float* g = (const float*)e[2];
    float* buf = (float*)e[3];
    const long n = e[5];
    for (long i = threadIdx.x; i < n; i += 256) {
        float d = fmaf(wd, p[i], g[i]);
        if (momentum != 0.f) {
            d = first ? d : fmaf(momentum, buf[i], d);
            buf[i] = d;
        }
        p[i] = fmaf(-lr, d, p[i]);
    }
}
__global__ __launch_bounds__(256) void sgd_kernel(const long* __restrict__ tab, float lr, float momentum, float wd, int first) {
    sgd_row(tab + (long)blockIdx.x * CH, lr, momentum, wd, first);
}

// ---- group-aware steps: ONE launch over the joined table of every param group.  A row names its hyper entry in the upper half of the flag column
// (flag >> 32); the entries travel BY VALUE in the kernel-argument segment (64 x 32 bytes = 2 KB of the 4 KB HIP allows): nothing is uploaded per
// step and no buffer can be overwritten under a step still queued.  The index comes from the table through blockIdx, so it is uniform for the
// workgroup and the entry is fetched with scalar loads from the argument segment.  The launch serves the entries [base, base + count): a row naming
// another entry returns before it reads anything else - an index never becomes an address outside the array.
constexpr int GROUPS_CAP = MFVIT_OPTIM_GROUPS_PER_LAUNCH;
struct adam_entry { float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt; unsigned decoupled; };
struct adam_entries { adam_entry e[GROUPS_CAP]; };
struct sgd_entry { float lr, momentum, wd, unused; };
struct sgd_entries { sgd_entry e[GROUPS_CAP]; };
static_assert(sizeof(adam_entries) == 2048 && sizeof(sgd_entries) == 1024, "entries are passed by value: stay well inside the 4 KB argument segment");

__device__ __forceinline__ unsigned row_entry(const long* e) { return (unsigned)((unsigned long)e[6] >> 32); }

__global__ __launch_bounds__(256) void adam_groups_kernel(const long* __restrict__ tab, const adam_entries hy, unsigned base, unsigned count) {
    const long* e = tab + (long)blockIdx.x * CH;
    const unsigned k = row_entry(e) - base;          // (an index below `base` wraps to a large value)
    if (k >= count) return;
    const adam_entry& h = hy.e[k];
    adam_row(e, h.decoupled != 0, h.lr, h.beta1, h.beta2, h.eps, h.wd, h.bc1, h.bc2_sqrt);
}
__global__ __launch_bounds__(256) void sgd_groups_kernel(const long* __restrict__ tab, const sgd_entries hy, unsigned base, unsigned count) {
    const long* e = tab + (long)blockIdx.x * CH;
    const unsigned k = row_entry(e) - base;
    if (k >= count) return;
    const sgd_entry& h = hy.e[k];
    sgd_row(e, h.lr, h.momentum, h.wd, 0);
}

// GradScaler.unscale_ (MAIN_MOCO:546-548 -> torch.cuda.amp.GradScaler.step): g *= inv_scale over every chunk of the table and
// *found_inf = 1 as soon as one gradient element is not finite (one flag store per wave that saw one; the flag is never cleared here).
__global__ __launch_bounds__(256) void amp_unscale_kernel(const long* __restrict__ tab, float inv_scale, float* __restrict__ found_inf) {
    const long* e = tab + (long)blockIdx.x * CH;
    float* g = (float*)e[2];
    const long n = e[5];
    bool bad = false;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float v = g[i];
        bad |= !(fabsf(v) <= 3.402823466e+38f);     // inf or nan
        g[i] = v * inv_scale;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) *found_inf = 1.0f;
}

// ---- gradient-norm clipping (torch.nn.utils.clip_grad_norm_): norm pass -> finalize -> scale pass, every sum in a fixed order.
// One gradient pointer per row, so a row off a 16-byte boundary is not read element by element: `head` (0..3) floats up to the boundary,
// 16-byte groups behind them, at most 3 floats of tail.
__device__ __forceinline__ long grad_head(const float* g, long n) {
    const long h = (long)((16 - ((size_t)g & 15)) & 15) >> 2;
    return h < n ? h : n;
}
// |x| as its bit pattern: non-negative floats order like integers, and every NaN lies above inf - an integer max keeps a NaN where fmaxf drops it
__device__ __forceinline__ int abs_bits(float x) { return __builtin_bit_cast(int, x) & 0x7fffffff; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// partials[row] = sum g^2 (KIND 0) or max |g| (KIND 1) of the row.  4 bytes of HBM traffic per element, two independent 16-byte loads per thread
// in flight.  Summation order (KIND 0; the tests' gate is derived from it): thread t takes the head element t into s0, the groups t, t + 512, ...
// into s0 and t + 256, t + 768, ... into s1, element by element with one fmaf each, the tail element t into s1, then s0 + s1, the 6 shuffle
// levels of wave_sum and the 4 wave sums in order.  A row of CHUNK = 16,384 elements: at most 8 groups = 32 roundings per accumulator.
template <int KIND> __global__ __launch_bounds__(256) void grad_norm_kernel(const long* __restrict__ tab, float* __restrict__ partials) {
    const long* e = tab + (long)blockIdx.x * CH;
    const float* g = (const float*)e[2];
    const long n = e[5];
    const long head = grad_head(g, n);
    const long n4 = (n - head) >> 2;
    const float4* g4 = (const float4*)(g + head);
    const float* tail = g + head + (n4 << 2);
    const long ntail = n - head - (n4 << 2);
    const int t = threadIdx.x;
    __shared__ float sc[4];
    if (KIND == 0) {
        float s0 = 0.f, s1 = 0.f;
        if (t < head) s0 = g[t] * g[t];
        for (long i = t; i < n4; i += 512) {
            const long j = i + 256;
            const bool two = j < n4;
            const float4 a = g4[i];
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (two) b = g4[j];
            s0 = fmaf(a.x, a.x, s0); s0 = fmaf(a.y, a.y, s0); s0 = fmaf(a.z, a.z, s0); s0 = fmaf(a.w, a.w, s0);
            s1 = fmaf(b.x, b.x, s1); s1 = fmaf(b.y, b.y, s1); s1 = fmaf(b.z, b.z, s1); s1 = fmaf(b.w, b.w, s1);
        }
        if (t < ntail) s1 = fmaf(tail[t], tail[t], s1);
        const float s = block_sum<256>(s0 + s1, sc);
        if (t == 0) partials[blockIdx.x] = s;
    } else {
        int m0 = 0, m1 = 0;
        if (t < head) m0 = abs_bits(g[t]);
        for (long i = t; i < n4; i += 512) {
            const long j = i + 256;
            const bool two = j < n4;
            const float4 a = g4[i];
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (two) b = g4[j];
            m0 = imax(imax(m0, abs_bits(a.x)), imax(abs_bits(a.y), imax(abs_bits(a.z), abs_bits(a.w))));
            m1 = imax(imax(m1, abs_bits(b.x)), imax(abs_bits(b.y), imax(abs_bits(b.z), abs_bits(b.w))));
        }
        if (t < ntail) m1 = imax(m1, abs_bits(tail[t]));
        int m = imax(m0, m1);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = imax(m, __shfl_xor(m, o, 64));
        int* si = (int*)sc;
        if ((t & 63) == 0) si[t >> 6] = m;
        __syncthreads();
        if (t == 0) partials[blockIdx.x] = __builtin_bit_cast(float, imax(imax(si[0], si[1]), imax(si[2], si[3])));
    }
}

// One workgroup.  Total: thread t sums the partials t, t + 256, ... in double in row order, then a fixed tree over the 256 threads (inf norm: the
// integer max of the bit patterns, exact).  Per-tensor norms (optional): thread k owns the tensors k, k + 256, ... and adds the partials of their rows
// in row order; the rows pass through LDS 256 at a time.
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const float* __restrict__ partials, const int* __restrict__ row_tensor, int nrows,
                                                             int ntensors, int kind, double max_norm, float* __restrict__ per_tensor,
                                                             float* __restrict__ out2) {
    const int t = threadIdx.x;
    __shared__ double red[256];
    __shared__ float sp[256];
    __shared__ int st[256];
    double acc = 0.0;          // non-negative either way; the inf norm carries |g| bit patterns as integers
    int mx = 0;
    for (int r = t; r < nrows; r += 256) {
        acc += (double)partials[r];
        mx = imax(mx, abs_bits(partials[r]));
    }
    if (kind == 0) {
        red[t] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) red[t] += red[t + o];
            __syncthreads();
        }
    } else {
        int* ri = (int*)red;
        ri[t] = mx;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) ri[t] = imax(ri[t], ri[t + o]);
            __syncthreads();
        }
    }
    if (t == 0) {
        const double total = kind == 0 ? sqrt(red[0]) : (double)__builtin_bit_cast(float, ((int*)red)[0]);
        const double c = max_norm / (total + 1e-6);
        out2[0] = (float)total;
        out2[1] = (float)(c > 1.0 ? 1.0 : c);      // (not fmin: a NaN total must give a NaN coefficient, as torch's clamp does)
    }
    if (!per_tensor) return;
    for (int k0 = 0; k0 < ntensors; k0 += 256) {
        const int k = k0 + t;
        double a = 0.0;
        int m = 0;
        for (int r0 = 0; r0 < nrows; r0 += 256) {
            __syncthreads();
            if (r0 + t < nrows) { sp[t] = partials[r0 + t]; st[t] = row_tensor[r0 + t]; }
            __syncthreads();
            const int cnt = nrows - r0 < 256 ? nrows - r0 : 256;
            for (int r = 0; r < cnt; ++r)
                if (st[r] == k) { a += (double)sp[r]; m = imax(m, abs_bits(sp[r])); }
        }
        if (k < ntensors) per_tensor[k] = kind == 0 ? (float)sqrt(a) : __builtin_bit_cast(float, m);
    }
}

// g *= *coef; 8 bytes of HBM traffic per element when the step clips, none when it does not: a coefficient of exactly 1 returns before any access
__global__ __launch_bounds__(256) void grad_scale_kernel(const long* __restrict__ tab, const float* __restrict__ coef) {
    const float c = *coef;
    if (c == 1.0f) return;
    const long* e = tab + (long)blockIdx.x * CH;
    float* g = (float*)e[2];
    const long n = e[5];
    const long head = grad_head(g, n);
    const long n4 = (n - head) >> 2;
    float4* g4 = (float4*)(g + head);
    float* tail = g + head + (n4 << 2);
    const long ntail = n - head - (n4 << 2);
    const int t = threadIdx.x;
    if (t < head) g[t] *= c;
    for (long i = t; i < n4; i += 512) {
        const long j = i + 256;
        const bool two = j < n4;
        float4 a = g4[i];
        float4 b = a;
        if (two) b = g4[j];
        a.x *= c; a.y *= c; a.z *= c; a.w *= c;
        g4[i] = a;
        if (two) {
            b.x *= c; b.y *= c; b.z *= c; b.w *= c;
            g4[j] = b;
        }
    }
    if (t < ntail) tail[t] *= c;
}

// ---- sharpness-aware minimisation (SAM, Foret et al. 2021; ASAM, Kwon et al. 2021): norm pass -> scale -> perturb ... restore, on the same tables
// with state0 = old_p.  The norm must be complete before the first parameter moves (every e depends on the total), so perturb cannot fuse with it.
// Four floats from p: one 16-byte load when p is on a boundary (`vec`), four 4-byte loads otherwise.
__device__ __forceinline__ float4 load4(const float* p, bool vec) {
    if (vec) return *(const float4*)p;
    return make_float4(p[0], p[1], p[2], p[3]);
}
// A product / a sum rounded to float on its own.  (__fmul_rn / __fadd_rn of this toolchain are a plain `x * y` / `x + y`, which the default
// -ffp-contract=fast-honor-pragmas fuses into an fma with its neighbour: the pragma is what keeps them apart.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
// the addend of the adaptive norm: t = |w| g rounded once, t^2 goes into the fmaf unrounded
__device__ __forceinline__ float asam_t(float w, float g) { return mul_rn(fabsf(w), g); }

// partials[row] = sum (|w| g)^2.  The split and the summation order are grad_norm_kernel<0>'s, taken from the GRADIENT pointer: head elements up to
// g's 16-byte boundary, groups behind them, tail.  w is read in 16-byte groups when it has g's phase and element by element otherwise - the same
// elements meet the same accumulators either way, so the partial does not depend on w's phase.  8 bytes of HBM traffic per element.
__global__ __launch_bounds__(256) void sam_norm_adaptive_kernel(const long* __restrict__ tab, float* __restrict__ partials) {
    const long* e = tab + (long)blockIdx.x * CH;
    const float* w = (const float*)e[1];
    const float* g = (const float*)e[2];
    const long n = e[5];
    const long head = grad_head(g, n);
    const long n4 = (n - head) >> 2;
    const bool wvec = (((size_t)w ^ (size_t)g) & 15) == 0;
    const float* gb = g + head;
    const float* wb = w + head;
    const long toff = head + (n4 << 2);
    const long ntail = n - toff;
    const int t = threadIdx.x;
    __shared__ float sc[4];
    float s0 = 0.f, s1 = 0.f;
    if (t < head) { const float x = asam_t(w[t], g[t]); s0 = x * x; }
    for (long i = t; i < n4; i += 512) {
        const long j = i + 256;
        const bool two = j < n4;
        const float4 ga = *(const float4*)(gb + (i << 2));
        const float4 wa = load4(wb + (i << 2), wvec);
        float4 gq = make_float4(0.f, 0.f, 0.f, 0.f), wq = gq;
        if (two) { gq = *(const float4*)(gb + (j << 2)); wq = load4(wb + (j << 2), wvec); }
        const float ax = asam_t(wa.x, ga.x), ay = asam_t(wa.y, ga.y), az = asam_t(wa.z, ga.z), aw = asam_t(wa.w, ga.w);
        const float bx = asam_t(wq.x, gq.x), by = asam_t(wq.y, gq.y), bz = asam_t(wq.z, gq.z), bw = asam_t(wq.w, gq.w);
        s0 = fmaf(ax, ax, s0); s0 = fmaf(ay, ay, s0); s0 = fmaf(az, az, s0); s0 = fmaf(aw, aw, s0);
        s1 = fmaf(bx, bx, s1); s1 = fmaf(by, by, s1); s1 = fmaf(bz, bz, s1); s1 = fmaf(bw, bw, s1);
    }
    if (t < ntail) { const float x = asam_t(w[toff + t], g[toff + t]); s1 = fmaf(x, x, s1); }
    const float s = block_sum<256>(s0 + s1, sc);
    if (t == 0) partials[blockIdx.x] = s;
}

// One workgroup.  The total of the partials in double, in grad_clip_coef_kernel's order (thread t: rows t, t + 256, ... then the tree), then
// out2[0] = |.|, out2[1] = 1 / (|.| + 1e-12) - the rho of `rho / (grad_norm + 1e-12)` belongs to the param group and is applied by the perturb
// pass.  out2[1] = 0 says "do not move": the total is not finite, or the GradScaler's flag is set.
__global__ __launch_bounds__(256) void sam_scale_kernel(const float* __restrict__ partials, int nrows, const float* __restrict__ found_inf,
                                                        float* __restrict__ out2) {
    const int t = threadIdx.x;
    __shared__ double red[256];
    double acc = 0.0;
    for (int r = t; r < nrows; r += 256) acc += (double)partials[r];
    red[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const double total = sqrt(red[0]);
        const bool ok = total <= 1.7976931348623157e308 && !(found_inf && *found_inf != 0.f);      // (a NaN total compares false)
        out2[0] = (float)total;
        out2[1] = ok ? (float)(1.0 / (total + 1e-12)) : 0.f;
    }
}

// e = g s (flag bit 0: e = ((w w) g) s), old_p = w, w = w + e with s = rho *inv; every product and the sum rounded on its own (no fma), so a host
// restatement gives the same bits.  16 bytes of HBM traffic per element; *inv == 0 returns before any other access.
__device__ __forceinline__ float sam_elem(float w, float g, float s, bool adaptive) {
    const float e = adaptive ? mul_rn(mul_rn(mul_rn(w, w), g), s) : mul_rn(g, s);
    return add_rn(w, e);
}
__device__ __forceinline__ float4 sam_elem4(float4 w, float4 g, float s, bool adaptive) {
    return make_float4(sam_elem(w.x, g.x, s, adaptive), sam_elem(w.y, g.y, s, adaptive), sam_elem(w.z, g.z, s, adaptive), sam_elem(w.w, g.w, s, adaptive));
}
__global__ __launch_bounds__(256) void sam_perturb_kernel(const long* __restrict__ tab, const float* __restrict__ inv, float rho) {
    const float iv = *inv;
    if (iv == 0.f) return;
    const float s = mul_rn(rho, iv);
    const long* e = tab + (long)blockIdx.x * CH;
    float* w = (float*)e[1];
    const float* g = (const float*)e[2];
    float* old = (float*)e[3];
    const long n = e[5];
    const bool adaptive = e[6] & 1;
    const int t = threadIdx.x;
    if (((((size_t)w ^ (size_t)g) | ((size_t)w ^ (size_t)old)) & 15) != 0) {       // the three phases differ: element by element
        for (long i = t; i < n; i += 256) {
            const float wv = w[i];
            old[i] = wv;
            w[i] = sam_elem(wv, g[i], s, adaptive);
        }
        return;
    }
    const long head = grad_head(w, n);
    const long n4 = (n - head) >> 2;
    float4* w4 = (float4*)(w + head);
    const float4* g4 = (const float4*)(g + head);
    float4* o4 = (float4*)(old + head);
    const long toff = head + (n4 << 2);
    const long ntail = n - toff;
    if (t < head) { const float wv = w[t]; old[t] = wv; w[t] = sam_elem(wv, g[t], s, adaptive); }
    for (long i = t; i < n4; i += 512) {
        const long j = i + 256;
        const bool two = j < n4;
        const float4 wa = w4[i], ga = g4[i];
        float4 wb = wa, gb = ga;
        if (two) { wb = w4[j]; gb = g4[j]; }
        o4[i] = wa;
        w4[i] = sam_elem4(wa, ga, s, adaptive);
        if (two) {
            o4[j] = wb;
            w4[j] = sam_elem4(wb, gb, s, adaptive);
        }
    }
    if (t < ntail) { const float wv = w[toff + t]; old[toff + t] = wv; w[toff + t] = sam_elem(wv, g[toff + t], s, adaptive); }
}

// w = old_p: 8 bytes of HBM traffic per element, none when nothing was perturbed (*inv == 0)
__global__ __launch_bounds__(256) void sam_restore_kernel(const long* __restrict__ tab, const float* __restrict__ inv) {
    if (*inv == 0.f) return;
    const long* e = tab + (long)blockIdx.x * CH;
    float* w = (float*)e[1];
    const float* old = (const float*)e[3];
    const long n = e[5];
    const int t = threadIdx.x;
    if ((((size_t)w ^ (size_t)old) & 15) != 0) {
        for (long i = t; i < n; i += 256) w[i] = old[i];
        return;
    }
    const long head = grad_head(w, n);
    const long n4 = (n - head) >> 2;
    float4* w4 = (float4*)(w + head);
    const float4* o4 = (const float4*)(old + head);
    const long toff = head + (n4 << 2);
    const long ntail = n - toff;
    if (t < head) w[t] = old[t];
    for (long i = t; i < n4; i += 512) {
        const long j = i + 256;
        const bool two = j < n4;
        const float4 a = o4[i];
        float4 b = a;
        if (two) b = o4[j];
        w4[i] = a;
        if (two) w4[j] = b;
    }
    if (t < ntail) w[toff + t] = old[toff + t];
}

}  // namespace mfvit

using namespace mfvit;

extern "C" {

int mfvit_lars_step(const int64_t* table, int nchunks, int ntensors, float* norms, float lr, float weight_decay, float momentum,
                    float trust_coefficient, mfvit_stream_t stream) {
    if (!table || !norms || nchunks <= 0 || ntensors <= 0) return MFVIT_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(norms, 0, sizeof(float) * 2 * ntensors, st) != hipSuccess) return MFVIT_ELAUNCH;
    MFVIT_LAUNCH(lars_norms_kernel, dim3(nchunks), dim3(256), 0, st, (const long*)table, weight_decay, norms);
    MFVIT_CHECK_LAUNCH();
    MFVIT_LAUNCH(lars_update_kernel, dim3(nchunks), dim3(256), 0, st, (const long*)table, norms, lr, weight_decay, momentum,
                       trust_coefficient);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_adam_step(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    mfvit_stream_t stream) {
    if (!table || nchunks <= 0 || step <= 0) return MFVIT_EINVAL;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
    MFVIT_LAUNCH(adam_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, lr, beta1, beta2, eps, weight_decay,
                       bc1, bc2s);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_adam_step_groups(const int64_t* table, int nchunks, const mfvit_adam_group* hyper, int nentries, mfvit_stream_t stream) {
    if (!table || !hyper || nchunks <= 0 || nentries <= 0) return MFVIT_EINVAL;
    for (int i = 0; i < nentries; ++i)
        if (hyper[i].step <= 0) return MFVIT_EINVAL;
    for (int base = 0; base < nentries; base += GROUPS_CAP) {
        const int count = nentries - base < GROUPS_CAP ? nentries - base : GROUPS_CAP;
        adam_entries hy = {};
        for (int i = 0; i < count; ++i) {
            const mfvit_adam_group& g = hyper[base + i];
            adam_entry& d = hy.e[i];
            d.lr = g.lr; d.beta1 = g.beta1; d.beta2 = g.beta2; d.eps = g.eps; d.wd = g.weight_decay;
            d.bc1 = 1.f - powf(g.beta1, (float)g.step);                      // (the float expressions of mfvit_adam_step)
            d.bc2_sqrt = sqrtf(1.f - powf(g.beta2, (float)g.step));
            d.decoupled = g.decoupled != 0;
        }
        MFVIT_LAUNCH(adam_groups_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, hy, (unsigned)base, (unsigned)count);
        MFVIT_CHECK_LAUNCH();
    }
    return MFVIT_OK;
}
int mfvit_sgd_step_groups(const int64_t* table, int nchunks, const mfvit_sgd_group* hyper, int nentries, mfvit_stream_t stream) {
    if (!table || !hyper || nchunks <= 0 || nentries <= 0) return MFVIT_EINVAL;
    for (int base = 0; base < nentries; base += GROUPS_CAP) {
        const int count = nentries - base < GROUPS_CAP ? nentries - base : GROUPS_CAP;
        sgd_entries hy = {};
        for (int i = 0; i < count; ++i) {
            const mfvit_sgd_group& g = hyper[base + i];
            hy.e[i].lr = g.lr; hy.e[i].momentum = g.momentum; hy.e[i].wd = g.weight_decay;
        }
        MFVIT_LAUNCH(sgd_groups_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, hy, (unsigned)base, (unsigned)count);
        MFVIT_CHECK_LAUNCH();
    }
    return MFVIT_OK;
}
int mfvit_amp_unscale(const int64_t* table, int nchunks, float inv_scale, float* found_inf, mfvit_stream_t stream) {
    if (!table || !found_inf || nchunks <= 0) return MFVIT_EINVAL;
    MFVIT_LAUNCH(amp_unscale_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, inv_scale, found_inf);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_grad_norm_partials(const int64_t* table, int nchunks, int norm_kind, float* partials, mfvit_stream_t stream) {
    if (!table || !partials || nchunks <= 0 || (norm_kind != 0 && norm_kind != 1)) return MFVIT_EINVAL;
    if (norm_kind == 0)
        MFVIT_LAUNCH(grad_norm_kernel<0>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, partials);
    else
        MFVIT_LAUNCH(grad_norm_kernel<1>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, partials);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_grad_clip_coef(const float* partials, const int32_t* row_tensor, int nrows, int ntensors, int norm_kind, double max_norm,
                         float* per_tensor, float* out2, mfvit_stream_t stream) {
    if (!partials || !out2 || nrows <= 0 || ntensors <= 0 || (norm_kind != 0 && norm_kind != 1)) return MFVIT_EINVAL;
    if (per_tensor && !row_tensor) return MFVIT_EINVAL;
    MFVIT_LAUNCH(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (const int*)row_tensor, nrows, ntensors, norm_kind,
                       max_norm, per_tensor, out2);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_grad_scale(const int64_t* table, int nchunks, const float* coef, mfvit_stream_t stream) {
    if (!table || !coef || nchunks <= 0) return MFVIT_EINVAL;
    MFVIT_LAUNCH(grad_scale_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, coef);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_sam_norm_partials(const int64_t* table, int nchunks, int adaptive, float* partials, mfvit_stream_t stream) {
    if (!table || !partials || nchunks <= 0 || (adaptive != 0 && adaptive != 1)) return MFVIT_EINVAL;
    if (adaptive == 0)          // the plain L2 norm of the gradients: the clipping kernel itself, so the partials are its bits
        MFVIT_LAUNCH(grad_norm_kernel<0>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, partials);
    else
        MFVIT_LAUNCH(sam_norm_adaptive_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, partials);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_sam_scale(const float* partials, int nrows, const float* found_inf, float* out2, mfvit_stream_t stream) {
    if (!partials || !out2 || nrows <= 0) return MFVIT_EINVAL;
    MFVIT_LAUNCH(sam_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nrows, found_inf, out2);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_sam_perturb(const int64_t* table, int nchunks, const float* inv, float rho, mfvit_stream_t stream) {
    if (!table || !inv || nchunks <= 0) return MFVIT_EINVAL;
    MFVIT_LAUNCH(sam_perturb_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, inv, rho);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_sam_restore(const int64_t* table, int nchunks, const float* inv, mfvit_stream_t stream) {
    if (!table || !inv || nchunks <= 0) return MFVIT_EINVAL;
    MFVIT_LAUNCH(sam_restore_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, inv);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
int mfvit_sgd_step(const int64_t* table, int nchunks, float lr, float momentum, float weight_decay, int first_step,
                   mfvit_stream_t stream) {
    if (!table || nchunks <= 0) return MFVIT_EINVAL;
    MFVIT_LAUNCH(sgd_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)table, lr, momentum, weight_decay, first_step);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // extern "C"
