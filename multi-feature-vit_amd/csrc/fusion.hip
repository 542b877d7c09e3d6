// Cross-attention token exchange + two-stream late fusion (Fus_CrossViT) on gfx950, forward and backward, all f32.
//
// Reference (paths relative to /root/reference/moco_pretraining/moco):
//   model/module.py:15-21      PreNorm (LayerNorm eps 1e-5)          model/module.py:108-137  CrossAttention (3 heads x 128)
//   model/crossvit_2vits_..._std002_sum.py:35-65   MultiScaleTransformerEncoder.forward (bidirectional cls<->patch exchange)
//   model/crossvit_2vits_..._std002_sum.py:126-157 Fus_CrossViT.forward (residual, cls pool, two heads, sum)
//
// Algebra: the query is ONE row (the cls token), so per head h
//     scores_h[t] = scale * z_t . (Wk_h^T (Wq z_0)_h)            =: scale * z_t . kq_h
//     attn_h . V_h = Wv_h (sum_t a_h[t] z_t)                     =: Wv_h u_h
// i.e. the two (B*T) x 384 x 384 K/V projections (99% of the reference's 117 MFLOP per direction) fold into three
// 384-vectors per sample.  What remains is HBM-bound: one streaming pass pair over the (B, T, 384) tokens of the other
// stream (roofline: HBM bytes = tokens read twice, second time from L2), plus batch-sized f32 MFMA GEMMs.
// With one exchange layer and pool = 'cls' only row 0 of the post-exchange LayerNorm / residual is consumed (FUS:144-145), so only that
// row is computed.  Deeper stacks (cross_attn_depth > 1) and pool = 'mean' take the full-row path (x_rows_* / x_post0_bwd / x_head_*,
// mfvit_fusion_ex_*): every layer's post-LN rows are materialised.  Kernels are templates on the width D (384 | 768); heads beyond 3 run
// in chunks of 3 (gridDim.z) with the token gradient of the backward in x_stream_dz_kernel.
//
// Parameter arena (f32, state-dict order of Fus_CrossViT; 8 D^2 + 10 D + 2 (C D + C) floats):
//   [0].norm.{w,b} [0].fn.{wq,wk,wv,proj.w,proj.b}  [1].{w,b}  [2].norm.{w,b} [2].fn.{...}  [3].{w,b}
//   mlp_head_cxr.0.{w,b}  mlp_head_enh.0.{w,b}
// Direction 0: CXR cls attends ENH patches through [0], post-norm [3], head cxr   (FUS:57-63)
// Direction 1: ENH cls attends CXR patches through [2], post-norm [1], head enh   (FUS:48-55)
#include "kernels.h"
#include "prof.h"

#include <string.h>

using namespace mfvit;

namespace {

constexpr int NH = 3;   // heads per streaming-pass workgroup (a head chunk; more heads run as more chunks, see x_stream_fwd_kernel)

struct FusLayout {  // parameter offsets (floats)
    long ca[2], post[2], head[2];
    long n_w, n_b, wq, wk, wv, wp, bp;  // inside a CA block
    long ca_stride;
    long total;
    int no_norm;   // bare CrossAttention (MOD:123-137 without the PreNorm around it): z = x, the norm entries of a block are never touched
};
FusLayout fus_layout(int D, int C) {
    FusLayout L;
    const long blk = 4L * D * D + 3L * D;
    L.n_w = 0; L.n_b = D; L.wq = 2L * D; L.wk = L.wq + (long)D * D; L.wv = L.wk + (long)D * D; L.wp = L.wv + (long)D * D;
    L.bp = L.wp + (long)D * D;
    const long o0 = 0, o1 = blk, o2 = o1 + 2 * D, o3 = o2 + blk, oh = o3 + 2 * D;
    L.ca[0] = o0; L.ca[1] = o2;
    L.post[0] = o3; L.post[1] = o1;
    L.head[0] = oh; L.head[1] = oh + (long)C * D + C;
    L.ca_stride = o2 - o0;
    L.total = oh + 2 * ((long)C * D + C);
    L.no_norm = 0;
    return L;
}

struct FusWs {  // workspace offsets (floats)
    long z0, st0, qv, kq, u, a, st, o, outp, fus, stc;          // forward (kept for backward)
    long wT;                                                     // [2][4][D*D] transposed wq, wk, wv, wp
    long dout, dqp, dob, du, dkq, dz0p, dqv, dz0q;               // backward scratch
    // per-sample partials of the small parameter gradients (round 6: plain stores + one fixed-order reduce instead of float atomics - the same bits on every run):
    //   pa [2][B][3 D]    d post-LN weight | bias | d proj.bias          (x_finish_bwd)
    //   pb [2][B][2 C D]  d head weight | d backbone-head weight          (x_finish_bwd)
    //   pc [2][B][2 C]    d head bias | d backbone-head bias              (x_finish_bwd)
    //   pd [2][2 B][2 D]  d pre-norm weight | bias: rows 0 .. B - 1 from x_stream_bwd (token rows 1 ..), rows B .. 2 B - 1 from x_row0_bwd (the cls row)
    long pa, pb, pc, pd;
    long ds;       // [2][B][heads][T] d scores of the chunked backward (heads > 3 only, x_stream_bwd_kernel<.., true> -> x_stream_dz_kernel)
    long total;
};
FusWs fus_ws(int B, int T, int C, int D, int NH) {
    FusWs W;
    long o = 0;
    auto take = [&](long n) { long r = o; o += (n + 63) & ~63L; return r; };
    W.z0 = take(2L * B * D); W.st0 = take(2L * B * 2); W.qv = take(2L * B * D); W.kq = take(2L * B * NH * D);
    W.u = take(2L * B * NH * D); W.a = take(2L * B * NH * T); W.st = take(2L * B * 2 * T); W.o = take(2L * B * D);
    W.outp = take(2L * B * D); W.fus = take(2L * B * D); W.stc = take(2L * B * 2);
    W.wT = take(2L * 4 * D * D);
    W.dout = take(2L * B * D); W.dqp = take(2L * B * D); W.dob = take(2L * B * D); W.du = take(2L * B * NH * D);
    W.dkq = take(2L * B * NH * D); W.dz0p = take(2L * B * D); W.dqv = take(2L * B * D); W.dz0q = take(2L * B * D);
    W.pa = take(2L * B * 3 * D); W.pb = take(2L * B * 2 * C * D); W.pc = take(2L * B * 2 * C); W.pd = take(2L * 2 * B * 2 * D);
    W.ds = NH > 3 ? take(2L * B * NH * T) : 0;
    W.total = o;
    return W;
}

// ---------------------------------------------------------------------------------------------- kernels
// Mean of a row from its sum: a true division.  sum * (1.f / D) carries the rounding of 1 / D, and with that product contracted into the
// subtraction x - mean (an fma) the error survives even where sum / D is exact: an exactly constant row came out as
// beta - 2^-26 x rstd gamma instead of beta (1.5e-5 gamma under the post-norm's eps of 1e-6), which the next layer's LayerNorm of that row
// (spread 0.05) turned into 3e-4 (tests/test_fusion_edges_gpu.py, the constant_row case on the full-row path).
template <int D> __device__ __forceinline__ float row_mean(float sum) { return sum / (float)D; }

// z0[dir][b] = LN_pre(own cls row); one wave per (b, dir)
template <int D>
__global__ __launch_bounds__(64) void x_cls_ln_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                       const float* __restrict__ params, FusLayout L, float eps, int B, int T,
                                                       float* __restrict__ z0, float* __restrict__ st0) {
    const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x;
    const float* row = (dir == 0 ? fc : fe) + (long)b * T * D;
    const float* g = params + L.ca[dir] + L.n_w;
    const float* be = params + L.ca[dir] + L.n_b;
    constexpr int NPL = D / 64;
    float v[NPL], s = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { v[i] = row[lane + 64 * i]; s += v[i]; }
    if (L.no_norm) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) z0[((long)dir * B + b) * D + lane + 64 * i] = v[i];
        if (lane == 0) { st0[((long)dir * B + b) * 2] = 0.f; st0[((long)dir * B + b) * 2 + 1] = 1.f; }
        return;
    }
    const float mu = row_mean<D>(wave_sum(s));
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { const float d = v[i] - mu; q += d * d; }
    const float rs = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
    for (int i = 0; i < NPL; ++i) z0[((long)dir * B + b) * D + lane + 64 * i] = (v[i] - mu) * rs * g[lane + 64 * i] + be[lane + 64 * i];
    if (lane == 0) { st0[((long)dir * B + b) * 2] = mu; st0[((long)dir * B + b) * 2 + 1] = rs; }
}

// Streaming pass over the T rows [own cls ; other stream's patches] of one (sample, direction):
//   stats, scores against kq_h, softmax over t, u_h = sum_t a_h[t] z_t.   LDS: sc[3][T] | st[2][T] | red[XW][18*64]
// XW waves per workgroup, a wave per row: ONE workgroup per CU (256 (sample, direction) pairs at the bench shape), so the rows in flight per
// CU are the waves of that workgroup - with four (round 1 - 3) the pass ran at 1.7 TB/s.
// CH: more than NH = 3 heads - workgroup z runs heads 3 z .. 3 z + 2 of the nh = 3 gridDim.z (the softmax is per head, so the chunks are
// independent; each re-derives the row statistics, the same values in every chunk).  A row stays NPL = D / 64 floats per lane.
template <int XW, int D, bool CH>
__global__ __launch_bounds__(XW * 64) void x_stream_fwd_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                           const float* __restrict__ params, FusLayout L, float eps, float scale, int B,
                                                           int T, const float* __restrict__ kq, float* __restrict__ u,
                                                           float* __restrict__ a_out, float* __restrict__ st_out) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    float* sc = xs;
    float* st = sc + NH * T;
    float* red = st + 2 * T;
    constexpr int NPL = D / 64;
    const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nh = CH ? NH * gridDim.z : NH, h0 = CH ? NH * blockIdx.z : 0;
    const float* own = (dir == 0 ? fc : fe) + (long)b * T * D;
    const float* oth = (dir == 0 ? fe : fc) + (long)b * T * D;
    float g[NPL], be[NPL], kqv[NH][NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        g[i] = L.no_norm ? 1.f : params[L.ca[dir] + L.n_w + lane + 64 * i];
        be[i] = L.no_norm ? 0.f : params[L.ca[dir] + L.n_b + lane + 64 * i];
#pragma unroll
        for (int h = 0; h < NH; ++h) kqv[h][i] = kq[(((long)dir * B + b) * nh + h0 + h) * D + lane + 64 * i];
    }
    for (int t = w; t < T; t += XW) {
        const float* row = t == 0 ? own : oth + (long)t * D;
        float v[NPL], s = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) { v[i] = row[lane + 64 * i]; s += v[i]; }
        const float mu = L.no_norm ? 0.f : row_mean<D>(wave_sum(s));
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) { v[i] -= mu; q += v[i] * v[i]; }
        const float rs = L.no_norm ? 1.f : rsqrtf(wave_sum(q) * (1.f / D) + eps);
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const float z = v[i] * rs * g[i] + be[i];
            d0 = fmaf(z, kqv[0][i], d0); d1 = fmaf(z, kqv[1][i], d1); d2 = fmaf(z, kqv[2][i], d2);
        }
        d0 = wave_sum(d0); d1 = wave_sum(d1); d2 = wave_sum(d2);
        if (lane == 0) {
            sc[t] = d0 * scale; sc[T + t] = d1 * scale; sc[2 * T + t] = d2 * scale;
            st[t] = mu; st[T + t] = rs;
        }
    }
    __syncthreads();
    if (w < NH) {  // softmax over t for head w
        float m = -INFINITY;
        for (int t = lane; t < T; t += 64) m = fmaxf(m, sc[w * T + t]);
        m = wave_max(m);
        float s = 0.f;
        for (int t = lane; t < T; t += 64) { const float e = __expf(sc[w * T + t] - m); sc[w * T + t] = e; s += e; }
        s = 1.f / wave_sum(s);
        for (int t = lane; t < T; t += 64) {
            const float p = sc[w * T + t] * s;
            sc[w * T + t] = p;
            a_out[(((long)dir * B + b) * nh + h0 + w) * T + t] = p;
        }
    } else if (w == NH && h0 == 0) {
        for (int t = lane; t < T; t += 64) {
            st_out[(((long)dir * B + b) * 2) * T + t] = st[t];
            st_out[(((long)dir * B + b) * 2 + 1) * T + t] = st[T + t];
        }
    }
    __syncthreads();
    float acc[NH][NPL];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int i = 0; i < NPL; ++i) acc[h][i] = 0.f;
    for (int t = w; t < T; t += XW) {
        const float* row = t == 0 ? own : oth + (long)t * D;
        const float mu = st[t], rs = st[T + t];
        const float a0 = sc[t], a1 = sc[T + t], a2 = sc[2 * T + t];
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const float z = (row[lane + 64 * i] - mu) * rs * g[i] + be[i];
            acc[0][i] = fmaf(a0, z, acc[0][i]); acc[1][i] = fmaf(a1, z, acc[1][i]); acc[2][i] = fmaf(a2, z, acc[2][i]);
        }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int i = 0; i < NPL; ++i) red[(w * NH + h) * D + lane + 64 * i] = acc[h][i];
    __syncthreads();
    for (int q = threadIdx.x; q < NH * D; q += XW * 64) {
        float v = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < XW; ++w2) v += red[w2 * NH * D + q];
        u[(((long)dir * B + b) * nh + h0) * D + q] = v;
    }
}

// cal = cls + outp ; c = LN_post(cal) ; fus_cls = cls + c ; ds = head(fus_cls) ; fused = ds_cxr + ds_enh ;
// x_S = backbone head_S(cls_S) (optional).  One block per sample, wave = direction.
template <int D>
__global__ __launch_bounds__(128) void x_finish_fwd_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                           const float* __restrict__ params, FusLayout L, float eps, int B, int T, int C,
                                                           const float* __restrict__ outp, float* __restrict__ fus,
                                                           float* __restrict__ stc, const float* __restrict__ hw_c,
                                                           const float* __restrict__ hb_c, const float* __restrict__ hw_e,
                                                           const float* __restrict__ hb_e, float* __restrict__ fused,
                                                           float* __restrict__ x_c, float* __restrict__ x_e) {
    constexpr int NPL = D / 64;
    __shared__ float dsm[2][64];
    const int b = blockIdx.x, dir = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* cls = (dir == 0 ? fc : fe) + (long)b * T * D;
    const float* op = outp + ((long)dir * B + b) * D;
    const float* g = params + L.post[dir];
    const float* be = g + D;
    float c0[NPL], v[NPL], s = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { c0[i] = cls[lane + 64 * i]; v[i] = c0[i] + op[lane + 64 * i]; s += v[i]; }
    const float mu = row_mean<D>(wave_sum(s));
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { v[i] -= mu; q += v[i] * v[i]; }
    const float rs = rsqrtf(wave_sum(q) * (1.f / D) + eps);
    float f[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        f[i] = c0[i] + v[i] * rs * g[lane + 64 * i] + be[lane + 64 * i];
        fus[((long)dir * B + b) * D + lane + 64 * i] = f[i];
    }
    if (lane == 0) { stc[((long)dir * B + b) * 2] = mu; stc[((long)dir * B + b) * 2 + 1] = rs; }
    const float* hw = params + L.head[dir];
    const float* hb = hw + (long)C * D;
    for (int c = 0; c < C; ++c) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) d = fmaf(f[i], hw[(long)c * D + lane + 64 * i], d);
        d = wave_sum(d);
        if (lane == 0) dsm[dir][c] = d + hb[c];
    }
    const float* bw = dir == 0 ? hw_c : hw_e;
    const float* bb = dir == 0 ? hb_c : hb_e;
    float* xo = dir == 0 ? x_c : x_e;
    if (bw && xo) {
        for (int c = 0; c < C; ++c) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < NPL; ++i) d = fmaf(c0[i], bw[(long)c * D + lane + 64 * i], d);
            d = wave_sum(d);
            if (lane == 0) xo[(long)b * C + c] = d + (bb ? bb[c] : 0.f);
        }
    }
    __syncthreads();
    if (threadIdx.x < C) fused[(long)b * C + threadIdx.x] = dsm[0][threadIdx.x] + dsm[1][threadIdx.x];
}

// Backward of x_finish_fwd: head, residual, post-LN; emits dout (= d outp) and the partial cls gradient dqp.
template <int D>
__global__ __launch_bounds__(128) void x_finish_bwd_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                           const float* __restrict__ params, FusLayout L, int B, int T, int C,
                                                           const float* __restrict__ outp, const float* __restrict__ fus,
                                                           const float* __restrict__ stc, const float* __restrict__ hw_c,
                                                           const float* __restrict__ hw_e, const float* __restrict__ dfused,
                                                           const float* __restrict__ dx_c, const float* __restrict__ dx_e,
                                                           float* __restrict__ dparams, float* __restrict__ dhw_c,
                                                           float* __restrict__ dhb_c, float* __restrict__ dhw_e,
                                                           float* __restrict__ dhb_e, float* __restrict__ dout, float* __restrict__ dqp,
                                                           float* __restrict__ pa, float* __restrict__ pb, float* __restrict__ pc) {
    constexpr int NPL = D / 64;
    const int b = blockIdx.x, dir = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // this sample's terms of the small parameter gradients: plain stores into its rows of the partial buffers (FusWs::pa / pb / pc), summed over the batch in a
    // fixed order by fus_reduce_partials
    float* pa_r = pa + ((long)dir * B + b) * 3 * D;
    float* pb_r = pb + ((long)dir * B + b) * 2 * C * D;
    float* pc_r = pc + ((long)dir * B + b) * 2 * C;
    const float* cls = (dir == 0 ? fc : fe) + (long)b * T * D;
    const float* op = outp + ((long)dir * B + b) * D;
    const float* g = params + L.post[dir];
    const float* hw = params + L.head[dir];
    const float mu = stc[((long)dir * B + b) * 2], rs = stc[((long)dir * B + b) * 2 + 1];
    float e[NPL], c0[NPL], f[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) { e[i] = 0.f; c0[i] = cls[lane + 64 * i]; f[i] = fus[((long)dir * B + b) * D + lane + 64 * i]; }
    for (int c = 0; c < C; ++c) {
        const float gc = dfused ? dfused[(long)b * C + c] : 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            e[i] = fmaf(gc, hw[(long)c * D + lane + 64 * i], e[i]);
            pb_r[(long)c * D + lane + 64 * i] = gc * f[i];
        }
        if (lane == 0) pc_r[c] = gc;
    }
    // post-LN backward: dc = e ; cal = cls + outp
    float xh[NPL], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        xh[i] = (c0[i] + op[lane + 64 * i] - mu) * rs;
        const float t = e[i] * g[lane + 64 * i];
        s1 += t; s2 += t * xh[i];
        pa_r[lane + 64 * i] = e[i] * xh[i];
        pa_r[D + lane + 64 * i] = e[i];
    }
    const float c1 = wave_sum(s1) * (1.f / D), c2 = wave_sum(s2) * (1.f / D);
    float dq[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const float dcal = rs * (e[i] * g[lane + 64 * i] - c1 - xh[i] * c2);
        dout[((long)dir * B + b) * D + lane + 64 * i] = dcal;
        pa_r[2 * D + lane + 64 * i] = dcal;
        dq[i] = e[i] + dcal;
    }
    // backbone classifier head on the cls row (x_S = head_S(cls_S)): FUS:131,135
    const float* bw = dir == 0 ? hw_c : hw_e;
    const float* dxs = dir == 0 ? dx_c : dx_e;
    for (int c = 0; c < C; ++c) {
        const float gc = bw && dxs ? dxs[(long)b * C + c] : 0.f;      // (no backbone head: zero rows - the reduce has no destination for them)
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            if (bw && dxs) dq[i] = fmaf(gc, bw[(long)c * D + lane + 64 * i], dq[i]);
            pb_r[(long)(C + c) * D + lane + 64 * i] = gc * c0[i];
        }
        if (lane == 0) pc_r[C + c] = gc;
    }
#pragma unroll
    for (int i = 0; i < NPL; ++i) dqp[((long)dir * B + b) * D + lane + 64 * i] = dq[i];
}

// Backward of the streaming pass.  LDS: sa[3][T] (a) | sd[3][T] (da -> ds) | st[2][T] | red[XW][5 D]
// CH (more than 3 heads): workgroup z owns heads 3 z .. 3 z + 2 and stops at dkq and the score gradients ds_out[dir][b][h][t]; the token
// gradient, which sums over ALL heads, is x_stream_dz_kernel's.
template <int XW, int D, bool CH>
__global__ __launch_bounds__(XW * 64) void x_stream_bwd_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                           const float* __restrict__ params, FusLayout L, float scale, int B, int T,
                                                           const float* __restrict__ kq, const float* __restrict__ a_in,
                                                           const float* __restrict__ st_in, const float* __restrict__ du,
                                                           float* __restrict__ dkq, float* __restrict__ dz0p, float* __restrict__ pd,
                                                           float* __restrict__ dfc, float* __restrict__ dfe, float* __restrict__ ds_out) {
    constexpr int NPL = D / 64;
    const int nh = CH ? NH * gridDim.z : NH, h0 = CH ? NH * blockIdx.z : 0;
    extern __shared__ __attribute__((aligned(16))) float xs[];
    float* sa = xs;
    float* sd = sa + NH * T;
    float* st = sd + NH * T;
    float* red = st + 2 * T;
    const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* own = (dir == 0 ? fc : fe) + (long)b * T * D;
    const float* oth = (dir == 0 ? fe : fc) + (long)b * T * D;
    float* doth = dir == 0 ? dfe : dfc;
    float g[NPL], be[NPL], kqv[NH][NPL], duv[NH][NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        g[i] = L.no_norm ? 1.f : params[L.ca[dir] + L.n_w + lane + 64 * i];
        be[i] = L.no_norm ? 0.f : params[L.ca[dir] + L.n_b + lane + 64 * i];
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            kqv[h][i] = kq[(((long)dir * B + b) * nh + h0 + h) * D + lane + 64 * i];
            duv[h][i] = du[(((long)dir * B + b) * nh + h0 + h) * D + lane + 64 * i];
        }
    }
    for (int q = threadIdx.x; q < NH * T; q += XW * 64) sa[q] = a_in[(((long)dir * B + b) * nh + h0) * T + q];
    for (int q = threadIdx.x; q < 2 * T; q += XW * 64) st[q] = st_in[((long)dir * B + b) * 2 * T + q];
    __syncthreads();
    for (int t = w; t < T; t += XW) {
        const float* row = t == 0 ? own : oth + (long)t * D;
        const float mu = st[t], rs = st[T + t];
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const float z = (row[lane + 64 * i] - mu) * rs * g[i] + be[i];
            d0 = fmaf(z, duv[0][i], d0); d1 = fmaf(z, duv[1][i], d1); d2 = fmaf(z, duv[2][i], d2);
        }
        d0 = wave_sum(d0); d1 = wave_sum(d1); d2 = wave_sum(d2);
        if (lane == 0) { sd[t] = d0; sd[T + t] = d1; sd[2 * T + t] = d2; }
    }
    __syncthreads();
    if (w < NH) {  // ds_h[t] = a_h[t] (da_h[t] - sum_t' a_h[t'] da_h[t'])
        float s = 0.f;
        for (int t = lane; t < T; t += 64) s = fmaf(sa[w * T + t], sd[w * T + t], s);
        s = wave_sum(s);
        for (int t = lane; t < T; t += 64) sd[w * T + t] = sa[w * T + t] * (sd[w * T + t] - s);
        if (CH)
            for (int t = lane; t < T; t += 64) ds_out[(((long)dir * B + b) * nh + h0 + w) * T + t] = sd[w * T + t];
    }
    __syncthreads();
    if constexpr (CH) {   // dkq_h = scale sum_t ds_h[t] z_t of this chunk's heads
        float akq[NH][NPL];
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int i = 0; i < NPL; ++i) akq[h][i] = 0.f;
        for (int t = w; t < T; t += XW) {
            const float* row = t == 0 ? own : oth + (long)t * D;
            const float mu = st[t], rs = st[T + t];
            const float s0 = sd[t] * scale, s1 = sd[T + t] * scale, s2 = sd[2 * T + t] * scale;
#pragma unroll
            for (int i = 0; i < NPL; ++i) {
                const float z = (row[lane + 64 * i] - mu) * rs * g[i] + be[i];
                akq[0][i] = fmaf(s0, z, akq[0][i]); akq[1][i] = fmaf(s1, z, akq[1][i]); akq[2][i] = fmaf(s2, z, akq[2][i]);
            }
        }
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int i = 0; i < NPL; ++i) red[(w * NH + h) * D + lane + 64 * i] = akq[h][i];
        __syncthreads();
        for (int q = threadIdx.x; q < NH * D; q += XW * 64) {
            float v = 0.f;
#pragma unroll
            for (int w2 = 0; w2 < XW; ++w2) v += red[w2 * NH * D + q];
            dkq[(((long)dir * B + b) * nh + h0) * D + q] = v;
        }
        return;
    }
    float akq[NH][NPL], ag[NPL], ab[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        ag[i] = ab[i] = 0.f;
#pragma unroll
        for (int h = 0; h < NH; ++h) akq[h][i] = 0.f;
    }
    for (int t = w; t < T; t += XW) {
        const float* row = t == 0 ? own : oth + (long)t * D;
        const float mu = st[t], rs = st[T + t];
        const float a0 = sa[t], a1 = sa[T + t], a2 = sa[2 * T + t];
        const float s0 = sd[t] * scale, s1 = sd[T + t] * scale, s2 = sd[2 * T + t] * scale;
        float xh[NPL], dz[NPL], p1 = 0.f, p2 = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            xh[i] = (row[lane + 64 * i] - mu) * rs;
            const float z = xh[i] * g[i] + be[i];
            akq[0][i] = fmaf(s0, z, akq[0][i]); akq[1][i] = fmaf(s1, z, akq[1][i]); akq[2][i] = fmaf(s2, z, akq[2][i]);
            dz[i] = a0 * duv[0][i] + a1 * duv[1][i] + a2 * duv[2][i] + s0 * kqv[0][i] + s1 * kqv[1][i] + s2 * kqv[2][i];
            const float tg = dz[i] * g[i];
            p1 += tg; p2 += tg * xh[i];
        }
        if (t == 0) {  // the cls row also receives Wq^T dqv later: LN backward for it runs in x_row0_bwd_kernel
#pragma unroll
            for (int i = 0; i < NPL; ++i) dz0p[((long)dir * B + b) * D + lane + 64 * i] = dz[i];
        } else {
#pragma unroll
            for (int i = 0; i < NPL; ++i) { ag[i] = fmaf(dz[i], xh[i], ag[i]); ab[i] += dz[i]; }
            if (doth) {
                const float c1 = L.no_norm ? 0.f : wave_sum(p1) * (1.f / D), c2 = L.no_norm ? 0.f : wave_sum(p2) * (1.f / D);
#pragma unroll
                for (int i = 0; i < NPL; ++i) doth[((long)b * T + t) * D + lane + 64 * i] = rs * (dz[i] * g[i] - c1 - xh[i] * c2);
            }
        }
    }
    // cross-wave reduce: 18 (dkq) + 6 (dgamma) + 6 (dbeta) values per lane
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
#pragma unroll
        for (int h = 0; h < NH; ++h) red[(w * 5 + h) * D + lane + 64 * i] = akq[h][i];
        red[(w * 5 + 3) * D + lane + 64 * i] = ag[i];
        red[(w * 5 + 4) * D + lane + 64 * i] = ab[i];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 5 * D; q += XW * 64) {
        float v = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < XW; ++w2) v += red[w2 * 5 * D + q];
        if (q < NH * D) dkq[((long)dir * B + b) * NH * D + q] = v;
        else if (L.no_norm) continue;
        else pd[((long)dir * 2 * B + b) * 2 * D + (q - 3 * D)] = v;        // this sample's d pre-norm weight | bias over its token rows 1 ..: row b of FusWs::pd
    }
}

// cls row of the pre-norm: dz0 = dz0p + dz0q (through Wq); LN backward; total cls gradient of the own stream.
template <int D>
__global__ __launch_bounds__(128) void x_row0_bwd_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                         const float* __restrict__ params, FusLayout L, int B, int T,
                                                         const float* __restrict__ st0, const float* __restrict__ dz0p,
                                                         const float* __restrict__ dz0q, const float* __restrict__ dqp,
                                                         float* __restrict__ pd, float* __restrict__ dfc, float* __restrict__ dfe) {
    constexpr int NPL = D / 64;
    const int b = blockIdx.x, dir = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* cls = (dir == 0 ? fc : fe) + (long)b * T * D;
    float* down = dir == 0 ? dfc : dfe;
    const float* g = params + L.ca[dir] + L.n_w;
    const float mu = st0[((long)dir * B + b) * 2], rs = st0[((long)dir * B + b) * 2 + 1];
    float dz[NPL], xh[NPL], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const long o = ((long)dir * B + b) * D + lane + 64 * i;
        dz[i] = dz0p[o] + dz0q[o];
        xh[i] = (cls[lane + 64 * i] - mu) * rs;
        if (L.no_norm) continue;
        const float t = dz[i] * g[lane + 64 * i];
        s1 += t; s2 += t * xh[i];
        pd[((long)dir * 2 * B + B + b) * 2 * D + lane + 64 * i] = dz[i] * xh[i];        // the cls row's terms: row B + b of FusWs::pd
        pd[((long)dir * 2 * B + B + b) * 2 * D + D + lane + 64 * i] = dz[i];
    }
    if (!down) return;
    if (L.no_norm) {   // (st0 = (0, 1): xh = x; no normalisation to differentiate)
#pragma unroll
        for (int i = 0; i < NPL; ++i) down[(long)b * T * D + lane + 64 * i] = dqp[((long)dir * B + b) * D + lane + 64 * i] + dz[i];
        return;
    }
    const float c1 = wave_sum(s1) * (1.f / D), c2 = wave_sum(s2) * (1.f / D);
#pragma unroll
    for (int i = 0; i < NPL; ++i)
        down[(long)b * T * D + lane + 64 * i] = dqp[((long)dir * B + b) * D + lane + 64 * i] + rs * (dz[i] * g[lane + 64 * i] - c1 - xh[i] * c2);
}

// Token gradient of the streaming pass for more than 3 heads (after x_stream_bwd_kernel<.., true>): per row t of [own cls ; other patches]
//   dz_t = sum_h a_h[t] du_h + scale ds_h[t] kq_h,  then the pre-norm LayerNorm backward as in the fused kernel.
// du_h / kq_h of all heads sit in LDS (2 heads D floats) instead of registers.  LDS: du[nh][D] | kq[nh][D] | a[nh][T] | ds[nh][T] | st[2][T];
// the cross-wave reduce buffer red[XW][2 D] reuses the front of it once the row loop is done.
template <int XW, int D>
__global__ __launch_bounds__(XW * 64) void x_stream_dz_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                          const float* __restrict__ params, FusLayout L, float scale, int B, int T, int nh,
                                                          const float* __restrict__ kq, const float* __restrict__ a_in,
                                                          const float* __restrict__ st_in, const float* __restrict__ du,
                                                          const float* __restrict__ ds_in, float* __restrict__ dz0p, float* __restrict__ pd,
                                                          float* __restrict__ dfc, float* __restrict__ dfe) {
    constexpr int NPL = D / 64;
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const long big = (long)2 * nh * D + 2L * nh * T, redn = (long)XW * 2 * D;
    float* sdu = xs;
    float* skq = sdu + nh * D;
    float* sa = skq + nh * D;
    float* sds = sa + nh * T;
    float* st = xs + (big > redn ? big : redn);
    float* red = xs;
    const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long sb = (long)dir * B + b;
    const float* own = (dir == 0 ? fc : fe) + (long)b * T * D;
    const float* oth = (dir == 0 ? fe : fc) + (long)b * T * D;
    float* doth = dir == 0 ? dfe : dfc;
    for (int q = threadIdx.x; q < nh * D; q += XW * 64) { sdu[q] = du[sb * nh * D + q]; skq[q] = kq[sb * nh * D + q]; }
    for (int q = threadIdx.x; q < nh * T; q += XW * 64) { sa[q] = a_in[sb * nh * T + q]; sds[q] = ds_in[sb * nh * T + q] * scale; }
    for (int q = threadIdx.x; q < 2 * T; q += XW * 64) st[q] = st_in[sb * 2 * T + q];
    float g[NPL], ag[NPL], ab[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) { g[i] = L.no_norm ? 1.f : params[L.ca[dir] + L.n_w + lane + 64 * i]; ag[i] = ab[i] = 0.f; }
    __syncthreads();
    for (int t = w; t < T; t += XW) {
        const float* row = t == 0 ? own : oth + (long)t * D;
        const float mu = st[t], rs = st[T + t];
        float xh[NPL], dz[NPL], p1 = 0.f, p2 = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) { xh[i] = (row[lane + 64 * i] - mu) * rs; dz[i] = 0.f; }
        for (int h = 0; h < nh; ++h) {
            const float a = sa[h * T + t], sc = sds[h * T + t];
#pragma unroll
            for (int i = 0; i < NPL; ++i) dz[i] = fmaf(sc, skq[h * D + lane + 64 * i], fmaf(a, sdu[h * D + lane + 64 * i], dz[i]));
        }
#pragma unroll
        for (int i = 0; i < NPL; ++i) { const float tg = dz[i] * g[i]; p1 += tg; p2 += tg * xh[i]; }
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < NPL; ++i) dz0p[sb * D + lane + 64 * i] = dz[i];
        } else {
#pragma unroll
            for (int i = 0; i < NPL; ++i) { ag[i] = fmaf(dz[i], xh[i], ag[i]); ab[i] += dz[i]; }
            if (doth) {
                const float c1 = L.no_norm ? 0.f : wave_sum(p1) * (1.f / D), c2 = L.no_norm ? 0.f : wave_sum(p2) * (1.f / D);
#pragma unroll
                for (int i = 0; i < NPL; ++i) doth[((long)b * T + t) * D + lane + 64 * i] = rs * (dz[i] * g[i] - c1 - xh[i] * c2);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPL; ++i) { red[(w * 2) * D + lane + 64 * i] = ag[i]; red[(w * 2 + 1) * D + lane + 64 * i] = ab[i]; }
    __syncthreads();
    if (L.no_norm) return;
    for (int q = threadIdx.x; q < 2 * D; q += XW * 64) {
        float v = 0.f;
        for (int w2 = 0; w2 < XW; ++w2) v += red[w2 * 2 * D + q];
        pd[((long)dir * 2 * B + b) * 2 * D + q] = v;
    }
}

// ------------------------------------------------------------------ full-row path (cross_attn_depth > 1 or pool = 'mean')
// Layer l of MultiScaleTransformerEncoder outputs LN_post([cls + CA ; own patches]) for ALL T rows (FUS:54-55,62-63); layer l + 1 reads them.
// Y[dir][b][t] = LN_post(t == 0 ? X_own[0] + outp : X_own[t]); the row statistics go to yst[dir][b][t][2] for the backward.
// pool (last layer only): 1 = cls: fusv = X0_own[0] + Y[0];  2 = mean: fusv = (1/T) sum_t (X0_own[t] + Y[t])  (FUS:141-145), the sum over t
// taken wave by wave and then over the waves in a fixed order.  X0 = the layer-0 input (the backbone features).
template <int XW, int D>
__global__ __launch_bounds__(XW * 64) void x_rows_fwd_kernel(const float* __restrict__ xc, const float* __restrict__ xe,
                                                         const float* __restrict__ x0c, const float* __restrict__ x0e,
                                                         const float* __restrict__ params, FusLayout L, float eps, int B, int T,
                                                         const float* __restrict__ outp, float* __restrict__ Y, float* __restrict__ yst,
                                                         int pool, float* __restrict__ fusv) {
    constexpr int NPL = D / 64;
    __shared__ float red[XW * D];
    const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long sb = (long)dir * B + b;
    const float* own = (dir == 0 ? xc : xe) + (long)b * T * D;
    const float* x0 = (dir == 0 ? x0c : x0e) + (long)b * T * D;
    const float* gp = params + L.post[dir];
    float g[NPL], be[NPL], acc[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) { g[i] = gp[lane + 64 * i]; be[i] = gp[D + lane + 64 * i]; acc[i] = 0.f; }
    for (int t = w; t < T; t += XW) {
        float v[NPL], s = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            v[i] = own[(long)t * D + lane + 64 * i] + (t == 0 ? outp[sb * D + lane + 64 * i] : 0.f);
            s += v[i];
        }
        const float mu = row_mean<D>(wave_sum(s));
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) { v[i] -= mu; q += v[i] * v[i]; }
        const float rs = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const float y = v[i] * rs * g[i] + be[i];
            Y[(sb * T + t) * D + lane + 64 * i] = y;
            if (pool == 2 || (pool == 1 && t == 0)) acc[i] += x0[(long)t * D + lane + 64 * i] + y;
        }
        if (lane == 0) { yst[(sb * T + t) * 2] = mu; yst[(sb * T + t) * 2 + 1] = rs; }
    }
    if (pool == 1 && w == 0) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) fusv[sb * D + lane + 64 * i] = acc[i];
    } else if (pool == 2) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) red[w * D + lane + 64 * i] = acc[i];
        __syncthreads();
        for (int q = threadIdx.x; q < D; q += XW * 64) {
            float v = 0.f;
            for (int w2 = 0; w2 < XW; ++w2) v += red[w2 * D + q];
            fusv[sb * D + q] = v / (float)T;
        }
    }
}

// heads on the pooled rows: ds = head(fusv) ; fused = ds_cxr + ds_enh ; x_S = backbone head_S(X0_S[0]) (optional).  One block per sample.
template <int D>
__global__ __launch_bounds__(128) void x_head_fwd_kernel(const float* __restrict__ x0c, const float* __restrict__ x0e,
                                                         const float* __restrict__ params, FusLayout L, int B, int T, int C,
                                                         const float* __restrict__ fusv, const float* __restrict__ hw_c,
                                                         const float* __restrict__ hb_c, const float* __restrict__ hw_e,
                                                         const float* __restrict__ hb_e, float* __restrict__ fused,
                                                         float* __restrict__ x_c, float* __restrict__ x_e) {
    constexpr int NPL = D / 64;
    __shared__ float dsm[2][64];
    const int b = blockIdx.x, dir = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* cls = (dir == 0 ? x0c : x0e) + (long)b * T * D;
    float c0[NPL], f[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) { c0[i] = cls[lane + 64 * i]; f[i] = fusv[((long)dir * B + b) * D + lane + 64 * i]; }
    const float* hw = params + L.head[dir];
    const float* hb = hw + (long)C * D;
    for (int c = 0; c < C; ++c) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) d = fmaf(f[i], hw[(long)c * D + lane + 64 * i], d);
        d = wave_sum(d);
        if (lane == 0) dsm[dir][c] = d + hb[c];
    }
    const float* bw = dir == 0 ? hw_c : hw_e;
    const float* bb = dir == 0 ? hb_c : hb_e;
    float* xo = dir == 0 ? x_c : x_e;
    if (bw && xo) {
        for (int c = 0; c < C; ++c) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < NPL; ++i) d = fmaf(c0[i], bw[(long)c * D + lane + 64 * i], d);
            d = wave_sum(d);
            if (lane == 0) xo[(long)b * C + c] = d + (bb ? bb[c] : 0.f);
        }
    }
    __syncthreads();
    if (threadIdx.x < C) fused[(long)b * C + threadIdx.x] = dsm[0][threadIdx.x] + dsm[1][threadIdx.x];
}

// Backward of x_head_fwd: per-sample head-gradient terms (pb / pc as in x_finish_bwd), ev = the gradient of each pooled row of X0 + Y
// (e = head^T dfused for cls, e / T for mean) and bb = the backbone head's gradient of X0[0].
template <int D>
__global__ __launch_bounds__(128) void x_head_bwd_kernel(const float* __restrict__ x0c, const float* __restrict__ x0e,
                                                         const float* __restrict__ params, FusLayout L, int B, int T, int C, int pool_mean,
                                                         const float* __restrict__ fusv, const float* __restrict__ hw_c,
                                                         const float* __restrict__ hw_e, const float* __restrict__ dfused,
                                                         const float* __restrict__ dx_c, const float* __restrict__ dx_e,
                                                         float* __restrict__ ev, float* __restrict__ bbv, float* __restrict__ pb,
                                                         float* __restrict__ pc) {
    constexpr int NPL = D / 64;
    const int b = blockIdx.x, dir = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long sb = (long)dir * B + b;
    float* pb_r = pb + sb * 2 * C * D;
    float* pc_r = pc + sb * 2 * C;
    const float* cls = (dir == 0 ? x0c : x0e) + (long)b * T * D;
    const float* hw = params + L.head[dir];
    float e[NPL], c0[NPL], f[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) { e[i] = 0.f; c0[i] = cls[lane + 64 * i]; f[i] = fusv[sb * D + lane + 64 * i]; }
    for (int c = 0; c < C; ++c) {
        const float gc = dfused ? dfused[(long)b * C + c] : 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            e[i] = fmaf(gc, hw[(long)c * D + lane + 64 * i], e[i]);
            pb_r[(long)c * D + lane + 64 * i] = gc * f[i];
        }
        if (lane == 0) pc_r[c] = gc;
    }
#pragma unroll
    for (int i = 0; i < NPL; ++i) ev[sb * D + lane + 64 * i] = pool_mean ? e[i] / (float)T : e[i];
    const float* bw = dir == 0 ? hw_c : hw_e;
    const float* dxs = dir == 0 ? dx_c : dx_e;
    float q[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) q[i] = 0.f;
    for (int c = 0; c < C; ++c) {
        const float gc = bw && dxs ? dxs[(long)b * C + c] : 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            if (bw && dxs) q[i] = fmaf(gc, bw[(long)c * D + lane + 64 * i], q[i]);
            pb_r[(long)(C + c) * D + lane + 64 * i] = gc * c0[i];
        }
        if (lane == 0) pc_r[C + c] = gc;
    }
#pragma unroll
    for (int i = 0; i < NPL; ++i) bbv[sb * D + lane + 64 * i] = q[i];
}

// Backward of row 0 of x_rows_fwd (cal = X_own[0] + outp -> LN_post): dout = dcal feeds the exchange's backward, dqp = dcal (+ ev + bb on
// layer 0, where X_own = X0 is also pooled / read by the backbone head).  dY = the full row gradient of the layer above, or ev on the top
// layer.  Partials: pr row B + b = (dy xh, dy) (post-LN weight | bias), pbp row b = dcal (proj.bias).
template <int D>
__global__ __launch_bounds__(128) void x_post0_bwd_kernel(const float* __restrict__ xc, const float* __restrict__ xe,
                                                          const float* __restrict__ params, FusLayout L, int B, int T,
                                                          const float* __restrict__ outp, const float* __restrict__ yst,
                                                          const float* __restrict__ dY, const float* __restrict__ ev,
                                                          const float* __restrict__ bbv, int first, float* __restrict__ dout,
                                                          float* __restrict__ dqp, float* __restrict__ pr, float* __restrict__ pbp) {
    constexpr int NPL = D / 64;
    const int b = blockIdx.x, dir = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long sb = (long)dir * B + b;
    const float* cls = (dir == 0 ? xc : xe) + (long)b * T * D;
    const float* g = params + L.post[dir];
    const float mu = yst[sb * T * 2], rs = yst[sb * T * 2 + 1];
    float dy[NPL], xh[NPL], s1 = 0.f, s2 = 0.f;
    float* pr_r = pr + ((long)dir * 2 * B + B + b) * 2 * D;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        dy[i] = dY ? dY[sb * T * D + lane + 64 * i] : ev[sb * D + lane + 64 * i];
        xh[i] = (cls[lane + 64 * i] + outp[sb * D + lane + 64 * i] - mu) * rs;
        const float t = dy[i] * g[lane + 64 * i];
        s1 += t; s2 += t * xh[i];
        pr_r[lane + 64 * i] = dy[i] * xh[i];
        pr_r[D + lane + 64 * i] = dy[i];
    }
    const float c1 = wave_sum(s1) * (1.f / D), c2 = wave_sum(s2) * (1.f / D);
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const float dcal = rs * (dy[i] * g[lane + 64 * i] - c1 - xh[i] * c2);
        dout[sb * D + lane + 64 * i] = dcal;
        pbp[sb * D + lane + 64 * i] = dcal;
        dqp[sb * D + lane + 64 * i] = first ? dcal + ev[sb * D + lane + 64 * i] + bbv[sb * D + lane + 64 * i] : dcal;
    }
}

// Backward of rows 1 .. T-1 of x_rows_fwd: dX_own[t] += LN_post backward of dY[t] (+ ev on layer 0 with mean pooling, where X0[t] itself is
// pooled).  dX_own rows 1 .. already hold the exchange's gradient (x_stream_bwd / x_stream_dz of the other direction).  mode: 0 = dY is a
// full (2, B, T, D) gradient, 1 = every row's gradient is ev (mean pooling, top layer), 2 = zero (cls pooling, top layer).
// Partials: pr row b = sum over t >= 1 of (dy xh, dy), per wave and then over the waves in a fixed order.
template <int XW, int D>
__global__ __launch_bounds__(XW * 64) void x_rows_bwd_kernel(const float* __restrict__ xc, const float* __restrict__ xe,
                                                         const float* __restrict__ params, FusLayout L, int B, int T,
                                                         const float* __restrict__ yst, const float* __restrict__ dY,
                                                         const float* __restrict__ ev, int mode, int add_ev, float* __restrict__ dxc,
                                                         float* __restrict__ dxe, float* __restrict__ pr) {
    constexpr int NPL = D / 64;
    __shared__ float red[XW * 2 * D];
    const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long sb = (long)dir * B + b;
    float* pr_r = pr + ((long)dir * 2 * B + b) * 2 * D;
    float* dx = dir == 0 ? dxc : dxe;
    if (mode == 2) {
        for (int q = threadIdx.x; q < 2 * D; q += XW * 64) pr_r[q] = 0.f;
        return;
    }
    const float* own = (dir == 0 ? xc : xe) + (long)b * T * D;
    const float* gp = params + L.post[dir];
    float g[NPL], e[NPL], ag[NPL], ab[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        g[i] = gp[lane + 64 * i];
        e[i] = mode == 1 || add_ev ? ev[sb * D + lane + 64 * i] : 0.f;
        ag[i] = ab[i] = 0.f;
    }
    for (int t = 1 + w; t < T; t += XW) {
        const float mu = yst[(sb * T + t) * 2], rs = yst[(sb * T + t) * 2 + 1];
        float dy[NPL], xh[NPL], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            dy[i] = mode == 0 ? dY[(sb * T + t) * D + lane + 64 * i] : e[i];
            xh[i] = (own[(long)t * D + lane + 64 * i] - mu) * rs;
            const float tg = dy[i] * g[i];
            s1 += tg; s2 += tg * xh[i];
            ag[i] = fmaf(dy[i], xh[i], ag[i]); ab[i] += dy[i];
        }
        if (dx) {
            const float c1 = wave_sum(s1) * (1.f / D), c2 = wave_sum(s2) * (1.f / D);
#pragma unroll
            for (int i = 0; i < NPL; ++i) {
                float* o = dx + ((long)b * T + t) * D + lane + 64 * i;
                *o = *o + rs * (dy[i] * g[i] - c1 - xh[i] * c2) + (add_ev ? e[i] : 0.f);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NPL; ++i) { red[(w * 2) * D + lane + 64 * i] = ag[i]; red[(w * 2 + 1) * D + lane + 64 * i] = ab[i]; }
    __syncthreads();
    for (int q = threadIdx.x; q < 2 * D; q += XW * 64) {
        float v = 0.f;
        for (int w2 = 0; w2 < XW; ++w2) v += red[w2 * 2 * D + q];
        pr_r[q] = v;
    }
}

// ------------------------------------------------------------------ exchange maps (mfvit_fusion_ex_attention / _grad_attention)
// The exchange's softmax probabilities as x_stream_fwd left them in FusWs::a [2][B][nh][T]: per head (fuse 0, out [2][B][nh][T]) or fused over
// ALL nh heads in head order (1 mean | 2 max | 3 min, out [2][B][T]).  One thread per output element.
__global__ __launch_bounds__(256) void x_attn_map_kernel(const float* __restrict__ a, int nh, int T, long n, int fuse, float* __restrict__ out) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    if (fuse == 0) { out[i] = a[i]; return; }
    const long sb = i / T;
    const int t = (int)(i - sb * T);
    const float* p = a + sb * nh * T + t;
    float f = p[0];
    for (int h = 1; h < nh; ++h) {
        const float v = p[(long)h * T];
        f = fuse == 1 ? f + v : fuse == 2 ? fmaxf(f, v) : fminf(f, v);
    }
    out[i] = fuse == 1 ? f / (float)nh : f;
}

// Gradient-weighted exchange map after the backward: da_h[t] = z_t . du_h (the first phase of x_stream_bwd_kernel), then
//   Abar[dir][b][t] = (1 / nh) sum_h max(0, a_h[t] da_h[t]),  the heads summed in head order.
// One workgroup per (sample, direction), a wave per row; more than NH = 3 heads: the chunks of 3 run one after the other INSIDE the workgroup (the
// mean crosses them), every chunk re-deriving z_t from the row and its statistics (the rows come from L2 after the first chunk).
// LDS: st[2][T] | acc[T]; row t of acc is only ever touched by the wave that owns the row.
template <int XW, int D>
__global__ __launch_bounds__(XW * 64) void x_grad_map_kernel(const float* __restrict__ fc, const float* __restrict__ fe,
                                                         const float* __restrict__ params, FusLayout L, int B, int T, int nh,
                                                         const float* __restrict__ a_in, const float* __restrict__ st_in,
                                                         const float* __restrict__ du, float* __restrict__ abar) {
    constexpr int NPL = D / 64;
    extern __shared__ __attribute__((aligned(16))) float xs[];
    float* st = xs;
    float* acc = st + 2 * T;
    const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long sb = (long)dir * B + b;
    const float* own = (dir == 0 ? fc : fe) + (long)b * T * D;
    const float* oth = (dir == 0 ? fe : fc) + (long)b * T * D;
    float g[NPL], be[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        g[i] = L.no_norm ? 1.f : params[L.ca[dir] + L.n_w + lane + 64 * i];
        be[i] = L.no_norm ? 0.f : params[L.ca[dir] + L.n_b + lane + 64 * i];
    }
    for (int q = threadIdx.x; q < 2 * T; q += XW * 64) st[q] = st_in[sb * 2 * T + q];
    __syncthreads();
    for (int h0 = 0; h0 < nh; h0 += NH) {
        float duv[NH][NPL];
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int i = 0; i < NPL; ++i) duv[h][i] = du[(sb * nh + h0 + h) * D + lane + 64 * i];
        for (int t = w; t < T; t += XW) {
            const float* row = t == 0 ? own : oth + (long)t * D;
            const float mu = st[t], rs = st[T + t];
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
            for (int i = 0; i < NPL; ++i) {
                const float z = (row[lane + 64 * i] - mu) * rs * g[i] + be[i];
                d0 = fmaf(z, duv[0][i], d0); d1 = fmaf(z, duv[1][i], d1); d2 = fmaf(z, duv[2][i], d2);
            }
            d0 = wave_sum(d0); d1 = wave_sum(d1); d2 = wave_sum(d2);
            if (lane == 0) {
                const float* ap = a_in + (sb * nh + h0) * T + t;
                float s = h0 == 0 ? 0.f : acc[t];
                s += fmaxf(0.f, ap[0] * d0);
                s += fmaxf(0.f, ap[T] * d1);
                s += fmaxf(0.f, ap[2 * T] * d2);
                acc[t] = s;
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += XW * 64) abar[sb * T + t] = acc[t] / (float)nh;
}

// waves per workgroup of the streaming passes: the same bytes in flight per CU at both widths (a D = 768 row is twice a D = 384 row; the
// backward holds ~100 registers per lane at D = 384, ~180 at D = 768)
template <int D> constexpr int xw_fwd() { return D == 384 ? 16 : 8; }
constexpr int XW_BWD = 8, XW_DZ = 8, XW_ROWS = 8;
constexpr int MAX_XDEPTH = 16;   // cross_attn_depth accepted by the _ex entry points
#define FUS_BY_DIM(dim, CALL) ((dim) == 384 ? CALL<384> : CALL<768>)

// Dynamic LDS (bytes) of the streaming passes, one helper per launch: the launch requests exactly this, and fus_ok refuses a token count whose
// passes would need more than the FUS_MAX_LDS they may request (max_lds) - before any HIP call, instead of a launch error in mid-call.
constexpr size_t FUS_MAX_LDS = 160 * 1024;
template <int D> size_t lds_stream_fwd_of(int T) { return (size_t)(5L * T + (long)xw_fwd<D>() * NH * D) * 4; }
size_t lds_stream_fwd(int D, int T) { return FUS_BY_DIM(D, lds_stream_fwd_of)(T); }
size_t lds_stream_bwd(int D, int T) { return (size_t)(8L * T + (long)XW_BWD * 5 * D) * 4; }
size_t lds_stream_dz(int D, int T, int nh) {   // (the layout x_stream_dz_kernel derives for itself)
    const long big = 2L * nh * D + 2L * nh * T, redn = (long)XW_DZ * 2 * D;
    return (size_t)((big > redn ? big : redn) + 2L * T) * 4;
}
size_t lds_grad_map(int T) { return (size_t)3 * T * 4; }   // x_grad_map_kernel: the rows' statistics and the map (tokens <= MAX_MAP_TOKENS)
bool fus_lds_ok(int D, int T, int nh) {
    return lds_stream_fwd(D, T) <= FUS_MAX_LDS && lds_stream_bwd(D, T) <= FUS_MAX_LDS && (nh == NH || lds_stream_dz(D, T, nh) <= FUS_MAX_LDS);
}

bool fus_ok(const mfvit_fusion_cfg* c) {
    return c && c->batch > 0 && c->tokens > 1 && (c->dim == 384 || c->dim == 768) && (c->heads == 3 || c->heads == 6 || c->heads == 12) &&
           c->num_classes > 0 && c->num_classes <= 64 && fus_lds_ok(c->dim, c->tokens, c->heads);
}
bool fus_ex_ok(const mfvit_fusion_cfg* c, int depth, int pool_mean) {
    return fus_ok(c) && depth >= 1 && depth <= MAX_XDEPTH && (pool_mean == 0 || pool_mean == 1);
}
// the full-row path: every row of every layer's post-LN is live (the default cls / one-layer form needs row 0 only)
bool fus_full(int depth, int pool_mean) { return depth > 1 || pool_mean; }

// An arena of `depth` exchange layers followed by the two heads, as layer 0 sees it.  A layer is the block of fus_layout (FUS_LAYER floats);
// layer l is layer 0 moved up by l of them (FusCtx::layer).  depth = 1 is fus_layout itself, field for field.
long fus_layer_floats(int D) { return 8L * D * D + 10L * D; }
FusLayout fus_arena_layout(int D, int C, int depth) {
    FusLayout L = fus_layout(D, C);
    L.head[0] = depth * fus_layer_floats(D);
    L.head[1] = L.head[0] + (long)C * D + C;
    L.total = depth * fus_layer_floats(D) + 2 * ((long)C * D + C);
    return L;
}

// workspace of the full-row path (floats): one slab per layer [FusWs | Y | yst | pr | pbp], then dx[2] | ev | bb | fusv
//   Y   [2][B][T][D]   the layer's output rows (the next layer's input)        yst [2][B][T][2]  their post-LN mean, rstd
//   pr  [2][2 B][2 D]  post-LN weight | bias partials: rows 0 .. B-1 rows 1 .. T-1 (x_rows_bwd), rows B .. 2B-1 row 0 (x_post0_bwd)
//   pbp [2][B][D]      proj.bias partials (x_post0_bwd)
//   dx  two [2][B][T][D] gradients of the intermediate rows (layer l writes dx[l & 1], reads dx[(l + 1) & 1]); only when depth > 1
//   ev, bb, fusv [2][B][D]   pooled-row gradient, backbone-head gradient of X0[0], pooled rows
struct FusExWs {
    long Y, yst, pr, pbp, slab;
    long dx, ev, bb, fusv;
    long total;
};
FusExWs fus_ex_ws(int B, int T, int C, int D, int NH, int depth) {
    FusExWs E;
    long o = 0;
    auto take = [&](long n) { long r = o; o += (n + 63) & ~63L; return r; };
    take(fus_ws(B, T, C, D, NH).total);
    E.Y = take(2L * B * T * D); E.yst = take(2L * B * T * 2); E.pr = take(2L * 2 * B * 2 * D); E.pbp = take(2L * B * D);
    E.slab = o;
    o = depth * E.slab;
    E.dx = take(depth > 1 ? 2 * 2L * B * T * D : 0);
    E.ev = take(2L * B * D); E.bb = take(2L * B * D); E.fusv = take(2L * B * D);
    E.total = o;
    return E;
}

template <typename K> void max_lds(K* kern, PerDeviceOnce& once) {
    if (once.first()) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FUS_MAX_LDS);
}

// ------------------------------------------------------------------------------------------------ per-call context of the entry points
// the caller's tensors (include/mfvit.h); whatever a call does not have stays NULL
struct FusHeads { const float *w_cxr, *b_cxr, *w_enh, *b_enh; };   // the backbones' own classifier heads (the biases: forward only)
struct FusOut { float *fused, *x_cxr, *x_enh; };
struct FusGradIn { const float *dfused, *dx_cxr, *dx_enh; };
struct FusGradOut { float *df_cxr, *df_enh, *dhw_cxr, *dhb_cxr, *dhw_enh, *dhb_enh; };

// one exchange layer as its kernels see it
struct FusLayer {
    FusLayout L;            // parameter offsets of the layer's blocks (and of the heads behind the last layer)
    float* ws;              // its FusWs (full-row path: its slab, the FusExWs offsets up to `slab` included)
    const float *xc, *xe;   // its input rows: the features, or the rows of the layer below
    const float* dY;        // backward of the full-row path: the gradient of its output rows (NULL: the top layer) ...
    float *dxc, *dxe;       // ... and, every backward, of its input rows: the caller's df_* at layer 0
};

struct FusCtx {
    int B, T, C, D, nh, DH;
    int ndir;               // 2: the model; 1: a stand-alone block (mfvit_prenorm_xattn_* / mfvit_xattn_*)
    int depth, pool_mean;
    float scale, eps_pre, eps_post;
    hipStream_t st;
    const float* params;
    float* dparams;
    const float *f_cxr, *f_enh;
    float* ws;
    FusLayout L0;           // layer 0
    FusWs W;
    FusExWs E;              // full-row path only (all zero otherwise: layer 0 is the workspace itself)
    FusHeads heads;
    FusOut out;
    FusGradIn gin;
    FusGradOut gout;

    // the one place that knows where a layer's parameters, workspace, input rows and row gradients are
    FusLayer layer(int l) const {
        const long btd = (long)B * T * D;
        FusLayer v;
        v.L = L0;
        for (int dir = 0; dir < 2; ++dir) { v.L.ca[dir] += l * fus_layer_floats(D); v.L.post[dir] += l * fus_layer_floats(D); }
        v.ws = ws + l * E.slab;
        v.xc = l == 0 ? f_cxr : ws + (l - 1) * E.slab + E.Y;
        v.xe = l == 0 ? f_enh : v.xc + btd;
        v.dY = l == depth - 1 ? nullptr : ws + E.dx + ((l + 1) & 1) * 2 * btd;
        v.dxc = l == 0 ? gout.df_cxr : ws + E.dx + (l & 1) * 2 * btd;
        v.dxe = l == 0 ? gout.df_enh : v.dxc + btd;
        return v;
    }
};

// L0: fus_arena_layout of the model, one_block_layout of a stand-alone block.  The entry point adds the tensors only it has (heads, out, gin, gout).
FusCtx fus_ctx(const mfvit_fusion_cfg* cfg, int ndir, int depth, int pool_mean, const FusLayout& L0, const float* params, float* dparams,
               const float* f_cxr, const float* f_enh, void* workspace, mfvit_stream_t stream) {
    FusCtx c = {};
    c.B = cfg->batch; c.T = cfg->tokens; c.C = cfg->num_classes; c.D = cfg->dim; c.nh = cfg->heads; c.DH = c.D / c.nh;
    c.ndir = ndir; c.depth = depth; c.pool_mean = pool_mean;
    c.scale = 1.0f / sqrtf((float)c.DH); c.eps_pre = cfg->eps_pre; c.eps_post = cfg->eps_post;
    c.st = (hipStream_t)stream;
    c.params = params; c.dparams = dparams; c.f_cxr = f_cxr; c.f_enh = f_enh; c.ws = (float*)workspace;
    c.L0 = L0;
    c.W = fus_ws(c.B, c.T, c.C, c.D, c.nh);
    if (fus_full(depth, pool_mean)) c.E = fus_ex_ws(c.B, c.T, c.C, c.D, c.nh, depth);
    return c;
}
FusCtx fus_model_ctx(const mfvit_fusion_cfg* cfg, int depth, int pool_mean, const float* params, float* dparams, const float* f_cxr,
                     const float* f_enh, void* workspace, mfvit_stream_t stream) {
    return fus_ctx(cfg, 2, depth, pool_mean, fus_arena_layout(cfg->dim, cfg->num_classes, depth), params, dparams, f_cxr, f_enh, workspace, stream);
}

// ------------------------------------------------------------------------------------------------ the batched f32 products of one layer
// One operand: its address for direction 0 (head 0), its leading dimension and the steps to the next direction and to the next head (floats).
// The five operand kinds below are the only place where a stride of this file's GEMMs is computed.
struct XOpnd { const float* p; long ld, s_dir, s_head; };
enum { WT_Q = 0, WT_K = 1, WT_V = 2, WT_P = 3 };   // the transposed copies in FusWs::wT

struct XGemm {
    const FusCtx& c;
    const FusLayer& v;

    // [dir][B][D] rows of the workspace; head h: the columns h DH ..
    XOpnd rows(long off) const { return {v.ws + off, c.D, (long)c.B * c.D, c.DH}; }
    // [dir][B][nh][D] head rows of the workspace
    XOpnd head_rows(long off) const { return {v.ws + off, (long)c.nh * c.D, (long)c.B * c.nh * c.D, c.D}; }
    // a D x D weight of block `dir` of the arena (or proj.bias, as the bias of per_dir) and its place in the gradient arena; head h: the rows h DH ..
    XOpnd weight(long off) const { return {c.params + v.L.ca[0] + off, c.D, v.L.ca_stride, (long)c.DH * c.D}; }
    XOpnd dweight(long off) const { return {c.dparams + v.L.ca[0] + off, c.D, v.L.ca_stride, (long)c.DH * c.D}; }
    // the transposed copy wT[dir][k]; head h: the columns h DH ..
    XOpnd weightT(int k) const { return {v.ws + c.W.wT + (long)k * c.D * c.D, c.D, 4L * c.D * c.D, c.DH}; }

    // The three batch shapes, M = B rows each: out = a w^T (gemm_nt_tile), or the weight gradient out += a^T w (fus_wgrad).
    // one product per direction (N = K = D)
    GemmP per_dir(XOpnd a, XOpnd w, XOpnd out, XOpnd bias = {}) const {
        GemmP p = batch(a, w, out, c.D, c.D, false);
        p.bias = bias.p; p.sBo = bias.s_dir;
        return p;
    }
    // one per (direction, head), the head slicing the contraction: K = DH, the columns of a
    GemmP per_head_k(XOpnd a, XOpnd w, XOpnd out) const { return batch(a, w, out, c.D, c.DH, true); }
    // one per (direction, head), the head slicing the output: N = DH, the columns of out (the rows of a weight gradient)
    GemmP per_head_n(XOpnd a, XOpnd w, XOpnd out) const { return batch(a, w, out, c.DH, c.D, true); }

    GemmP batch(XOpnd a, XOpnd w, XOpnd out, int N, int K, bool by_head) const {
        GemmP p = nt(a.p, a.ld, w.p, w.ld, c.B, N, K);
        p.out0 = const_cast<float*>(out.p); p.ldo0 = out.ld;   // (an output is rows of the workspace or a dweight: writable)
        p.nb = c.ndir * (by_head ? c.nh : 1); p.nbi = by_head ? c.nh : 1;
        p.sAo = a.s_dir; p.sWo = w.s_dir; p.sOo = out.s_dir;
        if (by_head) { p.sAi = a.s_head; p.sWi = w.s_head; p.sOi = out.s_head; }
        return p;
    }
};

}  // namespace

// PreNorm -> CrossAttention of c.ndir directions up to the projection output outp[dir][b][D] (MOD:20,123-137)
template <int D>
static int xattn_core_forward(const FusCtx& c, const FusLayer& v) {
    const FusLayout& L = v.L;
    const FusWs& W = c.W;
    float* const ws = v.ws;
    const int B = c.B, T = c.T, nh = c.nh, ndir = c.ndir;
    const hipStream_t st = c.st;
    const XGemm g{c, v};
    // transposed copies of wq, wk, wv, wp (used by kq here and by the backward)
    for (int dir = 0; dir < ndir; ++dir) {
        const long offs[4] = {L.wq, L.wk, L.wv, L.wp};
        for (int k = 0; k < 4; ++k)
            MFVIT_TRY(cast_transpose(MFVIT_F32, c.params + L.ca[dir] + offs[k], nullptr, ws + W.wT + ((long)dir * 4 + k) * D * D, D, D, st));
    }
    MFVIT_LAUNCH(x_cls_ln_kernel<D>, dim3(B, ndir), dim3(64), 0, st, v.xc, v.xe, c.params, L, c.eps_pre, B, T, ws + W.z0, ws + W.st0);
    MFVIT_CHECK_LAUNCH();
    // qv = z0 Wq^T
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_NONE, g.per_dir(g.rows(W.z0), g.weight(L.wq), g.rows(W.qv)), st));
    // kq_h = qv_h Wk_h  (W operand = WkT[:, h*DH ..])
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_NONE, g.per_head_k(g.rows(W.qv), g.weightT(WT_K), g.head_rows(W.kq)), st));
    {
        constexpr int XW = xw_fwd<D>();
        const size_t lds = lds_stream_fwd(D, T);
        static PerDeviceOnce attr1, attrc;
        ProfScope ps(PROF_XATTN_FWD, 0, 2.0 * B * T * D * 4 * 2 * (nh / NH), st);
        if (nh == NH) {
            max_lds((x_stream_fwd_kernel<XW, D, false>), attr1);
            MFVIT_LAUNCH((x_stream_fwd_kernel<XW, D, false>), dim3(B, ndir), dim3(XW * 64), lds, st, v.xc, v.xe, c.params, L, c.eps_pre, c.scale, B, T,
                               ws + W.kq, ws + W.u, ws + W.a, ws + W.st);
        } else {
            max_lds((x_stream_fwd_kernel<XW, D, true>), attrc);
            MFVIT_LAUNCH((x_stream_fwd_kernel<XW, D, true>), dim3(B, ndir, nh / NH), dim3(XW * 64), lds, st, v.xc, v.xe, c.params, L, c.eps_pre, c.scale,
                               B, T, ws + W.kq, ws + W.u, ws + W.a, ws + W.st);
        }
        MFVIT_CHECK_LAUNCH();
    }
    // o_h = u_h Wv_h^T
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_NONE, g.per_head_n(g.head_rows(W.u), g.weight(L.wv), g.rows(W.o)), st));
    // outp = o Wp^T + bp
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_BIAS, g.per_dir(g.rows(W.o), g.weight(L.wp), g.rows(W.outp), g.weight(L.bp)), st));
    return MFVIT_OK;
}

// d pre-norm weight | bias of direction `dir` += the sum over its 2 B partial rows (x_stream_bwd / x_stream_dz: token rows 1 ..,
// x_row0_bwd: the cls row), fixed order
static int fus_prenorm_job(const FusCtx& c, const FusLayer& v, int dir) {
    if (v.L.no_norm) return MFVIT_OK;
    float* dn = c.dparams + v.L.ca[dir];
    return colpart_reduce(v.ws + c.W.pd + (long)dir * 2 * c.B * 2 * c.D, 2 * c.B, c.D, 2, dn + v.L.n_w, dn + v.L.n_b, nullptr, c.st);
}
// d head weight | bias of direction `dir` - and of that stream's backbone head, where the caller has one - += the sums over the B partial rows
// that x_finish_bwd / x_head_bwd left in pb, pc of layer v (the top layer)
static int fus_head_job(const FusCtx& c, const FusLayer& v, int dir) {
    const int B = c.B, C = c.C, D = c.D;
    float* dhw = c.dparams + v.L.head[dir];
    MFVIT_TRY(colpart_reduce(v.ws + c.W.pb + (long)dir * B * 2 * C * D, B, C * D, 2, dhw, dir == 0 ? c.gout.dhw_cxr : c.gout.dhw_enh, nullptr, c.st));
    return colpart_reduce(v.ws + c.W.pc + (long)dir * B * 2 * C, B, C, 2, dhw + (long)C * D, dir == 0 ? c.gout.dhb_cxr : c.gout.dhb_enh, nullptr, c.st);
}

// A weight gradient of the exchange, dW += A^T X over the batch rows (f32, plain operands), on gemm_small.hip's kernel at EVERY batch: one
// workgroup per 32 x 32 output tile sums all rows in a fixed order and adds the total into dparams once.  gemm_tn hands more than 512 rows to the
// 128 x 128 tile kernel, which splits the rows over several workgroups and - batch addressing (nb > 1) leaves it no partial scratch - adds them by
// float atomics in arrival order; in one split it would be 9 to 36 workgroups walking every row, where this is 144 and more.
static int fus_wgrad(const GemmP& p, hipStream_t st) { return gemm_tn_small(p, st); }

// backward of xattn_core_forward: consumes ws.dout (= d outp) and ws.dqp (cls gradient that bypasses the attention); the gradient of the
// layer's input rows goes to v.dxc / v.dxe (NULL: not wanted)
template <int D>
static int xattn_core_backward(const FusCtx& c, const FusLayer& v) {
    const FusLayout& L = v.L;
    const FusWs& W = c.W;
    float* const ws = v.ws;
    const int B = c.B, T = c.T, nh = c.nh, ndir = c.ndir;
    const hipStream_t st = c.st;
    const XGemm g{c, v};
    // dWp += dout^T o
    MFVIT_TRY(fus_wgrad(g.per_dir(g.rows(W.dout), g.rows(W.o), g.dweight(L.wp)), st));
    // do = dout Wp   (W operand = WpT)
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_NONE, g.per_dir(g.rows(W.dout), g.weightT(WT_P), g.rows(W.dob)), st));
    // dWv_h += do_h^T u_h
    MFVIT_TRY(fus_wgrad(g.per_head_n(g.rows(W.dob), g.head_rows(W.u), g.dweight(L.wv)), st));
    // du_h = do_h Wv_h   (W operand = WvT[:, h*DH ..])
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_NONE, g.per_head_k(g.rows(W.dob), g.weightT(WT_V), g.head_rows(W.du)), st));
    {
        const size_t lds = lds_stream_bwd(D, T);
        static PerDeviceOnce attr1, attrc, attrz;
        ProfScope ps(PROF_XATTN_BWD, 0, 2.0 * B * T * D * 4 * 3 * (nh == NH ? 1 : nh / NH + 1), st);
        if (nh == NH) {
            max_lds((x_stream_bwd_kernel<XW_BWD, D, false>), attr1);
            MFVIT_LAUNCH((x_stream_bwd_kernel<XW_BWD, D, false>), dim3(B, ndir), dim3(XW_BWD * 64), lds, st, v.xc, v.xe, c.params, L, c.scale, B, T,
                               ws + W.kq, ws + W.a, ws + W.st, ws + W.du, ws + W.dkq, ws + W.dz0p, ws + W.pd, v.dxc, v.dxe, nullptr);
            MFVIT_CHECK_LAUNCH();
        } else {   // heads in chunks of 3 (dkq, ds), then the token gradient over all heads
            max_lds((x_stream_bwd_kernel<XW_BWD, D, true>), attrc);
            MFVIT_LAUNCH((x_stream_bwd_kernel<XW_BWD, D, true>), dim3(B, ndir, nh / NH), dim3(XW_BWD * 64), lds, st, v.xc, v.xe, c.params, L, c.scale,
                               B, T, ws + W.kq, ws + W.a, ws + W.st, ws + W.du, ws + W.dkq, ws + W.dz0p, ws + W.pd, v.dxc, v.dxe, ws + W.ds);
            MFVIT_CHECK_LAUNCH();
            const size_t ldz = lds_stream_dz(D, T, nh);
            max_lds((x_stream_dz_kernel<XW_DZ, D>), attrz);
            MFVIT_LAUNCH((x_stream_dz_kernel<XW_DZ, D>), dim3(B, ndir), dim3(XW_DZ * 64), ldz, st, v.xc, v.xe, c.params, L, c.scale, B, T, nh,
                               ws + W.kq, ws + W.a, ws + W.st, ws + W.du, ws + W.ds, ws + W.dz0p, ws + W.pd, v.dxc, v.dxe);
            MFVIT_CHECK_LAUNCH();
        }
    }
    // dWk_h += qv_h^T dkq_h
    MFVIT_TRY(fus_wgrad(g.per_head_n(g.rows(W.qv), g.head_rows(W.dkq), g.dweight(L.wk)), st));
    // dqv_h = dkq_h Wk_h^T
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_NONE, g.per_head_n(g.head_rows(W.dkq), g.weight(L.wk), g.rows(W.dqv)), st));
    // dWq += dqv^T z0
    MFVIT_TRY(fus_wgrad(g.per_dir(g.rows(W.dqv), g.rows(W.z0), g.dweight(L.wq)), st));
    // dz0q = dqv Wq   (W operand = WqT)
    MFVIT_TRY(gemm_nt_tile(MFVIT_F32, EPI_NONE, g.per_dir(g.rows(W.dqv), g.weightT(WT_Q), g.rows(W.dz0q)), st));
    MFVIT_LAUNCH(x_row0_bwd_kernel<D>, dim3(B), dim3(64 * ndir), 0, st, v.xc, v.xe, c.params, L, B, T, ws + W.st0, ws + W.dz0p, ws + W.dz0q,
                       ws + W.dqp, ws + W.pd, v.dxc, v.dxe);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

// ------------------------------------------------------------------------------------------------ Fus_CrossViT, one exchange layer, cls pooling
template <int D>
static int fusion_forward(const FusCtx& c) {
    const FusLayer v = c.layer(0);
    const FusWs& W = c.W;
    MFVIT_TRY(xattn_core_forward<D>(c, v));
    MFVIT_LAUNCH(x_finish_fwd_kernel<D>, dim3(c.B), dim3(128), 0, c.st, v.xc, v.xe, c.params, v.L, c.eps_post, c.B, c.T, c.C, v.ws + W.outp,
                       v.ws + W.fus, v.ws + W.stc, c.heads.w_cxr, c.heads.b_cxr, c.heads.w_enh, c.heads.b_enh, c.out.fused, c.out.x_cxr, c.out.x_enh);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

template <int D>
static int fusion_backward(const FusCtx& c) {
    const FusLayer v = c.layer(0);
    const FusLayout& L = v.L;
    const FusWs& W = c.W;
    float* const ws = v.ws;
    float* const dparams = c.dparams;
    const int B = c.B;
    MFVIT_LAUNCH(x_finish_bwd_kernel<D>, dim3(B), dim3(128), 0, c.st, v.xc, v.xe, c.params, L, B, c.T, c.C, ws + W.outp, ws + W.fus,
                       ws + W.stc, c.heads.w_cxr, c.heads.w_enh, c.gin.dfused, c.gin.dx_cxr, c.gin.dx_enh, dparams, c.gout.dhw_cxr, c.gout.dhb_cxr,
                       c.gout.dhw_enh, c.gout.dhb_enh, ws + W.dout, ws + W.dqp, ws + W.pa, ws + W.pb, ws + W.pc);
    MFVIT_CHECK_LAUNCH();
    MFVIT_TRY(xattn_core_backward<D>(c, v));
    // the batch sums of the small gradients, every one in a fixed order (one launch)
    ColpartScope batch;
    for (int dir = 0; dir < 2; ++dir) {
        float* dg = dparams + L.post[dir];
        MFVIT_TRY(colpart_reduce(ws + W.pa + (long)dir * B * 3 * D, B, D, 3, dg, dg + D, dparams + L.ca[dir] + L.bp, c.st));
        MFVIT_TRY(fus_head_job(c, v, dir));
        MFVIT_TRY(fus_prenorm_job(c, v, dir));
    }
    return colpart_batch_flush(c.st);
}

// ------------------------------------------------------------------------------------------------ Fus_CrossViT, full-row path
template <int D>
static int fusion_full_forward(const FusCtx& c) {
    const FusWs& W = c.W;
    const FusExWs& E = c.E;
    const int B = c.B, T = c.T;
    for (int l = 0; l < c.depth; ++l) {
        const FusLayer v = c.layer(l);
        MFVIT_TRY(xattn_core_forward<D>(c, v));
        const int pool = l < c.depth - 1 ? 0 : (c.pool_mean ? 2 : 1);
        MFVIT_LAUNCH((x_rows_fwd_kernel<XW_ROWS, D>), dim3(B, 2), dim3(XW_ROWS * 64), 0, c.st, v.xc, v.xe, c.f_cxr, c.f_enh, c.params, v.L, c.eps_post,
                           B, T, v.ws + W.outp, v.ws + E.Y, v.ws + E.yst, pool, c.ws + E.fusv);
        MFVIT_CHECK_LAUNCH();
    }
    MFVIT_LAUNCH(x_head_fwd_kernel<D>, dim3(B), dim3(128), 0, c.st, c.f_cxr, c.f_enh, c.params, c.layer(c.depth - 1).L, B, T, c.C, c.ws + E.fusv,
                       c.heads.w_cxr, c.heads.b_cxr, c.heads.w_enh, c.heads.b_enh, c.out.fused, c.out.x_cxr, c.out.x_enh);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

template <int D>
static int fusion_full_backward(const FusCtx& c) {
    const FusWs& W = c.W;
    const FusExWs& E = c.E;
    const int B = c.B, T = c.T;
    float* const dparams = c.dparams;
    const FusLayer top = c.layer(c.depth - 1);
    MFVIT_LAUNCH(x_head_bwd_kernel<D>, dim3(B), dim3(128), 0, c.st, c.f_cxr, c.f_enh, c.params, top.L, B, T, c.C, c.pool_mean, c.ws + E.fusv,
                       c.heads.w_cxr, c.heads.w_enh, c.gin.dfused, c.gin.dx_cxr, c.gin.dx_enh, c.ws + E.ev, c.ws + E.bb, top.ws + W.pb, top.ws + W.pc);
    MFVIT_CHECK_LAUNCH();
    ColpartScope batch;
    for (int l = c.depth - 1; l >= 0; --l) {
        const FusLayer v = c.layer(l);
        const FusLayout& L = v.L;
        MFVIT_LAUNCH(x_post0_bwd_kernel<D>, dim3(B), dim3(128), 0, c.st, v.xc, v.xe, c.params, L, B, T, v.ws + W.outp, v.ws + E.yst, v.dY, c.ws + E.ev,
                           c.ws + E.bb, l == 0 ? 1 : 0, v.ws + W.dout, v.ws + W.dqp, v.ws + E.pr, v.ws + E.pbp);
        MFVIT_CHECK_LAUNCH();
        MFVIT_TRY(xattn_core_backward<D>(c, v));
        const int mode = l == c.depth - 1 ? (c.pool_mean ? 1 : 2) : 0;
        MFVIT_LAUNCH((x_rows_bwd_kernel<XW_ROWS, D>), dim3(B, 2), dim3(XW_ROWS * 64), 0, c.st, v.xc, v.xe, c.params, L, B, T, v.ws + E.yst, v.dY,
                           c.ws + E.ev, mode, l == 0 && c.pool_mean ? 1 : 0, v.dxc, v.dxe, v.ws + E.pr);
        MFVIT_CHECK_LAUNCH();
        for (int dir = 0; dir < 2; ++dir) {
            float* dg = dparams + L.post[dir];
            MFVIT_TRY(colpart_reduce(v.ws + E.pr + (long)dir * 2 * B * 2 * D, 2 * B, D, 2, dg, dg + D, nullptr, c.st));
            MFVIT_TRY(colpart_reduce(v.ws + E.pbp + (long)dir * B * D, B, D, 1, dparams + L.ca[dir] + L.bp, nullptr, nullptr, c.st));
            MFVIT_TRY(fus_prenorm_job(c, v, dir));
        }
    }
    for (int dir = 0; dir < 2; ++dir) MFVIT_TRY(fus_head_job(c, top, dir));
    return colpart_batch_flush(c.st);
}

extern "C" {

size_t mfvit_fusion_param_count(const mfvit_fusion_cfg* cfg) { return fus_ok(cfg) ? (size_t)fus_layout(cfg->dim, cfg->num_classes).total : 0; }
size_t mfvit_fusion_workspace_bytes(const mfvit_fusion_cfg* cfg) {
    return fus_ok(cfg) ? (size_t)fus_ws(cfg->batch, cfg->tokens, cfg->num_classes, cfg->dim, cfg->heads).total * 4 : 0;
}

int mfvit_fusion_forward(const mfvit_fusion_cfg* cfg, const float* params, const float* f_cxr, const float* f_enh, const float* hw_cxr,
                         const float* hb_cxr, const float* hw_enh, const float* hb_enh, void* workspace, float* fused, float* x_cxr,
                         float* x_enh, mfvit_stream_t stream) {
    if (!fus_ok(cfg) || !params || !f_cxr || !f_enh || !workspace || !fused) return MFVIT_EINVAL;
    FusCtx c = fus_model_ctx(cfg, 1, 0, params, nullptr, f_cxr, f_enh, workspace, stream);
    c.heads = {hw_cxr, hb_cxr, hw_enh, hb_enh};
    c.out = {fused, x_cxr, x_enh};
    return FUS_BY_DIM(cfg->dim, fusion_forward)(c);
}

int mfvit_fusion_backward(const mfvit_fusion_cfg* cfg, const float* params, const float* f_cxr, const float* f_enh, const float* hw_cxr,
                          const float* hw_enh, void* workspace, const float* dfused, const float* dx_cxr, const float* dx_enh,
                          float* dparams, float* df_cxr, float* df_enh, float* dhw_cxr, float* dhb_cxr, float* dhw_enh, float* dhb_enh,
                          mfvit_stream_t stream) {
    if (!fus_ok(cfg) || !params || !f_cxr || !f_enh || !workspace || !dparams) return MFVIT_EINVAL;
    if ((df_cxr == nullptr) != (df_enh == nullptr)) return MFVIT_EINVAL;
    FusCtx c = fus_model_ctx(cfg, 1, 0, params, dparams, f_cxr, f_enh, workspace, stream);
    c.heads = {hw_cxr, nullptr, hw_enh, nullptr};
    c.gin = {dfused, dx_cxr, dx_enh};
    c.gout = {df_cxr, df_enh, dhw_cxr, dhb_cxr, dhw_enh, dhb_enh};
    return FUS_BY_DIM(cfg->dim, fusion_backward)(c);
}

size_t mfvit_fusion_ex_param_count(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean) {
    return fus_ex_ok(cfg, cross_attn_depth, pool_mean) ? (size_t)fus_arena_layout(cfg->dim, cfg->num_classes, cross_attn_depth).total : 0;
}
size_t mfvit_fusion_ex_workspace_bytes(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean) {
    if (!fus_ex_ok(cfg, cross_attn_depth, pool_mean)) return 0;
    if (!fus_full(cross_attn_depth, pool_mean)) return mfvit_fusion_workspace_bytes(cfg);
    return (size_t)fus_ex_ws(cfg->batch, cfg->tokens, cfg->num_classes, cfg->dim, cfg->heads, cross_attn_depth).total * 4;
}

int mfvit_fusion_ex_forward(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const float* params, const float* f_cxr,
                            const float* f_enh, const float* hw_cxr, const float* hb_cxr, const float* hw_enh, const float* hb_enh,
                            void* workspace, float* fused, float* x_cxr, float* x_enh, mfvit_stream_t stream) {
    if (!fus_ex_ok(cfg, cross_attn_depth, pool_mean) || !params || !f_cxr || !f_enh || !workspace || !fused) return MFVIT_EINVAL;
    if (!fus_full(cross_attn_depth, pool_mean))
        return mfvit_fusion_forward(cfg, params, f_cxr, f_enh, hw_cxr, hb_cxr, hw_enh, hb_enh, workspace, fused, x_cxr, x_enh, stream);
    FusCtx c = fus_model_ctx(cfg, cross_attn_depth, pool_mean, params, nullptr, f_cxr, f_enh, workspace, stream);
    c.heads = {hw_cxr, hb_cxr, hw_enh, hb_enh};
    c.out = {fused, x_cxr, x_enh};
    return FUS_BY_DIM(cfg->dim, fusion_full_forward)(c);
}

int mfvit_fusion_ex_backward(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const float* params, const float* f_cxr,
                             const float* f_enh, const float* hw_cxr, const float* hw_enh, void* workspace, const float* dfused,
                             const float* dx_cxr, const float* dx_enh, float* dparams, float* df_cxr, float* df_enh, float* dhw_cxr,
                             float* dhb_cxr, float* dhw_enh, float* dhb_enh, mfvit_stream_t stream) {
    if (!fus_ex_ok(cfg, cross_attn_depth, pool_mean) || !params || !f_cxr || !f_enh || !workspace || !dparams) return MFVIT_EINVAL;
    if ((df_cxr == nullptr) != (df_enh == nullptr)) return MFVIT_EINVAL;
    if (!fus_full(cross_attn_depth, pool_mean))
        return mfvit_fusion_backward(cfg, params, f_cxr, f_enh, hw_cxr, hw_enh, workspace, dfused, dx_cxr, dx_enh, dparams, df_cxr, df_enh,
                                     dhw_cxr, dhb_cxr, dhw_enh, dhb_enh, stream);
    FusCtx c = fus_model_ctx(cfg, cross_attn_depth, pool_mean, params, dparams, f_cxr, f_enh, workspace, stream);
    c.heads = {hw_cxr, nullptr, hw_enh, nullptr};
    c.gin = {dfused, dx_cxr, dx_enh};
    c.gout = {df_cxr, df_enh, dhw_cxr, dhb_cxr, dhw_enh, dhb_enh};
    return FUS_BY_DIM(cfg->dim, fusion_full_backward)(c);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ exchange maps
constexpr int MAX_MAP_TOKENS = 8192;   // as the rollout / relevance chains (include/mfvit.h)

template <int D>
static int fusion_grad_map(const FusCtx& c, int layer, float* abar) {
    const FusLayer v = c.layer(layer);
    const FusWs& W = c.W;
    const int B = c.B, T = c.T, nh = c.nh;
    // What this reads of the workspace and who wrote it last: a, st - x_stream_fwd (the forward; the backward only reads them); du - the
    // "du_h = do_h Wv_h" GEMM of xattn_core_backward, which nothing after it writes (x_stream_bwd / x_stream_dz read it; dkq, dz0p, dqv, dz0q, pd,
    // ds and the full-row path's dx / pr / pbp are regions of their own in fus_ws / fus_ex_ws).
    static PerDeviceOnce attr;
    max_lds((x_grad_map_kernel<XW_BWD, D>), attr);
    ProfScope ps(PROF_OTHER, 2.0 * 2 * B * (double)T * D * nh, 2.0 * B * T * D * 4 * (nh / NH), c.st);
    MFVIT_LAUNCH((x_grad_map_kernel<XW_BWD, D>), dim3(B, 2), dim3(XW_BWD * 64), lds_grad_map(T), c.st, v.xc, v.xe, c.params, v.L, B, T, nh,
                 v.ws + W.a, v.ws + W.st, v.ws + W.du, abar);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

extern "C" {

int mfvit_fusion_ex_attention(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const void* workspace, int layer, int fuse,
                              float* out, mfvit_stream_t stream) {
    if (!fus_ex_ok(cfg, cross_attn_depth, pool_mean) || !workspace || !out || layer < 0 || layer >= cross_attn_depth || fuse < 0 || fuse > 3 ||
        cfg->tokens > MAX_MAP_TOKENS)
        return MFVIT_EINVAL;
    // (the maps only read the workspace)
    const FusCtx c = fus_model_ctx(cfg, cross_attn_depth, pool_mean, nullptr, nullptr, nullptr, nullptr, const_cast<void*>(workspace), stream);
    const long n = 2L * c.B * (fuse ? 1 : c.nh) * c.T;
    ProfScope ps(PROF_OTHER, 0, (2.0 * c.B * c.nh * c.T + (double)n) * 4, c.st);
    MFVIT_LAUNCH(x_attn_map_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.st, c.layer(layer).ws + c.W.a, c.nh, c.T, n, fuse, out);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int mfvit_fusion_ex_grad_attention(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const float* params, const float* f_cxr,
                                   const float* f_enh, const void* workspace, int layer, float* abar, mfvit_stream_t stream) {
    if (!fus_ex_ok(cfg, cross_attn_depth, pool_mean) || !params || !f_cxr || !f_enh || !workspace || !abar || layer < 0 ||
        layer >= cross_attn_depth || cfg->tokens > MAX_MAP_TOKENS)
        return MFVIT_EINVAL;
    const FusCtx c = fus_model_ctx(cfg, cross_attn_depth, pool_mean, params, nullptr, f_cxr, f_enh, const_cast<void*>(workspace), stream);
    return FUS_BY_DIM(cfg->dim, fusion_grad_map)(c, layer, abar);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ stand-alone PreNorm(CrossAttention)
__global__ void x_copy_out_kernel(const float* __restrict__ src, float* __restrict__ dst, long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// layout of ONE cross-attention block as the parameter arena: norm.{w,b}, wq, wk, wv, proj.{w,b}; bare: the block starts at wq
// (L.ca[0] = -2 D puts wq at offset 0; the norm offsets are never dereferenced under no_norm)
static FusLayout one_block_layout(const mfvit_fusion_cfg* cfg, bool bare) {
    FusLayout L = fus_layout(cfg->dim, cfg->num_classes);
    L.ca[0] = bare ? -2L * cfg->dim : 0;
    L.no_norm = bare ? 1 : 0;
    return L;
}
// one direction, one layer: x_own's cls row attends x_oth's patches
static FusCtx one_block_ctx(const mfvit_fusion_cfg* cfg, bool bare, const float* params, float* dparams, const float* x_own, const float* x_oth,
                            void* workspace, mfvit_stream_t stream) {
    return fus_ctx(cfg, 1, 1, 0, one_block_layout(cfg, bare), params, dparams, x_own, x_oth, workspace, stream);
}
template <int D>
static int xattn_one_forward_t(const FusCtx& c, float* out) {
    const FusLayer v = c.layer(0);
    const long n = (long)c.B * D;
    MFVIT_TRY(xattn_core_forward<D>(c, v));
    MFVIT_LAUNCH(x_copy_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.st, v.ws + c.W.outp, out, n);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}
static int xattn_one_forward(const mfvit_fusion_cfg* cfg, bool bare, const float* params, const float* x_own, const float* x_oth,
                             void* workspace, float* out, mfvit_stream_t stream) {
    if (!fus_ok(cfg) || !params || !x_own || !x_oth || !workspace || !out) return MFVIT_EINVAL;
    return FUS_BY_DIM(cfg->dim, xattn_one_forward_t)(one_block_ctx(cfg, bare, params, nullptr, x_own, x_oth, workspace, stream), out);
}

template <int D>
static int xattn_one_backward_t(const FusCtx& c, const float* dout) {
    const FusLayer v = c.layer(0);
    const long n = (long)c.B * D;
    MFVIT_LAUNCH(x_copy_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.st, dout, v.ws + c.W.dout, n);
    MFVIT_CHECK_LAUNCH();
    if (hipMemsetAsync(v.ws + c.W.dqp, 0, sizeof(float) * n, c.st) != hipSuccess) return MFVIT_ELAUNCH;
    // d proj.bias = column sums of dout (x_finish_bwd does this in the fused model)
    MFVIT_TRY(colsum_rows(dout, D, c.dparams + v.L.ca[0] + v.L.bp, c.B, 1, 0, D, c.st));
    MFVIT_TRY(xattn_core_backward<D>(c, v));
    return fus_prenorm_job(c, v, 0);
}
static int xattn_one_backward(const mfvit_fusion_cfg* cfg, bool bare, const float* params, const float* x_own, const float* x_oth,
                              void* workspace, const float* dout, float* dparams, float* dx_own, float* dx_oth, mfvit_stream_t stream) {
    if (!fus_ok(cfg) || !params || !x_own || !x_oth || !workspace || !dout || !dparams) return MFVIT_EINVAL;
    if ((dx_own == nullptr) != (dx_oth == nullptr)) return MFVIT_EINVAL;
    FusCtx c = one_block_ctx(cfg, bare, params, dparams, x_own, x_oth, workspace, stream);
    c.gout.df_cxr = dx_own; c.gout.df_enh = dx_oth;
    return FUS_BY_DIM(cfg->dim, xattn_one_backward_t)(c, dout);
}

extern "C" {

int mfvit_prenorm_xattn_forward(const mfvit_fusion_cfg* cfg, const float* params, const float* x_own, const float* x_oth,
                                void* workspace, float* out, mfvit_stream_t stream) {
    return xattn_one_forward(cfg, false, params, x_own, x_oth, workspace, out, stream);
}
int mfvit_prenorm_xattn_backward(const mfvit_fusion_cfg* cfg, const float* params, const float* x_own, const float* x_oth,
                                 void* workspace, const float* dout, float* dparams, float* dx_own, float* dx_oth,
                                 mfvit_stream_t stream) {
    return xattn_one_backward(cfg, false, params, x_own, x_oth, workspace, dout, dparams, dx_own, dx_oth, stream);
}
int mfvit_xattn_forward(const mfvit_fusion_cfg* cfg, const float* params, const float* x, void* workspace, float* out, mfvit_stream_t stream) {
    return xattn_one_forward(cfg, true, params, x, x, workspace, out, stream);
}
int mfvit_xattn_backward(const mfvit_fusion_cfg* cfg, const float* params, const float* x, void* workspace, const float* dout,
                         float* dparams, float* dx, mfvit_stream_t stream) {
    return xattn_one_backward(cfg, true, params, x, x, workspace, dout, dparams, dx, dx, stream);
}

}  // extern "C"
