// Internal launcher declarations (host side) shared by the composite encoder and the C ABI.
#pragma once
#include "gemm.cuh"

#include <string.h>

namespace mfvit {

enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_GELU_BWD = 2, EPI_NONE = 3, EPI_BIAS_RELU = 4,    // 4: out0 = relu'(pre), out1 = relu(pre)
       EPI_BIAS_X3F16 = 5,                                                                    // 5: bias, output written as split FP16 (sbf16 inputs only: qkv)
       EPI_BIAS_GELU_DROP = 6,     // 6: EPI_BIAS_GELU with dropout on the activation (GemmP::drop, element m * N + n): out1 = gelu * mask, out0 = gelu' * mask
       EPI_COL2IM16 = 7 };         // 7: gemm.hip tile kernel only - the patch-embedding data gradient stored straight into an f32 NCHW image (see there)
enum { REPI_RES_LN = 0, REPI_LNBWD_RES = 1,
       REPI_RES_LN_DP = 2 };   // 2: gemm_rowp only - REPI_RES_LN with x = aux + drop_mul(drop, row / drop_tpr) * (products + bias) (drop path)

int gemm_nt_tile(int dtype, int epi, const GemmP& p, hipStream_t st);
bool gemm_nt_pp_supported(int dtype, int epi, const GemmP& p);     // gemm_pp.hip (round 6): persistent 256 x 128 ping-pong tile kernel, 16-bit types, large M
int gemm_nt_pp(int dtype, int epi, const GemmP& p, hipStream_t st);
int gemm_nt_row(int dtype, int repi, const GemmP& p, hipStream_t st);
bool gemm_nt_rowp_supported(int dtype, int repi, const GemmP& p);   // gemm_rowp.hip: one tall row-complete tile per CU (split bf16)
int gemm_nt_rowp(int dtype, int repi, const GemmP& p, hipStream_t st);
int input_transform(const unsigned char* src, const long long* desc, const int* tables, int n, int S, int out_h, int out_w,
                    const float* mean, const float* stdv, float* out, hipStream_t st);   // input.hip
int input_transform_u8(const unsigned char* src, const long long* desc, const int* tables, int n, int S, unsigned* frames,
                       hipStream_t st);   // input.hip: the same gather, stopped at the uint8 S x S frame (R | G << 8 | B << 16 per pixel)
size_t input_photometric_workspace_bytes(int n, int S);   // photometric.hip
int input_photometric(const unsigned char* src, const long long* desc, const int* tables, const int* photo, int n, int S, int max_radius,
                      void* workspace, const float* mean, const float* stdv, float* out, hipStream_t st);
int eval_counts(const float* scores, long ld, const int64_t* labels, int n, int C, unsigned long long* conf, unsigned long long* u2,
                unsigned long long* npos, int64_t* preds, hipStream_t st);   // metrics.hip
// evalstats.hip: bootstrap replicates (r0 .. r0 + R - 1, replicate 0 the sample itself) and DeLong components of the epoch metrics, what a host loop
// of R scikit-learn calls around MAIN_CA:886-911 / MAIN_SS:797-821 would compute; scores f32 [M][n][C] (row stride ld, model stride ms)
size_t boot_work_bytes(int n, int C, int M, long long R);
int boot_counts(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, unsigned long long seed, long long r0, long long R,
                int stratified, void* work, size_t work_bytes, unsigned long long* conf, unsigned long long* u2, unsigned long long* npos,
                hipStream_t st);
int delong_counts(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, void* work, size_t work_bytes, int* v2,
                  unsigned long long* pos_xy, unsigned long long* neg_xy, unsigned long long* u2, unsigned long long* npos, hipStream_t st);
// evalstats.hip, on the same ordered columns: the ROC / PR curve of the sample as integer counts, operating points of bootstrap replicates, and
// calibration sums of logits at several temperatures (temps: a HOST pointer)
int curve_counts(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, void* work, size_t work_bytes, float* thr,
                 unsigned* tp, unsigned* fp, int* nthr, int* nnan, unsigned long long* npos, hipStream_t st);
int boot_points(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, unsigned long long seed, long long r0, long long R,
                int stratified, const int* req, int Q, void* work, size_t work_bytes, unsigned* tp, unsigned* fp, float* thr, unsigned long long* npos,
                hipStream_t st);
int calib_sums(const float* logits, long ld, long ms, const int64_t* labels, int n, int C, int M, const float* temps, int Kt, int NB,
               unsigned long long* bin_n, unsigned long long* bin_hit, double* bin_conf, double* sums, unsigned long long* skipped, hipStream_t st);
int gemm_tn(int dtype, const GemmP& p, hipStream_t st);
// What a weight-gradient launch of `p` decides on the host before it launches: which kernel, the reduction rows per stage, the split count and the
// KR-rounded rows per split, whether the tile partials go through p.cpart and the bias column sums through the [split][N] rows behind them.  Filled by
// the launchers' own decision functions (gemm.hip::plan_tn, gemm_tn2.hip::plan_t2), which each launcher calls first; gemm_tn_plan / gemm_tn_pair_plan
// route like gemm_tn / the paired launch and touch no device.
enum { TN_KERNEL_SMALL = 0, TN_KERNEL_TILE = 1, TN_KERNEL_GLDS = 2 };
struct TnPlan { int kernel, kr, splits, chunk, tiles; bool cpart, kpart; };
int gemm_tn_plan(int dtype, const GemmP& p, TnPlan* plan);
int gemm_tn_glds_plan(int dtype, const GemmP& p, TnPlan* plan);                       // gemm_tn2.hip
int gemm_tn_pair_plan(int dtype, const GemmP& a, const GemmP& b, TnPlan* plan);       // gemm_tn2.hip (MFVIT_ENOSYS: not a pair)
bool gemm_nt_small_supported(int dtype, int epi, const GemmP& p);   // gemm_small.hip: f32, a handful of rows (the fusion module's per-sample rows)
int gemm_nt_small(int epi, GemmP p, hipStream_t st);
bool gemm_tn_small_supported(int dtype, const GemmP& p);
int gemm_tn_small(GemmP p, hipStream_t st);
bool gemm_tn_glds_supported(int dtype, const GemmP& p);   // gemm_tn2.hip
int gemm_tn_glds(int dtype, GemmP p, hipStream_t st);
int colpart_reduce(const float* part, int G, int ncols, int nq, float* d0, float* d1, float* d2, hipStream_t st);
// deferred / batched form: between colpart_batch_begin(&batch) and colpart_batch_begin(previous) every colpart_reduce call of this thread
// is queued (its partial buffer must stay untouched until the flush) and colpart_batch_flush reduces all queued jobs in ONE launch
struct ColpartJob { const float* part; float* d[3]; int G, ncols, nq; };
struct ColpartBatch { static constexpr int MAXJ = 48; int n; ColpartJob job[MAXJ]; };
ColpartBatch* colpart_batch_begin(ColpartBatch* b);
int colpart_batch_flush(hipStream_t st);
// The bracket as a scope: queues this thread's colpart_reduce calls in a batch of its own and puts the previous batch back on EVERY way out
// (an early return on an error included: the thread-local pointer never outlives the batch).  Flushing stays explicit.  on = false: no bracket.
struct ColpartScope {
    ColpartBatch batch;
    ColpartBatch* prev = nullptr;
    const bool on;
    explicit ColpartScope(bool on_ = true) : on(on_) { if (on) prev = colpart_batch_begin(&batch); }
    ~ColpartScope() { if (on) colpart_batch_begin(prev); }
    ColpartScope(const ColpartScope&) = delete;
    ColpartScope& operator=(const ColpartScope&) = delete;
};
bool gemm_tn_pair_supported(int dtype, const GemmP& a, const GemmP& b);   // gemm_tn2.hip: two weight gradients in one launch
int gemm_tn_glds_pair(int dtype, GemmP a, const GemmP& b, hipStream_t st);
// out[n][k] += sum over the splits of part[s * stride + n * K + k]  (fixed order: deterministic).  Between tnpart_batch_begin(&batch) and
// tnpart_batch_begin(previous) every call of this thread is queued (its partial buffer must stay untouched until the flush) and
// tnpart_batch_flush reduces all queued jobs in ONE launch - the weight gradients of a whole encoder-backward call (round 5).
int tn_partial_reduce(const float* part, int splits, long stride, int N, int K, float* out, long ldo, hipStream_t st);
struct TnPartJob { const float* part; float* out; long stride, ldo; int splits, N, K; long first4; };   // first4: prefix of float4 counts
struct TnPartBatch { static constexpr int MAXJ = 56; int n; long total4; TnPartJob job[MAXJ]; };
TnPartBatch* tnpart_batch_begin(TnPartBatch* b);
int tnpart_batch_flush(hipStream_t st);
struct TnPartScope {   // the same scope for the split partials (see ColpartScope)
    TnPartBatch batch;
    TnPartBatch* prev = nullptr;
    const bool on;
    explicit TnPartScope(bool on_ = true) : on(on_) { if (on) prev = tnpart_batch_begin(&batch); }
    ~TnPartScope() { if (on) tnpart_batch_begin(prev); }
    TnPartScope(const TnPartScope&) = delete;
    TnPartScope& operator=(const TnPartScope&) = delete;
};

int attn_fwd_exact(int dtype, const void* qkv, void* out, float* lse, int B, int Tn, int H, int HD, hipStream_t st);
int attn_bwd_exact(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* dbias, int B, int Tn,
                   int H, int HD, hipStream_t st);

// dtype of the qkv tensor the attention kernels want for activations of `dtype` (MFVIT_X3F16 for split bf16 where the whole-head kernels apply)
int attn_qkv_dtype(int dtype, int Tn, int HD);
int attn_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int Tn, int H, int HD, hipStream_t st);
// domax (optional, MFVIT_X3F16 only): the largest |dout| of every (image, head) as f32 bits, [B][H], when the producer of dout has it (GemmP::omax)
int attn_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* dbias, int B, int Tn,
             int H, int HD, hipStream_t st, const unsigned* domax = nullptr);

// What an attention launch decides on the host (mfvit_attention_plan, include/mfvit.h): filled by the launchers' own decision functions
// (attention.hip::plan_exact, attention_mfma.hip::plan_fwd_t / plan_bwd_t, attention_tiled.hip::tl_plan), which each launcher calls first;
// attn_plan routes like attn_fwd / attn_bwd and touches no device.  (struct AttnPlan: common.cuh)
int attn_plan(int dtype, int B, int Tn, int H, int HD, bool backward, AttnPlan* plan);

int im2col16(int dtype, const float* img, void* P, int B, int H, int W, hipStream_t st);
int ln_rows(int dtype, int N, const float* in0, long ld0, const float* in1, long ld1, int mod1, float* xout, long ldx, void* y, long ldy,
            int y_f32, const float* gamma, const float* beta, float eps, float* mean, float* rstd, int rows, int row_stride, int row_off,
            int in0_bcast, hipStream_t st);
int ln_bwd_rows(int dtype, int N, const float* dy, long lddy, const float* x, long ldx, const float* mean, const float* rstd,
                const float* gamma, const float* dres, long ldres, float* dx, long lddx, void* dxT, long lddxT, float* dgamma, float* dbeta,
                float* dcol, float* cpart, int rows, int row_stride, int row_off, hipStream_t st, const void* dyT = nullptr, long lddyT = 0);
// v = tin[g] (operand type) (+ pos[go % pmod]) (+ res[go]) -> x[go], y[go] = LN(v), statistics; go = (g / rin) * rout + roff + g % rin (rin = 0: g)
int add_ln_rows(int dtype, int N, const void* tin, long ldt, const float* pos, long ldp, int pmod, const float* res, long ldres, int rin, int rout,
                int roff, float* xout, long ldx, void* y, long ldy, int y_f32, const float* gamma, const float* beta, float eps, float* mean,
                float* rstd, int rows, hipStream_t st);
int cast_transpose(int dtype, const float* src, void* dst, void* dstT, int R, int C, hipStream_t st);
int cast_transpose_batched(int dtype, const float* src, void* dst, void* dstT, int R, int C, int nb, long s_src, long s_dst, long s_dstT,
                           hipStream_t st);
int linear_small_fwd(const float* x, long ldx, const float* W, const float* b, float* y, long ldy, int M, int N, int K, int accumulate,
                     hipStream_t st);
int linear_small_bwd(const float* dy, long lddy, const float* x, long ldx, const float* W, float* dx, long lddx, int dx_accumulate, float* dW,
                     float* db, int M, int N, int K, hipStream_t st);
int ce_small(const float* logits, const long* target, float* loss_mean, float* dlogits, long* preds, int B, int C, hipStream_t st);
int add_rows(float* dst, long ldd, const float* src, long lds_, int rows, int N, hipStream_t st);
int axpy(float* y, const float* x, float a, long n, hipStream_t st);
int colsum_rows(const float* x, long ld, float* out, int rows, int row_stride, int row_off, int N, hipStream_t st);
int batch_sum(const float* x, float* out, int B, long n, hipStream_t st);   // out[i] += sum_b x[b * n + i]

// attention with dropout on the probabilities (TransFuser GPT); streaming kernels only (attention_tiled.hip)
int attn_fwd_tiled_drop(int dtype, const void* qkv, void* out, float* lse, int B, int Tn, int H, int HDim, DropP drop, hipStream_t st);
int attn_bwd_tiled_drop(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int Tn, int H, int HDim,
                        DropP drop, hipStream_t st);
bool attn_tiled_supported(int dtype, int Tn, int HDim);
// elementwise.hip: the keep mask (1 / 0 bytes) of n elements of one dropout site - what the kernels regenerate from (seed, site, index)
int dropout_mask(DropP drop, long n, unsigned char* out, hipStream_t st);
// x = res + dpath(row / tpr) * drop(t) -> LayerNorm (t: a GEMM output in the operand type, or a0 (+ a1[row % mod1]) in f32); see elementwise.hip
int drop_add_ln_rows(int dtype, int N, const void* tin, long ldt, const float* a0, long lda0, const float* a1, long lda1, int mod1,
                     const float* res, long ldres, DropP drop, DropP dpath, int tpr, float* xout, long ldx, void* y, long ldy, int y_f32,
                     const float* gamma, const float* beta, float eps, float* mean, float* rstd, int rows, hipStream_t st);
int mask_scale_rows(int dtype, bool f32, const void* src, long lds_, void* dst, long ldd, DropP drop, DropP dpath, int tpr, int rows, int N,
                    hipStream_t st);
// attention_maps.hip: the softmax probabilities of one block's attention forward, recomputed from its qkv (storage tag qdt, as
// attn_qkv_dtype reports it) and lse: out [B][H][rows][T] (fuse 0) or fused over the heads (1 mean, 2 max, 3 min) [B][rows][T] with the fused
// rows' sums [B][rows] in `sums` (fused forms only; may be NULL); rows = T, or 1 with cls_only.  And the cls row of the attention rollout over
// `depth` such fused maps (depth x [B][T][T], row sums depth x [B][T]) -> out [B][T-1].
int attn_probs(int qdt, const void* qkv, const float* lse, int B, int Tn, int H, int HD, int fuse, int cls_only, float* out, float* sums,
               hipStream_t st);
int attn_rollout(const float* maps, const float* sums, int depth, int B, int Tn, float* out, hipStream_t st);
// attention_maps.hip, relevance (Chefer et al. 2021) behind one block's attention backward: from its qkv (tag qdt), lse and dO (the proj data
// gradient, activation tag ddt), map [B][T][T] (or NULL) = A = mean over heads of max(0, P o dO V^T), and part [B][ceil(T/32)][T] (or NULL) =
// per 32-query tile the rows' share of v A, v [B][T] (first: e_0, not read).  attn_rel_update: v <- v + the parts (tile order); first: v = e_0
// before; out [B][T-1] (or NULL) = v[:, 1:].
int attn_rel_map(int qdt, int ddt, const void* qkv, const float* lse, const void* dout, int B, int Tn, int H, int HD, float* map, const float* v,
                 float* part, int first, hipStream_t st);
int attn_rel_update(float* v, const float* part, int B, int Tn, int first, float* out, hipStream_t st);
// attention_maps.hip, per-head statistics of the same probabilities without the maps: stats [nblk][B][H][6] double = mean attention distance
// (cls row and column dropped; not renormalised / renormalised per row), mean row entropy, cls-row entropy (nats), the patches' mass on cls, mean
// diagonal mass - include/mfvit.h, mfvit_attention_stats.  Block l's qkv / lse lie l * qstride / l * lstride BYTES behind block 0's; all blocks in
// one launch + a finish launch over the tile partials in `work` (attn_stats_work_bytes).  Tn = 1 + gh * gw, patch = the patch edge in pixels.
// MFVIT_EINVAL before any HIP call for an argument outside the domain, MFVIT_ENOSYS for a head_dim other than 32 / 64 / 96.
size_t attn_stats_work_bytes(int nblk, int B, int Tn, int H);
int attn_stats(int qdt, const void* qkv, const float* lse, long qstride, long lstride, int nblk, int B, int Tn, int H, int HD, int gh, int gw,
               float patch, double* stats, void* work, size_t work_bytes, hipStream_t st);

// lora.hip: low-rank adapters.  One (Linear, adapter) pair of a batched launch; the table rides in the kernel arguments.
//   merge: o0[n][k] (row stride ldo) = w[n][k] (row stride ldw) + scale * sum_j b[n][j] a[j][k]        (a: [r][K], b: [N][r], both dense)
//   grad:  w = dW [N][K] (row stride ldw);  o0 = dA [r][K] = scale * b^T dW,  o1 = dB [N][r] = scale * dW a^T   (ldo unused)
struct LoraPair { const float* w; const float* a; const float* b; float* o0; float* o1; int N, K, ldw, ldo; };
constexpr int LORA_MAXP = 64;      // pairs per launch (56 bytes each: the table stays inside 4 KB of kernel arguments); longer tables take more launches
struct LoraBatch { int n, r; float scale; LoraPair pair[LORA_MAXP]; };
bool lora_pair_ok(const LoraPair& p, int r, bool grad);
int lora_merge_batch(const LoraPair* pairs, int n, int r, float scale, hipStream_t st);   // MFVIT_EINVAL before any launch when a pair is outside the domain
int lora_grad_batch(const LoraPair* pairs, int n, int r, float scale, hipStream_t st);

// out = A W^T (A: M x K, W: N x K): the operands and the shape, every other field zero
inline GemmP nt(const void* A, long lda, const void* W, long ldw, int M, int N, int K) {
    GemmP p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = lda; p.W = W; p.ldw = ldw;
    p.M = M; p.N = N; p.K = K;
    return p;
}
}  // namespace mfvit

#define MFVIT_TRY(expr)            \
    do {                           \
        int rc__ = (expr);         \
        if (rc__ != MFVIT_OK) return rc__; \
    } while (0)
