// C ABI entry points of include/mfvit.h for the single ops: argument checks, then one launcher call each.  No allocation, no
// synchronisation: every launch goes to the caller's stream, all memory is caller-owned.
#include "../../include/mfvit.h"
#include "kernels.h"

using namespace mfvit;

extern "C" {

int mfvit_input_transform(const uint8_t* src, const int64_t* desc, const int32_t* tables, int n, int S, int crop, const float* mean3,
                          const float* std3, float* out, mfvit_stream_t stream) {
    if (!src || !desc || !tables || !mean3 || !std3 || !out) return MFVIT_EINVAL;   // mean3 / std3 are HOST pointers (3 floats each)
    if (crop > S) return MFVIT_EINVAL;
    return input_transform(src, (const long long*)desc, tables, n, S, crop, crop, mean3, std3, out, (hipStream_t)stream);
}
int mfvit_input_transform_rect(const uint8_t* src, const int64_t* desc, const int32_t* tables, int n, int S, int out_h, int out_w,
                               const float* mean3, const float* std3, float* out, mfvit_stream_t stream) {
    if (!src || !desc || !tables || !mean3 || !std3 || !out) return MFVIT_EINVAL;
    return input_transform(src, (const long long*)desc, tables, n, S, out_h, out_w, mean3, std3, out, (hipStream_t)stream);
}
size_t mfvit_input_photometric_workspace_bytes(int n, int S) { return input_photometric_workspace_bytes(n, S); }
int mfvit_input_photometric(const uint8_t* src, const int64_t* desc, const int32_t* tables, const int32_t* photo, int n, int S, int max_radius,
                            void* workspace, const float* mean3, const float* std3, float* out, mfvit_stream_t stream) {
    if (!src || !desc || !tables || !photo || !workspace || !mean3 || !std3 || !out) return MFVIT_EINVAL;   // mean3 / std3: HOST pointers
    return input_photometric(src, (const long long*)desc, tables, photo, n, S, max_radius, workspace, mean3, std3, out, (hipStream_t)stream);
}
int mfvit_eval_counts(const float* scores, int64_t ld, const int64_t* labels, int n, int C, uint64_t* confusion, int64_t* preds,
                      uint64_t* u2, uint64_t* npos, mfvit_stream_t stream) {
    if (!scores || !labels || (!confusion && !(u2 && npos))) return MFVIT_EINVAL;
    return eval_counts(scores, ld, labels, n, C, (unsigned long long*)confusion, (unsigned long long*)u2, (unsigned long long*)npos, preds,
                       (hipStream_t)stream);
}
size_t mfvit_boot_work_bytes(int n, int C, int M, int64_t R) { return boot_work_bytes(n, C, M, R); }
int mfvit_boot_counts(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, uint64_t seed, int64_t r0,
                      int64_t R, int stratified, void* work, size_t work_bytes, uint64_t* conf, uint64_t* u2, uint64_t* npos, mfvit_stream_t stream) {
    return boot_counts(scores, ld, model_stride, labels, n, C, M, seed, r0, R, stratified, work, work_bytes, (unsigned long long*)conf,
                       (unsigned long long*)u2, (unsigned long long*)npos, (hipStream_t)stream);
}
int mfvit_delong_counts(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, void* work,
                        size_t work_bytes, int32_t* v2, uint64_t* pos_xy, uint64_t* neg_xy, uint64_t* u2, uint64_t* npos, mfvit_stream_t stream) {
    return delong_counts(scores, ld, model_stride, labels, n, C, M, work, work_bytes, v2, (unsigned long long*)pos_xy, (unsigned long long*)neg_xy,
                         (unsigned long long*)u2, (unsigned long long*)npos, (hipStream_t)stream);
}
int mfvit_curve_counts(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, void* work,
                       size_t work_bytes, float* thr, uint32_t* tp, uint32_t* fp, int32_t* nthr, int32_t* nnan, uint64_t* npos, mfvit_stream_t stream) {
    return curve_counts(scores, ld, model_stride, labels, n, C, M, work, work_bytes, thr, tp, fp, nthr, nnan, (unsigned long long*)npos,
                        (hipStream_t)stream);
}
int mfvit_boot_points(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, uint64_t seed, int64_t r0,
                      int64_t R, int stratified, const int32_t* requests, int Q, void* work, size_t work_bytes, uint32_t* tp, uint32_t* fp, float* thr,
                      uint64_t* npos, mfvit_stream_t stream) {
    return boot_points(scores, ld, model_stride, labels, n, C, M, seed, r0, R, stratified, requests, Q, work, work_bytes, tp, fp, thr,
                       (unsigned long long*)npos, (hipStream_t)stream);
}
int mfvit_calib_sums(const float* logits, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, const float* temps, int Kt,
                     int NB, uint64_t* bin_n, uint64_t* bin_hit, double* bin_conf, double* sums, uint64_t* skipped, mfvit_stream_t stream) {
    return calib_sums(logits, ld, model_stride, labels, n, C, M, temps, Kt, NB, (unsigned long long*)bin_n, (unsigned long long*)bin_hit, bin_conf, sums,
                      (unsigned long long*)skipped, (hipStream_t)stream);
}
int mfvit_linear_fwd(int dtype, int epilogue, const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, void* y,
                     int64_t ldy, void* y2, int64_t ldy2, int M, int N, int K, mfvit_stream_t stream) {
    if (!x || !w || (!y && epilogue != EPI_BIAS_GELU)) return MFVIT_EINVAL;      // GELU: y = NULL skips the saved derivative
    if (epilogue != EPI_BIAS && epilogue != EPI_BIAS_GELU && epilogue != EPI_NONE && epilogue != EPI_BIAS_X3F16) return MFVIT_EINVAL;
    if (epilogue == EPI_BIAS_GELU && !y2) return MFVIT_EINVAL;
    GemmP p = nt(x, ldx, w, ldw, M, N, K);
    p.bias = bias; p.out0 = y; p.ldo0 = ldy; p.out1 = y2; p.ldo1 = ldy2;
    return gemm_nt_tile(dtype, epilogue, p, (hipStream_t)stream);
}
int mfvit_linear_dgrad_act(int dtype, const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const void* act_grad, int64_t ldg,
                           void* dx, int64_t lddx, int M, int N, int K, mfvit_stream_t stream) {
    if (!dy || !wt || !act_grad || !dx) return MFVIT_EINVAL;
    GemmP p = nt(dy, lddy, wt, ldwt, M, N, K);
    p.aux = act_grad; p.ldaux = ldg; p.out0 = dx; p.ldo0 = lddx;
    return gemm_nt_tile(dtype, EPI_GELU_BWD, p, (hipStream_t)stream);
}
int mfvit_linear_wgrad(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, int M, int N, int K,
                       mfvit_stream_t stream) {
    if (!dy || !x || !dw) return MFVIT_EINVAL;
    GemmP p = nt(dy, lddy, x, ldx, M, N, K);
    p.out0 = dw; p.ldo0 = lddw;
    return gemm_tn(dtype, p, (hipStream_t)stream);
}
int mfvit_linear_wgrad_ws(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, int M, int N,
                          int K, float* scratch, mfvit_stream_t stream) {
    if (!dy || !x || !dw) return MFVIT_EINVAL;
    GemmP p = nt(dy, lddy, x, ldx, M, N, K);
    p.out0 = dw; p.ldo0 = lddw;
    p.cpart = scratch;
    return gemm_tn(dtype, p, (hipStream_t)stream);
}
static bool wgrad_remap_ok(int rows_in, int rows_out, int row_off) {
    if (rows_in == 0) return rows_out == 0 && row_off == 0;
    return rows_in > 0 && row_off >= 0 && rows_out >= rows_in + row_off;
}
int mfvit_linear_wgrad_ex(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, int M, int N, int K,
                          float* scratch, float* dbias, int rows_in, int rows_out, int row_off, mfvit_stream_t stream) {
    if (!dy || !x || !dw || !wgrad_remap_ok(rows_in, rows_out, row_off)) return MFVIT_EINVAL;
    GemmP p = nt(dy, lddy, x, ldx, M, N, K);
    p.out0 = dw; p.ldo0 = lddw;
    p.cpart = scratch;
    p.cs0 = dbias;
    p.orow_in = rows_in; p.orow_out = rows_out; p.orow_off = row_off;
    return gemm_tn(dtype, p, (hipStream_t)stream);
}
int mfvit_linear_wgrad_plan(int dtype, int M, int N, int K, int N2, int64_t lddy, int64_t ldx, int64_t lddw, int64_t lddy2, int64_t ldx2,
                            int64_t lddw2, int flags, int32_t* plan) {
    if (!plan || N2 < 0 || (flags & ~15)) return MFVIT_EINVAL;
    // stand-ins for the caller's buffers: the decision code looks at whether a pointer is given and at its 16-byte alignment, nothing is read
    char* const given = (char*)(size_t)4096;
    GemmP p = nt(given, lddy, given, ldx, M, N, K);
    p.out0 = given; p.ldo0 = lddw;
    if (flags & MFVIT_WGRAD_PLAN_BIAS) p.cs0 = (float*)(given + ((flags & MFVIT_WGRAD_PLAN_BIAS_UNALIGNED) ? 4 : 0));
    if (flags & MFVIT_WGRAD_PLAN_SCRATCH) p.cpart = (float*)given;
    if (flags & MFVIT_WGRAD_PLAN_REMAP) { p.orow_in = 1; p.orow_out = 1; }
    TnPlan pl;
    int rc;
    if (N2 > 0) {
        if (flags & (MFVIT_WGRAD_PLAN_SCRATCH | MFVIT_WGRAD_PLAN_REMAP)) return MFVIT_EINVAL;   // (mfvit_linear_wgrad_pair takes neither)
        GemmP b = nt(given, lddy2, given, ldx2, M, N2, K);
        b.out0 = given; b.ldo0 = lddw2;
        rc = gemm_tn_pair_plan(dtype, p, b, &pl);
    } else {
        rc = gemm_tn_plan(dtype, p, &pl);
    }
    if (rc != MFVIT_OK) return rc;
    plan[0] = pl.kernel; plan[1] = pl.kr; plan[2] = pl.splits; plan[3] = pl.chunk;
    plan[4] = M - (pl.splits - 1) * pl.chunk;
    plan[5] = pl.cpart; plan[6] = pl.kpart; plan[7] = pl.tiles;
    return MFVIT_OK;
}
int mfvit_linear_wgrad_pair(int dtype, const void* dy_a, int64_t lddy_a, const void* x_a, int64_t ldx_a, float* dw_a, int64_t lddw_a, float* dbias_a,
                            int Na, const void* dy_b, int64_t lddy_b, const void* x_b, int64_t ldx_b, float* dw_b, int64_t lddw_b, int Nb, int M, int K,
                            mfvit_stream_t stream) {
    if (!dy_a || !x_a || !dw_a || !dy_b || !x_b || !dw_b) return MFVIT_EINVAL;
    GemmP a = nt(dy_a, lddy_a, x_a, ldx_a, M, Na, K), b = nt(dy_b, lddy_b, x_b, ldx_b, M, Nb, K);
    a.out0 = dw_a; a.ldo0 = lddw_a; a.cs0 = dbias_a;
    b.out0 = dw_b; b.ldo0 = lddw_b;
    if (!gemm_tn_pair_supported(dtype, a, b)) return MFVIT_ENOSYS;
    return gemm_tn_glds_pair(dtype, a, b, (hipStream_t)stream);
}
int mfvit_linear_res_ln_fwd(int dtype, const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const float* res,
                            int64_t ldres, float* x_out, void* y, int y_f32, const float* gamma, const float* beta, float eps,
                            float* mean, float* rstd, int M, int K, mfvit_stream_t stream) {
    return mfvit_linear_res_ln_fwd_ws(dtype, a, lda, w, ldw, bias, res, ldres, x_out, y, y_f32, gamma, beta, eps, mean, rstd, M, K, nullptr, stream);
}
int mfvit_linear_res_ln_fwd_ws(int dtype, const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const float* res,
                               int64_t ldres, float* x_out, void* y, int y_f32, const float* gamma, const float* beta, float eps,
                               float* mean, float* rstd, int M, int K, float* scratch, mfvit_stream_t stream) {
    if (!a || !w || !y || !gamma || !beta || ((size_t)scratch & 15)) return MFVIT_EINVAL;
    GemmP p = nt(a, lda, w, ldw, M, 384, K);
    p.kpart = scratch;
    p.bias = bias; p.res = res; p.ldres = ldres;
    p.out0 = x_out; p.ldo0 = 384; p.out1 = y; p.ldo1 = (dtype == MFVIT_BF16X3 && !y_f32) ? 768 : 384; p.y_f32 = y_f32;
    p.gamma = gamma; p.beta = beta; p.eps = eps; p.mean = mean; p.rstd = rstd;
    return gemm_nt_row(dtype, REPI_RES_LN, p, (hipStream_t)stream);
}
int mfvit_linear_dgrad_ln_bwd(int dtype, const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const float* x, const float* mean,
                              const float* rstd, const float* gamma, const float* dres, float* dx, void* dx_t, float* dgamma,
                              float* dbeta, float* dcol, int M, int K, mfvit_stream_t stream) {
    return mfvit_linear_dgrad_ln_bwd_ws(dtype, dy, lddy, wt, ldwt, x, mean, rstd, gamma, dres, dx, dx_t, dgamma, dbeta, dcol, M, K, nullptr, stream);
}
int mfvit_linear_dgrad_ln_bwd_ws(int dtype, const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const float* x, const float* mean,
                                 const float* rstd, const float* gamma, const float* dres, float* dx, void* dx_t, float* dgamma,
                                 float* dbeta, float* dcol, int M, int K, float* scratch, mfvit_stream_t stream) {
    if (!dy || !wt || !x || !mean || !rstd || !gamma || !dx || ((size_t)scratch & 15)) return MFVIT_EINVAL;
    GemmP p = nt(dy, lddy, wt, ldwt, M, 384, K);
    p.kpart = scratch;
    p.aux = x; p.ldaux = 384; p.mean = (float*)mean; p.rstd = (float*)rstd; p.gamma = gamma;
    p.res = dres; p.ldres = 384;
    p.out0 = dx; p.ldo0 = 384; p.out1 = dx_t; p.ldo1 = dtype == MFVIT_BF16X3 ? 768 : 384;
    p.cs0 = dgamma; p.cs1 = dbeta; p.cs2 = dcol;
    return gemm_nt_row(dtype, REPI_LNBWD_RES, p, (hipStream_t)stream);
}
int mfvit_attention_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int T, int H, int head_dim, mfvit_stream_t stream) {
    if (!qkv || !out || !lse || B <= 0 || T <= 0 || H <= 0) return MFVIT_EINVAL;
    return attn_fwd(dtype, qkv, out, lse, B, T, H, head_dim, (hipStream_t)stream);
}
int mfvit_attention_qkv_dtype(int dtype, int T, int head_dim) { return attn_qkv_dtype(dtype, T, head_dim); }
int mfvit_attention_plan(int dtype, int B, int T, int H, int head_dim, int backward, int32_t* plan) {
    if (!plan || B <= 0 || T <= 0 || H <= 0) return MFVIT_EINVAL;
    AttnPlan pl;
    const int rc = attn_plan(dtype, B, T, H, head_dim, backward != 0, &pl);
    if (rc != MFVIT_OK) return rc;
    plan[0] = pl.family; plan[1] = pl.tiles; plan[2] = pl.lds; plan[3] = pl.grid; plan[4] = pl.threads; plan[5] = pl.lds2;
    return MFVIT_OK;
}
size_t mfvit_attention_stats_work_bytes(int nblk, int B, int T, int H) { return attn_stats_work_bytes(nblk, B, T, H); }
int mfvit_attention_stats(int qkv_dtype, const void* qkv, const float* lse, int64_t qkv_stride, int64_t lse_stride, int nblk, int B, int T, int H,
                          int head_dim, int gh, int gw, float patch, double* stats, void* work, size_t work_bytes, mfvit_stream_t stream) {
    return attn_stats(qkv_dtype, qkv, lse, (long)qkv_stride, (long)lse_stride, nblk, B, T, H, head_dim, gh, gw, patch, stats, work, work_bytes,
                      (hipStream_t)stream);
}
int mfvit_attention_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* dbias_qkv,
                        int B, int T, int H, int head_dim, mfvit_stream_t stream) {
    if (!qkv || !out || !dout || !lse || !dqkv || B <= 0 || T <= 0 || H <= 0) return MFVIT_EINVAL;
    return attn_bwd(dtype, qkv, out, dout, lse, dqkv, dbias_qkv, B, T, H, head_dim, (hipStream_t)stream);
}
int mfvit_attention_drop_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int T, int H, int head_dim, float p, uint64_t seed,
                             uint32_t site, mfvit_stream_t stream) {
    if (!qkv || !out || !lse || B <= 0 || T <= 0 || H <= 0 || !(p >= 0.f && p < 1.f)) return MFVIT_EINVAL;
    if (!attn_tiled_supported(dtype, T, head_dim)) return MFVIT_ENOSYS;
    return attn_fwd_tiled_drop(dtype, qkv, out, lse, B, T, H, head_dim, make_drop(p, seed, site), (hipStream_t)stream);
}
int mfvit_attention_drop_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int T, int H,
                             int head_dim, float p, uint64_t seed, uint32_t site, mfvit_stream_t stream) {
    if (!qkv || !out || !dout || !lse || !dqkv || B <= 0 || T <= 0 || H <= 0 || !(p >= 0.f && p < 1.f)) return MFVIT_EINVAL;
    if (!attn_tiled_supported(dtype, T, head_dim)) return MFVIT_ENOSYS;
    return attn_bwd_tiled_drop(dtype, qkv, out, dout, lse, dqkv, B, T, H, head_dim, make_drop(p, seed, site), (hipStream_t)stream);
}
int mfvit_dropout_mask(float p, uint64_t seed, uint32_t site, int64_t n, uint8_t* keep, mfvit_stream_t stream) {
    if (!keep || !(p >= 0.f && p < 1.f)) return MFVIT_EINVAL;
    return dropout_mask(make_drop(p, seed, site), n, keep, (hipStream_t)stream);
}
int mfvit_layernorm_fwd(int dtype, const float* x, void* y, int y_f32, const float* gamma, const float* beta, float eps, float* mean,
                        float* rstd, int rows, int N, mfvit_stream_t stream) {
    if (!x || !y || !gamma || !beta) return MFVIT_EINVAL;
    return ln_rows(dtype, N, x, N, nullptr, 0, 0, nullptr, 0, y, (dtype == MFVIT_BF16X3 && !y_f32) ? 2 * N : N, y_f32, gamma, beta, eps, mean, rstd, rows, 1, 0,
                   0, (hipStream_t)stream);
}
int mfvit_layernorm_bwd(int dtype, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        const float* dres, float* dx, void* dx_t, float* dgamma, float* dbeta, float* dcol, int rows, int N,
                        mfvit_stream_t stream) {
    if (!dy || !x || !mean || !rstd || !gamma) return MFVIT_EINVAL;
    return ln_bwd_rows(dtype, N, dy, N, x, N, mean, rstd, gamma, dres, N, dx, N, dx_t, dtype == MFVIT_BF16X3 ? 2 * N : N, dgamma, dbeta, dcol, nullptr, rows, 1, 0,
                       (hipStream_t)stream);
}
int mfvit_cast_transpose(int dtype, const float* src, void* dst, void* dst_t, int R, int C, mfvit_stream_t stream) {
    if (!src || R <= 0 || C <= 0) return MFVIT_EINVAL;
    return cast_transpose(dtype, src, dst, dst_t, R, C, (hipStream_t)stream);
}
int mfvit_head_fwd(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy, int M, int N, int K, int accumulate,
                   mfvit_stream_t stream) {
    if (!x || !w || !y) return MFVIT_EINVAL;
    return linear_small_fwd(x, ldx, w, b, y, ldy, M, N, K, accumulate, (hipStream_t)stream);
}
int mfvit_head_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* w, float* dx, int64_t lddx, int dx_accumulate,
                   float* dw, float* db, int M, int N, int K, mfvit_stream_t stream) {
    if (!dy || !x || !w) return MFVIT_EINVAL;
    return linear_small_bwd(dy, lddy, x, ldx, w, dx, lddx, dx_accumulate, dw, db, M, N, K, (hipStream_t)stream);
}
int mfvit_cross_entropy(const float* logits, const int64_t* target, float* loss_mean, float* dlogits, int64_t* preds, int B, int C,
                        mfvit_stream_t stream) {
    if (!logits || !target || !loss_mean) return MFVIT_EINVAL;
    return ce_small(logits, (const long*)target, loss_mean, dlogits, (long*)preds, B, C, (hipStream_t)stream);
}

}  // extern "C"
