// Scenarios over the encoder's C ABI (include/mfvit.h), run against the recording stubs of stubs.cpp: every scenario prints the launch sequence
// its calls produce.  Nothing is computed - device pointers are fake addresses inside named regions, sizes are chosen for the branches of
// csrc/vit.hip they reach.  Host arrays (drop_path, mfvit_lora_req::items) are real memory.
//   driver            every scenario          driver --list          the names          driver --only NAME          one of them
#include "../../include/mfvit.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>

namespace tr {   // stubs.cpp
void reset();
void region(const char* name, const void* base, size_t bytes);
void name_handle(const void* h, const char* name);
void knob(const char* name, long v);
void note(const char* fmt, ...);
std::string take();
int find_call(const char* prefix, int nth);
}  // namespace tr

namespace {

// fake device memory: region r starts at (r + 16) TiB and is 64 GiB long
enum { PARAMS, SHADOW, WS, IMG, FEATS, DFEATS, DPARAMS, DIMG, DTOKENS, MAPS, ROLLOUT, RELEVANCE, SCRATCH, EFF, DW, LA, LB, LDA, LDB, NREG };
const char* const REGION[NREG] = {"params", "shadow", "ws", "img", "feats", "dfeats", "dparams", "dimg", "dtokens", "maps", "rollout", "relevance",
                                  "scratch", "eff", "dw", "a", "b", "da", "db"};
template <typename T = void> T* at(int r, size_t off = 0) { return (T*)(((uintptr_t)(r + 16) << 40) + off); }
float* const P = at<float>(PARAMS);
void* const SH = at(SHADOW);
void* const W = at(WS);
float* const IM = at<float>(IMG);
float* const FE = at<float>(FEATS);
float* const DF = at<float>(DFEATS);
float* const DP = at<float>(DPARAMS);
float* const DI = at<float>(DIMG);
float* const DT = at<float>(DTOKENS);
const mfvit_stream_t MAIN = (mfvit_stream_t)0x5100, MAIN2 = (mfvit_stream_t)0x5200;

#define RC(call)                        \
    do {                                \
        tr::note("call %s", #call);     \
        const int rc_ = (call);         \
        tr::note("rc %d", rc_);         \
    } while (0)

void begin() {
    tr::reset();
    for (int r = 0; r < NREG; ++r) tr::region(REGION[r], at(r), (size_t)1 << 36);
    tr::name_handle(MAIN, "main");
    tr::name_handle(MAIN2, "main2");
    unsetenv("MFVIT_UNFUSED_ROWS");
    unsetenv("MFVIT_DO_MAX");
    mfvit_set_wgrad_stream(1);
    mfvit_set_stream_share(1);
}

mfvit_vit_cfg image_cfg(int dtype, int batch, int hw, int dim, int heads, int depth, int save = 1) {
    mfvit_vit_cfg c;
    memset(&c, 0, sizeof(c));
    c.dtype = dtype; c.batch = batch; c.img_h = c.img_w = hw; c.dim = dim; c.depth = depth; c.heads = heads; c.mlp_dim = 4 * dim;
    c.save_for_backward = save; c.ln_eps = 1e-6f;
    return c;
}
// M = 10 token rows: no side stream, no dO maximum (T < 64)
mfvit_vit_cfg small_cfg(int dtype = MFVIT_BF16X3, int save = 1) { return image_cfg(dtype, 2, 32, 384, 6, 2, save); }
// T = 197: M = 197 batch; the weight-gradient side stream runs for 1,024 <= M <= 4,096
mfvit_vit_cfg side_cfg(int batch = 6) { return image_cfg(MFVIT_BF16X3, batch, 224, 384, 6, 3); }
mfvit_vit_cfg gpt_cfg(int dtype) {
    mfvit_vit_cfg c = image_cfg(dtype, 2, 0, 384, 6, 2);
    c.token_input = 1; c.tokens = 8; c.ln_eps = 1e-5f;
    return c;
}

// the size and layout queries of a cfg (drop: NULL or the scenario's)
void sizes(const mfvit_vit_cfg& c, const mfvit_vit_drop* drop = nullptr) {
    int64_t L[9] = {};
    const int rc = mfvit_vit_param_layout(&c, L);
    tr::note("sizes params=%zu shadow=%zu ws=%zu ws_drop=%zu ws_ex0=%zu ws_ex1=%zu layout(rc %d)=%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld",
             mfvit_vit_param_count(&c), mfvit_vit_shadow_bytes(&c), mfvit_vit_workspace_bytes(&c), mfvit_vit_workspace_bytes_drop(&c, drop),
             mfvit_vit_workspace_bytes_ex(&c, drop, 0), mfvit_vit_workspace_bytes_ex(&c, drop, 1), rc, (long long)L[0], (long long)L[1],
             (long long)L[2], (long long)L[3], (long long)L[4], (long long)L[5], (long long)L[6], (long long)L[7], (long long)L[8]);
}

// ------------------------------------------------------------------ 1. image mode, small
void fwd_nosave() {
    mfvit_vit_cfg c = small_cfg(MFVIT_BF16X3, 0);
    sizes(c);
    RC(mfvit_vit_forward(&c, P, SH, IM, W, FE, MAIN));
}
void fwd_bwd_full() {
    mfvit_vit_cfg c = small_cfg();
    sizes(c);
    RC(mfvit_vit_forward(&c, P, SH, IM, W, FE, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, -1, MAIN));
}
void bwd_staged() {
    mfvit_vit_cfg c = small_cfg();
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 2, 1, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, 0, -1, MAIN));
}
void bwd_single_stages() {
    mfvit_vit_cfg c = small_cfg();
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 2, 2, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, 1, 0, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, -1, -1, MAIN));
}
void fwd_bwd_dtype(int dtype) {
    mfvit_vit_cfg c = small_cfg(dtype);
    sizes(c);
    RC(mfvit_vit_forward(&c, P, SH, IM, W, FE, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, -1, MAIN));
}
void fwd_bwd_f32() { fwd_bwd_dtype(MFVIT_F32); }
void fwd_bwd_bf16() { fwd_bwd_dtype(MFVIT_BF16); }
void fwd_bwd_f16() { fwd_bwd_dtype(MFVIT_F16); }

// ------------------------------------------------------------------ 2. the weight-gradient side stream
void side_full() {
    mfvit_vit_cfg c = side_cfg();
    sizes(c);
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, -1, MAIN));
}
void side_staged() {
    mfvit_vit_cfg c = side_cfg();
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 2, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, 1, -1, MAIN));
}
void side_gates() {   // each call runs without the side stream - and none creates one
    mfvit_vit_cfg c = side_cfg();
    mfvit_set_wgrad_stream(0);
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 2, MAIN));
    mfvit_set_wgrad_stream(1);
    tr::knob("capturing", 1);
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 2, MAIN));
    tr::knob("capturing", 0);
    c = side_cfg(5);    // M = 985
    sizes(c);
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 2, MAIN));
    setenv("MFVIT_DO_MAX", "0", 1);
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 2, MAIN));
    unsetenv("MFVIT_DO_MAX");
    c = side_cfg(21);   // M = 4,137
    sizes(c);
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 2, MAIN));
}
void side_second_caller_stream() {
    mfvit_vit_cfg c = side_cfg();
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 3, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 2, MAIN2));
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 3, 3, MAIN));   // (the first stream's side stream again)
}
void side_stream_share2() {
    mfvit_vit_cfg c = side_cfg();
    c.stream_share = 2;
    sizes(c);
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, 0, -1, MAIN));
    c = small_cfg(MFVIT_BF16X3, 0);
    c.stream_share = 2;
    RC(mfvit_vit_forward(&c, P, SH, IM, W, FE, MAIN));
}

// ------------------------------------------------------------------ 3. the paired weight gradient (4., MFVIT_DO_MAX=0: in side_gates)
void pair_unsupported() {
    mfvit_vit_cfg c = small_cfg();
    tr::knob("pair_ok", 0);
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, 1, 1, MAIN));
}

// ------------------------------------------------------------------ 5. unfused row passes
void unfused_768() {
    mfvit_vit_cfg c = image_cfg(MFVIT_BF16X3, 2, 32, 768, 12, 2);
    sizes(c);
    RC(mfvit_vit_forward(&c, P, SH, IM, W, FE, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, -1, MAIN));
}
void unfused_env_384() {
    mfvit_vit_cfg c = small_cfg();
    setenv("MFVIT_UNFUSED_ROWS", "1", 1);
    sizes(c);
    RC(mfvit_vit_forward(&c, P, SH, IM, W, FE, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, -1, MAIN));
}

// ------------------------------------------------------------------ 6. mfvit_vit_drop
const float DPATH[2] = {0.f, 0.1f};
void drop_case(float drop, float attn_drop, bool dpath, bool ex, int dtype = MFVIT_BF16, int hi = 2, int lo = -1) {
    mfvit_vit_cfg c = small_cfg(dtype);
    mfvit_vit_drop x = {drop, attn_drop, dpath ? DPATH : nullptr, 0x1234567890abcdefull};
    sizes(c, &x);
    RC(mfvit_vit_forward_drop(&c, &x, P, SH, IM, W, FE, MAIN));
    if (ex) RC(mfvit_vit_backward_ex(&c, &x, P, SH, W, DF, DP, nullptr, hi, lo, MAIN));
    else RC(mfvit_vit_backward_drop(&c, &x, P, SH, W, DF, DP, hi, lo, MAIN));
}
void drop_rate() { drop_case(0.1f, 0.f, false, false); }
void drop_attn_only() { drop_case(0.f, 0.1f, false, false, MFVIT_BF16, 1, 1); }
void drop_path_rowp() { drop_case(0.f, 0.f, true, true, MFVIT_BF16X3, 2, 1); }
void drop_path_no_rowp() {
    tr::knob("rowp_ok", 0);
    drop_case(0.f, 0.f, true, false, MFVIT_BF16X3, 0, 0);   // (the decision is the forward's)
}
void drop_all_three() { drop_case(0.1f, 0.2f, true, true); }
void drop_f32_invalid() { drop_case(0.1f, 0.f, false, false, MFVIT_F32); }

// ------------------------------------------------------------------ 7. / 8. stop_grad_conv1; image gradients
void stop_grad_conv1() {
    mfvit_vit_cfg c = small_cfg();
    c.stop_grad_conv1 = 1;
    sizes(c);
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, 0, -1, MAIN));
}
void dimg_with_dparams() {
    mfvit_vit_cfg c = small_cfg();
    sizes(c);
    RC(mfvit_vit_backward_ex(&c, nullptr, P, SH, W, nullptr, DP, DI, 0, -1, MAIN));
}
void dimg_only() {
    mfvit_vit_cfg c = small_cfg();
    RC(mfvit_vit_backward_ex(&c, nullptr, P, SH, W, DF, nullptr, DI, c.depth, -1, MAIN));
}
void dimg_pos_dropout() {
    mfvit_vit_cfg c = small_cfg(MFVIT_BF16);
    mfvit_vit_drop x = {0.1f, 0.f, nullptr, 77};
    sizes(c, &x);
    RC(mfvit_vit_backward_ex(&c, &x, P, SH, W, nullptr, DP, DI, -1, -1, MAIN));
    RC(mfvit_vit_backward_ex(&c, &x, P, SH, W, nullptr, nullptr, DI, -1, -1, MAIN));
}

// ------------------------------------------------------------------ 9. attention maps and relevance
void attn_case(unsigned long long blocks, int fuse, int cls_only, bool maps, bool rollout) {
    mfvit_vit_cfg c = small_cfg(MFVIT_BF16X3, 0);
    mfvit_vit_attn_req r = {blocks, fuse, cls_only, maps ? at<float>(MAPS) : nullptr, rollout ? at<float>(ROLLOUT) : nullptr, at(SCRATCH)};
    tr::note("attn_scratch_bytes %zu", mfvit_vit_attn_scratch_bytes(&c, &r));
    RC(mfvit_vit_forward_attn(&c, &r, P, SH, IM, W, FE, MAIN));
}
void attn_requests() {
    attn_case(2, 0, 0, true, false);    // a block subset
    attn_case(3, 0, 1, true, false);    // cls_only
    attn_case(1, 2, 0, true, false);    // fused
    attn_case(0, 1, 0, false, true);    // rollout only
    attn_case(3, 1, 1, true, true);     // maps + rollout
}
void rel_case(unsigned long long blocks, bool relevance) {
    mfvit_vit_cfg c = small_cfg();
    mfvit_vit_rel_req r = {blocks, blocks ? at<float>(MAPS) : nullptr, relevance ? at<float>(RELEVANCE) : nullptr, at(SCRATCH)};
    tr::note("rel_scratch_bytes %zu", mfvit_vit_rel_scratch_bytes(&c, &r));
    RC(mfvit_vit_backward_rel(&c, &r, P, SH, W, DF, MAIN));
}
void rel_requests() {
    rel_case(2, false);   // maps only
    rel_case(0, true);    // relevance only
    rel_case(3, true);    // both
}

// ------------------------------------------------------------------ 10. LoRA
mfvit_lora_item lora_item(int i, int block, int target) {
    const size_t off = (size_t)i << 20;
    return {block, target, at<float>(LA, off), at<float>(LB, off), at<float>(LDA, off), at<float>(LDB, off)};
}
void lora_prepare_shadow() {
    mfvit_vit_cfg c = small_cfg();
    const mfvit_lora_item items[] = {lora_item(0, 0, MFVIT_LORA_Q), lora_item(1, 1, MFVIT_LORA_FC2)};
    const mfvit_lora_req r = {8, 0.5f, 2, items};
    sizes(c);
    RC(mfvit_vit_prepare_shadow_lora(&c, P, &r, at<float>(EFF), SH, MAIN));
}
void lora_backward(const std::vector<mfvit_lora_item>& items, float* dimg, int stage_lo) {
    mfvit_vit_cfg c = small_cfg();
    const mfvit_lora_req r = {8, 0.5f, (int)items.size(), items.data()};
    tr::note("lora items %d dimg %s stage_lo %d", r.n, dimg ? "yes" : "no", stage_lo);
    sizes(c);
    RC(mfvit_vit_backward_lora(&c, nullptr, P, SH, W, DF, &r, at<float>(DW), dimg, c.depth, stage_lo, MAIN));
}
void lora_every_target() {
    std::vector<mfvit_lora_item> items;
    for (int l = 0; l < 2; ++l)
        for (int t = MFVIT_LORA_Q; t <= MFVIT_LORA_FC2; ++t) items.push_back(lora_item((int)items.size(), l, t));
    lora_backward(items, nullptr, 0);
}
void lora_proj_only() { lora_backward({lora_item(0, 0, MFVIT_LORA_PROJ), lora_item(1, 1, MFVIT_LORA_PROJ)}, nullptr, 0); }
void lora_lowest_block_1() { lora_backward({lora_item(0, 1, MFVIT_LORA_V), lora_item(1, 1, MFVIT_LORA_FC1)}, nullptr, 1); }
void lora_with_dimg() { lora_backward({lora_item(0, 1, MFVIT_LORA_K)}, DI, -1); }
void lora_grad() {
    mfvit_vit_cfg c = small_cfg();
    const mfvit_lora_item items[] = {lora_item(0, 0, MFVIT_LORA_PROJ), lora_item(1, 1, MFVIT_LORA_FC1)};
    const mfvit_lora_req r = {4, 2.f, 2, items};
    sizes(c);
    RC(mfvit_vit_lora_grad(&c, &r, DP, MAIN));
}
void lora_duplicate_item() { lora_backward({lora_item(0, 1, MFVIT_LORA_V), lora_item(1, 1, MFVIT_LORA_V)}, nullptr, 1); }

// ------------------------------------------------------------------ 11. the token-input GPT
void gpt_plain() {
    mfvit_vit_cfg c = gpt_cfg(MFVIT_BF16X3);
    sizes(c);
    RC(mfvit_gpt_forward(&c, P, SH, IM, W, FE, MAIN));
    RC(mfvit_gpt_backward(&c, P, SH, W, DF, DP, DT, MAIN));
}
void gpt_pos_relu_dropout() {
    mfvit_vit_cfg c = gpt_cfg(MFVIT_BF16);
    c.use_pos = 1; c.act = 1; c.p_embd = 0.1f; c.p_attn = 0.1f; c.p_resid = 0.1f; c.seed_lo = 7; c.seed_hi = 9;
    sizes(c);
    RC(mfvit_gpt_forward(&c, P, SH, IM, W, FE, MAIN));
    RC(mfvit_gpt_backward(&c, P, SH, W, DF, DP, DT, MAIN));
}
void gpt_pos_no_dropout() {
    mfvit_vit_cfg c = gpt_cfg(MFVIT_BF16X3);
    c.use_pos = 1; c.act = 1;
    sizes(c);
    RC(mfvit_gpt_forward(&c, P, SH, IM, W, FE, MAIN));
}
void gpt_tiled_unsupported() {
    mfvit_vit_cfg c = gpt_cfg(MFVIT_BF16);
    c.p_attn = 0.1f;
    sizes(c);
    tr::knob("tiled_ok", 0);
    RC(mfvit_gpt_forward(&c, P, SH, IM, W, FE, MAIN));
}
void gpt_f32_too_long() {   // the model's own 394 tokens at head_dim 64: past the exact attention's LDS image (T <= 315), refused with nothing launched
    mfvit_vit_cfg c = gpt_cfg(MFVIT_F32);
    c.tokens = 394; c.use_pos = 1; c.act = 1;
    sizes(c);
    RC(mfvit_gpt_forward(&c, P, SH, IM, W, FE, MAIN));
    RC(mfvit_gpt_backward(&c, P, SH, W, DF, DP, DT, MAIN));
    RC(mfvit_vit_prepare_shadow(&c, P, SH, MAIN));
    c.tokens = 315;             // the longest accepted sequence
    sizes(c);
}

// ------------------------------------------------------------------ 12. weight shadows
void prepare_shadow() {
    mfvit_vit_cfg c = small_cfg(MFVIT_F32);
    sizes(c);
    RC(mfvit_vit_prepare_shadow(&c, P, SH, MAIN));
    c = small_cfg(MFVIT_BF16);
    sizes(c);
    RC(mfvit_vit_prepare_shadow(&c, P, SH, MAIN));
    c = gpt_cfg(MFVIT_BF16);
    RC(mfvit_vit_prepare_shadow(&c, P, SH, MAIN));
}

// ------------------------------------------------------------------ 13. argument errors: MFVIT_EINVAL, nothing launched
void argument_errors() {
    mfvit_vit_cfg c = small_cfg();
    RC(mfvit_vit_forward(&c, nullptr, SH, IM, W, FE, MAIN));
    RC(mfvit_vit_backward(&c, nullptr, SH, W, DF, DP, c.depth, -1, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, 0, 1, MAIN));
    RC(mfvit_vit_backward_ex(&c, nullptr, P, SH, W, DF, DP, DI, c.depth, 0, MAIN));
    RC(mfvit_vit_backward_ex(&c, nullptr, P, SH, W, DF, nullptr, nullptr, c.depth, -1, MAIN));
    mfvit_vit_cfg n = small_cfg(MFVIT_BF16X3, 0);
    RC(mfvit_vit_backward(&n, P, SH, W, DF, DP, n.depth, -1, MAIN));
    RC(mfvit_vit_backward(&c, P, SH, W, nullptr, DP, c.depth, -1, MAIN));   // (no dfeatures for the final norm: after the call's set-up)
}

// ------------------------------------------------------------------ 14. an injected failure inside the side-stream backward
// after a first call that creates the side stream, the call is run once to find the number of the call to fail, then again with fail_at set
void fail_case(const char* prefix, int nth) {
    mfvit_vit_cfg c = side_cfg();
    mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, c.depth, MAIN);
    tr::take();
    mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, -1, MAIN);
    const int n = tr::find_call(prefix, nth);
    tr::take();
    tr::note("fail_at %d: call %d starting with '%s'", n, nth, prefix);
    tr::knob("fail_at", n);
    RC(mfvit_vit_backward(&c, P, SH, W, DF, DP, c.depth, -1, MAIN));
}
void fail_tile_gemm() { fail_case("gemm_nt_tile bf16x3 NONE", 1); }   // in the middle of a block
void fail_side_wgrad() { fail_case("gemm_tn ", 1); }
void fail_fork_record() { fail_case("hipEventRecord ev=ev1 ", 1); }

// ------------------------------------------------------------------ 15. the given-x0 and block-range entry points
// include/mfvit.h: the range [0, depth) issues exactly the launches of the whole-stack entry points (image_in = 1) / of the given-x0 entry points
// (image_in = 0).  Each pair of scenarios below makes the same requests through both; the traces must agree in every line but the `call` lines.
mfvit_vit_cfg range_cfg(int dtype = MFVIT_BF16X3) { return image_cfg(dtype, 2, 64, 384, 6, 2); }   // T = 17
const int X0_TOKENS = 9;
const mfvit_vit_drop RANGE_DROP = {0.1f, 0.1f, DPATH, 0x1234567890abcdefull};

// forward, an unstaged and a staged backward with parameter gradients, the data-gradient chain alone; drop: NULL or RANGE_DROP
void full_image_case(bool seg, const mfvit_vit_drop* x) {
    mfvit_vit_cfg c = range_cfg(x ? MFVIT_BF16 : MFVIT_BF16X3);
    const mfvit_vit_seg s = {0, c.depth, 17, 1};
    auto bwd = [&](float* dp, float* di, int hi, int lo) {
        if (seg) RC(mfvit_vit_backward_seg(&c, x, &s, P, SH, W, DF, dp, nullptr, di, hi, lo, MAIN));
        else RC(mfvit_vit_backward_ex(&c, x, P, SH, W, DF, dp, di, hi, lo, MAIN));
    };
    if (seg) RC(mfvit_vit_forward_seg(&c, x, &s, P, SH, IM, W, FE, MAIN));
    else if (x) RC(mfvit_vit_forward_drop(&c, x, P, SH, IM, W, FE, MAIN));
    else RC(mfvit_vit_forward(&c, P, SH, IM, W, FE, MAIN));
    bwd(DP, nullptr, c.depth, -1);
    bwd(DP, DI, c.depth, -1);
    bwd(DP, nullptr, 2, 1);
    bwd(DP, nullptr, 0, -1);
    bwd(DP, nullptr, 2, 1);
    bwd(DP, DI, 0, -1);
    bwd(nullptr, DI, c.depth, -1);
}
void stack_full_image() { full_image_case(false, nullptr); full_image_case(false, &RANGE_DROP); }
void seg_full_image() { full_image_case(true, nullptr); full_image_case(true, &RANGE_DROP); }

void full_x0_case(bool seg, const mfvit_vit_drop* x) {
    mfvit_vit_cfg c = range_cfg(x ? MFVIT_BF16 : MFVIT_BF16X3);
    const mfvit_vit_seg s = {0, c.depth, X0_TOKENS, 0};
    auto bwd = [&](float* dp, int hi, int lo) {
        if (seg) RC(mfvit_vit_backward_seg(&c, x, &s, P, SH, W, DF, dp, DT, nullptr, hi, lo, MAIN));
        else RC(mfvit_vit_backward_x0(&c, x, X0_TOKENS, P, SH, W, DF, dp, DT, hi, lo, MAIN));
    };
    if (seg) RC(mfvit_vit_forward_seg(&c, x, &s, P, SH, IM, W, FE, MAIN));
    else RC(mfvit_vit_forward_x0(&c, x, X0_TOKENS, P, SH, IM, W, FE, MAIN));
    bwd(DP, c.depth, -1);
    bwd(DP, 2, 1);
    bwd(DP, 0, -1);
    bwd(nullptr, c.depth, -1);
}
void x0_full() { full_x0_case(false, nullptr); full_x0_case(false, &RANGE_DROP); }
void seg_full_x0() { full_x0_case(true, nullptr); full_x0_case(true, &RANGE_DROP); }

// [0,1) on the full grid, then [1,2) on a shortened sequence, each on a workspace of its own; the backward range by range: every range in one
// call, then every range cut between its entry stage and its block, and between its block and what feeds it
void seg_two_ranges() {
    mfvit_vit_cfg c = range_cfg();
    const mfvit_vit_seg s0 = {0, 1, 17, 1}, s1 = {1, 2, X0_TOKENS, 0};
    void* const W1 = at(WS, (size_t)1 << 32);
    float *const X1 = at<float>(FEATS, (size_t)1 << 28), *const OUT = at<float>(FEATS, (size_t)2 << 28);
    float *const DX1 = DT, *const DOUT0 = at<float>(DTOKENS, (size_t)1 << 28);
    RC(mfvit_vit_forward_seg(&c, nullptr, &s0, P, SH, IM, W, FE, MAIN));
    RC(mfvit_vit_forward_seg(&c, nullptr, &s1, P, SH, X1, W1, OUT, MAIN));
    RC(mfvit_vit_backward_seg(&c, nullptr, &s1, P, SH, W1, DF, DP, DX1, nullptr, 2, 0, MAIN));
    RC(mfvit_vit_backward_seg(&c, nullptr, &s0, P, SH, W, DOUT0, DP, nullptr, DI, 1, -1, MAIN));
    RC(mfvit_vit_backward_seg(&c, nullptr, &s1, P, SH, W1, DF, DP, DX1, nullptr, 2, 2, MAIN));
    RC(mfvit_vit_backward_seg(&c, nullptr, &s1, P, SH, W1, DF, DP, DX1, nullptr, 1, 0, MAIN));
    RC(mfvit_vit_backward_seg(&c, nullptr, &s0, P, SH, W, DOUT0, DP, nullptr, nullptr, 1, 0, MAIN));
    RC(mfvit_vit_backward_seg(&c, nullptr, &s0, P, SH, W, DOUT0, DP, nullptr, DI, -1, -1, MAIN));
}

struct Scenario { const char* name; void (*run)(); };
#define S(f) {#f, f}
const Scenario SCENARIOS[] = {
    S(fwd_nosave), S(fwd_bwd_full), S(bwd_staged), S(bwd_single_stages), S(fwd_bwd_f32), S(fwd_bwd_bf16), S(fwd_bwd_f16),
    S(side_full), S(side_staged), S(side_gates),
    S(side_second_caller_stream), S(side_stream_share2), S(pair_unsupported), S(unfused_768), S(unfused_env_384),
    S(drop_rate), S(drop_attn_only), S(drop_path_rowp), S(drop_path_no_rowp), S(drop_all_three), S(drop_f32_invalid),
    S(stop_grad_conv1), S(dimg_with_dparams), S(dimg_only), S(dimg_pos_dropout),
    S(attn_requests), S(rel_requests),
    S(lora_prepare_shadow), S(lora_every_target), S(lora_proj_only), S(lora_lowest_block_1), S(lora_with_dimg), S(lora_grad), S(lora_duplicate_item),
    S(gpt_plain), S(gpt_pos_relu_dropout), S(gpt_pos_no_dropout), S(gpt_tiled_unsupported), S(gpt_f32_too_long), S(prepare_shadow), S(argument_errors),
    S(fail_tile_gemm), S(fail_side_wgrad), S(fail_fork_record),
    S(stack_full_image), S(seg_full_image), S(x0_full), S(seg_full_x0), S(seg_two_ranges),
};
#undef S

}  // namespace

int main(int argc, char** argv) {
    setenv("MFVIT_AB_LIVE", "1", 1);   // environment switches are read afresh on every call
    const char* only = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--list")) {
            for (const Scenario& s : SCENARIOS) puts(s.name);
            return 0;
        }
        if (!strcmp(argv[i], "--only") && i + 1 < argc) { only = argv[++i]; continue; }
        fprintf(stderr, "usage: %s [--list | --only NAME]\n", argv[0]);
        return 2;
    }
    int ran = 0;
    for (const Scenario& s : SCENARIOS) {
        if (only && strcmp(only, s.name)) continue;
        // a thread per scenario: the library's per-thread state (its table of side streams) starts empty
        std::thread([&s] { begin(); s.run(); }).join();
        printf("== %s\n%s", s.name, tr::take().c_str());
        ++ran;
    }
    if (!ran) { fprintf(stderr, "no scenario named %s\n", only); return 2; }
    return 0;
}
