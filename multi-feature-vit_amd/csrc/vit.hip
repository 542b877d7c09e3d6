// Composite ViT-S/16 encoder forward / backward: host-side launch sequences over the gfx950 kernels, plus the
// C ABI entry points of include/mfvit.h for the encoder and the single ops.  No allocation, no synchronisation:
// every launch goes to the caller's stream, all memory (parameters, shadows, workspace) is caller-owned.
#include "../../include/mfvit.h"
#include "kernels.h"
#include "prof.h"

#include <atomic>
#include <stdlib.h>

using namespace mfvit;

namespace mfvit {
static std::atomic<int> g_stream_share{1};
// the hint of the encoder call this thread is inside of (mfvit_vit_cfg::stream_share), or 0: the process-wide default
static thread_local int t_stream_share = 0;
int stream_share() { return t_stream_share > 0 ? t_stream_share : g_stream_share.load(std::memory_order_relaxed); }
namespace {
struct ShareScope {
    int prev;
    explicit ShareScope(const mfvit_vit_cfg* cfg) : prev(t_stream_share) { if (cfg && cfg->stream_share > 0) t_stream_share = cfg->stream_share > 8 ? 8 : cfg->stream_share; }
    ~ShareScope() { t_stream_share = prev; }
};
}  // namespace
}  // namespace mfvit

namespace {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Dims {
    int Tp;                             // token rows of the ARENA's pos_embed (= T, but for the given-x0 entry points: 1 + gh gw there, T = the shortened sequence)
    bool x0in;                          // given-x0 entry points (mfvit_vit_forward_x0): the embedding stage is the caller's, stage -1 of the backward writes d x_0
    int l0, l1;                         // the blocks [l0, l1) a call runs: the whole stack, but for the block-range entry points (mfvit_vit_forward_seg)
    int dtype, B, T, np, D, depth, H, HD, F, M, Mp, es, ep;   // es: bytes per LOGICAL element of a dtype tensor; ep: storage elements per logical one
    bool save, tok, use_pos;
    int act;
    float p_embd, p_attn, p_resid;      // dropout sites (0 = off): token-input mode from the cfg, image mode from mfvit_vit_drop
    float p_gelu;                       // image mode: dropout after the MLP activation (timm Mlp.drop, folded into the fc1 epilogue)
    const float* dpr;                   // image mode: drop-path rate of every block (host array of depth entries) or NULL
    unsigned long long seed;
    bool drop;                          // any site active
    bool rdrop;                         // a residual branch is masked (p_resid > 0 or a drop path): branch -> scratch, then a dropout + residual + LN row pass
    bool unfused;                       // residual + LayerNorm (and its backward) as row passes behind plain tile GEMMs instead of the row-complete GEMM kernels
};

bool get_dims(const mfvit_vit_cfg* c, Dims& d) {
    if (!c) return false;
    if (c->dtype != MFVIT_F32 && c->dtype != MFVIT_BF16 && c->dtype != MFVIT_BF16X3 && c->dtype != MFVIT_F16) return false;
    d.tok = c->token_input != 0;
    if (c->batch <= 0) return false;
    if (d.tok ? c->tokens <= 0 : (c->img_h <= 0 || c->img_w <= 0 || c->img_h % 16 || c->img_w % 16)) return false;
    if (c->act != 0 && c->act != 1) return false;
    // embed dim: 384 (vit_small: the row-complete GEMM kernels with their fused LayerNorm epilogues) or 768 (vit_base: plain tile GEMMs + row passes)
    if ((c->dim != 384 && c->dim != 768) || c->depth <= 0 || c->heads <= 0 || c->dim % c->heads) return false;
    if (c->mlp_dim % 128 || c->mlp_dim <= 0) return false;
    d.dtype = c->dtype;
    d.B = c->batch;
    d.np = d.tok ? c->tokens : (c->img_h / 16) * (c->img_w / 16);
    d.T = d.tok ? c->tokens : d.np + 1;
    d.Tp = d.T;
    d.x0in = false;
    d.l0 = 0;
    d.l1 = c->depth;
    d.use_pos = c->use_pos != 0;
    d.act = c->act;
    d.D = c->dim;
    d.depth = c->depth;
    d.H = c->heads;
    d.HD = c->dim / c->heads;
    d.F = c->mlp_dim;
    d.M = d.B * d.T;
    d.Mp = d.B * d.np;
    d.es = (c->dtype == MFVIT_BF16 || c->dtype == MFVIT_F16) ? 2 : 4;   // split bf16: hi + lo = 4 bytes
    d.ep = c->dtype == MFVIT_BF16X3 ? 2 : 1;
    d.save = c->save_for_backward != 0;
    d.p_embd = d.tok ? c->p_embd : 0.f;
    d.p_attn = d.tok ? c->p_attn : 0.f;
    d.p_resid = d.tok ? c->p_resid : 0.f;
    for (float pp : {d.p_embd, d.p_attn, d.p_resid})
        if (!(pp >= 0.f && pp < 1.f)) return false;
    d.p_gelu = 0.f;
    d.dpr = nullptr;
    d.drop = d.p_embd > 0.f || d.p_attn > 0.f || d.p_resid > 0.f;
    d.rdrop = d.p_resid > 0.f;
    if (d.drop && c->dtype == MFVIT_F32) return false;               // the dropout stages exist for the 16-bit operand types
    d.seed = ((unsigned long long)c->seed_hi << 32) | c->seed_lo;
    if (d.HD != 32 && d.HD != 64 && d.HD != 96) return false;
    if (d.HD == 96 && c->dtype == MFVIT_F32) return false;      // head_dim 96 runs on the streaming MFMA kernels (16-bit types, split bf16)
    if (c->dtype == MFVIT_BF16X3 && d.HD % 32) return false;    // a head's row piece is whole [hi x 32 | lo x 32] groups
    // MFVIT_F32 runs the exact attention kernels (attention.hip), which hold a head's K and V in LDS: the backward's image, K / V plus two [T]
    // vectors, is the larger one and must fit 160 KiB (head_dim 64: T <= 315, head_dim 32: T <= 620).  Refused here, with every other limit,
    // and not by the attention launcher in the middle of block 0.
    if (c->dtype == MFVIT_F32 && 2 * (size_t)d.T * d.HD * 4 + 2 * (size_t)d.T * 4 > 160 * 1024) return false;
    // MFVIT_UNFUSED_ROWS=1 forces the unfused path at dim 384 too (tests: the same encoder through both paths; tools: A/B at small M)
    // (read on every call, not cached: the workspace layout depends on it, and a test flips it between two encoders of one process)
    const char* ue = getenv("MFVIT_UNFUSED_ROWS");
    d.unfused = d.D != 384 || (ue && ue[0] == '1');
    return true;
}

// Image mode in training (mfvit_vit_drop; NULL = none): timm's dropout sites.  pos_drop, proj_drop, the MLP's two drops: x->drop; the attention
// probabilities: x->attn_drop; the drop path of block l's two branches: x->drop_path[l].  Sites: see include/mfvit.h.
bool get_dims(const mfvit_vit_cfg* c, const mfvit_vit_drop* x, Dims& d) {
    if (!get_dims(c, d)) return false;
    if (!x) return true;
    if (d.tok) return false;                                           // (the GPT keeps its own three sites in the cfg)
    for (float pp : {x->drop, x->attn_drop})
        if (!(pp >= 0.f && pp < 1.f)) return false;
    bool dpath = false;
    if (x->drop_path)
        for (int l = 0; l < d.depth; ++l) {
            if (!(x->drop_path[l] >= 0.f && x->drop_path[l] < 1.f)) return false;
            dpath = dpath || x->drop_path[l] > 0.f;
        }
    d.p_embd = d.p_resid = d.p_gelu = x->drop;
    d.p_attn = x->attn_drop;
    d.dpr = dpath ? x->drop_path : nullptr;
    d.seed = x->seed;
    d.drop = x->drop > 0.f || x->attn_drop > 0.f || dpath;
    d.rdrop = x->drop > 0.f || dpath;
    if (d.drop && c->dtype == MFVIT_F32) return false;                 // the dropout stages exist for the 16-bit operand types
    return true;
}

// A block range of the image-mode stack (mfvit_vit_forward_seg): blocks [block_lo, block_hi) at `tokens` rows per image, entered with the image
// (the embedding stage: block_lo == 0 on the full grid only) or with the residual stream x_{block_lo}: an ordinary image-mode cfg whose arena keeps
// the full grid (Tp = 1 + gh gw rows of pos_embed), every activation and launch at T = tokens.
// (the limits of get_dims hold for the full grid - the same model runs it in eval() - and with them for every shorter sequence)
bool get_dims_seg(const mfvit_vit_cfg* c, const mfvit_vit_drop* x, const mfvit_vit_seg* s, Dims& d) {
    if (!s || !get_dims(c, x, d) || d.tok) return false;
    if (s->block_lo < 0 || s->block_lo >= s->block_hi || s->block_hi > d.depth) return false;
    if (s->tokens < 2 || s->tokens > d.Tp || (s->image_in != 0 && s->image_in != 1)) return false;
    if (s->image_in && (s->block_lo != 0 || s->tokens != d.Tp)) return false;
    d.T = s->tokens;
    d.M = d.B * s->tokens;
    d.x0in = !s->image_in;
    d.l0 = s->block_lo;
    d.l1 = s->block_hi;
    return true;
}
// the stack on a given x_0 (mfvit_vit_forward_x0; timm PatchDropout shortens the sequence in front of the blocks): the range [0, depth) entered with x_0
mfvit_vit_seg x0_seg(const mfvit_vit_cfg* c, int tokens) { return {0, c ? c->depth : 0, tokens, 0}; }

// ------------------------------------------------------------------ parameter arena layout (floats)
struct ParamLayout {
    long cls, pos, pe_w, pe_b, blk0, blk_stride, norm_w, norm_b, total;
    // offsets inside a block
    long ln1_w, ln1_b, qkv_w, qkv_b, proj_w, proj_b, ln2_w, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b;
};
ParamLayout param_layout(const Dims& d) {
    ParamLayout L;
    const long D = d.D, F = d.F;
    long o = 0;
    L.cls = o; o += d.tok ? 0 : D;                   // token-input mode: no cls token, no patch embedding
    L.pos = o; o += (long)d.Tp * D;
    L.pe_w = o; o += d.tok ? 0 : D * 768;
    L.pe_b = o; o += d.tok ? 0 : D;
    L.blk0 = o;
    long b = 0;
    L.ln1_w = b; b += D;
    L.ln1_b = b; b += D;
    L.qkv_w = b; b += 3 * D * D;
    L.qkv_b = b; b += 3 * D;
    L.proj_w = b; b += D * D;
    L.proj_b = b; b += D;
    L.ln2_w = b; b += D;
    L.ln2_b = b; b += D;
    L.fc1_w = b; b += F * D;
    L.fc1_b = b; b += F;
    L.fc2_w = b; b += D * F;
    L.fc2_b = b; b += D;
    L.blk_stride = b;
    o += b * d.depth;
    L.norm_w = o; o += D;
    L.norm_b = o; o += D;
    L.total = o;
    return L;
}

// ------------------------------------------------------------------ weight shadow layout (bytes)
struct ShadowLayout {
    size_t pe_w;                       // [D][768] dtype (bf16 only; f32 reads the arena)
    size_t blk0, blk_stride;           // per block:
    size_t qkv_w, qkv_t, proj_w, proj_t, fc1_w, fc1_t, fc2_w, fc2_t;
    size_t total;
};
ShadowLayout shadow_layout(const Dims& d) {
    ShadowLayout S;
    const size_t D = d.D, F = d.F, es = d.es;
    const bool hw = d.dtype != MFVIT_F32;  // keep straight copies only when a cast is needed
    size_t o = 0;
    S.pe_w = o; o += (hw && !d.tok) ? align256(D * 768 * es) : 0;
    S.blk0 = o;
    size_t b = 0;
    S.qkv_w = b; b += hw ? align256(3 * D * D * es) : 0;
    S.qkv_t = b; b += align256(3 * D * D * es);
    S.proj_w = b; b += hw ? align256(D * D * es) : 0;
    S.proj_t = b; b += align256(D * D * es);
    S.fc1_w = b; b += hw ? align256(F * D * es) : 0;
    S.fc1_t = b; b += align256(F * D * es);
    S.fc2_w = b; b += hw ? align256(D * F * es) : 0;
    S.fc2_t = b; b += align256(D * F * es);
    S.blk_stride = b;
    o += b * d.depth;
    S.total = o;
    return S;
}

// ------------------------------------------------------------------ workspace layout (bytes)
constexpr int TN_SLOTS = 5;
struct WsLayout {
    size_t patches;
    size_t x0, x_stride;        // f32 [M][D], depth+1 (save) or 1 copies
    size_t st0, st_stride;      // LN1 / final-norm stats: mean [M] then rstd [M], depth+1 or 1 copies
    size_t blk0, blk_stride;    // per block (depth or 1 copies):
    size_t y1, qkv, attn, lse, xmid, st2, y2, hpre, hact;
    // backward scratch
    size_t gx, gmid, gxT, gmidT, dhpre, dattn, dqkv, colscratch, colpart, colpart_stride = 0, tnpart, tnpart_stride = 0;
    size_t dtmp;                // with a masked residual branch (Dims::rdrop): [M][D] of the operand type (branch output before the dropout; masked dY)
    size_t kpart;               // gemm_rowp with K splits (small M): partial accumulator tiles, 264 workgroups x 7 x 12 x 512 floats (gemm_rowp.hip)
    size_t utmp;                // unfused path: [M][D] of the operand type (output of the plain tile GEMM in front of a LayerNorm / LayerNorm-backward row pass)
    size_t domax;               // backward: the largest |d attn| of every (image, head) of every block, f32 bits [depth][B][H] (proj data gradient -> attention backward)
    size_t pp_stride;           // distance between the two ping-pong copies of gxT / gmidT / dhpre / dqkv (0 = none)
    size_t total;
    size_t ytail;               // a block range that ends below the final norm: [M][D] of the operand type (the LayerNorm output of its last fc2 epilogue, read by nobody)
    size_t wpeT, total_dimg;    // image gradient (mfvit_vit_backward_ex): W_pe^T [768][D] of the operand type behind `total` - a workspace of total_dimg bytes
};
WsLayout ws_layout(const Dims& d) {
    WsLayout W;
    const size_t M = d.M, D = d.D, F = d.F, es = d.es;
    const size_t nl = d.save ? d.l1 - d.l0 : 1;        // block copies: the blocks of this call
    const size_t nlp = d.save ? d.depth : 1;            // (the column-sum partial buffers keep the whole stack's count: BwdCtx::next_colpart)
    size_t o = 0;
    W.patches = o; o += (d.tok || d.x0in) ? 0 : align256((size_t)d.Mp * 768 * es);
    W.x0 = o; W.x_stride = align256(M * D * 4); o += W.x_stride * (d.save ? nl + 1 : 1);
    W.st0 = o; W.st_stride = align256(2 * M * 4); o += W.st_stride * (d.save ? nl + 1 : 1);
    W.blk0 = o;
    size_t b = 0;
    W.y1 = b; b += align256(M * D * es);
    W.qkv = b; b += align256(M * 3 * D * es);
    W.attn = b; b += align256(M * D * es);
    W.lse = b; b += align256((size_t)d.B * d.H * d.T * 4);
    W.xmid = b; b += align256(M * D * 4);
    W.st2 = b; b += align256(2 * M * 4);
    W.y2 = b; b += align256(M * D * es);
    W.hpre = b; b += d.save ? align256(M * F * (d.dtype == MFVIT_BF16X3 ? 2 : es)) : 0;   // act'(pre): plain fp16 for split tensors; not kept by no-grad forwards
    W.hact = b; b += align256(M * F * es);
    W.blk_stride = b;
    o += b * nl;
    if (d.save) {
        W.gx = o; o += align256(M * D * 4);
        W.gmid = o; o += align256(M * D * 4);
        // dY buffers read by the weight-gradient kernels on the side stream: two copies, used by layer parity
        W.gxT = o; o += align256(M * D * es);
        W.gmidT = o; o += align256(M * D * es);
        W.dhpre = o; o += align256(M * F * es);
        W.dqkv = o; o += align256(M * 3 * D * es);
        W.pp_stride = o - W.gxT;
        o += W.pp_stride;
        W.dattn = o; o += align256(M * D * es);
        W.colscratch = o; o += align256(2 * D * 4);
        {   // per-workgroup column-sum partials: max over the kernels that use them
            // row kernels: one partial row set [3][D] per workgroup - gemm_rowp launches at most one tile per CU and round (<= max(#CUs, M / 16) tiles),
            // gemm_nt_row full 64-row tiles (the former M / 64 + 256 bound belonged to the removed balanced-rows option)
            const size_t tiles_row = (M + 63) / 64 > 256 ? (M + 63) / 64 : 256;
            size_t a = tiles_row * 3 * D, b2 = 4 * ((M + 191) / 192) * F, c2 = 256 * 3 * D;      // (b2: the x act' tile epilogue - one row of F sums per wave-row block of a tile; tiles are 256 or 192 rows)
            size_t n = a > b2 ? a : b2;
            n = n > c2 ? n : c2;
            W.colpart = o; o += (3 * nlp + 2) * align256(n * 4);          // one partial buffer per launch of a backward call that leaves column sums (batched reduce)
            W.colpart_stride = align256(n * 4);
        }
        // split partials of the weight-gradient GEMMs: one slot per launch of a BLOCK (at most 4) + 1 for the patch embedding, each tiles * splits <= 384
        // blocks of 128 x 128 floats; reduced by one batched launch per block, in a fixed order (deterministic sums, round 5), then reused
        W.tnpart_stride = align256((size_t)384 * 128 * 128 * 4);
        W.tnpart = o; o += (size_t)TN_SLOTS * W.tnpart_stride;
    } else {
        W.gx = W.gmid = W.gxT = W.gmidT = W.dhpre = W.dattn = W.dqkv = W.colscratch = W.colpart = W.tnpart = o;
        W.pp_stride = 0;
    }
    W.dtmp = o; o += d.rdrop ? align256(M * D * es) : 0;
    W.kpart = o; o += d.D == 384 ? align256((size_t)264 * 7 * 12 * 512 * 4) : 0;
    W.utmp = o; o += align256(M * D * es);     // always there (1 / 200 of the workspace): the layout does not depend on which path a call takes
    W.domax = o; o += d.save ? align256((size_t)d.depth * d.B * d.H * 4) : 0;
    W.ytail = o; o += d.l1 < d.depth ? align256(M * D * es) : 0;
    W.total = o;
    W.wpeT = o; o += (d.save && !d.tok && !d.x0in) ? align256((size_t)768 * D * es) : 0;
    W.total_dimg = o;
    return W;
}

// ------------------------------------------------------------------ per-call context of encoder_forward / encoder_backward
struct EncCtx {
    const mfvit_vit_cfg* const cfg;
    const Dims d;
    const ParamLayout L;
    const ShadowLayout S;
    const WsLayout W;
    char* const ws;
    const char* const sh;
    const float* const params;
    const hipStream_t st;
    const long D, F;
    const long e;            // leading dimensions of dtype tensors are in storage elements
    const bool hw;           // 16-bit / split operands: the forward GEMMs read the weight shadows, f32 reads the arena
    // only split bf16 (hi + lo = the f32 value to 2^-17) drops the f32 residual-gradient copies; plain bf16 / fp16 keep them: re-rounding the residual
    // gradient to 8 / 11 mantissa bits at each of the 2 x depth LayerNorm-backward stages departs from the reference's autocast (fp32 residual grads)
    const bool lean_grad;    // (the unfused row passes read the f32 residual gradient)
    const float eps;
    const DropP off = make_drop(0.f, 0, 0);

    EncCtx(const mfvit_vit_cfg* cfg_, const Dims& dims, const float* params_, const void* shadow, void* workspace, mfvit_stream_t stream)
        : cfg(cfg_), d(dims), L(param_layout(dims)), S(shadow_layout(dims)), W(ws_layout(dims)), ws((char*)workspace), sh((const char*)shadow), params(params_),
          st((hipStream_t)stream), D(dims.D), F(dims.F), e(dims.ep), hw(dims.dtype != MFVIT_F32),
          lean_grad(dims.dtype == MFVIT_BF16X3 && !dims.unfused), eps(cfg_->ln_eps) {}

    // activations are kept per block for a backward (save), in one copy otherwise
    size_t slot(int l) const { return d.save ? (size_t)(l - d.l0) : 0; }
    float* xbuf(int l) const { return (float*)(ws + W.x0 + slot(l) * W.x_stride); }
    float* stat(int l) const { return (float*)(ws + W.st0 + slot(l) * W.st_stride); }
    char* blk(int l) const { return ws + W.blk0 + slot(l) * W.blk_stride; }
    const float* pblk(int l) const { return params + L.blk0 + (long)l * L.blk_stride; }
    const char* sblk(int l) const { return sh + S.blk0 + (size_t)l * S.blk_stride; }
    float* kpart() const { return (float*)(ws + W.kpart); }
    // the W operand of a forward GEMM
    const void* weight(const char* shadow_w, const float* arena_w) const { return hw ? (const void*)shadow_w : (const void*)arena_w; }
    // dropout sites (include/mfvit.h): the GPT's from the cfg, the ViT's from mfvit_vit_drop
    static unsigned site(int l, int which) { return 16u * (unsigned)l + (unsigned)which; }
    DropP dpath(int l, int which) const { return make_drop(d.dpr ? d.dpr[l] : 0.f, d.seed, site(l, which)); }   // per sample: keep of row r = sample r / T
};

struct BranchDrop { DropP drop, dpath; };   // masks of a residual branch: the element dropout and the per-sample drop path

// the plain tile GEMM of the same product: operands, shape and bias, nothing else
GemmP operands_of(const GemmP& p) {
    GemmP q = nt(p.A, p.lda, p.W, p.ldw, p.M, p.N, p.K);
    q.bias = p.bias;
    return q;
}

// One "Linear, then residual + LayerNorm" site of the forward.  p: the REPI_RES_LN parameters of the site (kpart included where the site has one).
// mask: the dropout of the branch and its drop path, NULL for a site whose branch is never masked (the patch embedding).  tag: the profiler tag
// of the row-complete launches.  The first path that applies:
//   1. drop path as the only masked branch (the fine-tune recipe: drop_rate = 0, drop_path_rate > 0) stays on the row-complete kernel: its
//      drop-path epilogue (REPI_RES_LN_DP, gemm_rowp.hip) adds the residual rows (aux) to the sample-scaled branch - where that kernel applies
//   2. a masked branch: plain GEMM + bias -> scratch, then dropout (element mask x per-sample drop-path factor) + residual + LayerNorm in one row pass
//   3. unfused: plain GEMM + bias -> scratch, then residual + LayerNorm as one row pass
//   4. the row-complete GEMM with the residual + LayerNorm epilogue
int linear_res_ln(const EncCtx& c, const GemmP& p, const BranchDrop* mask, int tag) {
    const Dims& d = c.d;
    const long De = c.D * c.e;
    const bool masked = mask && d.rdrop;
    if (masked && !(d.p_resid > 0.f) && !d.unfused) {
        GemmP r = p;
        r.aux = p.res; r.ldaux = p.ldres; r.res = nullptr; r.ldres = 0;
        r.drop = mask->dpath; r.drop_tpr = d.T;
        ProfTag scope(tag);
        if (gemm_nt_rowp_supported(d.dtype, REPI_RES_LN_DP, r)) return gemm_nt_rowp(d.dtype, REPI_RES_LN_DP, r, c.st);
    }
    if (masked || d.unfused) {
        GemmP q = operands_of(p);
        q.out0 = c.ws + (masked ? c.W.dtmp : c.W.utmp); q.ldo0 = De;
        MFVIT_TRY(gemm_nt_tile(d.dtype, EPI_BIAS, q, c.st));
        if (masked)
            return drop_add_ln_rows(d.dtype, d.D, q.out0, De, nullptr, 0, nullptr, 0, 0, p.res, p.ldres, mask->drop, mask->dpath, d.T, (float*)p.out0,
                                    p.ldo0, p.out1, p.ldo1, p.y_f32, p.gamma, p.beta, p.eps, p.mean, p.rstd, p.M, c.st);
        // a periodic residual (res_mod) is a table indexed by the output row: the row pass takes it as `pos`, with the site's row remap
        const bool table = p.res_mod != 0;
        return add_ln_rows(d.dtype, d.D, q.out0, De, table ? p.res : nullptr, table ? p.ldres : 0, table ? p.orow_out : 0, table ? nullptr : p.res,
                           table ? 0 : p.ldres, p.orow_in, p.orow_out, p.orow_off, (float*)p.out0, p.ldo0, p.out1, p.ldo1, p.y_f32, p.gamma, p.beta,
                           p.eps, p.mean, p.rstd, p.M, c.st);
    }
    ProfTag scope(tag);
    return gemm_nt_row(d.dtype, REPI_RES_LN, p, c.st);
}

// One "data-gradient GEMM, then LayerNorm backward + residual gradient + column sums" site of the backward.  p: the product, the LayerNorm input
// (aux), its statistics and weight, the column-sum targets and kpart.  The residual gradient comes in f32 (res) - or, lean_grad, in the operand
// type alone (res_t); the result goes to dx (f32, NULL: not kept) and dx_t (operand type).
// 16-bit modes: the f32 copies were a second 38.7 MB store per launch (14 % of it) read by nobody else but the embedding stage.
int dgrad_ln_bwd(const EncCtx& c, GemmP p, const float* res, const void* res_t, float* dx, void* dx_t) {
    const Dims& d = c.d;
    const long D = c.D, De = c.D * c.e;
    if (d.unfused) {
        // plain data-gradient GEMM -> scratch, then the LayerNorm backward + residual-gradient add + column sums as one row pass
        GemmP q = operands_of(p);
        q.out0 = c.ws + c.W.utmp; q.ldo0 = De;
        MFVIT_TRY(gemm_nt_tile(d.dtype, EPI_NONE, q, c.st));
        return ln_bwd_rows(d.dtype, d.D, nullptr, 0, (const float*)p.aux, p.ldaux, p.mean, p.rstd, p.gamma, res, D, dx, D, dx_t, De, p.cs0, p.cs1,
                           p.cs2, p.cpart, p.M, 1, 0, c.st, q.out0, De);
    }
    if (c.lean_grad) { p.res_t = res_t; p.ldres_t = De; }
    else { p.res = res; p.ldres = D; }
    p.out0 = dx; p.ldo0 = D; p.out1 = dx_t; p.ldo1 = De;
    return gemm_nt_row(d.dtype, REPI_LNBWD_RES, p, c.st);
}

// Weight-gradient GEMMs are leaves of the backward graph: they CAN run on a second (library-owned, lazily created) HIP stream beside the
// dgrad chain, ordered by events.  Round 3 made the caller's stream the default; round 5 brought the side stream back at small M only (the rule
// in wgrad_side_stream).  The side stream was worth 3 - 4 % while the weight-gradient and row kernels left half of every CU's LDS and issue slots
// free (round 2); now they are one-workgroup-per-CU kernels that own the chip while they run, nothing co-resides with them, and the second queue
// only adds event waits and a worse launch order: measured on one box, three alternating repeats, 31.25 / 31.33 / 31.36 ms per step with the side
// stream, 30.81 / 30.80 / 30.86 without (profiles/r03_streams_ab.txt).
struct SideStream {
    hipStream_t owner = nullptr;    // caller stream this side stream is paired with
    hipStream_t s = nullptr;
    hipEvent_t in = nullptr, end = nullptr;
    hipEvent_t done[64] = {};
    bool ok = false;
};
std::atomic<int> g_wgrad_stream{1};   // runtime switch (mfvit_set_wgrad_stream): attribution passes serialise the backward
SideStream& side_stream(hipStream_t caller) {
    // one side stream per (thread, caller stream): two encoders running on two caller streams do not share a side queue
    static thread_local SideStream ss[8];
    static thread_local int used = 0;
    SideStream* px = nullptr;
    for (int i = 0; i < used; ++i)
        if (ss[i].owner == caller) px = &ss[i];
    if (!px) {
        px = &ss[used < 8 ? used++ : 7];
        if (px->owner != caller && px->s) return *px;   // table full: share the last one
        px->owner = caller;
    }
    SideStream& x = *px;
    if (!x.s) {   // (created on first use)
        if (hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&x.in, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&x.end, hipEventDisableTiming) == hipSuccess) {
            x.ok = true;
            for (auto& e : x.done) x.ok = x.ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        }
        if (!x.ok && !x.s) x.s = (hipStream_t)-1;   // do not retry
    }
    return x;
}

// The side stream a backward call runs its weight gradients on, or NULL: everything on the caller's stream.  Decided before the side stream of
// this caller stream is looked up - and created - at all.
// (never inside a caller's stream capture: the library-owned side stream is not part of the caller's capture, and its last weight gradients are joined by the
// NEXT call's fork, not before this one returns - a capture ending in between would hold unjoined work.  The package itself no longer captures steps:
// the whole-step HIP graph of round 5 gained nothing, 8.22 vs 8.12 ms, and was removed in round 6)
// (residual dropout / drop path: the masked dY copies live in ONE scratch buffer - everything stays on the caller's stream)
// Default since round 5: the side stream at SMALL M only (1,024 ... 4,096 token rows: 6 - 20 images) - there no kernel fills the chip, the launches of a
// block are a dependent chain of ~10 us kernels with ~5 us of dispatch gap each, and the weight gradients (leaves) beside the data-gradient chain
// shorten it: 20 pairs per step 7.31 -> 6.66 ms, 16 pairs 6.31 -> 6.10 (then host-bound), 8 pairs 5.18 -> 4.96; 4 pairs LOSE (host-bound either way, 5.1 ->
// 6.9 ms) and 32 pairs gain 1 % (profiles/r05_small_batch.txt).
SideStream* wgrad_side_stream(const EncCtx& c, bool wg) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(c.st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    const bool side_wanted = wg && c.d.M >= 1024 && c.d.M <= 4096 && g_wgrad_stream.load(std::memory_order_relaxed) != 0 && !c.d.rdrop && !capturing;
    if (!side_wanted) return nullptr;
    SideStream& ss = side_stream(c.st);
    return ss.ok && c.W.pp_stride != 0 ? &ss : nullptr;
}

// Where the weight gradients of one backward call go, and how that queue is ordered against the data-gradient chain on the caller's stream.
// (with the side stream every weight gradient AND every reduce of their partials runs on it - the patch embedding's too - so the scratch slots
// are still written and read in one stream's order)
struct WgradQueue {
    SideStream* const side;         // NULL: no second queue, every member below but `s` does nothing
    const hipStream_t main, s;      // the caller's stream; the stream of the weight-gradient GEMMs and of the reduces of their partials
    const int top;                  // the highest block of this call
    WgradQueue(SideStream* side_, hipStream_t main_, int top_) : side(side_), main(main_), s(side_ ? side_->s : main_), top(top_) {}
    // main -> side dependency at this point of the main stream: the side stream may only start after everything already queued on the caller's
    // stream (activations, zeroed gradients)
    int fork() const {
        return !side || (hipEventRecord(side->in, main) == hipSuccess && hipStreamWaitEvent(s, side->in, 0) == hipSuccess) ? MFVIT_OK : MFVIT_ELAUNCH;
    }
    int wait_layer(int l) const {   // main waits until the wgrads of layer l (a layer of this call) have finished
        if (!side || l < 0 || l > top) return MFVIT_OK;
        return hipStreamWaitEvent(main, side->done[l & 63], 0) == hipSuccess ? MFVIT_OK : MFVIT_ELAUNCH;
    }
    int mark_done(int l) const {    // everything queued so far is what layer l's wgrads are
        return !side || hipEventRecord(side->done[l & 63], s) == hipSuccess ? MFVIT_OK : MFVIT_ELAUNCH;
    }
    int join() const {              // everything the side stream did is ordered before whatever the caller queues next
        return !side || (hipEventRecord(side->end, s) == hipSuccess && hipStreamWaitEvent(main, side->end, 0) == hipSuccess) ? MFVIT_OK : MFVIT_ELAUNCH;
    }
};

}  // namespace

extern "C" {

int mfvit_abi_version(void) { return 5; }
int mfvit_set_stream_share(int n) {
    mfvit::g_stream_share.store(n < 1 ? 1 : (n > 8 ? 8 : n), std::memory_order_relaxed);
    return MFVIT_OK;
}
int mfvit_set_wgrad_stream(int enabled) {
    g_wgrad_stream.store(enabled ? 1 : 0, std::memory_order_relaxed);
    return MFVIT_OK;
}
const char* mfvit_build_info(void) { return "libmfvit_hip gfx950 (MFMA bf16 | split-bf16 x3 | f16 32x32x16, f32 32x32x2), wave64, abi 5"; }

size_t mfvit_vit_param_count(const mfvit_vit_cfg* cfg) {
    Dims d;
    if (!get_dims(cfg, d)) return 0;
    return (size_t)param_layout(d).total;
}
int mfvit_vit_param_layout(const mfvit_vit_cfg* cfg, int64_t out[9]) {
    Dims d;
    if (!get_dims(cfg, d) || !out) return MFVIT_EINVAL;
    const ParamLayout L = param_layout(d);
    out[0] = L.cls; out[1] = L.pos; out[2] = L.pe_w; out[3] = L.pe_b; out[4] = L.blk0; out[5] = L.blk_stride;
    out[6] = L.norm_w; out[7] = L.norm_b; out[8] = L.total;
    return MFVIT_OK;
}
size_t mfvit_vit_shadow_bytes(const mfvit_vit_cfg* cfg) {
    Dims d;
    if (!get_dims(cfg, d)) return 0;
    return shadow_layout(d).total;
}
size_t mfvit_vit_workspace_bytes(const mfvit_vit_cfg* cfg) {
    Dims d;
    if (!get_dims(cfg, d)) return 0;
    return ws_layout(d).total;
}
size_t mfvit_vit_workspace_bytes_drop(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop) {
    Dims d;
    if (!get_dims(cfg, drop, d)) return 0;
    return ws_layout(d).total;
}
size_t mfvit_vit_workspace_bytes_ex(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int want_dimg) {
    Dims d;
    if (!get_dims(cfg, drop, d)) return 0;
    if (!want_dimg) return ws_layout(d).total;
    if (d.tok || !d.save) return 0;                  // the image gradient exists in image mode, behind a forward that saved its activations
    return ws_layout(d).total_dimg;
}
int mfvit_vit_hidden_layout(const mfvit_vit_cfg* cfg, int64_t out[2]) {
    Dims d;
    if (!get_dims(cfg, d) || !out || !d.save) return MFVIT_EINVAL;
    const WsLayout W = ws_layout(d);
    out[0] = (int64_t)W.x0; out[1] = (int64_t)W.x_stride;
    return MFVIT_OK;
}
int mfvit_vit_attn_layout(const mfvit_vit_cfg* cfg, int64_t out[4]) {
    Dims d;
    if (!get_dims(cfg, d) || !out || !d.save || d.tok) return MFVIT_EINVAL;
    const WsLayout W = ws_layout(d);
    out[0] = (int64_t)(W.blk0 + W.qkv); out[1] = (int64_t)(W.blk0 + W.lse); out[2] = (int64_t)W.blk_stride;
    out[3] = attn_qkv_dtype(d.dtype, d.T, d.HD);     // (image mode: no attention dropout in the cfg's own forward)
    return MFVIT_OK;
}

int mfvit_vit_prepare_shadow(const mfvit_vit_cfg* cfg, const float* params, void* shadow, mfvit_stream_t stream) {
    Dims d;
    if (!get_dims(cfg, d) || !params || !shadow) return MFVIT_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const ParamLayout L = param_layout(d);
    const ShadowLayout S = shadow_layout(d);
    char* sh = (char*)shadow;
    const bool hw = d.dtype != MFVIT_F32;
    if (hw && !d.tok) MFVIT_TRY(cast_transpose(d.dtype, params + L.pe_w, sh + S.pe_w, nullptr, d.D, 768, st));
    // one launch per weight type covers all `depth` blocks (identical shapes at fixed arena / shadow strides)
    const float* pb = params + L.blk0;
    char* sb = sh + S.blk0;
    const long ss = L.blk_stride, sd = (long)S.blk_stride;
    MFVIT_TRY(cast_transpose_batched(d.dtype, pb + L.qkv_w, hw ? sb + S.qkv_w : nullptr, sb + S.qkv_t, 3 * d.D, d.D, d.depth, ss, sd, sd, st));
    MFVIT_TRY(cast_transpose_batched(d.dtype, pb + L.proj_w, hw ? sb + S.proj_w : nullptr, sb + S.proj_t, d.D, d.D, d.depth, ss, sd, sd, st));
    MFVIT_TRY(cast_transpose_batched(d.dtype, pb + L.fc1_w, hw ? sb + S.fc1_w : nullptr, sb + S.fc1_t, d.F, d.D, d.depth, ss, sd, sd, st));
    MFVIT_TRY(cast_transpose_batched(d.dtype, pb + L.fc2_w, hw ? sb + S.fc2_w : nullptr, sb + S.fc2_t, d.D, d.F, d.depth, ss, sd, sd, st));
    return MFVIT_OK;
}

}  // extern "C"

// Low-rank adapters (include/mfvit.h, mfvit_lora_req): the checked request of one call.  mask[l]: bit t = block l has an item for target t.
struct LoraPlan {
    const mfvit_lora_req* req;
    unsigned char mask[256];
    int lowest;            // lowest block with an item
    float* dw;             // mfvit_vit_backward_lora: the dW_eff scratch in the gradient-arena layout
};
enum { LORA_QKV = 7, LORA_PROJ = 8, LORA_FC1 = 16, LORA_FC2 = 32 };
static bool lora_plan(const Dims& d, const mfvit_lora_req* r, bool grads, LoraPlan& pl) {
    if (!r || d.tok || d.depth > 256 || r->rank < 1 || r->rank > 64 || r->n < 1 || r->n > 6 * d.depth || !r->items) return false;
    memset(pl.mask, 0, sizeof(pl.mask));
    pl.req = r;
    pl.lowest = d.depth;
    pl.dw = nullptr;
    for (int i = 0; i < r->n; ++i) {
        const mfvit_lora_item& it = r->items[i];
        if (it.block < 0 || it.block >= d.depth || it.target < 0 || it.target > MFVIT_LORA_FC2) return false;
        if (!it.a || !it.b || (grads && (!it.da || !it.db))) return false;
        if (pl.mask[it.block] & (1 << it.target)) return false;
        pl.mask[it.block] |= (unsigned char)(1 << it.target);
        pl.lowest = it.block < pl.lowest ? it.block : pl.lowest;
    }
    return true;
}
// The (weight, adapter) pair of item `it` over an arena-layout buffer `base` (the parameters, or a gradient arena); out: the merge's target arena
static LoraPair lora_pair(const Dims& d, const ParamLayout& L, const mfvit_lora_item& it, const float* base, float* out, bool grad) {
    const long D = d.D;
    long off = L.blk0 + (long)it.block * L.blk_stride;
    int N = d.D, K = d.D;
    if (it.target <= MFVIT_LORA_V) off += L.qkv_w + (long)it.target * D * D;
    else if (it.target == MFVIT_LORA_PROJ) off += L.proj_w;
    else if (it.target == MFVIT_LORA_FC1) { off += L.fc1_w; N = d.F; }
    else { off += L.fc2_w; K = d.F; }
    LoraPair p = {base + off, it.a, it.b, grad ? it.da : out + off, grad ? it.db : nullptr, N, K, K, K};
    return p;
}
// merge (grad = false: base = params, out = the effective arena) or gradient contraction (grad = true: base = a gradient arena) of every item:
// all pairs are checked before the first launch
static int lora_run(const Dims& d, const mfvit_lora_req* r, const float* base, float* out, bool grad, hipStream_t st) {
    const ParamLayout L = param_layout(d);
    for (int i = 0; i < r->n; ++i)
        if (!lora_pair_ok(lora_pair(d, L, r->items[i], base, out, grad), r->rank, grad)) return MFVIT_EINVAL;
    LoraPair chunk[LORA_MAXP];
    for (int i0 = 0; i0 < r->n; i0 += LORA_MAXP) {
        const int m = r->n - i0 < LORA_MAXP ? r->n - i0 : LORA_MAXP;
        for (int i = 0; i < m; ++i) chunk[i] = lora_pair(d, L, r->items[i0 + i], base, out, grad);
        MFVIT_TRY(grad ? lora_grad_batch(chunk, m, r->rank, r->scale, st) : lora_merge_batch(chunk, m, r->rank, r->scale, st));
    }
    return MFVIT_OK;
}

// Attention maps (mfvit_vit_forward_attn): validity of a request, and the optional per-block step behind block l's attention forward - its
// probabilities into req->maps (the block's slot among the selected ones) and, for a rollout, its fused map and row sums into the scratch.
static bool attn_req_ok(const mfvit_vit_cfg* cfg, const mfvit_vit_attn_req* r, Dims& d) {
    if (!r || !get_dims(cfg, d) || d.tok) return false;
    if (d.depth < 64 && (r->blocks >> d.depth) != 0) return false;
    if (r->fuse < 0 || r->fuse > 3 || (r->cls_only != 0 && r->cls_only != 1)) return false;
    if (r->rollout && (r->fuse == 0 || 2 * (size_t)d.T * 4 > 64 * 1024)) return false;   // (the rollout kernel keeps two [T] vectors in LDS)
    if ((r->blocks != 0) != (r->maps != nullptr)) return false;
    return r->blocks != 0 || r->rollout != nullptr;
}
// scratch of a rollout: the depth fused maps [B][T][T], then their row sums [B][T]
static float* attn_scratch_sums(const Dims& d, const mfvit_vit_attn_req* r) { return (float*)r->scratch + (size_t)d.depth * d.B * d.T * d.T; }
static int attn_block_step(const Dims& d, const mfvit_vit_attn_req* r, int l, int qdt, const void* qkv, const float* lse, hipStream_t st) {
    if ((r->blocks >> l) & 1) {
        const size_t slot = __builtin_popcountll(r->blocks & ((1ull << l) - 1));
        const size_t per = (size_t)d.B * (r->fuse ? 1 : d.H) * (r->cls_only ? 1 : d.T) * d.T;
        MFVIT_TRY(attn_probs(qdt, qkv, lse, d.B, d.T, d.H, d.HD, r->fuse, r->cls_only, r->maps + slot * per, nullptr, st));
    }
    if (r->rollout)
        MFVIT_TRY(attn_probs(qdt, qkv, lse, d.B, d.T, d.H, d.HD, r->fuse, 0, (float*)r->scratch + (size_t)l * d.B * d.T * d.T,
                             attn_scratch_sums(d, r) + (size_t)l * d.B * d.T, st));
    return MFVIT_OK;
}

// Relevance (mfvit_vit_backward_rel): validity of a request; its scratch is v [B][T] then the per-tile parts [B][ceil(T/32)][T] (relevance only);
// and the step behind block l's attention backward - A_l into req->maps (the block's slot among the selected ones) and, for the relevance, the
// row product and update of v.
static bool rel_req_ok(const mfvit_vit_cfg* cfg, const mfvit_vit_rel_req* r, Dims& d) {
    if (!r || !get_dims(cfg, d) || d.tok || !d.save || d.T > 8192) return false;
    if (d.depth < 64 && (r->blocks >> d.depth) != 0) return false;
    if ((r->blocks != 0) != (r->maps != nullptr)) return false;
    return r->blocks != 0 || r->relevance != nullptr;
}
static int rel_block_step(const Dims& d, const mfvit_vit_rel_req* r, int l, int qdt, const void* qkv, const float* lse, const void* dout,
                          hipStream_t st) {
    const bool sel = (r->blocks >> l) & 1;
    if (!sel && !r->relevance) return MFVIT_OK;
    float* map = nullptr;
    if (sel) map = r->maps + (size_t)__builtin_popcountll(r->blocks & ((1ull << l) - 1)) * d.B * d.T * d.T;
    // (a maps-only request has 256 bytes of scratch: neither v nor the parts exist then)
    float* v = r->relevance ? (float*)r->scratch : nullptr;
    float* part = r->relevance ? v + (size_t)d.B * d.T : nullptr;
    const int first = l == d.depth - 1;
    MFVIT_TRY(attn_rel_map(qdt, d.dtype, qkv, lse, dout, d.B, d.T, d.H, d.HD, map, v, part, first, st));
    if (r->relevance) MFVIT_TRY(attn_rel_update(v, part, d.B, d.T, first, l == 0 ? r->relevance : nullptr, st));
    return MFVIT_OK;
}

// ------------------------------------------------------------------ forward: the embedding, then block 0 .. depth-1
// x_0 and LN1_0 -> y1_0 from the input, in one of the three embedding forms
static int fwd_embed(const EncCtx& c, const float* img) {
    const Dims& d = c.d;
    const long D = c.D, De = c.D * c.e;
    const float* const pos = c.params + c.L.pos;
    // (the first block of the call: block 0, but for a block range entered with x_{l0} - always through the given-x0 row pass below)
    float* const x0 = c.xbuf(d.l0);
    char* const y1_0 = c.blk(d.l0) + c.W.y1;
    const float *const g0 = c.pblk(d.l0) + c.L.ln1_w, *const b0 = c.pblk(d.l0) + c.L.ln1_b;
    float *const mean0 = c.stat(d.l0), *const rstd0 = c.stat(d.l0) + d.M;
    if (d.x0in && d.p_embd > 0.f && d.l0 == 0)
        // given x_0 (img = (B, T, D) f32: cat(cls, kept patches) + their pos_embed rows): timm pos_drop on the shortened rows; LN1_0 -> y1_0
        return drop_add_ln_rows(d.dtype, d.D, nullptr, 0, img, D, nullptr, 0, 0, nullptr, 0, make_drop(d.p_embd, d.seed, 1), c.off, 1, x0, D, y1_0, De, 0,
                                g0, b0, c.eps, mean0, rstd0, d.M, c.st);
    if (d.x0in)
        return ln_rows(d.dtype, d.D, img, D, nullptr, 0, 0, x0, D, y1_0, De, 0, g0, b0, c.eps, mean0, rstd0, d.M, 1, 0, 0, c.st);
    if (d.tok && d.p_embd > 0.f)
        // x_0 = drop(tokens + pos_emb) (fuseattention.py:187 `self.drop(self.pos_emb + token_embeddings)`); LN1_0 -> y1_0
        return drop_add_ln_rows(d.dtype, d.D, nullptr, 0, img, D, d.use_pos ? pos : nullptr, D, d.T, nullptr, 0, make_drop(d.p_embd, d.seed, 1), c.off, 1,
                                x0, D, y1_0, De, 0, g0, b0, c.eps, mean0, rstd0, d.M, c.st);
    if (d.tok)
        // token input (fuseattention.py:186-189): x_0 = tokens (+ pos_emb, shared by the batch); LN1_0 -> y1_0.  One row kernel pass.
        return ln_rows(d.dtype, d.D, img, D, d.use_pos ? pos : nullptr, D, d.T, x0, D, y1_0, De, 0, g0, b0, c.eps, mean0, rstd0, d.M, 1, 0, 0, c.st);
    // patch embedding: im2col -> GEMM + bias + pos_embed, the patch rows of image b behind its cls row -> x_0, LN1_0 -> y1_0
    MFVIT_TRY(im2col16(d.dtype, img, c.ws + c.W.patches, d.B, c.cfg->img_h, c.cfg->img_w, c.st));
    GemmP p = nt(c.ws + c.W.patches, 768 * c.e, c.weight(c.sh + c.S.pe_w, c.params + c.L.pe_w), 768 * c.e, d.Mp, d.D, 768);
    p.bias = c.params + c.L.pe_b;
    p.res = pos; p.ldres = D; p.res_mod = d.np; p.res_off = 1;
    p.orow_in = d.np; p.orow_out = d.T; p.orow_off = 1;
    p.out0 = x0; p.ldo0 = D;
    p.out1 = y1_0; p.ldo1 = De;
    p.gamma = g0; p.beta = b0; p.eps = c.eps;
    p.mean = mean0; p.rstd = rstd0;
    MFVIT_TRY(linear_res_ln(c, p, nullptr, PROF_TAG_NONE));
    // cls rows: x_0[b,0] = cls_token + pos_embed[0]; LN1_0
    MFVIT_TRY(ln_rows(d.dtype, d.D, c.params + c.L.cls, 0, pos, D, 1, x0, D, y1_0, De, 0, g0, b0, c.eps, mean0, rstd0, d.B, d.T, 0, 1, c.st));
    if (d.p_embd > 0.f)
        // timm pos_drop: x_0 = drop(cat(cls, patch_embed(x)) + pos_embed), cls rows included; in place, then LN1_0 again
        MFVIT_TRY(drop_add_ln_rows(d.dtype, d.D, nullptr, 0, x0, D, nullptr, 0, 0, nullptr, 0, make_drop(d.p_embd, d.seed, 1), c.off, 1, x0, D, y1_0, De, 0,
                                   g0, b0, c.eps, mean0, rstd0, d.M, c.st));
    return MFVIT_OK;
}

// block l: x_l, y1_l -> x_{l+1} and the next LayerNorm's output (the last block: the final norm -> features)
static int fwd_block(const EncCtx& c, int l, float* features, const mfvit_vit_attn_req* attn) {
    const Dims& d = c.d;
    const long D = c.D, F = c.F, De = c.D * c.e, Fe = c.F * c.e;
    char* const b = c.blk(l);
    const float* const pb = c.pblk(l);
    const char* const sb = c.sblk(l);
    // qkv tensor format: split FP16 for the whole-head attention kernels in bf16x3 mode (attention_mfma.hip), the activation dtype otherwise
    const int qdt = d.p_attn > 0.f ? d.dtype : attn_qkv_dtype(d.dtype, d.T, d.HD);
    {   // qkv = y1 Wqkv^T + b
        GemmP p = nt(b + c.W.y1, De, c.weight(sb + c.S.qkv_w, pb + c.L.qkv_w), De, d.M, 3 * d.D, d.D);
        p.bias = pb + c.L.qkv_b;
        p.out0 = b + c.W.qkv; p.ldo0 = 3 * De;
        ProfTag tag(PROF_TAG_MHSA_QKV);
        MFVIT_TRY(gemm_nt_tile(d.dtype, qdt == MFVIT_X3F16 ? EPI_BIAS_X3F16 : EPI_BIAS, p, c.st));
    }
    if (d.p_attn > 0.f) {
        if (!attn_tiled_supported(d.dtype, d.T, d.HD)) return MFVIT_ENOSYS;
        MFVIT_TRY(attn_fwd_tiled_drop(d.dtype, b + c.W.qkv, b + c.W.attn, (float*)(b + c.W.lse), d.B, d.T, d.H, d.HD,
                                      make_drop(d.p_attn, d.seed, c.site(l, 2)), c.st));
    } else {
        MFVIT_TRY(attn_fwd(qdt, b + c.W.qkv, b + c.W.attn, (float*)(b + c.W.lse), d.B, d.T, d.H, d.HD, c.st));
    }
    if (attn) MFVIT_TRY(attn_block_step(d, attn, l, qdt, b + c.W.qkv, (const float*)(b + c.W.lse), c.st));
    {   // xmid = x + attn Wproj^T + b ; y2 = LN2(xmid)
        // (masked: xmid = x + resid_drop(proj(attn)), fuseattention.py:57; timm: x + drop_path(proj_drop(proj(attn))))
        GemmP p = nt(b + c.W.attn, De, c.weight(sb + c.S.proj_w, pb + c.L.proj_w), De, d.M, d.D, d.D);
        p.bias = pb + c.L.proj_b;
        p.res = c.xbuf(l); p.ldres = D;
        p.out0 = b + c.W.xmid; p.ldo0 = D;
        p.out1 = b + c.W.y2; p.ldo1 = De;
        p.gamma = pb + c.L.ln2_w; p.beta = pb + c.L.ln2_b; p.eps = c.eps;
        p.mean = (float*)(b + c.W.st2); p.rstd = (float*)(b + c.W.st2) + d.M;
        p.kpart = c.kpart();
        const BranchDrop mask = {make_drop(d.p_resid, d.seed, c.site(l, 3)), c.dpath(l, 6)};
        MFVIT_TRY(linear_res_ln(c, p, &mask, PROF_TAG_MHSA_PROJ));
    }
    {   // hpre = y2 W1^T + b1 ; hact = gelu(hpre)   (training: hact = drop(gelu(hpre)), out0 = gelu'(hpre) * mask - timm Mlp.drop)
        GemmP p = nt(b + c.W.y2, De, c.weight(sb + c.S.fc1_w, pb + c.L.fc1_w), De, d.M, d.F, d.D);
        p.bias = pb + c.L.fc1_b;
        p.out0 = d.save ? b + c.W.hpre : nullptr; p.ldo0 = F;      // act'(pre) in act_grad_type<T> (gemm.hip): F elements per row
        p.out1 = b + c.W.hact; p.ldo1 = Fe;
        p.drop = make_drop(d.p_gelu, d.seed, c.site(l, 5));
        MFVIT_TRY(gemm_nt_tile(d.dtype, d.act == 1 ? EPI_BIAS_RELU : (d.p_gelu > 0.f ? EPI_BIAS_GELU_DROP : EPI_BIAS_GELU), p, c.st));
    }
    // x_{l+1} = xmid + hact W2^T + b2 ; y = LN(next norm1 | final norm)
    // (masked: x_{l+1} = xmid + Dropout(fc2(relu(fc1(y2)))), fuseattention.py:67-72,80; timm: xmid + drop_path(drop(fc2(..))))
    GemmP p = nt(b + c.W.hact, Fe, c.weight(sb + c.S.fc2_w, pb + c.L.fc2_w), Fe, d.M, d.D, d.F);
    p.bias = pb + c.L.fc2_b;
    p.res = (const float*)(b + c.W.xmid); p.ldres = D;
    p.out0 = c.xbuf(l + 1); p.ldo0 = D;
    if (l + 1 == d.depth) {
        p.out1 = features; p.ldo1 = D; p.y_f32 = 1;
        p.gamma = c.params + c.L.norm_w; p.beta = c.params + c.L.norm_b;
    } else if (l + 1 == d.l1) {
        // a block range that ends here: the raw residual stream x_{l1} is the call's output; the epilogue's LayerNorm (block l1's norm1) goes to scratch
        p.out0 = features;
        p.out1 = c.ws + c.W.ytail; p.ldo1 = De;
        p.gamma = c.pblk(l + 1) + c.L.ln1_w; p.beta = c.pblk(l + 1) + c.L.ln1_b;
    } else {
        p.out1 = c.blk(l + 1) + c.W.y1; p.ldo1 = De;
        p.gamma = c.pblk(l + 1) + c.L.ln1_w; p.beta = c.pblk(l + 1) + c.L.ln1_b;
    }
    p.eps = c.eps;
    p.mean = c.stat(l + 1); p.rstd = c.stat(l + 1) + d.M;
    p.kpart = c.kpart();
    const BranchDrop mask = {make_drop(d.p_resid, d.seed, c.site(l, 4)), c.dpath(l, 7)};
    return linear_res_ln(c, p, &mask, PROF_TAG_NONE);
}

// Shared forward of the two front ends: ViT-S/16 (img = (B,3,H,W) image, patch embedding + cls token) and the token-input GPT
// (img = (B,T,dim) tokens, + pos_emb).  Everything behind x_0 / LN1_0 is the same pre-LN block stack.
static int encoder_forward(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* dropcfg, const float* params, const void* shadow, const float* img,
                           void* workspace, float* features, mfvit_stream_t stream, bool want_tokens,
                           const mfvit_vit_attn_req* attn = nullptr, const mfvit_vit_seg* seg = nullptr) {
    Dims d;
    if (!(seg ? get_dims_seg(cfg, dropcfg, seg, d) : get_dims(cfg, dropcfg, d)) || !params || !shadow || !img || !workspace || !features)
        return MFVIT_EINVAL;
    if (d.tok != want_tokens) return MFVIT_EINVAL;
    const EncCtx c(cfg, d, params, shadow, workspace, stream);
    MFVIT_TRY(fwd_embed(c, img));
    for (int l = d.l0; l < d.l1; ++l) MFVIT_TRY(fwd_block(c, l, features, attn));
    return MFVIT_OK;
}

// ------------------------------------------------------------------ backward: the final norm, block depth-1 .. 0, the embedding
// What a backward call was asked for.  dinput (token-input mode only): d loss / d tokens, written by the embedding stage.  dimg (image mode only,
// stage_lo == -1; the workspace then has mfvit_vit_workspace_bytes_ex(.., 1) bytes): d loss / d image, overwritten.  dparams == NULL (with dimg):
// the data-gradient chain alone - no weight-gradient GEMM, no split-partial reduce, no bias / LayerNorm column sum, no side stream.  rel (dparams
// == dimg == NULL, stages depth .. 0): that chain with the relevance step of mfvit_vit_backward_rel behind every block's attention backward; it
// ends at block 0's step (no attention backward or LN1 backward of block 0).  lora (dparams == NULL; mfvit_vit_backward_lora): that chain plus
// the weight-gradient GEMMs of the adapted Linears into lora->dw, the split-partial reduce of each block and, at the end, the batched contraction
// to dA / dB; without dimg the chain ends behind the weight gradients of the lowest adapted block.
namespace {
struct BwdArgs {
    const float* dfeatures; float *dparams, *dinput, *dimg;
    int stage_hi, stage_lo;
    const mfvit_vit_rel_req* rel; const LoraPlan* lora;
};

// The weight gradients of one block that are not launched where they are built: at_fork - queued behind the block's fork (side stream); pend -
// dWproj, held back to ride along with dWqkv (one launch for both)
struct BlockWgrads {
    GemmP at_fork[2];
    int n_fork = 0;
    GemmP pend = {};
    bool have_pend = false;
};

// The attention backward's split-fp16 core scales dO (= the proj data gradient) per (image, head) by a power of two from the pair's largest |dO|.  The
// GEMM that produces dO leaves those maxima behind (GemmP::omax: atomicMax of f32 bits, one slice per block, zeroed for the blocks of a call), and
// the attention kernel reads ONE number per pair instead of prefetching the hi parts of all of dO's rows a pair ahead.  MFVIT_DO_MAX=0: the prefetch.
static bool dout_max_applies(const Dims& d, int qdt_bwd) {
    static int s_domax = INT_MIN;
    return env_switch("MFVIT_DO_MAX", 1, s_domax) != 0 && qdt_bwd == MFVIT_X3F16 && (d.HD == 32 || d.HD == 64) && d.T >= 64 && d.D % 128 == 0 &&
           !(d.p_attn > 0.f);
}

// per-call context of encoder_backward: EncCtx, the request, and the scratch slots and queue the stages share
struct BwdCtx : EncCtx, BwdArgs {
    const bool wg;                  // parameter gradients wanted (false: data-gradient-only backward)
    float* const gbase;             // where weight gradients go: the gradient arena, or the adapters' dW_eff scratch
    float *const gx, *const gmid, *const colscr;
    // column-sum partials: every row-kernel launch of this call writes its own buffer, ONE batched launch reduces them (before the embedding
    // stage, which reads a sum, and at the end of the call); with residual dropout (intermediate sums are consumed at once) nothing is deferred
    int colpart_used = 0;
    ColpartScope colpart_scope;
    // split partials of the weight-gradient GEMMs through scratch - plain stores, every launch into its OWN slot - and ONE batched reduce launch at
    // the end of every BLOCK that adds the splits in a fixed order: dW is the same bits on every run (the float atomics it replaces add in whatever
    // order the workgroups finish).  Round 3 measured the same idea with a reduce launch behind EVERY gradient as a loss (77.2 -> 80.8 us per
    // launch); batched it costs 0.4 - 0.6 % of the step (round 5, profiles/r05_wgrad_partials_ab.txt: weight-gradient class 95.6 -> 90.8 us per launch,
    // the reduce launches take most of it back; per block - partials still in the Infinity Cache - beats per call by 0.07 ms).  (With the weight-gradient
    // side stream the partial path stays ON: every weight gradient and every reduce of a call then runs in the side stream's order.)
    int tn_used = 0;
    TnPartScope tnpart_scope;
    const WgradQueue q;
    const int qdt_bwd;
    const bool do_max;              // dout_max_applies

    BwdCtx(const mfvit_vit_cfg* cfg, const Dims& dims, const float* params_, const void* shadow, void* workspace, mfvit_stream_t stream,
           const BwdArgs& a)
        : EncCtx(cfg, dims, params_, shadow, workspace, stream), BwdArgs(a), wg(a.dparams != nullptr),
          gbase(wg ? a.dparams : (a.lora ? a.lora->dw : nullptr)), gx((float*)(ws + W.gx)), gmid((float*)(ws + W.gmid)),
          colscr((float*)(ws + W.colscratch)), colpart_scope(!dims.rdrop), q(wgrad_side_stream(*this, wg), st, a.stage_hi < dims.l1 ? a.stage_hi : dims.l1 - 1),
          qdt_bwd(attn_qkv_dtype(dims.dtype, dims.T, dims.HD)), do_max(dout_max_applies(dims, qdt_bwd)) {}

    float* gblk(int l) const { return gbase ? gbase + L.blk0 + (long)l * L.blk_stride : nullptr; }
    float* next_colpart() { return (float*)(ws + W.colpart + (size_t)(colpart_used++ % (3 * d.depth + 2)) * W.colpart_stride); }
    float* next_tnpart() {          // (more launches than slots between two flushes: float atomics for the rest - never a slot still in use)
        return tn_used < TN_SLOTS ? (float*)(ws + W.tnpart + (size_t)(tn_used++) * W.tnpart_stride) : nullptr;
    }
    // dY buffers by layer parity (the embed stage counts as layer -1 -> parity 1)
    void* pp(size_t off, int l) const { return (void*)(ws + off + (size_t)(l & 1) * W.pp_stride); }
    unsigned* domax(int l) const { return (unsigned*)(ws + W.domax) + (size_t)l * d.B * d.H; }

    // Is the weight gradient of a Linear of block l formed (1 / 0; -1: error)?  With wg, all of them; without, the adapted ones (`bits` of
    // lora->mask[l]) - zeroed first: the GEMMs and the reduce accumulate
    int wgrad_wanted(int l, int bits, long off, long count) const {
        if (wg) return 1;
        if (!lora || !(lora->mask[l] & bits)) return 0;
        return hipMemsetAsync(gblk(l) + off, 0, (size_t)count * sizeof(float), st) == hipSuccess ? 1 : -1;
    }
    // One "weight gradient of a Linear" site of block l: dW [N][K] at `woff` of the block's gradients += dY^T X over the M token rows, the column
    // sums of dY into `bias` (or NULL); split partials: plain stores into a fresh slot, reduced in a fixed order at the end of the block
    GemmP wgrad_site(int l, const void* dY, long lddy, const void* X, long ldx, int N, int K, long woff, float* bias) {
        GemmP p = nt(dY, lddy, X, ldx, d.M, N, K);
        p.cs0 = bias;
        p.out0 = gblk(l) + woff; p.ldo0 = K;
        p.cpart = next_tnpart();
        return p;
    }
    // When a weight gradient of a block is launched - the one place that decides:
    //   held (pairable = dWproj) to ride along with dWqkv - by default when the weight gradients run on the caller's stream (nothing to overlap: one
    //     launch less is a pure gain, 30.81 -> 30.68 ms per step) and with the side stream alike; not with a masked branch;
    //   at the block's fork, with the side stream: the four weight gradients of a block are queued TOGETHER, behind the attention backward (their
    //     last input), with ONE main -> side dependency per block: an event record + wait costs the host ~9 us on this ROCm, and a fork in front of
    //     every gradient made the host the bottleneck of a small-batch step (B = 8: 5.1 -> 6.1 ms).  Their inputs are this layer parity's copies,
    //     untouched until then;
    //   now, otherwise.
    int route_wgrad(BlockWgrads& bw, const GemmP& g, bool pairable) const {
        if (pairable && !d.rdrop) { bw.pend = g; bw.have_pend = true; return MFVIT_OK; }
        if (q.side) { bw.at_fork[bw.n_fork++] = g; return MFVIT_OK; }
        return gemm_tn(d.dtype, g, q.s);
    }
};
}  // namespace

// final LayerNorm backward: dfeatures -> gx (grad of x_depth); dcol = d fc2_b of the last block
static int bwd_final_norm(BwdCtx& c) {
    const Dims& d = c.d;
    if (!c.dfeatures) return MFVIT_EINVAL;
    float* const dcol = !c.wg ? nullptr : d.rdrop ? c.colscr + c.D : c.gblk(d.depth - 1) + c.L.fc2_b;
    return ln_bwd_rows(d.dtype, d.D, c.dfeatures, c.D, c.xbuf(d.depth), c.D, c.stat(d.depth), c.stat(d.depth) + d.M, c.params + c.L.norm_w, nullptr, 0,
                       c.gx, c.D, c.pp(c.W.gxT, d.depth - 1), c.D * c.e, c.wg ? c.dparams + c.L.norm_w : nullptr,
                       c.wg ? c.dparams + c.L.norm_b : nullptr, dcol, c.wg ? c.next_colpart() : nullptr, d.M, 1, 0, c.st);
}

// The top stage of a block range that ends below the final norm (stage l1 < depth): dfeatures = d x_{l1} becomes gx and its operand-type copy;
// its column sums are d fc2_b of block l1 - 1 (what the LayerNorm backward above that block leaves in a whole-stack call)
static int bwd_seg_entry(BwdCtx& c) {
    const Dims& d = c.d;
    if (!c.dfeatures) return MFVIT_EINVAL;
    if (!c.lean_grad && hipMemcpyAsync(c.gx, c.dfeatures, (size_t)d.M * c.D * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess)
        return MFVIT_ELAUNCH;
    MFVIT_TRY(cast_transpose(d.dtype, c.dfeatures, c.pp(c.W.gxT, d.l1 - 1), nullptr, d.M, d.D, c.st));
    if (c.wg && !d.rdrop) MFVIT_TRY(colsum_rows(c.dfeatures, c.D, c.gblk(d.l1 - 1) + c.L.fc2_b, d.M, 1, 0, d.D, c.st));
    return MFVIT_OK;
}

// dY of a residual branch of block l: the residual gradient itself, or - where the branch was dropped - its masked copy in the scratch buffer
// (the residual gradient passes unscaled: `dy` stays the residual operand of the LayerNorm backward behind the branch)
static int mask_branch_grad(const BwdCtx& c, int l, int drop_site, int dpath_site, const void*& dy) {
    const Dims& d = c.d;
    if (!d.rdrop) return MFVIT_OK;
    const long De = c.D * c.e;
    MFVIT_TRY(mask_scale_rows(d.dtype, false, dy, De, c.ws + c.W.dtmp, De, make_drop(d.p_resid, d.seed, c.site(l, drop_site)), c.dpath(l, dpath_site),
                              d.T, d.M, d.D, c.st));
    dy = c.ws + c.W.dtmp;
    return MFVIT_OK;
}

// Behind block l's attention backward: dqkv - and with it every input of this block's weight gradients - is ready.  Fork, the gradients queued
// for it, dWqkv (with the held dWproj), the reduce of the block's split partials, and the block's `done` mark.
static int bwd_block_wgrads(BwdCtx& c, int l, const BlockWgrads& bw, bool want_qkv, const void* dqkv) {
    const Dims& d = c.d;
    const long De = c.D * c.e;
    MFVIT_TRY(c.q.fork());
    for (int i = 0; i < bw.n_fork; ++i) MFVIT_TRY(gemm_tn(d.dtype, bw.at_fork[i], c.q.s));
    if (want_qkv) {   // dWqkv += dqkv^T y1 ; d qkv_b += column sums of dqkv (ones-fragment MFMA inside the wgrad kernel)
        const GemmP p = c.wgrad_site(l, dqkv, 3 * De, c.blk(l) + c.W.y1, De, 3 * d.D, d.D, c.L.qkv_w, c.wg ? c.gblk(l) + c.L.qkv_b : nullptr);
        // dWproj rides along when the LDS-DMA kernel takes both (same rows, same K = 384: 27 + 9 tiles x 7 splits = 252 workgroups): the
        // float atomics of one launch (16.5 MB, 12.5 us) and one prologue less per block
        GemmP pend_nc = bw.pend;
        pend_nc.cpart = nullptr;                              // (in the paired launch both gradients' partials go to dWqkv's slot)
        if (bw.have_pend && gemm_tn_pair_supported(d.dtype, p, pend_nc)) {
            MFVIT_TRY(gemm_tn_glds_pair(d.dtype, p, pend_nc, c.q.s));
        } else {
            if (bw.have_pend) MFVIT_TRY(gemm_tn(d.dtype, bw.pend, c.q.s));
            MFVIT_TRY(gemm_tn(d.dtype, p, c.q.s));
        }
    } else if (bw.have_pend) {
        MFVIT_TRY(gemm_tn(d.dtype, bw.pend, c.q.s));          // (adapters on proj without any on q / k / v)
    }
    MFVIT_TRY(tnpart_batch_flush(c.q.s));                     // dW += this block's split partials, splits in a fixed order; the slots are free again
    c.tn_used = 0;
    return c.q.mark_done(l);
}

// block l: gx = d x_{l+1} (f32 and / or its operand-type copy of this layer parity) -> d x_l, and the block's parameter gradients
static int bwd_block(BwdCtx& c, int l) {
    const Dims& d = c.d;
    const long D = c.D, F = c.F, De = c.D * c.e, Fe = c.F * c.e;
    char* const b = c.blk(l);
    const float* const pb = c.pblk(l);
    const char* const sb = c.sblk(l);
    float* const gb = c.gblk(l);
    void* const gxT = c.pp(c.W.gxT, l);
    void* const gmidT = c.pp(c.W.gmidT, l);
    void* const dhpre = c.pp(c.W.dhpre, l);
    void* const dqkv = c.pp(c.W.dqkv, l);
    const bool masked_bias = d.rdrop && c.wg;               // the bias gradients of proj / fc2 then come from the MASKED dY (wgrad column sums)
    MFVIT_TRY(c.q.wait_layer(l + 2));                       // layer l+2's wgrads read this parity's dhpre / gmidT / dqkv
    BlockWgrads bw;
    const void* gy2 = gxT;                                  // dY of fc2
    MFVIT_TRY(mask_branch_grad(c, l, 4, 7, gy2));
    const int w_fc2 = c.wgrad_wanted(l, LORA_FC2, c.L.fc2_w, D * F), w_fc1 = c.wgrad_wanted(l, LORA_FC1, c.L.fc1_w, F * D),
              w_proj = c.wgrad_wanted(l, LORA_PROJ, c.L.proj_w, D * D), w_qkv = c.wgrad_wanted(l, LORA_QKV, c.L.qkv_w, 3 * D * D);
    if (w_fc2 < 0 || w_fc1 < 0 || w_proj < 0 || w_qkv < 0) return MFVIT_ELAUNCH;
    if (w_fc2)   // dW2 += gx^T hact
        MFVIT_TRY(c.route_wgrad(bw, c.wgrad_site(l, gy2, De, b + c.W.hact, Fe, d.D, d.F, c.L.fc2_w, masked_bias ? gb + c.L.fc2_b : nullptr), false));
    {   // dhpre = (gx W2) * gelu'(hpre)
        GemmP p = nt(gy2, De, sb + c.S.fc2_t, De, d.M, d.F, d.D);
        p.aux = b + c.W.hpre; p.ldaux = F;
        p.out0 = dhpre; p.ldo0 = Fe;
        if (c.wg) { p.cs0 = gb + c.L.fc1_b; p.cpart = c.next_colpart(); }   // d fc1_b += column sums of dhpre from the accumulators of this epilogue (partials, fixed-order reduce)
        MFVIT_TRY(gemm_nt_tile(d.dtype, EPI_GELU_BWD, p, c.st));
    }
    if (w_fc1)   // dW1 += dhpre^T y2   (d fc1_b: from the fc2 data gradient's epilogue, above)
        MFVIT_TRY(c.route_wgrad(bw, c.wgrad_site(l, dhpre, Fe, b + c.W.y2, De, d.F, d.D, c.L.fc1_w, nullptr), false));
    {   // gmid = LN2bwd(dhpre W1) + gx ; d ln2_w, d ln2_b, d proj_b
        GemmP p = nt(dhpre, Fe, sb + c.S.fc1_t, Fe, d.M, d.D, d.F);
        p.aux = b + c.W.xmid; p.ldaux = D;
        p.mean = (float*)(b + c.W.st2); p.rstd = (float*)(b + c.W.st2) + d.M;
        p.gamma = pb + c.L.ln2_w;
        p.kpart = c.kpart();
        if (c.wg) { p.cs0 = gb + c.L.ln2_w; p.cs1 = gb + c.L.ln2_b; p.cs2 = d.rdrop ? c.colscr + D : gb + c.L.proj_b; p.cpart = c.next_colpart(); }
        MFVIT_TRY(dgrad_ln_bwd(c, p, c.gx, gxT, c.lean_grad ? nullptr : c.gmid, gmidT));
    }
    const void* gyp = gmidT;                                // dY of proj
    MFVIT_TRY(mask_branch_grad(c, l, 3, 6, gyp));
    if (w_proj)   // dWproj += gmid^T attn
        MFVIT_TRY(c.route_wgrad(bw, c.wgrad_site(l, gyp, De, b + c.W.attn, De, d.D, d.D, c.L.proj_w, masked_bias ? gb + c.L.proj_b : nullptr), true));
    {   // dattn = gmid Wproj
        GemmP p = nt(gyp, De, sb + c.S.proj_t, De, d.M, d.D, d.D);
        p.out0 = c.ws + c.W.dattn; p.ldo0 = De;
        if (c.do_max) { p.omax = c.domax(l); p.omax_rows = d.T; p.omax_hd = d.HD; }
        MFVIT_TRY(gemm_nt_tile(d.dtype, EPI_NONE, p, c.st));
    }
    if (c.rel && l == 0)   // the relevance is complete after block 0's step: nothing reads block 0's dqkv or d x_0
        return rel_block_step(d, c.rel, l, c.qdt_bwd, b + c.W.qkv, (const float*)(b + c.W.lse), c.ws + c.W.dattn, c.st);
    if (d.p_attn > 0.f)
        MFVIT_TRY(attn_bwd_tiled_drop(d.dtype, b + c.W.qkv, b + c.W.attn, c.ws + c.W.dattn, (const float*)(b + c.W.lse), dqkv, d.B, d.T, d.H, d.HD,
                                      make_drop(d.p_attn, d.seed, c.site(l, 2)), c.st));
    else
        MFVIT_TRY(attn_bwd(c.qdt_bwd, b + c.W.qkv, b + c.W.attn, c.ws + c.W.dattn, (const float*)(b + c.W.lse), dqkv, nullptr, d.B, d.T, d.H, d.HD, c.st,
                           c.do_max ? c.domax(l) : nullptr));
    if (c.rel) MFVIT_TRY(rel_block_step(d, c.rel, l, c.qdt_bwd, b + c.W.qkv, (const float*)(b + c.W.lse), c.ws + c.W.dattn, c.st));
    MFVIT_TRY(bwd_block_wgrads(c, l, bw, w_qkv != 0, dqkv));
    MFVIT_TRY(c.q.wait_layer(l + 1));                       // fc2-wgrad of layer l+1 reads the gxT copy written next
    if (c.lora && !c.dimg && l == c.stage_lo) return MFVIT_OK;   // adapters only: nobody reads d x of the lowest adapted block
    // gx = LN1bwd(dqkv Wqkv) + gmid ; d ln1_w, d ln1_b, d fc2_b of block l-1 (or scratch for the embed stage)
    // (the first block of a block range: the row sums of d x_{l0} belong to no bias of this call - the range below adds its own from its dx_out)
    if (c.wg && l == d.l0 && hipMemsetAsync(c.colscr, 0, 2 * D * sizeof(float), c.st) != hipSuccess) return MFVIT_ELAUNCH;
    GemmP p = nt(dqkv, 3 * De, sb + c.S.qkv_t, 3 * De, d.M, d.D, 3 * d.D);
    p.aux = c.xbuf(l); p.ldaux = D;
    p.mean = c.stat(l); p.rstd = c.stat(l) + d.M;
    p.gamma = pb + c.L.ln1_w;
    p.kpart = c.kpart();
    if (c.wg) { p.cs0 = gb + c.L.ln1_w; p.cs1 = gb + c.L.ln1_b; p.cs2 = (l > d.l0 && !d.rdrop) ? c.gblk(l - 1) + c.L.fc2_b : c.colscr; p.cpart = c.next_colpart(); }
    // (lean_grad keeps the f32 result at block 0 only: the embedding stage reads gx)
    return dgrad_ln_bwd(c, p, c.gmid, gmidT, c.lean_grad && l > d.l0 ? nullptr : c.gx, c.pp(c.W.gxT, l - 1));
}

// token-input embedding stage: gx = d x_0 = d tokens; d pos_emb = sum over the batch (fuseattention.py:187)
static int bwd_embed_tokens(BwdCtx& c) {
    const Dims& d = c.d;
    MFVIT_TRY(colpart_batch_flush(c.st));
    if (d.p_embd > 0.f)      // d (tokens + pos_emb) = d x_0 * mask / (1 - p)
        MFVIT_TRY(mask_scale_rows(d.dtype, true, c.gx, c.D, c.gx, c.D, make_drop(d.p_embd, d.seed, 1), c.off, 1, d.M, d.D, c.st));
    if (c.dinput && hipMemcpyAsync(c.dinput, c.gx, (size_t)d.M * c.D * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess)
        return MFVIT_ELAUNCH;
    if (d.use_pos) MFVIT_TRY(batch_sum(c.gx, c.dparams + c.L.pos, d.B, (long)d.T * c.D, c.st));
    return MFVIT_OK;
}

// given-x0 embedding stage: gx = d x_0 (through pos_drop) -> dinput; no parameter gradient is formed here (the caller's front end owns cls_token and
// the patch embedding)
static int bwd_embed_x0(BwdCtx& c) {
    const Dims& d = c.d;
    MFVIT_TRY(colpart_batch_flush(c.st));
    if (d.p_embd > 0.f && d.l0 == 0)
        MFVIT_TRY(mask_scale_rows(d.dtype, true, c.gx, c.D, c.gx, c.D, make_drop(d.p_embd, d.seed, 1), c.off, 1, d.M, d.D, c.st));
    if (hipMemcpyAsync(c.dinput, c.gx, (size_t)d.M * c.D * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess) return MFVIT_ELAUNCH;
    return MFVIT_OK;
}

// image embedding stage: gx = d x_0 -> d img (the patch-embedding data gradient), d cls_token, d pe_b, d pe_w
static int bwd_embed_image(BwdCtx& c) {
    const Dims& d = c.d;
    const long D = c.D, De = c.D * c.e;
    MFVIT_TRY(colpart_batch_flush(c.st));                   // (colscr, read below, is one of the deferred sums)
    if (d.p_embd > 0.f) {
        // pos_drop: d (cat(cls, patch_embed) + pos_embed) = d x_0 * mask / (1 - p) - the f32 rows (cls, pe_b) and their operand-type copy
        // (pe_w) - and colscr[0:D] becomes the column sum of the masked rows
        // (the operand-type copy is cast afresh from the masked f32 rows: no second rounding of the split copy)
        MFVIT_TRY(mask_scale_rows(d.dtype, true, c.gx, D, c.gx, D, make_drop(d.p_embd, d.seed, 1), c.off, 1, d.M, d.D, c.st));
        MFVIT_TRY(cast_transpose(d.dtype, c.gx, c.pp(c.W.gxT, -1), nullptr, d.M, d.D, c.st));
        if (c.wg) {
            if (hipMemsetAsync(c.colscr, 0, D * sizeof(float), c.st) != hipSuccess) return MFVIT_ELAUNCH;
            MFVIT_TRY(colsum_rows(c.gx, D, c.colscr, d.M, 1, 0, d.D, c.st));
        }
    }
    if (c.dimg) {
        // d img = col2im(gx[patch rows] W_pe): W_pe^T of the operand type into the workspace (the shadow keeps W_pe [D][768] only; W_pe takes
        // part in the data gradient under stop_grad_conv1 too), then one tile GEMM whose epilogue stores the f32 image (EPI_COL2IM16, gemm.hip).
        // A = the operand-type copy of gx from token row 1 on: B T - 1 rows, the cls rows of images 1 .. B-1 among them (skipped by the epilogue).
        char* const wpeT = c.ws + c.W.wpeT;
        MFVIT_TRY(cast_transpose(d.dtype, c.params + c.L.pe_w, nullptr, wpeT, d.D, 768, c.st));
        GemmP p = nt((const char*)c.pp(c.W.gxT, -1) + (size_t)D * d.es, De, wpeT, De, d.M - 1, 768, d.D);
        p.orow_in = d.np; p.orow_out = d.T;
        p.out0 = c.dimg; p.ldo0 = c.cfg->img_w;
        MFVIT_TRY(gemm_nt_tile(d.dtype, EPI_COL2IM16, p, c.st));
    }
    if (!c.wg) return MFVIT_OK;
    // d cls_token = sum_b gx[b,0]; d pe_b = sum over patch rows; d pe_w = gx_patch^T patches.
    // pos_embed is a fixed table (requires_grad = False upstream): no gradient.
    MFVIT_TRY(colsum_rows(c.gx, D, c.dparams + c.L.cls, d.B, d.T, 0, d.D, c.st));
    if (c.cfg->stop_grad_conv1) return MFVIT_OK;
    // colscr[0:D] = sum of gx over ALL rows (cs2 of the LN1_0 backward); colscr[D:2D] = sum over the cls rows
    MFVIT_TRY(colsum_rows(c.gx, D, c.colscr + D, d.B, d.T, 0, d.D, c.st));
    MFVIT_TRY(axpy(c.dparams + c.L.pe_b, c.colscr, 1.0f, d.D, c.st));
    MFVIT_TRY(axpy(c.dparams + c.L.pe_b, c.colscr + D, -1.0f, d.D, c.st));
    GemmP p = nt(c.pp(c.W.gxT, -1), De, c.ws + c.W.patches, 768 * c.e, d.Mp, d.D, 768);   // d pe_w += gx[patch rows]^T patches
    p.orow_in = d.np; p.orow_out = d.T; p.orow_off = 1;
    p.out0 = c.dparams + c.L.pe_w; p.ldo0 = 768;
    p.cpart = c.next_tnpart();
    MFVIT_TRY(c.q.fork());                                  // (the residual gradient of block 0 is ready on the main stream)
    return gemm_tn(d.dtype, p, c.q.s);
}

// Shared backward of the two front ends (BwdArgs: what is asked for): stages stage_hi .. stage_lo in descending order - depth: the final norm,
// depth-1 .. 0: the blocks, -1: the embedding - then whatever the stages left pending.
static int encoder_backward(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* dropcfg, const float* params, const void* shadow, void* workspace,
                            const BwdArgs& a, mfvit_stream_t stream, bool want_tokens, const mfvit_vit_seg* seg = nullptr) {
    Dims d;
    if (!(seg ? get_dims_seg(cfg, dropcfg, seg, d) : get_dims(cfg, dropcfg, d)) || !params || !shadow || !workspace)
        return MFVIT_EINVAL;
    if (d.x0in ? (!a.dinput || a.dimg || a.rel || a.lora) : (!a.dparams && !a.dimg && !a.rel && !a.lora)) return MFVIT_EINVAL;
    if (!d.save || d.tok != want_tokens) return MFVIT_EINVAL;
    // stages of a block range [l0, l1): l1 (the final norm, or the range's entry from dx_out) down to l0 - 1 (what feeds block l0)
    if (a.stage_hi > d.l1 || a.stage_lo < d.l0 - 1 || a.stage_lo > a.stage_hi) return MFVIT_EINVAL;
    if (a.dimg && (d.tok || a.stage_lo != -1)) return MFVIT_EINVAL;
    BwdCtx c(cfg, d, params, shadow, workspace, stream, a);
    if (c.do_max) {   // the maxima of the blocks of this call start at zero
        const int l0 = a.stage_lo > d.l0 ? a.stage_lo : d.l0, l1 = a.stage_hi < d.l1 - 1 ? a.stage_hi : d.l1 - 1;
        if (l1 >= l0 && hipMemsetAsync(c.domax(l0), 0, (size_t)(l1 - l0 + 1) * d.B * d.H * 4, c.st) != hipSuccess) return MFVIT_ELAUNCH;
    }
    for (int s = a.stage_hi; s >= a.stage_lo; --s)
        MFVIT_TRY(s == d.depth ? bwd_final_norm(c) : s == d.l1 ? bwd_seg_entry(c) : s >= d.l0 ? bwd_block(c, s) : d.x0in ? bwd_embed_x0(c) :
                  d.tok ? bwd_embed_tokens(c) : bwd_embed_image(c));
    MFVIT_TRY(colpart_batch_flush(c.st));
    MFVIT_TRY(tnpart_batch_flush(c.q.s));   // dW += the split partials still pending (the patch embedding's), splits in a fixed order
    if (a.lora) MFVIT_TRY(lora_run(d, a.lora->req, a.lora->dw, nullptr, true, c.st));   // dA, dB of every item from the dW_eff slices
    return c.q.join();
}

extern "C" {

int mfvit_vit_forward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, const float* img, void* workspace,
                      float* features, mfvit_stream_t stream) {
    ShareScope share(cfg);
    return encoder_forward(cfg, nullptr, params, shadow, img, workspace, features, stream, false);
}
int mfvit_vit_forward_drop(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, const float* img,
                           void* workspace, float* features, mfvit_stream_t stream) {
    if (!drop) return MFVIT_EINVAL;
    ShareScope share(cfg);
    return encoder_forward(cfg, drop, params, shadow, img, workspace, features, stream, false);
}
size_t mfvit_vit_attn_scratch_bytes(const mfvit_vit_cfg* cfg, const mfvit_vit_attn_req* req) {
    Dims d;
    if (!attn_req_ok(cfg, req, d)) return 0;
    return req->rollout ? align256((size_t)d.depth * d.B * d.T * (d.T + 1) * 4) : 256;
}
int mfvit_vit_forward_attn(const mfvit_vit_cfg* cfg, const mfvit_vit_attn_req* req, const float* params, const void* shadow, const float* img,
                           void* workspace, float* features, mfvit_stream_t stream) {
    Dims d;
    if (!attn_req_ok(cfg, req, d) || !req->scratch) return MFVIT_EINVAL;
    ShareScope share(cfg);
    MFVIT_TRY(encoder_forward(cfg, nullptr, params, shadow, img, workspace, features, stream, false, req));
    if (req->rollout) MFVIT_TRY(attn_rollout((const float*)req->scratch, attn_scratch_sums(d, req), d.depth, d.B, d.T, req->rollout, (hipStream_t)stream));
    return MFVIT_OK;
}
size_t mfvit_vit_rel_scratch_bytes(const mfvit_vit_cfg* cfg, const mfvit_vit_rel_req* req) {
    Dims d;
    if (!rel_req_ok(cfg, req, d)) return 0;
    return req->relevance ? align256((size_t)d.B * d.T * ((d.T + 31) / 32 + 1) * 4) : 256;
}
int mfvit_vit_backward_rel(const mfvit_vit_cfg* cfg, const mfvit_vit_rel_req* req, const float* params, const void* shadow, void* workspace,
                           const float* dfeatures, mfvit_stream_t stream) {
    Dims d;
    if (!rel_req_ok(cfg, req, d) || !req->scratch || !dfeatures || !params || !shadow || !workspace) return MFVIT_EINVAL;
    ShareScope share(cfg);
    return encoder_backward(cfg, nullptr, params, shadow, workspace, {dfeatures, nullptr, nullptr, nullptr, d.depth, 0, req}, stream, false);
}
int mfvit_vit_backward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, void* workspace, const float* dfeatures,
                       float* dparams, int stage_hi, int stage_lo, mfvit_stream_t stream) {
    if (!dparams) return MFVIT_EINVAL;
    ShareScope share(cfg);
    return encoder_backward(cfg, nullptr, params, shadow, workspace, {dfeatures, dparams, nullptr, nullptr, stage_hi, stage_lo}, stream, false);
}
int mfvit_vit_backward_ex(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, void* workspace,
                          const float* dfeatures, float* dparams, float* dimg, int stage_hi, int stage_lo, mfvit_stream_t stream) {
    ShareScope share(cfg);
    return encoder_backward(cfg, drop, params, shadow, workspace, {dfeatures, dparams, nullptr, dimg, stage_hi, stage_lo}, stream, false);
}
size_t mfvit_vit_workspace_bytes_x0(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int tokens) {
    const mfvit_vit_seg seg = x0_seg(cfg, tokens);
    return mfvit_vit_workspace_bytes_seg(cfg, drop, &seg, 0);
}
int mfvit_vit_forward_x0(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int tokens, const float* params, const void* shadow, const float* x0,
                         void* workspace, float* features, mfvit_stream_t stream) {
    const mfvit_vit_seg seg = x0_seg(cfg, tokens);
    ShareScope share(cfg);
    return encoder_forward(cfg, drop, params, shadow, x0, workspace, features, stream, false, nullptr, &seg);
}
int mfvit_vit_backward_x0(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int tokens, const float* params, const void* shadow, void* workspace,
                          const float* dfeatures, float* dparams, float* dx0, int stage_hi, int stage_lo, mfvit_stream_t stream) {
    if (!cfg || tokens < 2 || !dx0 || (!dfeatures && stage_hi >= cfg->depth)) return MFVIT_EINVAL;
    const mfvit_vit_seg seg = x0_seg(cfg, tokens);
    ShareScope share(cfg);
    return encoder_backward(cfg, drop, params, shadow, workspace, {dfeatures, dparams, dx0, nullptr, stage_hi, stage_lo}, stream, false, &seg);
}
size_t mfvit_vit_workspace_bytes_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, int want_dimg) {
    Dims d;
    if (!get_dims_seg(cfg, drop, seg, d)) return 0;
    if (!want_dimg) return ws_layout(d).total;
    if (d.x0in || !d.save) return 0;                 // the image gradient belongs to the range that takes the image, behind a forward that saved
    return ws_layout(d).total_dimg;
}
int mfvit_vit_attn_layout_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, int64_t out[4]) {
    Dims d;
    if (!get_dims_seg(cfg, drop, seg, d) || !out) return MFVIT_EINVAL;
    const WsLayout W = ws_layout(d);
    out[0] = (int64_t)(W.blk0 + W.qkv); out[1] = (int64_t)(W.blk0 + W.lse); out[2] = d.save ? (int64_t)W.blk_stride : 0;
    out[3] = d.p_attn > 0.f ? d.dtype : attn_qkv_dtype(d.dtype, d.T, d.HD);
    return MFVIT_OK;
}
int mfvit_vit_forward_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, const float* params, const void* shadow,
                          const float* x_in, void* workspace, float* x_out, mfvit_stream_t stream) {
    if (!seg) return MFVIT_EINVAL;
    ShareScope share(cfg);
    return encoder_forward(cfg, drop, params, shadow, x_in, workspace, x_out, stream, false, nullptr, seg);
}
int mfvit_vit_backward_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, const float* params, const void* shadow,
                           void* workspace, const float* dx_out, float* dparams, float* dx_in, float* dimg, int stage_hi, int stage_lo,
                           mfvit_stream_t stream) {
    if (!cfg || !seg || (!dx_out && stage_hi >= seg->block_hi)) return MFVIT_EINVAL;
    ShareScope share(cfg);
    return encoder_backward(cfg, drop, params, shadow, workspace, {dx_out, dparams, dx_in, dimg, stage_hi, stage_lo}, stream, false, seg);
}
int mfvit_vit_backward_drop(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, void* workspace,
                            const float* dfeatures, float* dparams, int stage_hi, int stage_lo, mfvit_stream_t stream) {
    if (!drop || !dparams) return MFVIT_EINVAL;
    ShareScope share(cfg);
    return encoder_backward(cfg, drop, params, shadow, workspace, {dfeatures, dparams, nullptr, nullptr, stage_hi, stage_lo}, stream, false);
}
int mfvit_vit_prepare_shadow_lora(const mfvit_vit_cfg* cfg, const float* params, const mfvit_lora_req* req, float* eff_params, void* shadow,
                                  mfvit_stream_t stream) {
    Dims d;
    LoraPlan pl;
    if (!get_dims(cfg, d) || !params || !shadow || !eff_params || !lora_plan(d, req, false, pl)) return MFVIT_EINVAL;
    const ParamLayout L = param_layout(d);
    const size_t total = (size_t)L.total;
    if ((eff_params <= params && params < eff_params + total) || (params <= eff_params && eff_params < params + total)) return MFVIT_EINVAL;
    for (int i = 0; i < req->n; ++i)
        if (!lora_pair_ok(lora_pair(d, L, req->items[i], params, eff_params, false), req->rank, false)) return MFVIT_EINVAL;
    if (hipMemcpyAsync(eff_params, params, total * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return MFVIT_ELAUNCH;
    MFVIT_TRY(lora_run(d, req, params, eff_params, false, (hipStream_t)stream));
    return mfvit_vit_prepare_shadow(cfg, eff_params, shadow, stream);
}
int mfvit_vit_backward_lora(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, void* workspace,
                            const float* dfeatures, const mfvit_lora_req* req, float* dw_scratch, float* dimg, int stage_hi, int stage_lo,
                            mfvit_stream_t stream) {
    Dims d;
    LoraPlan pl;
    if (!get_dims(cfg, drop, d) || !dw_scratch || !dfeatures || !lora_plan(d, req, true, pl)) return MFVIT_EINVAL;
    if (stage_hi != d.depth || stage_lo > pl.lowest || stage_lo < -1 || (dimg && stage_lo != -1)) return MFVIT_EINVAL;
    pl.dw = dw_scratch;
    {   // every contraction checked before the first launch of the chain
        const ParamLayout L = param_layout(d);
        for (int i = 0; i < req->n; ++i)
            if (!lora_pair_ok(lora_pair(d, L, req->items[i], dw_scratch, nullptr, true), req->rank, true)) return MFVIT_EINVAL;
    }
    ShareScope share(cfg);
    return encoder_backward(cfg, drop, params, shadow, workspace, {dfeatures, nullptr, nullptr, dimg, stage_hi, dimg ? -1 : pl.lowest, nullptr, &pl},
                            stream, false);
}
int mfvit_vit_lora_grad(const mfvit_vit_cfg* cfg, const mfvit_lora_req* req, const float* dparams, mfvit_stream_t stream) {
    Dims d;
    LoraPlan pl;
    if (!get_dims(cfg, d) || !dparams || !lora_plan(d, req, true, pl)) return MFVIT_EINVAL;
    return lora_run(d, req, dparams, nullptr, true, (hipStream_t)stream);
}
int mfvit_gpt_forward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, const float* tokens, void* workspace, float* out,
                      mfvit_stream_t stream) {
    ShareScope share(cfg);
    return encoder_forward(cfg, nullptr, params, shadow, tokens, workspace, out, stream, true);
}
int mfvit_gpt_backward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, void* workspace, const float* dout, float* dparams,
                       float* dtokens, mfvit_stream_t stream) {
    if (!cfg || !dtokens || !dout || !dparams) return MFVIT_EINVAL;
    ShareScope share(cfg);
    return encoder_backward(cfg, nullptr, params, shadow, workspace, {dout, dparams, dtokens, nullptr, cfg->depth, -1}, stream, true);
}

}  // extern "C"
