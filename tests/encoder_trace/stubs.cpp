// Recording stubs for everything csrc/vit.hip links against: the launchers of kernels.h, prof_set_tag and the seven HIP runtime calls it makes.
// Linked with vit.hip compiled host-only and driver.cpp, they turn a call of the C ABI into a text trace of its launch sequence - on a machine
// without a GPU.  No stub dereferences a device pointer: addresses are printed relative to the fake regions the driver registers.  A launcher
// vit.hip starts to use and this file lacks is a link error, on purpose.
#include "../../include/mfvit.h"
#include "kernels.h"
#include "prof.h"

#include <map>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

namespace tr {   // the interface driver.cpp declares again
struct Region { std::string name; const char* base; size_t bytes; };
static std::vector<Region> regions;
static std::map<const void*, std::string> handles;   // streams and events by name
static std::map<std::string, long> knobs;
static std::string text;
static int n_streams, n_events, n_calls, tag_now, tag_shown;
static uintptr_t next_handle = 0x7000;
static std::vector<size_t> call_starts;   // offset in `text` of the line of every call that can fail (find_call)

void reset() {
    regions.clear(); handles.clear(); knobs.clear(); text.clear(); call_starts.clear();
    n_streams = n_events = n_calls = tag_now = tag_shown = 0;
}
void region(const char* name, const void* base, size_t bytes) { regions.push_back({name, (const char*)base, bytes}); }
void name_handle(const void* h, const char* name) { handles[h] = name; }
void knob(const char* name, long v) { knobs[name] = v; }
static long knob_or(const char* name, long dflt) { auto it = knobs.find(name); return it == knobs.end() ? dflt : it->second; }
void note(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    text += buf;
    text += '\n';
}
std::string take() { std::string t; t.swap(text); n_calls = 0; call_starts.clear(); return t; }
// number (1-based, as fail_at counts) of the nth call among those recorded so far whose line starts with `prefix`; 0: none
int find_call(const char* prefix, int nth);
}  // namespace tr

namespace {

const char* dt(int d) {
    static const char* n[] = {"f32", "bf16", "bf16x3", "f16", "x3f16"};
    return d >= 0 && d <= 4 ? n[d] : "dtype?";
}
const char* epi(int e) {
    static const char* n[] = {"BIAS", "BIAS_GELU", "GELU_BWD", "NONE", "BIAS_RELU", "BIAS_X3F16", "BIAS_GELU_DROP", "COL2IM16"};
    return e >= 0 && e <= 7 ? n[e] : "epi?";
}
const char* repi(int e) {
    static const char* n[] = {"RES_LN", "LNBWD_RES", "RES_LN_DP"};
    return e >= 0 && e <= 2 ? n[e] : "repi?";
}

// One trace line: the call's name, then its arguments in order.  end(): a launcher's status; status(): a HIP call's.
struct Line {
    std::string s;
    explicit Line(const char* name) : s(name) {}
    Line& raw(const char* k, const char* v) { s += ' '; if (*k) { s += k; s += k[0] == '-' ? ' ' : '='; } s += v; return *this; }
    Line& i(const char* k, long long v) { return raw(k, std::to_string(v).c_str()); }
    Line& u(const char* k, unsigned long long v) { return raw(k, std::to_string(v).c_str()); }
    Line& f(const char* k, float v) { char b[48]; snprintf(b, sizeof(b), "%a", (double)v); return raw(k, b); }
    Line& p(const char* k, const void* v) {
        if (!v) return raw(k, "null");
        for (const tr::Region& r : tr::regions)
            if ((const char*)v >= r.base && (const char*)v < r.base + r.bytes)
                return raw(k, (r.name + "+" + std::to_string((const char*)v - r.base)).c_str());
        char b[32];
        snprintf(b, sizeof(b), "?0x%llx", (unsigned long long)(uintptr_t)v);
        return raw(k, b);
    }
    Line& h(const char* k, const void* v) {   // a stream or an event
        auto it = tr::handles.find(v);
        if (it != tr::handles.end()) return raw(k, it->second.c_str());
        return p(k, v);
    }
    Line& d(const char* k, const mfvit::DropP& v) {
        char b[64];
        snprintf(b, sizeof(b), "%u/%a/%u", v.thr, (double)v.scale, v.key);
        return raw(k, b);
    }
    Line& g(const char* k, const mfvit::GemmP& q) {   // non-zero fields only
        s += ' '; s += k; s += '{';
        Line in("");
#define P_(x) if (q.x) in.p(#x, q.x)
#define I_(x) if (q.x) in.i(#x, q.x)
        P_(A); I_(lda); P_(W); I_(ldw); I_(M); I_(N); I_(K); P_(bias); P_(out0); I_(ldo0); P_(out1); I_(ldo1); P_(aux); I_(ldaux); P_(res); I_(ldres);
        P_(res_t); I_(ldres_t); I_(res_mod); I_(res_off); I_(orow_in); I_(orow_out); I_(orow_off); P_(gamma); P_(beta);
        if (q.eps != 0.f) in.f("eps", q.eps);
        P_(mean); P_(rstd); P_(cs0); P_(cs1); P_(cs2); P_(cpart); I_(y_f32); I_(splits); P_(kpart); P_(kcnt); I_(rows_per_wg); P_(omax); I_(omax_rows);
        I_(omax_hd); I_(nb); I_(nbi); I_(sAo); I_(sAi); I_(sWo); I_(sWi); I_(sOo); I_(sOi); I_(sBo); I_(sBi);
        if (q.drop.thr || q.drop.key || q.drop.scale != 0.f) in.d("drop", q.drop);
        I_(drop_tpr);
#undef P_
#undef I_
        s += in.s.empty() ? "" : in.s.substr(1);
        s += '}';
        return *this;
    }
    Line& gemm_tail(hipStream_t st) { h("st", st); return i("share", mfvit::stream_share()); }
    static void emit_tag() {
        tr::text += "prof_tag " + std::to_string(tr::tag_now) + "\n";
        tr::tag_shown = tr::tag_now;
    }
    void emit() {
        if (tr::tag_now != tr::tag_shown) emit_tag();
        tr::text += s;
        tr::text += '\n';
    }
    void query() { emit(); }
    bool failing() {
        if (tr::tag_now != tr::tag_shown) { emit_tag(); }
        tr::call_starts.push_back(tr::text.size());
        ++tr::n_calls;
        const bool fail = tr::knob_or("fail_at", 0) == tr::n_calls;
        if (fail) s += "  <- fails";
        emit();
        return fail;
    }
    int end() { return failing() ? MFVIT_ELAUNCH : MFVIT_OK; }
    hipError_t status() { return failing() ? hipErrorUnknown : hipSuccess; }
};

}  // namespace

int tr::find_call(const char* prefix, int nth) {
    const size_t len = strlen(prefix);
    for (int c = 0; c < (int)call_starts.size(); ++c)
        if (text.compare(call_starts[c], len, prefix) == 0 && --nth == 0) return c + 1;
    return 0;
}

// an argument under its own name: .i_(rows) is .i("rows", rows)
#define i_(x) i(#x, x)
#define u_(x) u(#x, x)
#define f_(x) f(#x, x)
#define p_(x) p(#x, x)
#define h_(x) h(#x, x)
#define d_(x) d(#x, x)

// ---------------------------------------------------------------------------------------------- HIP runtime
extern "C" {
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t st) {
    return Line("hipMemsetAsync").p_(dst).i_(value).u_(bytes).h_(st).status();
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    return Line("hipMemcpyAsync").p_(dst).p_(src).u_(bytes).i_(kind).h_(st).status();
}
hipError_t hipStreamIsCapturing(hipStream_t st, hipStreamCaptureStatus* status) {
    const long cap = tr::knob_or("capturing", 0);
    *status = cap ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return Line("hipStreamIsCapturing").h_(st).raw("->", cap ? "active" : "none").status();
}
hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned flags) {
    *st = (hipStream_t)(tr::next_handle += 0x10);
    tr::name_handle(*st, ("side" + std::to_string(++tr::n_streams)).c_str());
    return Line("hipStreamCreateWithFlags").u_(flags).h("->", *st).status();
}
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned flags) {
    *ev = (hipEvent_t)(tr::next_handle += 0x10);
    const std::string name = "ev" + std::to_string(++tr::n_events);
    tr::name_handle(*ev, name.c_str());
    // a run of creations is one line, "-> ev3..ev66": the line before this one, if it is a creation, is extended
    const std::string head = "hipEventCreateWithFlags flags=" + std::to_string(flags) + " -> ";
    const size_t nl = tr::text.size() < 2 ? std::string::npos : tr::text.rfind('\n', tr::text.size() - 2);
    const size_t b = nl == std::string::npos ? 0 : nl + 1;
    if (tr::text.compare(b, head.size(), head) != 0 || tr::text.find('<', b) != std::string::npos)
        return Line("hipEventCreateWithFlags").u_(flags).h("->", *ev).status();
    const size_t e = tr::text.find_first_of(".\n", b + head.size());
    const std::string first = tr::text.substr(b + head.size(), e - b - head.size());
    tr::text.erase(b);
    return Line("hipEventCreateWithFlags").u_(flags).raw("->", (first + ".." + name).c_str()).status();
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) { return Line("hipEventRecord").h_(ev).h_(st).status(); }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned flags) {
    return Line("hipStreamWaitEvent").h_(st).h_(ev).u_(flags).status();
}
}  // extern "C"

// ---------------------------------------------------------------------------------------------- launchers and decisions of kernels.h
namespace mfvit {

void prof_set_tag(int tag) { tr::tag_now = tag; }

// decisions: answered from the scenario's knobs, recorded with their arguments
int attn_qkv_dtype(int dtype, int Tn, int HD) {
    const long k = tr::knob_or("qkv_dtype", -1);
    const int r = k >= 0 ? (int)k : (dtype == MFVIT_BF16X3 ? MFVIT_X3F16 : dtype);
    Line("attn_qkv_dtype?").raw("", dt(dtype)).i("T", Tn).i_(HD).raw("->", dt(r)).query();
    return r;
}
bool gemm_nt_rowp_supported(int dtype, int e, const GemmP& p) {
    const bool r = tr::knob_or("rowp_ok", 1) != 0;
    Line("gemm_nt_rowp_supported?").raw("", dt(dtype)).raw("", repi(e)).g("p", p).i("->", r).query();
    return r;
}
bool gemm_tn_pair_supported(int dtype, const GemmP& a, const GemmP& b) {
    const bool r = tr::knob_or("pair_ok", 1) != 0;
    Line("gemm_tn_pair_supported?").raw("", dt(dtype)).g("a", a).g("b", b).i("->", r).query();
    return r;
}
bool attn_tiled_supported(int dtype, int Tn, int HDim) {
    const bool r = tr::knob_or("tiled_ok", 1) != 0;
    Line("attn_tiled_supported?").raw("", dt(dtype)).i("T", Tn).i("HD", HDim).i("->", r).query();
    return r;
}
bool lora_pair_ok(const LoraPair& p, int r, bool grad) {
    const bool ok = tr::knob_or("lora_ok", 1) != 0;
    Line("lora_pair_ok?").p("w", p.w).p("a", p.a).p("b", p.b).p("o0", p.o0).p("o1", p.o1).i("N", p.N).i("K", p.K).i("ldw", p.ldw).i("ldo", p.ldo)
        .i_(r).i_(grad).i("->", ok).query();
    return ok;
}

int gemm_nt_tile(int dtype, int e, const GemmP& p, hipStream_t st) {
    return Line("gemm_nt_tile").raw("", dt(dtype)).raw("", epi(e)).g("p", p).gemm_tail(st).end();
}
int gemm_nt_row(int dtype, int e, const GemmP& p, hipStream_t st) {
    return Line("gemm_nt_row").raw("", dt(dtype)).raw("", repi(e)).g("p", p).gemm_tail(st).end();
}
int gemm_nt_rowp(int dtype, int e, const GemmP& p, hipStream_t st) {
    return Line("gemm_nt_rowp").raw("", dt(dtype)).raw("", repi(e)).g("p", p).gemm_tail(st).end();
}
int gemm_tn(int dtype, const GemmP& p, hipStream_t st) { return Line("gemm_tn").raw("", dt(dtype)).g("p", p).gemm_tail(st).end(); }
int gemm_tn_glds_pair(int dtype, GemmP a, const GemmP& b, hipStream_t st) {
    return Line("gemm_tn_glds_pair").raw("", dt(dtype)).g("a", a).g("b", b).gemm_tail(st).end();
}

static thread_local ColpartBatch* t_colpart = nullptr;
static thread_local TnPartBatch* t_tnpart = nullptr;
ColpartBatch* colpart_batch_begin(ColpartBatch* b) {
    Line("colpart_batch_begin").raw("", b ? "batch" : "null").query();
    ColpartBatch* prev = t_colpart;
    t_colpart = b;
    return prev;
}
int colpart_batch_flush(hipStream_t st) { return Line("colpart_batch_flush").h_(st).end(); }
TnPartBatch* tnpart_batch_begin(TnPartBatch* b) {
    Line("tnpart_batch_begin").raw("", b ? "batch" : "null").query();
    TnPartBatch* prev = t_tnpart;
    t_tnpart = b;
    return prev;
}
int tnpart_batch_flush(hipStream_t st) { return Line("tnpart_batch_flush").h_(st).end(); }

int attn_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int Tn, int H, int HD, hipStream_t st) {
    return Line("attn_fwd").raw("", dt(dtype)).p_(qkv).p_(out).p_(lse).i_(B).i("T", Tn).i_(H).i_(HD).h_(st).end();
}
int attn_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* dbias, int B, int Tn, int H, int HD,
             hipStream_t st, const unsigned* domax) {
    return Line("attn_bwd").raw("", dt(dtype)).p_(qkv).p_(out).p_(dout).p_(lse).p_(dqkv).p_(dbias).i_(B)
        .i("T", Tn).i_(H).i_(HD).h_(st).p_(domax).end();
}
int attn_fwd_tiled_drop(int dtype, const void* qkv, void* out, float* lse, int B, int Tn, int H, int HDim, DropP drop, hipStream_t st) {
    return Line("attn_fwd_tiled_drop").raw("", dt(dtype)).p_(qkv).p_(out).p_(lse).i_(B).i("T", Tn).i_(H).i("HD", HDim)
        .d_(drop).h_(st).end();
}
int attn_bwd_tiled_drop(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int Tn, int H, int HDim,
                        DropP drop, hipStream_t st) {
    return Line("attn_bwd_tiled_drop").raw("", dt(dtype)).p_(qkv).p_(out).p_(dout).p_(lse).p_(dqkv).i_(B).i("T", Tn)
        .i_(H).i("HD", HDim).d_(drop).h_(st).end();
}
int attn_probs(int qdt, const void* qkv, const float* lse, int B, int Tn, int H, int HD, int fuse, int cls_only, float* out, float* sums,
               hipStream_t st) {
    return Line("attn_probs").raw("", dt(qdt)).p_(qkv).p_(lse).i_(B).i("T", Tn).i_(H).i_(HD).i_(fuse)
        .i_(cls_only).p_(out).p_(sums).h_(st).end();
}
int attn_rollout(const float* maps, const float* sums, int depth, int B, int Tn, float* out, hipStream_t st) {
    return Line("attn_rollout").p_(maps).p_(sums).i_(depth).i_(B).i("T", Tn).p_(out).h_(st).end();
}
int attn_rel_map(int qdt, int ddt, const void* qkv, const float* lse, const void* dout, int B, int Tn, int H, int HD, float* map, const float* v,
                 float* part, int first, hipStream_t st) {
    return Line("attn_rel_map").raw("", dt(qdt)).raw("", dt(ddt)).p_(qkv).p_(lse).p_(dout).i_(B).i("T", Tn).i_(H).i_(HD)
        .p_(map).p_(v).p_(part).i_(first).h_(st).end();
}
int attn_rel_update(float* v, const float* part, int B, int Tn, int first, float* out, hipStream_t st) {
    return Line("attn_rel_update").p_(v).p_(part).i_(B).i("T", Tn).i_(first).p_(out).h_(st).end();
}

int im2col16(int dtype, const float* img, void* P, int B, int H, int W, hipStream_t st) {
    return Line("im2col16").raw("", dt(dtype)).p_(img).p_(P).i_(B).i_(H).i_(W).h_(st).end();
}
int ln_rows(int dtype, int N, const float* in0, long ld0, const float* in1, long ld1, int mod1, float* xout, long ldx, void* y, long ldy, int y_f32,
            const float* gamma, const float* beta, float eps, float* mean, float* rstd, int rows, int row_stride, int row_off, int in0_bcast,
            hipStream_t st) {
    return Line("ln_rows").raw("", dt(dtype)).i_(N).p_(in0).i_(ld0).p_(in1).i_(ld1).i_(mod1).p_(xout)
        .i_(ldx).p_(y).i_(ldy).i_(y_f32).p_(gamma).p_(beta).f_(eps).p_(mean).p_(rstd)
        .i_(rows).i_(row_stride).i_(row_off).i_(in0_bcast).h_(st).end();
}
int ln_bwd_rows(int dtype, int N, const float* dy, long lddy, const float* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                const float* dres, long ldres, float* dx, long lddx, void* dxT, long lddxT, float* dgamma, float* dbeta, float* dcol, float* cpart,
                int rows, int row_stride, int row_off, hipStream_t st, const void* dyT, long lddyT) {
    return Line("ln_bwd_rows").raw("", dt(dtype)).i_(N).p_(dy).i_(lddy).p_(x).i_(ldx).p_(mean).p_(rstd)
        .p_(gamma).p_(dres).i_(ldres).p_(dx).i_(lddx).p_(dxT).i_(lddxT).p_(dgamma)
        .p_(dbeta).p_(dcol).p_(cpart).i_(rows).i_(row_stride).i_(row_off).h_(st)
        .p_(dyT).i_(lddyT).end();
}
int add_ln_rows(int dtype, int N, const void* tin, long ldt, const float* pos, long ldp, int pmod, const float* res, long ldres, int rin, int rout,
                int roff, float* xout, long ldx, void* y, long ldy, int y_f32, const float* gamma, const float* beta, float eps, float* mean,
                float* rstd, int rows, hipStream_t st) {
    return Line("add_ln_rows").raw("", dt(dtype)).i_(N).p_(tin).i_(ldt).p_(pos).i_(ldp).i_(pmod).p_(res)
        .i_(ldres).i_(rin).i_(rout).i_(roff).p_(xout).i_(ldx).p_(y).i_(ldy).i_(y_f32)
        .p_(gamma).p_(beta).f_(eps).p_(mean).p_(rstd).i_(rows).h_(st).end();
}
int drop_add_ln_rows(int dtype, int N, const void* tin, long ldt, const float* a0, long lda0, const float* a1, long lda1, int mod1, const float* res,
                     long ldres, DropP drop, DropP dpath, int tpr, float* xout, long ldx, void* y, long ldy, int y_f32, const float* gamma,
                     const float* beta, float eps, float* mean, float* rstd, int rows, hipStream_t st) {
    return Line("drop_add_ln_rows").raw("", dt(dtype)).i_(N).p_(tin).i_(ldt).p_(a0).i_(lda0).p_(a1).i_(lda1)
        .i_(mod1).p_(res).i_(ldres).d_(drop).d_(dpath).i_(tpr).p_(xout).i_(ldx).p_(y)
        .i_(ldy).i_(y_f32).p_(gamma).p_(beta).f_(eps).p_(mean).p_(rstd).i_(rows).h_(st)
        .end();
}
int mask_scale_rows(int dtype, bool f32, const void* src, long lds_, void* dst, long ldd, DropP drop, DropP dpath, int tpr, int rows, int N,
                    hipStream_t st) {
    return Line("mask_scale_rows").raw("", dt(dtype)).i_(f32).p_(src).i("lds", lds_).p_(dst).i_(ldd).d_(drop)
        .d_(dpath).i_(tpr).i_(rows).i_(N).h_(st).end();
}
int cast_transpose(int dtype, const float* src, void* dst, void* dstT, int R, int C, hipStream_t st) {
    return Line("cast_transpose").raw("", dt(dtype)).p_(src).p_(dst).p_(dstT).i_(R).i_(C).h_(st).end();
}
int cast_transpose_batched(int dtype, const float* src, void* dst, void* dstT, int R, int C, int nb, long s_src, long s_dst, long s_dstT,
                           hipStream_t st) {
    return Line("cast_transpose_batched").raw("", dt(dtype)).p_(src).p_(dst).p_(dstT).i_(R).i_(C).i_(nb)
        .i_(s_src).i_(s_dst).i_(s_dstT).h_(st).end();
}
int axpy(float* y, const float* x, float a, long n, hipStream_t st) { return Line("axpy").p_(y).p_(x).f_(a).i_(n).h_(st).end(); }
int colsum_rows(const float* x, long ld, float* out, int rows, int row_stride, int row_off, int N, hipStream_t st) {
    return Line("colsum_rows").p_(x).i_(ld).p_(out).i_(rows).i_(row_stride).i_(row_off).i_(N)
        .h_(st).end();
}
int batch_sum(const float* x, float* out, int B, long n, hipStream_t st) {
    return Line("batch_sum").p_(x).p_(out).i_(B).i_(n).h_(st).end();
}

static int lora_batch(const char* name, const LoraPair* pairs, int n, int r, float scale, hipStream_t st) {
    Line l(name);
    l.i_(n).i_(r).f_(scale).h_(st);
    for (int i = 0; i < n; ++i) {
        const LoraPair& p = pairs[i];
        l.raw("", "|").p("w", p.w).p("a", p.a).p("b", p.b).p("o0", p.o0).p("o1", p.o1).i("N", p.N).i("K", p.K).i("ldw", p.ldw).i("ldo", p.ldo);
    }
    return l.end();
}
int lora_merge_batch(const LoraPair* pairs, int n, int r, float scale, hipStream_t st) { return lora_batch("lora_merge_batch", pairs, n, r, scale, st); }
int lora_grad_batch(const LoraPair* pairs, int n, int r, float scale, hipStream_t st) { return lora_batch("lora_grad_batch", pairs, n, r, scale, st); }

}  // namespace mfvit
