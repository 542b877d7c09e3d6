// Bootstrap replicates and DeLong components of the epoch metrics on the device (replaces the host loop a user would put around MAIN_CA:886-911 /
// MAIN_SS:797-821: R resamples, each three scikit-learn calls or one O(n^2) mfvit_eval_counts).  Every result is an integer: the same bits on every run.
// Each (model, class) column is ordered ONCE by counting; after that a replicate costs O(n) per column.
//   order_kernel       per column and sample i: lt = #{key_j < key_i}, eq = #{key_j == key_i}, eqb = #{key_j == key_i, j < i} over rank_key's integer
//                      keys, the column streamed through LDS 1,024 keys at a time (as auc_pairs_kernel streams it).  pos = lt + eqb is the sample's
//                      place in the total order (key ascending, index ascending); ent[pos] = i | nan << 30 | positive << 31 and
//                      grp[pos] = lt | (lt + eq) << 16, the tie group [gs, ge) of that place.  One more "column" orders the samples by stratum.
//   preds_kernel       first-maximum argmax per model as a byte, the label as a byte (255: outside [0, C)).
//   weights_kernel     one workgroup per replicate: the n draws into a histogram of 16-bit counters in LDS (integer atomics, two counters a word),
//                      written out as w u16 [R][npad].  Replicate 0 is the sample itself.
//   scan_kernel        one workgroup per (replicate, column): the weights in sorted order, the inclusive prefix of the negatives' weights in LDS
//                      (u32, 128 KiB at n = 32768), then every positive of tie group [gs, ge) adds w (E[gs] + E[ge]), E the exclusive prefix: twice the
//                      negatives below plus once the negatives tied.  NaN keys sort first and carry the nan flag: in no pair, on either side.
//                      The DeLong form (unit weights) emits the structural components v2 instead; a negative reads the positives' counts, which are
//                      the places minus the negatives' prefix.
//   conf_kernel        one workgroup per replicate: M C^2 counters in LDS.
//   moments_kernel     pos_xy / neg_xy of the DeLong covariance: exact sums of products of v2.
// The curve itself, operating points and calibration (mfvit_curve_counts, mfvit_boot_points, mfvit_calib_sums) sit on the same ordered columns:
//   curve_kernel       one workgroup per column: per tie group of numbers, largest first, its score and the positives / negatives at or above it
//                      (sklearn's _binary_clf_curve as integers).
//   points_kernel      one workgroup per (replicate, column), as scan_kernel: the positives' and the negatives' weighted prefixes share one LDS word
//                      per place (16 bits each), and a request (a cap on FP, a floor on TP, or a threshold) is a bisection on them.
//   calib_kernel       one workgroup per (model, temperature): softmax in double per row, bin counters by integer LDS atomics, the double sums as
//                      per-thread partials added in a fixed order.
#include "common.cuh"
#include "kernels.h"

namespace mfvit {

namespace {

constexpr int BOOT_MAXN = 32768, BOOT_MAXC = 64, BOOT_MAXM = 8;
constexpr int ORD_T = 256;          // samples per workgroup of the order kernel
constexpr int ORD_CHUNK = 1024;     // keys per LDS chunk
constexpr int SCAN_T = 512;         // places per tile of the prefix scan
constexpr int W_T = 1024, CONF_T = 256, MOM_T = 256;
constexpr unsigned ENT_IDX = 0x7fffu, ENT_NAN = 1u << 30, ENT_POS = 1u << 31;
constexpr unsigned PAD_KEY = 0xffffffffu;     // above every key (the largest, +inf, is 0xff800001): neither below nor tied with any sample

// perturb.hip's rank_key: a > b <=> key(a) > key(b) for numbers, -0.0 and +0.0 share a key, every NaN has key 1, below -inf.
__device__ __forceinline__ unsigned score_key(float x) {
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 1u;
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) + 1u;
}

// column col < K: model col / C, class col % C.  col == K: the strata (label 0 .. C - 1, then everything else).
__global__ __launch_bounds__(ORD_T) void order_kernel(const float* __restrict__ scores, long ld, long ms, const int64_t* __restrict__ labels, int n,
                                                      int C, int K, int col0, unsigned* __restrict__ ent, unsigned* __restrict__ grp) {
    __shared__ uint4 keys4[ORD_CHUNK / 4];
    unsigned* keys = (unsigned*)keys4;
    const int col = col0 + blockIdx.y;
    const bool strata = col == K;
    const int m = col / C, c = col - m * C;
    const float* s = scores + (long)m * ms + c;
    auto key_of = [&](int j) -> unsigned {
        if (strata) {
            const int64_t t = labels[j];
            return (unsigned)(t >= 0 && t < C ? t : C) + 1u;
        }
        return score_key(s[(long)j * ld]);
    };
    const int i = blockIdx.x * ORD_T + threadIdx.x;
    const unsigned ki = i < n ? key_of(i) : 0u;
    int lt = 0, eq = 0, eqb = 0;
    for (int j0 = 0; j0 < n; j0 += ORD_CHUNK) {
        __syncthreads();
        for (int t = threadIdx.x; t < ORD_CHUNK; t += ORD_T) keys[t] = j0 + t < n ? key_of(j0 + t) : PAD_KEY;
        __syncthreads();
        if (i < n) {
            const int before = i - j0;                                   // the chunk's elements t < before come before sample i
            const int m4 = (min(n - j0, ORD_CHUNK) + 3) >> 2;
            for (int t = 0; t < m4; ++t) {
                const uint4 k = keys4[t];                                // (every lane reads the same 16 bytes: an LDS broadcast)
                const int b = 4 * t;
                lt += (k.x < ki) + (k.y < ki) + (k.z < ki) + (k.w < ki);
                eq += (k.x == ki) + (k.y == ki) + (k.z == ki) + (k.w == ki);
                eqb += (k.x == ki && b < before) + (k.y == ki && b + 1 < before) + (k.z == ki && b + 2 < before) + (k.w == ki && b + 3 < before);
            }
        }
    }
    if (i < n) {
        const int pos = lt + eqb;                                        // a total order: every place 0 .. n - 1 has exactly one writer
        unsigned e = (unsigned)i;
        if (!strata) e |= (ki == 1u ? ENT_NAN : 0u) | (labels[i] == c ? ENT_POS : 0u);
        ent[(long)col * n + pos] = e;
        grp[(long)col * n + pos] = (unsigned)lt | (unsigned)(lt + eq) << 16;
    }
}

__global__ __launch_bounds__(256) void preds_kernel(const float* __restrict__ scores, long ld, long ms, const int64_t* __restrict__ labels, int n, int C,
                                                    unsigned char* __restrict__ preds8, unsigned char* __restrict__ lab8) {
    const int i = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (i >= n) return;
    const float* s = scores + (long)m * ms + (long)i * ld;
    int best = 0;
    float bv = s[0];
    for (int c = 1; c < C; ++c) {
        const float v = s[c];
        if (first_max_takes(v, bv)) { bv = v; best = c; }
    }
    preds8[(long)m * n + i] = (unsigned char)best;
    if (m == 0) {
        const int64_t t = labels[i];
        lab8[i] = t >= 0 && t < C ? (unsigned char)t : (unsigned char)255;
    }
}

// replicate r = r0 + blockIdx.x; dynamic LDS: npad / 2 words.  sent / sgrp: the stratum order (NULL: plain resampling).
__global__ __launch_bounds__(W_T) void weights_kernel(int n, int npad, unsigned seed_lo, unsigned seed_hi, unsigned r0, const unsigned* __restrict__ sent,
                                                      const unsigned* __restrict__ sgrp, unsigned short* __restrict__ w) {
    extern __shared__ unsigned hist[];
    const unsigned r = r0 + blockIdx.x;
    unsigned* out = (unsigned*)(w + (long)blockIdx.x * npad);
    const int words = npad >> 1;
    if (r == 0) {                                                        // the original sample
        for (int t = threadIdx.x; t < words; t += W_T) out[t] = (2 * t < n ? 1u : 0u) | (2 * t + 1 < n ? 0x10000u : 0u);
        return;
    }
    for (int t = threadIdx.x; t < words; t += W_T) hist[t] = 0u;
    __syncthreads();
    const unsigned key = lowbias32(seed_lo ^ lowbias32(seed_hi + 0x9E3779B9u * (r + 1u)));
    for (int k = threadIdx.x; k < n; k += W_T) {
        const unsigned h = lowbias32((unsigned)k ^ key);
        unsigned idx;
        if (sent) {
            const unsigned g = sgrp[k], off = g & 0xffffu, ns = (g >> 16) - off;
            idx = sent[off + (unsigned)(((unsigned long long)h * ns) >> 32)] & ENT_IDX;
        } else {
            idx = (unsigned)(((unsigned long long)h * (unsigned)n) >> 32);
        }
        atomicAdd(hist + (idx >> 1), 1u << (16 * (idx & 1u)));           // a counter holds at most n = 32768 < 2^16: no carry into its neighbour
    }
    __syncthreads();
    for (int t = threadIdx.x; t < words; t += W_T) out[t] = hist[t];
}

// blockIdx.x = rl * K + col.  dynamic LDS: n words (the inclusive prefix of the negatives' weights).
template <bool DELONG>
__global__ __launch_bounds__(SCAN_T) void scan_kernel(const unsigned* __restrict__ ent, const unsigned* __restrict__ grp, const unsigned short* __restrict__ w,
                                                      int npad, int n, int C, int K, unsigned long long* __restrict__ u2,
                                                      unsigned long long* __restrict__ npos, int* __restrict__ v2w, int* __restrict__ v2out) {
    extern __shared__ unsigned incl[];
    __shared__ unsigned wtot[SCAN_T / 64];
    __shared__ unsigned long long red[SCAN_T];
    __shared__ unsigned redn[SCAN_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = blockIdx.x % K, rl = blockIdx.x / K;
    const unsigned* e_ = ent + (long)col * n;
    const unsigned* g_ = grp + (long)col * n;
    const unsigned short* w_ = DELONG ? nullptr : w + (long)rl * npad;
    unsigned carry = 0;
    for (int p0 = 0; p0 < n; p0 += SCAN_T) {
        const int p = p0 + tid;
        unsigned x = 0;
        if (p < n) {
            const unsigned e = e_[p];
            if (!(e & (ENT_NAN | ENT_POS))) x = DELONG ? 1u : (unsigned)w_[e & ENT_IDX];
        }
        for (int o = 1; o < 64; o <<= 1) {                               // inclusive scan inside the wave
            const unsigned y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        unsigned below = 0, total = 0;
        for (int v = 0; v < SCAN_T / 64; ++v) {
            const unsigned t = wtot[v];
            below += v < wave ? t : 0u;
            total += t;
        }
        if (p < n) incl[p] = carry + below + x;
        carry += total;
        __syncthreads();
    }
    auto excl = [&](unsigned q) -> unsigned { return q ? incl[q - 1] : 0u; };
    unsigned long long acc = 0;
    unsigned np = 0;
    unsigned nn = 0, ptot = 0;
    if (DELONG) {
        nn = (e_[0] & ENT_NAN) ? g_[0] >> 16 : 0u;                       // the NaN keys are the first tie group
        ptot = (unsigned)n - nn - incl[n - 1];                           // positives that are numbers
    }
    for (int p = tid; p < n; p += SCAN_T) {
        const unsigned e = e_[p], g = g_[p], gs = g & 0xffffu, ge = g >> 16;
        const bool pos = e & ENT_POS, nan = e & ENT_NAN;
        if (DELONG) {
            unsigned v = 0;
            if (!nan) v = pos ? excl(gs) + excl(ge) : 2u * ptot - ((ge - nn) - excl(ge)) - ((gs - nn) - excl(gs));
            const long o = (long)col * n + (e & ENT_IDX);
            v2w[o] = (int)v;
            if (v2out) v2out[o] = (int)v;
            if (pos) { acc += v; ++np; }
        } else if (pos) {
            const unsigned wv = w_[e & ENT_IDX];
            np += wv;
            if (!nan) acc += (unsigned long long)wv * (excl(gs) + excl(ge));
        }
    }
    red[tid] = acc;
    redn[tid] = np;
    __syncthreads();
    for (int o = SCAN_T / 2; o > 0; o >>= 1) {
        if (tid < o) { red[tid] += red[tid + o]; redn[tid] += redn[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        u2[(long)rl * K + col] = red[0];
        if (col < C) npos[(long)rl * C + col] = redn[0];                 // model 0's columns
    }
}

// replicate blockIdx.x; dynamic LDS: M C^2 words
__global__ __launch_bounds__(CONF_T) void conf_kernel(const unsigned char* __restrict__ preds8, const unsigned char* __restrict__ lab8,
                                                      const unsigned short* __restrict__ w, int npad, int n, int C, int M,
                                                      unsigned long long* __restrict__ conf) {
    extern __shared__ unsigned cnt[];
    const int cells = M * C * C;
    for (int t = threadIdx.x; t < cells; t += CONF_T) cnt[t] = 0u;
    __syncthreads();
    const unsigned short* w_ = w + (long)blockIdx.x * npad;
    for (int i = threadIdx.x; i < n; i += CONF_T) {
        const unsigned t = lab8[i], wv = w_[i];
        if (t >= (unsigned)C || !wv) continue;
        for (int m = 0; m < M; ++m) atomicAdd(cnt + (m * C + t) * C + preds8[(long)m * n + i], wv);
    }
    __syncthreads();
    unsigned long long* out = conf + (long)blockIdx.x * cells;
    for (int t = threadIdx.x; t < cells; t += CONF_T) out[t] = cnt[t];
}

// blockIdx.x = m * M + m', blockIdx.y = c: pos_xy / neg_xy [c][m][m']
__global__ __launch_bounds__(MOM_T) void moments_kernel(const int* __restrict__ v2w, const int64_t* __restrict__ labels, int n, int C, int M,
                                                        unsigned long long* __restrict__ pos_xy, unsigned long long* __restrict__ neg_xy) {
    __shared__ unsigned long long rp[MOM_T], rn[MOM_T];
    const int a = blockIdx.x / M, b = blockIdx.x - a * M, c = blockIdx.y, tid = threadIdx.x;
    const int* va = v2w + ((long)a * C + c) * n;
    const int* vb = v2w + ((long)b * C + c) * n;
    unsigned long long sp = 0, sn = 0;
    for (int i = tid; i < n; i += MOM_T) {
        const unsigned long long prod = (unsigned long long)(unsigned)va[i] * (unsigned)vb[i];
        if (labels[i] == c) sp += prod; else sn += prod;
    }
    rp[tid] = sp; rn[tid] = sn;
    __syncthreads();
    for (int o = MOM_T / 2; o > 0; o >>= 1) {
        if (tid < o) { rp[tid] += rp[tid + o]; rn[tid] += rn[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        const long o = ((long)c * M + a) * M + b;
        pos_xy[o] = rp[0];
        neg_xy[o] = rn[0];
    }
}

// ---------------------------------------------------------------------------------------------------- curves, operating points, calibration
// Siblings of scan_kernel on the same ordered columns.  A weighted prefix is at most n = 32768 < 2^16, so ONE LDS word per place holds two inclusive
// prefixes (low and high half; neither half can carry into the other) - the 4 n bytes scan_kernel takes for one.
constexpr int PTS_MAXQ = 64, CAL_MAXK = 16, CAL_MAXB = 64, CAL_T = 256;

// incl[p] = sum of value(q) over the places q <= p (both halves at once); every thread gets the total.  The tiles and the order of scan_kernel.
template <typename F>
__device__ __forceinline__ unsigned packed_prefix(int n, unsigned* incl, unsigned* wtot, F value) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned carry = 0;
    for (int p0 = 0; p0 < n; p0 += SCAN_T) {
        const int p = p0 + tid;
        unsigned x = p < n ? value(p) : 0u;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        unsigned below = 0, total = 0;
        for (int v = 0; v < SCAN_T / 64; ++v) {
            const unsigned t = wtot[v];
            below += v < wave ? t : 0u;
            total += t;
        }
        if (p < n) incl[p] = carry + below + x;
        carry += total;
        __syncthreads();
    }
    return carry;
}

// One workgroup per column; dynamic LDS: n words, low half the prefix of the positives that are numbers, high half the prefix of the tie groups' first
// places.  The group whose first place is gs holds the samples at or above its score from place gs on: tp = positives there, fp = (n - gs) - tp (NaN
// keys sort first).  Entry k counts the groups from the top; ent[gs] is the group's first sample in index order, whose score is the one reported.
__global__ __launch_bounds__(SCAN_T) void curve_kernel(const float* __restrict__ scores, long ld, long ms, const unsigned* __restrict__ ent,
                                                       const unsigned* __restrict__ grp, int n, int C, float* __restrict__ thr, unsigned* __restrict__ tp,
                                                       unsigned* __restrict__ fp, int* __restrict__ nthr, int* __restrict__ nnan,
                                                       unsigned long long* __restrict__ npos) {
    extern __shared__ unsigned incl[];
    __shared__ unsigned wtot[SCAN_T / 64];
    __shared__ unsigned allpos;
    const int tid = threadIdx.x, col = blockIdx.x, m = col / C, c = col - m * C;
    const unsigned* e_ = ent + (long)col * n;
    const unsigned* g_ = grp + (long)col * n;
    const float* s = scores + (long)m * ms + c;
    if (tid == 0) allpos = 0u;
    __syncthreads();
    unsigned mypos = 0;
    const unsigned total = packed_prefix(n, incl, wtot, [&](int p) -> unsigned {
        const unsigned e = e_[p];
        mypos += (e & ENT_POS) ? 1u : 0u;
        if (e & ENT_NAN) return 0u;
        return ((e & ENT_POS) ? 1u : 0u) | ((g_[p] & 0xffffu) == (unsigned)p ? 0x10000u : 0u);
    });
    if (mypos) atomicAdd(&allpos, mypos);                               // an integer: any order gives the same bits
    const unsigned G = total >> 16, ptot = total & 0xffffu;
    const long o = (long)col * n;
    for (int p = tid; p < n; p += SCAN_T) {
        const unsigned e = e_[p];
        if ((e & ENT_NAN) || (g_[p] & 0xffffu) != (unsigned)p) continue;
        const unsigned k = G - (incl[p] >> 16);                         // groups above this one
        const unsigned t = ptot - (p ? incl[p - 1] & 0xffffu : 0u);
        thr[o + k] = s[(long)(e & ENT_IDX) * ld];
        tp[o + k] = t;
        fp[o + k] = (unsigned)(n - p) - t;
    }
    for (int k = (int)G + tid; k < n; k += SCAN_T) {                    // past the last group: every output element is written
        thr[o + k] = __uint_as_float(0x7fc00000u);
        tp[o + k] = 0u;
        fp[o + k] = 0u;
    }
    __syncthreads();
    if (tid == 0) {
        nthr[col] = (int)G;
        nnan[col] = (e_[0] & ENT_NAN) ? (int)(g_[0] >> 16) : 0;
        if (m == 0) npos[c] = allpos;
    }
}

// blockIdx.x = rl * K + col; dynamic LDS: n words, low half the prefix of the positives' weights, high half the negatives', numbers only.
// A threshold is a place q in [nn, n] that starts a tie group (nn: the NaN keys, q = n: above everything): tp = P' - exclP(q), fp = N' - exclN(q),
// both monotone in q - thread t < Q answers request t by a bisection on its half of the words.
__global__ __launch_bounds__(SCAN_T) void points_kernel(const float* __restrict__ scores, long ld, long ms, const unsigned* __restrict__ ent,
                                                        const unsigned* __restrict__ grp, const unsigned short* __restrict__ w, int npad, int n, int C,
                                                        int K, const int* __restrict__ req, int Q, unsigned* __restrict__ tp, unsigned* __restrict__ fp,
                                                        float* __restrict__ thr, unsigned long long* __restrict__ npos) {
    extern __shared__ unsigned incl[];
    __shared__ unsigned wtot[SCAN_T / 64];
    __shared__ unsigned allpos;
    const int tid = threadIdx.x, col = blockIdx.x % K, rl = blockIdx.x / K, m = col / C, c = col - m * C;
    const unsigned* e_ = ent + (long)col * n;
    const unsigned* g_ = grp + (long)col * n;
    const unsigned short* w_ = w + (long)rl * npad;
    const float* s = scores + (long)m * ms + c;
    if (tid == 0) allpos = 0u;
    __syncthreads();
    unsigned mypos = 0;
    const unsigned total = packed_prefix(n, incl, wtot, [&](int p) -> unsigned {
        const unsigned e = e_[p], wv = w_[e & ENT_IDX];
        if (e & ENT_POS) mypos += wv;
        if (e & ENT_NAN) return 0u;
        return (e & ENT_POS) ? wv : wv << 16;
    });
    if (mypos) atomicAdd(&allpos, mypos);
    __syncthreads();
    const long long P = allpos, N = n - P, pn = total & 0xffffu, nn_ = total >> 16;      // P, N: NaN-scored samples included; pn, nn_: numbers only
    if (tid < Q) {
        const int kind = req[3 * tid], a = req[3 * tid + 1], b = req[3 * tid + 2];
        const int nan0 = (e_[0] & ENT_NAN) ? (int)(g_[0] >> 16) : 0;
        auto exclP = [&](int q) -> long long { return q ? (long long)(incl[q - 1] & 0xffffu) : 0ll; };
        auto exclN = [&](int q) -> long long { return q ? (long long)(incl[q - 1] >> 16) : 0ll; };
        const bool frac_ok = a >= 0 && b >= 1 && a <= b && b <= (1 << 20);
        int q = -1;
        if (kind == 0 && frac_ok) {                                     // the lowest threshold with fp <= floor(a N / b)
            const long long need = nn_ - (long long)a * N / b;
            int lo = nan0, hi = n;                                      // exclN(n) = N' >= need: the search always ends on a place that qualifies
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (exclN(mid) >= need) hi = mid; else lo = mid + 1;
            }
            q = lo;
            if (q < n && (g_[q] & 0xffffu) != (unsigned)q) q = (int)(g_[q] >> 16);       // inside a group: its start does not qualify, the next start does
        } else if (kind == 1 && frac_ok) {                              // the highest threshold with tp >= ceil(a P / b)
            const long long lim = pn - ((long long)a * P + b - 1) / b;
            if (lim < 0) {
                q = nan0;                                               // out of reach (positives with NaN scores): the lowest boundary
            } else {
                int lo = nan0, hi = n;                                  // exclP(nan0) = 0 <= lim
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (exclP(mid) <= lim) lo = mid; else hi = mid - 1;
                }
                q = lo < n ? (int)(g_[lo] & 0xffffu) : n;
            }
        } else if (kind == 2) {                                         // score >= tau, on the order's integer keys
            const unsigned kt = score_key(__int_as_float(a));
            q = n;
            if (kt != 1u) {
                int lo = nan0, hi = n;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (score_key(s[(long)(e_[mid] & ENT_IDX) * ld]) >= kt) hi = mid; else lo = mid + 1;
                }
                q = lo;
            }
        }
        const long o = ((long)rl * K + col) * Q + tid;
        if (q < 0) {                                                    // not a request
            tp[o] = 0u; fp[o] = 0u; thr[o] = __uint_as_float(0x7fc00000u);
        } else {
            tp[o] = (unsigned)(pn - exclP(q));
            fp[o] = (unsigned)(nn_ - exclN(q));
            thr[o] = q < n ? s[(long)(e_[q] & ENT_IDX) * ld] : __uint_as_float(0x7f800000u);
        }
    }
    if (tid == 0 && col < C) npos[(long)rl * C + col] = allpos;
}

struct CalTemps { float t[CAL_MAXK]; };

// blockIdx.x = m * Kt + kt.  Dynamic LDS only (a 16-byte aligned base): part f64 [NB][CAL_T], red f64 [3][CAL_T], cn, ch u32 [CAL_MAXB], sk u32.
// Every thread walks its rows in index order; a bin's confidence sum is the thread's own partial (no float atomics), then lanes add their four
// partials in thread order and the wave a fixed tree; the three sums take the tree of perturb_score_kernel.
__global__ __launch_bounds__(CAL_T) void calib_kernel(const float* __restrict__ logits, long ld, long ms, const int64_t* __restrict__ labels, int n, int C,
                                                      CalTemps temps, int Kt, int NB, unsigned long long* __restrict__ bin_n,
                                                      unsigned long long* __restrict__ bin_hit, double* __restrict__ bin_conf, double* __restrict__ sums,
                                                      unsigned long long* __restrict__ skipped) {
    extern __shared__ __attribute__((aligned(16))) double part[];
    double* red = part + NB * CAL_T;
    unsigned* cn = (unsigned*)(red + 3 * CAL_T);
    unsigned* ch = cn + CAL_MAXB;
    unsigned* sk = ch + CAL_MAXB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.x / Kt, kt = blockIdx.x - m * Kt;
    const double beta = 1.0 / (double)temps.t[kt];
    for (int i = tid; i < NB * CAL_T; i += CAL_T) part[i] = 0.0;
    if (tid < CAL_MAXB) { cn[tid] = 0u; ch[tid] = 0u; }
    if (tid == 0) *sk = 0u;
    __syncthreads();
    double snll = 0.0, sbr = 0.0, sdb = 0.0;
    unsigned nskip = 0;
    for (int i = tid; i < n; i += CAL_T) {
        const float* z = logits + (long)m * ms + (long)i * ld;
        float mx = z[0];
        int am = 0;
        bool finite = isfinite(mx);
        for (int k = 1; k < C; ++k) {
            const float v = z[k];
            finite = finite && isfinite(v);
            if (v > mx) { mx = v; am = k; }                             // finite rows: the first maximum
        }
        const int64_t t = labels[i];
        if (!finite || t < 0 || t >= C) { ++nskip; continue; }
        double den = 0.0;
        for (int k = 0; k < C; ++k) den += exp(beta * ((double)z[k] - (double)mx));
        const double dt = (double)z[t] - (double)mx;
        double ez = 0.0, br = 0.0;
        for (int k = 0; k < C; ++k) {
            const double d = (double)z[k] - (double)mx, p = exp(beta * d) / den, e = p - (k == (int)t ? 1.0 : 0.0);
            ez += p * d;
            br += e * e;
        }
        const double conf = 1.0 / den;                                  // the top label's term is exp(0) = 1
        snll += log(den) - beta * dt;
        sbr += br;
        sdb += ez - dt;
        const int bin = min(NB - 1, max(0, (int)ceil(conf * (double)NB) - 1));
        atomicAdd(cn + bin, 1u);
        if (am == (int)t) atomicAdd(ch + bin, 1u);
        part[bin * CAL_T + tid] += conf;
    }
    if (nskip) atomicAdd(sk, nskip);
    red[tid] = snll; red[CAL_T + tid] = sbr; red[2 * CAL_T + tid] = sdb;
    __syncthreads();
    for (int o = CAL_T / 2; o > 0; o >>= 1) {
        if (tid < o) {
            red[tid] += red[tid + o]; red[CAL_T + tid] += red[CAL_T + tid + o]; red[2 * CAL_T + tid] += red[2 * CAL_T + tid + o];
        }
        __syncthreads();
    }
    const long ob = (long)blockIdx.x * NB;
    for (int b = wave; b < NB; b += CAL_T / 64) {
        const double* pb = part + b * CAL_T;
        double v = ((pb[lane] + pb[lane + 64]) + pb[lane + 128]) + pb[lane + 192];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) bin_conf[ob + b] = v;
    }
    for (int b = tid; b < NB; b += CAL_T) { bin_n[ob + b] = cn[b]; bin_hit[ob + b] = ch[b]; }
    if (tid == 0) {
        sums[3 * (long)blockIdx.x] = red[0];
        sums[3 * (long)blockIdx.x + 1] = red[CAL_T];
        sums[3 * (long)blockIdx.x + 2] = red[2 * CAL_T];
        if (kt == 0) skipped[m] = *sk;
    }
}

size_t calib_lds_bytes(int NB) { return ((size_t)NB * CAL_T + 3 * CAL_T) * 8 + (2 * CAL_MAXB + 4) * 4; }

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the scratch buffer: ent, grp u32 [K + 1][n] | preds8 u8 [M][n] | lab8 u8 [n] | then w u16 [R][npad] (bootstrap) or v2 i32 [K][n] (DeLong)
struct BootWork {
    size_t ent, grp, preds8, lab8, tail, total;
    int npad;
};

bool boot_shape_ok(int n, int C, int M) { return n >= 1 && n <= BOOT_MAXN && C >= 1 && C <= BOOT_MAXC && M >= 1 && M <= BOOT_MAXM; }

BootWork boot_layout(int n, int C, int M, long long R) {
    BootWork L;
    const size_t K = (size_t)M * C;
    L.npad = (n + 7) & ~7;
    L.ent = 0;
    L.grp = L.ent + up256((K + 1) * n * 4);
    L.preds8 = L.grp + up256((K + 1) * n * 4);
    L.lab8 = L.preds8 + up256((size_t)M * n);
    L.tail = L.lab8 + up256((size_t)n);
    const size_t wbytes = (size_t)R * L.npad * 2, vbytes = K * n * 4;
    L.total = L.tail + up256(wbytes > vbytes ? wbytes : vbytes);
    return L;
}

bool scores_ok(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, const void* work) {
    if (!scores || !labels || !work || !boot_shape_ok(n, C, M)) return false;
    if (ld < C || (M > 1 && ms < (long)(n - 1) * ld + C)) return false;
    return (uintptr_t)work % 16 == 0;
}

// the kernels' dynamic LDS may pass the 64 KiB a launch gets by default (scan: 4 n bytes, confusion: 4 M C^2 bytes, both up to 128 KiB of the CU's 160)
int allow_big_lds() {
    static PerDeviceOnce once;
    if (!once.first()) return MFVIT_OK;
    const int big = 4 * BOOT_MAXN;
    if (hipFuncSetAttribute((const void*)scan_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, big) != hipSuccess ||
        hipFuncSetAttribute((const void*)scan_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, big) != hipSuccess ||
        hipFuncSetAttribute((const void*)conf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * BOOT_MAXM * BOOT_MAXC * BOOT_MAXC) != hipSuccess ||
        hipFuncSetAttribute((const void*)weights_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * BOOT_MAXN) != hipSuccess ||
        hipFuncSetAttribute((const void*)curve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, big) != hipSuccess ||
        hipFuncSetAttribute((const void*)points_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, big) != hipSuccess ||
        hipFuncSetAttribute((const void*)calib_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)calib_lds_bytes(CAL_MAXB)) != hipSuccess)
        return MFVIT_ELAUNCH;
    return MFVIT_OK;
}

}  // namespace

size_t boot_work_bytes(int n, int C, int M, long long R) {
    if (!boot_shape_ok(n, C, M) || R < 1 || R > (1ll << 31)) return 0;
    return boot_layout(n, C, M, R).total;
}

int boot_counts(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, unsigned long long seed, long long r0, long long R,
                int stratified, void* work, size_t work_bytes, unsigned long long* conf, unsigned long long* u2, unsigned long long* npos,
                hipStream_t st) {
    if (!scores_ok(scores, ld, ms, labels, n, C, M, work)) return MFVIT_EINVAL;
    if (R < 1 || r0 < 0 || r0 + R > (1ll << 31) || (stratified != 0 && stratified != 1)) return MFVIT_EINVAL;      // r + 1 is a 32-bit hash input
    if ((u2 != nullptr) != (npos != nullptr) || (!conf && !u2)) return MFVIT_EINVAL;
    const BootWork L = boot_layout(n, C, M, R);
    if (work_bytes < L.total) return MFVIT_EINVAL;
    MFVIT_TRY(allow_big_lds());
    char* wk = (char*)work;
    unsigned* ent = (unsigned*)(wk + L.ent);
    unsigned* grp = (unsigned*)(wk + L.grp);
    unsigned char* preds8 = (unsigned char*)(wk + L.preds8);
    unsigned char* lab8 = (unsigned char*)(wk + L.lab8);
    unsigned short* w = (unsigned short*)(wk + L.tail);
    const int K = M * C;
    // the score columns when the pair counts are asked for, the strata (column K) when the resampling is stratified
    const int col0 = u2 ? 0 : K, cols = (u2 ? K : 0) + (stratified ? 1 : 0);
    if (cols) {
        MFVIT_LAUNCH(order_kernel, dim3((n + ORD_T - 1) / ORD_T, cols), dim3(ORD_T), 0, st, scores, ld, ms, labels, n, C, K, col0, ent, grp);
        MFVIT_CHECK_LAUNCH();
    }
    if (conf) {
        MFVIT_LAUNCH(preds_kernel, dim3((n + 255) / 256, M), dim3(256), 0, st, scores, ld, ms, labels, n, C, preds8, lab8);
        MFVIT_CHECK_LAUNCH();
    }
    const unsigned* sent = stratified ? ent + (long)K * n : nullptr;
    const unsigned* sgrp = stratified ? grp + (long)K * n : nullptr;
    const long long step = 1 << 16;                                     // replicates per launch: the grids stay far below their limits
    for (long long rb = 0; rb < R; rb += step) {
        const int rn = (int)(R - rb < step ? R - rb : step);
        unsigned short* wr = w + rb * L.npad;
        MFVIT_LAUNCH(weights_kernel, dim3(rn), dim3(W_T), (size_t)L.npad * 2, st, n, L.npad, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)(r0 + rb),
                     sent, sgrp, wr);
        MFVIT_CHECK_LAUNCH();
        if (u2) {
            MFVIT_LAUNCH(scan_kernel<false>, dim3((unsigned)(rn * K)), dim3(SCAN_T), (size_t)n * 4, st, ent, grp, wr, L.npad, n, C, K, u2 + rb * K,
                         npos + rb * C, (int*)nullptr, (int*)nullptr);
            MFVIT_CHECK_LAUNCH();
        }
        if (conf) {
            MFVIT_LAUNCH(conf_kernel, dim3(rn), dim3(CONF_T), (size_t)K * C * 4, st, preds8, lab8, wr, L.npad, n, C, M, conf + rb * K * C);
            MFVIT_CHECK_LAUNCH();
        }
    }
    return MFVIT_OK;
}

int delong_counts(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, void* work, size_t work_bytes, int* v2,
                  unsigned long long* pos_xy, unsigned long long* neg_xy, unsigned long long* u2, unsigned long long* npos, hipStream_t st) {
    if (!scores_ok(scores, ld, ms, labels, n, C, M, work) || !pos_xy || !neg_xy || !u2 || !npos) return MFVIT_EINVAL;
    const BootWork L = boot_layout(n, C, M, 1);
    if (work_bytes < L.total) return MFVIT_EINVAL;
    MFVIT_TRY(allow_big_lds());
    char* wk = (char*)work;
    unsigned* ent = (unsigned*)(wk + L.ent);
    unsigned* grp = (unsigned*)(wk + L.grp);
    int* v2w = (int*)(wk + L.tail);
    const int K = M * C;
    MFVIT_LAUNCH(order_kernel, dim3((n + ORD_T - 1) / ORD_T, K), dim3(ORD_T), 0, st, scores, ld, ms, labels, n, C, K, 0, ent, grp);
    MFVIT_CHECK_LAUNCH();
    MFVIT_LAUNCH(scan_kernel<true>, dim3(K), dim3(SCAN_T), (size_t)n * 4, st, ent, grp, (const unsigned short*)nullptr, L.npad, n, C, K, u2, npos, v2w, v2);
    MFVIT_CHECK_LAUNCH();
    MFVIT_LAUNCH(moments_kernel, dim3(M * M, C), dim3(MOM_T), 0, st, v2w, labels, n, C, M, pos_xy, neg_xy);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int curve_counts(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, void* work, size_t work_bytes, float* thr,
                 unsigned* tp, unsigned* fp, int* nthr, int* nnan, unsigned long long* npos, hipStream_t st) {
    if (!scores_ok(scores, ld, ms, labels, n, C, M, work) || !thr || !tp || !fp || !nthr || !nnan || !npos) return MFVIT_EINVAL;
    const BootWork L = boot_layout(n, C, M, 1);
    if (work_bytes < L.total) return MFVIT_EINVAL;
    MFVIT_TRY(allow_big_lds());
    char* wk = (char*)work;
    unsigned* ent = (unsigned*)(wk + L.ent);
    unsigned* grp = (unsigned*)(wk + L.grp);
    const int K = M * C;
    MFVIT_LAUNCH(order_kernel, dim3((n + ORD_T - 1) / ORD_T, K), dim3(ORD_T), 0, st, scores, ld, ms, labels, n, C, K, 0, ent, grp);
    MFVIT_CHECK_LAUNCH();
    MFVIT_LAUNCH(curve_kernel, dim3(K), dim3(SCAN_T), (size_t)n * 4, st, scores, ld, ms, ent, grp, n, C, thr, tp, fp, nthr, nnan, npos);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

int boot_points(const float* scores, long ld, long ms, const int64_t* labels, int n, int C, int M, unsigned long long seed, long long r0, long long R,
                int stratified, const int* req, int Q, void* work, size_t work_bytes, unsigned* tp, unsigned* fp, float* thr, unsigned long long* npos,
                hipStream_t st) {
    if (!scores_ok(scores, ld, ms, labels, n, C, M, work) || !req || !tp || !fp || !thr || !npos) return MFVIT_EINVAL;
    if (R < 1 || r0 < 0 || r0 + R > (1ll << 31) || (stratified != 0 && stratified != 1) || Q < 1 || Q > PTS_MAXQ) return MFVIT_EINVAL;
    const BootWork L = boot_layout(n, C, M, R);
    if (work_bytes < L.total) return MFVIT_EINVAL;
    MFVIT_TRY(allow_big_lds());
    char* wk = (char*)work;
    unsigned* ent = (unsigned*)(wk + L.ent);
    unsigned* grp = (unsigned*)(wk + L.grp);
    unsigned short* w = (unsigned short*)(wk + L.tail);
    const int K = M * C;
    MFVIT_LAUNCH(order_kernel, dim3((n + ORD_T - 1) / ORD_T, K + (stratified ? 1 : 0)), dim3(ORD_T), 0, st, scores, ld, ms, labels, n, C, K, 0, ent, grp);
    MFVIT_CHECK_LAUNCH();
    const unsigned* sent = stratified ? ent + (long)K * n : nullptr;
    const unsigned* sgrp = stratified ? grp + (long)K * n : nullptr;
    const long long step = 1 << 16;                                     // replicates per launch, as boot_counts
    for (long long rb = 0; rb < R; rb += step) {
        const int rn = (int)(R - rb < step ? R - rb : step);
        unsigned short* wr = w + rb * L.npad;
        MFVIT_LAUNCH(weights_kernel, dim3(rn), dim3(W_T), (size_t)L.npad * 2, st, n, L.npad, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)(r0 + rb),
                     sent, sgrp, wr);
        MFVIT_CHECK_LAUNCH();
        const long long ob = rb * K * Q;
        MFVIT_LAUNCH(points_kernel, dim3((unsigned)(rn * K)), dim3(SCAN_T), (size_t)n * 4, st, scores, ld, ms, ent, grp, wr, L.npad, n, C, K, req, Q,
                     tp + ob, fp + ob, thr + ob, npos + rb * C);
        MFVIT_CHECK_LAUNCH();
    }
    return MFVIT_OK;
}

int calib_sums(const float* logits, long ld, long ms, const int64_t* labels, int n, int C, int M, const float* temps, int Kt, int NB,
               unsigned long long* bin_n, unsigned long long* bin_hit, double* bin_conf, double* sums, unsigned long long* skipped, hipStream_t st) {
    if (!logits || !labels || !temps || !bin_n || !bin_hit || !bin_conf || !sums || !skipped || !boot_shape_ok(n, C, M)) return MFVIT_EINVAL;
    if (ld < C || (M > 1 && ms < (long)(n - 1) * ld + C) || Kt < 1 || Kt > CAL_MAXK || NB < 1 || NB > CAL_MAXB) return MFVIT_EINVAL;
    CalTemps t = {};
    for (int k = 0; k < Kt; ++k) {
        if (!(temps[k] > 0.f) || !std::isfinite(temps[k])) return MFVIT_EINVAL;
        t.t[k] = temps[k];
    }
    MFVIT_TRY(allow_big_lds());
    MFVIT_LAUNCH(calib_kernel, dim3(M * Kt), dim3(CAL_T), calib_lds_bytes(NB), st, logits, ld, ms, labels, n, C, t, Kt, NB, bin_n, bin_hit, bin_conf, sums,
                 skipped);
    MFVIT_CHECK_LAUNCH();
    return MFVIT_OK;
}

}  // namespace mfvit
