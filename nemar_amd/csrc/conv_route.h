// Route plans of the three convolution operators: WHICH kernel family serves a call and with which workspace layout, decided once, on
// the host, without a launch or a device pointer.  conv.hip's operators switch on the plan, and every host-side size query
// (nemar_conv2d_*_workspace, _scratch, _gy_planes_bytes, _bwd_data_fusable, _bwd_data_addend_ok) asks the same planning code with the
// canonical call-time facts filled in.  DESIGN.md "Convolution routes" is the table read off this file.
//
// Part of conv.hip's translation unit (the route switches below are what its nemar_tune sets): no other file may include it.
#pragma once
#ifndef NEMAR_CONV_HIP
#error "conv_route.h holds conv.hip's own switches: include it from conv.hip only"
#endif
#include "common.h"
#include "conv_exact.h"
#include "conv_split16.h"
#include "conv_s16g.h"
#include "conv_k7.h"

// conv_narrow.hip: VALU + LDS-halo kernels for layers with <= 4 output channels
bool nemar_narrow_eligible(int K, int C1, int R, int S, int stride, int N, int OH, int OW);
int nemar_narrow_wgrad_splits(int N, int C, int OH, int OW);
// conv_wgrad.hip: wave-specialised weight gradient for wide layers
bool nemar_wgrad2_eligible(int K, int OH, int OW, bool gy_aligned16);
void nemar_wgrad2_plan(int K, int J, int P, int target_blocks, int* splits_out, int* pix_per_split_out);

using namespace nemar_exact;

namespace {

// The route switches (nemar_tune keys; the measurements behind the defaults are in DESIGN.md 4c - 4i)
static NEMAR_SWITCH(int, g_split16, 1);                // 20: wide 3x3 / 4x4 stride-1 layers on the split-16 kernels when the call brings a large-enough arena
static NEMAR_SWITCH(long long, g_split16_min_mmac, 2000);   // 23: ... from this many million multiply-adds (below, the extra launches cost more than they save)
static NEMAR_SWITCH(int, g_split16_variant, 4);        // 21: 4 = fp16 x 3 products (default), 3 = bf16 x 6 products
static NEMAR_SWITCH(int, g_k7, 1);                     // 33: the 7x7 stem / head layers (<= 4 channels on one side) on the 16-bit matrix pipe (conv_k7.hip)
static NEMAR_SWITCH(int, g_s16g, 1);                   // 24: general layers on the 16-bit matrix pipe with the in-kernel operand split (conv_s16g.hip)
static NEMAR_SWITCH(long long, g_s16g_min_mmac, 30);   // 25: ... from this many million multiply-adds (tiny layers are launch-bound either way)
static NEMAR_SWITCH(int, g_s16g_wgrad, 1);             // 29: weight gradients on the in-kernel-split kernels (conv_s16g_wgrad.hip)
static NEMAR_SWITCH(int, g_s16g_wgrad_first, 0);       // 26: 1 = ... also those of the wide residual-block layers (faster alone, slower inside a step: off)
static NEMAR_SWITCH(int, g_s16g_fold, 1);              // 30: stride-1 reflect data gradients on the padded domain + fold
static NEMAR_SWITCH(int, g_split_act, 1);              // 36: reduction-split forward layers with a fused ReLU / LeakyReLU (activation in the sum pass)
static NEMAR_SWITCH(int, g_fold_small, 1);             // 43: stride-1 reflect data gradients of tiny maps on the exact route: padded domain + sum-and-fold pass
static NEMAR_SWITCH(int, g_dual_gy, 1);                // 35: the data-gradient call's split pass also writes the weight gradient's gy planes
static NEMAR_SWITCH(int, g_reflect_aux, 1);            // 8: 3x3 reflect data gradient folds the border into the main launch (1) / ring launch (0)
static NEMAR_SWITCH(int, g_deterministic, 1);          // 14: 1 = split reductions through per-split slabs summed in order (bitwise reproducible), 0 = fp32 atomics
static NEMAR_SWITCH(int, g_ksplit, 1);                 // 12: allow reduction splits on the exact route
static NEMAR_SWITCH(int, g_narrow, 1);                 // 3: <= 4-channel layers on the VALU kernels
static NEMAR_SWITCH(int, g_wgrad, 0);                  // 4: 0 = wave-specialised weight gradient, 1 = VGPR-staged kernel, 2 = wave-specialised without 16-byte source loads
static NEMAR_SWITCH(int, g_wgrad_blocks, 512);         // 5: workgroups targeted by its pixel split

enum { ROUTE_EXACT = 0, ROUTE_NARROW = 1, ROUTE_SPLIT16 = 2, ROUTE_S16G = 3, ROUTE_K7 = 4 };      // the kernel families (nemar_last_route)

// A layer as every operator sees it: x [N, C0 + C1, H, W] -> y / gy [N, K, OH, OW]
struct ConvShape {
    int N, C0, C1, H, W, K, R, S, stride, pad, pad_mode;
    int oh = 0, ow = 0;           // the weight gradient is told the size of gy
    int C() const { return C0 + C1; }
    int OH() const { return oh ? oh : (H + 2 * pad - R) / stride + 1; }
    int OW() const { return ow ? ow : (W + 2 * pad - S) / stride + 1; }
    bool refl() const { return pad_mode == BORDER_REFLECT && pad > 0; }
    long long macs() const { return (long long)N * OH() * OW() * K * C() * R * S; }
};
// What a route may depend on besides the shape.  The size queries plan with canonical(): the defaults + a large-enough arena and gy-planes buffer.
struct ConvFacts {
    bool bias = false;
    int act = ACT_NONE;
    float slope = 0.f;
    bool gx0 = true, gx1 = false;           // data gradient: destinations present
    bool part = true;                       // weight gradient: slabs of the fixed-order reduction exist (g_deterministic)
    size_t scratch_bytes = 0;               // the call's arena (0: none)
    size_t gy_planes_bytes = 0;             // data gradient: room offered for the weight gradient's gy planes (0: none)
    bool gy_aligned = true, part_aligned = true;      // weight gradient: gy / the workspace on a 16-byte boundary
    static ConvFacts canonical() { ConvFacts f; f.scratch_bytes = f.gy_planes_bytes = ~(size_t)0; return f; }
};

inline void grow(size_t& a, size_t b) { if (b > a) a = b; }
constexpr int WBK = 32;           // pixels per LDS stage of wgrad_kernel (conv.hip)
constexpr int BIAS_CHUNK = 4096;  // plane elements per workgroup of bias_grad_kernel

// Reduction split for tiny, deep problems on the generic kernels: enough splits for ~256 workgroups, >= 4 stages each.
int small_problem_split(int M, int P, int Kred) {
    const TileChoice t = igemm_tile(M, P, nemar_cdiv(Kred, BK));
    if (t.bm == 128) return 1;
    const long long tiles = (long long)nemar_cdiv(M, t.bm) * nemar_cdiv(P, t.bn);
    const int stages = nemar_cdiv(Kred, BK);
    if (tiles >= 128 || stages < 16) return 1;
    int ks = nemar_cdiv(256, (int)tiles);
    if (ks > stages / 4) ks = stages / 4;
    return ks < 1 ? 1 : ks;
}

void fwd_taps(TapTable& t, int R, int S, int pad) {
    t.n = R * S;
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < S; ++s) {
            t.dy[r * S + s] = (short)(r - pad);
            t.dx[r * S + s] = (short)(s - pad);
            t.dyx[r * S + s] = ((r - pad) << 16) | ((s - pad) & 0xffff);
            t.wofs[r * S + s] = r * S + s;
        }
}

// taps of output-pixel parity class (ph, pw) of a stride-`stride` data gradient: r with (ph + pad - r) % stride == 0
void dgrad_taps(TapTable& t, int R, int S, int pad, int stride, int ph, int pw) {
    t.n = 0;
    for (int r = 0; r < R; ++r) {
        if ((ph + pad - r) % stride != 0) continue;
        for (int s = 0; s < S; ++s) {
            if ((pw + pad - s) % stride != 0) continue;
            t.dy[t.n] = (short)((ph + pad - r) / stride);
            t.dx[t.n] = (short)((pw + pad - s) / stride);
            t.dyx[t.n] = ((int)t.dy[t.n] << 16) | ((int)t.dx[t.n] & 0xffff);
            t.wofs[t.n] = r * S + s;
            t.n++;
        }
    }
}

// every split of a reduction must own at least one stage (its slab is summed unconditionally)
int normalize_ksplit(int Kred, int ksplit) {
    if (ksplit <= 1) return 1;
    const int nk_all = nemar_cdiv(Kred, BK);
    const int nk_per = nemar_cdiv(nk_all, ksplit);
    return nemar_cdiv(nk_all, nk_per);
}

// Could the wide (split-16) route of each operator take this shape, whatever a call brings?  Asked with the default operand format and zero
// padding: the per-shape sizes (packed images, the arena) are taken for these candidates; a call tests its own padding mode and format.
struct WideCandidates { bool fwd, dgrad, wgrad; };
WideCandidates wide_candidates(const ConvShape& s) {
    return {nemar_split16_eligible(s.N, s.H, s.W, s.K, s.C(), s.R, s.S, s.stride, s.pad, SPLIT16_ZERO, 4),
            nemar_split16_eligible(s.N, s.H, s.W, s.C(), s.K, s.R, s.S, s.stride, s.pad, SPLIT16_ZERO, 4),
            nemar_split16_wgrad_eligible(s.N, s.C(), s.H, s.W, s.K, s.R, s.S, s.stride, s.pad)};
}
bool split16_worth_it(int N, int OH, int OW, int K, int C, int R, int S) {
    return (long long)N * OH * OW * K * C * R * S >= g_split16_min_mmac * 1000000ll;
}

// ---- problems of conv_s16g.hip (general layers on the 16-bit matrix pipe): geometry only, the operator fills the pointers ------------
void s16g_set_class(S16gProblem& q, int c, const TapTable& t, int OHc, int OWc, int ooy, int oox) {
    q.ntaps[c] = t.n;
    for (int i = 0; i < t.n && i < S16G_MAX_TAPS; ++i) { q.dy[c][i] = t.dy[i]; q.dx[c][i] = t.dx[i]; q.wofs[c][i] = t.wofs[i]; }
    q.OH[c] = OHc; q.OW[c] = OWc; q.ooy[c] = ooy; q.oox[c] = oox;
}
bool s16g_worth_it(long long macs) { return g_s16g && macs >= g_s16g_min_mmac * 1000000ll; }

// forward; false = not this route
bool s16g_fwd_problem(S16gProblem& q, S16gPlan& pl, int N, int C0, int C1, int H, int W, int K, int R, int S, int stride, int pad,
                      int pad_mode, int act, float slope) {
    const int C = C0 + C1;
    if (R * S > S16G_MAX_TAPS || stride > 2 || stride < 1) return false;
    const int OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
    if (OH <= 0 || OW <= 0 || !s16g_worth_it((long long)N * OH * OW * K * C * R * S)) return false;
    q = S16gProblem();
    q.C0 = C0; q.C1 = C1; q.Hs = H; q.Ws = W; q.N = N; q.M = K; q.M0 = K;
    q.act = act; q.slope = slope; q.border = pad_mode; q.sstride = stride;
    q.OHf = OH; q.OWf = OW; q.osy = 1; q.osx = 1; q.ncls = 1;
    TapTable t;
    fwd_taps(t, R, S, pad);
    s16g_set_class(q, 0, t, OH, OW, 0, 0);
    pl = nemar_s16g_plan(q);
    return pl.ok != 0;
}

// data gradient / transposed convolution (zero padding): one class per output parity
bool s16g_dgrad_problem(S16gProblem& q, S16gPlan& pl, int N, int C, int mskip, int H, int W, int K, int OH, int OW, int R, int S,
                        int stride, int pad, int act, float slope) {
    if (R * S > S16G_MAX_TAPS || stride > 2 || stride < 1) return false;
    if (!s16g_worth_it((long long)N * OH * OW * K * (C - mskip) * R * S)) return false;
    q = S16gProblem();
    q.C0 = K; q.C1 = 0; q.Hs = OH; q.Ws = OW; q.N = N; q.M = C - mskip;
    q.act = act; q.slope = slope; q.border = BORDER_ZERO; q.sstride = 1;
    q.OHf = H; q.OWf = W; q.osy = stride; q.osx = stride; q.ncls = 0;
    for (int ph = 0; ph < stride; ++ph)
        for (int pw = 0; pw < stride; ++pw) {
            TapTable t;
            dgrad_taps(t, R, S, pad, stride, ph, pw);
            const int OHc = (H - ph + stride - 1) / stride, OWc = (W - pw + stride - 1) / stride;
            if (t.n == 0 || OHc <= 0 || OWc <= 0 || t.n > (stride > 1 ? S16G_CLS_TAPS : S16G_MAX_TAPS)) return false;
            s16g_set_class(q, q.ncls++, t, OHc, OWc, ph, pw);
        }
    pl = nemar_s16g_plan(q);
    return pl.ok != 0;
}

// ---- 7x7 / pad-3 layers with <= 4 channels on the OUTPUT side: a SEVEN-TAP VERTICAL convolution with the 32 (k, dx) pairs as
// output channels on the general 16-bit-pipe kernel, P = [N][32][PH][PW] over src = [N][Cb][Hs][Ws] seen through a border of `spad` (3; 6, zero:
// reflect gradient on the padded domain), then a horizontal shift-sum (conv.hip).  Workspace: [re-arranged weights][their packed image][P].
struct K7MfPlan {
    S16gProblem q;
    S16gPlan pl;
    size_t wt_off, pack_off, p_off, total;      // floats
    int PH, PW;
    bool ok;
};
K7MfPlan k7_mf_plan(int N, int Cb, int Hs, int Ws, int spad, int border) {
    K7MfPlan m;
    m.ok = false;
    m.PH = Hs + 2 * spad - 6;
    m.PW = Ws + 2 * spad;
    S16gProblem& q = m.q;
    q = S16gProblem();
    q.C0 = Cb; q.C1 = 0; q.Hs = Hs; q.Ws = Ws; q.N = N; q.M = 32; q.M0 = 32;
    q.act = ACT_NONE; q.slope = 0.f; q.border = border; q.sstride = 1;
    q.OHf = m.PH; q.OWf = m.PW; q.osy = 1; q.osx = 1; q.ncls = 1;
    TapTable t;
    t.n = 7;
    for (int i = 0; i < 7; ++i) { t.dy[i] = (short)(i - spad); t.dx[i] = (short)(-spad); t.dyx[i] = ((i - spad) << 16) | ((-spad) & 0xffff); t.wofs[i] = i; }
    s16g_set_class(q, 0, t, m.PH, m.PW, 0, 0);
    m.pl = nemar_s16g_plan(q);
    if (!m.pl.ok) return m;
    m.wt_off = 0;
    m.pack_off = ((size_t)32 * Cb * 7 + 3) & ~(size_t)3;
    m.p_off = (m.pack_off + (nemar_s16g_pack_bytes(q, m.pl) + 3) / 4 + 3) & ~(size_t)3;
    m.total = m.p_off + (size_t)N * 32 * m.PH * m.PW;
    m.ok = true;
    return m;
}
bool k7_mf_eligible(int Cb, int Ks, int R, int S, int stride, int pad) {
    return g_k7 && R == 7 && S == 7 && stride == 1 && pad == 3 && Ks >= 1 && Ks <= 4 && Cb >= 16 && Cb % 16 == 0;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
// Workspace (floats): [packed weights][slabs of a split reduction (tiny, deep layers)].  The sizes cover EVERY route the shape could take (the
// caller caches them per shape, prepacked weight images live at these offsets): they do not depend on the call-time facts.
struct FwdPlan {
    int route;
    enum Sub { PLAIN, K7_MANY_FEW, K7_FEW_MANY, SPLIT, SPLIT_ACT } sub;      // 7x7 head / stem; exact: reduction split, its activation in the sum pass
    size_t pack, slab_off, total;       // floats
    int ksplit;                         // of the split candidate (the exact route uses it under SPLIT / SPLIT_ACT)
    K7MfPlan k7;                        // K7_MANY_FEW
    S16gProblem q; S16gPlan pl;         // ROUTE_S16G
};
FwdPlan plan_fwd(const ConvShape& s, const ConvFacts& f) {
    FwdPlan P;
    const int N = s.N, H = s.H, W = s.W, K = s.K, C = s.C(), R = s.R, S = s.S, stride = s.stride, pad = s.pad, OH = s.OH(), OW = s.OW();
    // -- what the shape could need
    P.pack = packed_floats(K, C * R * S);
    if (wide_candidates(s).fwd)      // room for either packed image
        grow(P.pack, (nemar_split16_pack_bytes(K, C, R) + 3) / 4);
    if (s16g_fwd_problem(P.q, P.pl, N, C, 0, H, W, K, R, S, stride, pad, BORDER_ZERO, ACT_NONE, 0.f))
        grow(P.pack, (nemar_s16g_pack_bytes(P.q, P.pl) + 3) / 4);
    const bool k7_fm = nemar_k7_fm_eligible(C, K, R, S, stride, pad);
    if (k7_fm) grow(P.pack, nemar_k7_fm_pack_floats(K));
    P.ksplit = 1;
    if (g_ksplit && OH > 0 && OW > 0 && K > 4) P.ksplit = normalize_ksplit(C * R * S, small_problem_split(K, N * OH * OW, C * R * S));
    P.slab_off = (P.pack + 3) & ~(size_t)3;
    P.total = P.slab_off + (P.ksplit > 1 ? (size_t)P.ksplit * N * K * OH * OW : 0);
    P.k7.ok = false;
    if (k7_mf_eligible(C, K, R, S, stride, pad)) {           // 7x7 head: [re-arranged weights | packed image | P]; sized with a zero border
        P.k7 = k7_mf_plan(N, C, H, W, 3, BORDER_ZERO);
        if (P.k7.ok) grow(P.total, P.k7.total);
        if (s.pad_mode != BORDER_ZERO) P.k7 = k7_mf_plan(N, C, H, W, 3, s.pad_mode);
    }
    // -- what this call takes
    const int mode = s.pad_mode == BORDER_REFLECT ? SPLIT16_REFLECT : SPLIT16_ZERO;
    P.sub = FwdPlan::PLAIN;
    if (s.C1 == 0 && P.k7.ok) { P.route = ROUTE_K7; P.sub = FwdPlan::K7_MANY_FEW; }
    else if (g_k7 && s.C1 == 0 && f.act != ACT_TANH && k7_fm) { P.route = ROUTE_K7; P.sub = FwdPlan::K7_FEW_MANY; }
    else if (nemar_narrow_eligible(K, s.C1, R, S, stride, N, OH, OW) && g_narrow) P.route = ROUTE_NARROW;
    else if (g_split16 && s.C1 == 0 && f.act == ACT_NONE && split16_worth_it(N, OH, OW, K, C, R, S) &&
             nemar_split16_eligible(N, H, W, K, C, R, S, stride, pad, mode, g_split16_variant) &&
             f.scratch_bytes && f.scratch_bytes >= nemar_split16_scratch_total(N, H, W, K, C, OH, OW)) P.route = ROUTE_SPLIT16;
    else if (s16g_fwd_problem(P.q, P.pl, N, s.C0, s.C1, H, W, K, R, S, stride, pad, s.pad_mode, f.act, f.slope)) P.route = ROUTE_S16G;
    else {
        // a layer with a fused ReLU / LeakyReLU splits too: the activation is applied by the sum pass (nemar_sum_partials_act)
        const bool split_act = g_split_act && (f.act == ACT_RELU || f.act == ACT_LRELU);
        P.route = ROUTE_EXACT;
        if (P.ksplit > 1 && (f.act == ACT_NONE || split_act)) P.sub = split_act ? FwdPlan::SPLIT_ACT : FwdPlan::SPLIT;
    }
    return P;
}

// ---- data gradient -------------------------------------------------------------------------------------------------------------------
// Workspace (floats): [packed weights x stride^2 parity classes][padded-domain scratch][flipped weights (C <= 4)][border-ring gradient][its slabs]
// [ksplit slabs][aux rows][aux columns], or the 7x7 layers' own (K7MfPlan; head: [packed weights | padded-domain gradient]); total = the largest.
struct DgradPlan {
    int route;
    enum Sub { K7_MANY_FEW, K7_FEW_MANY, SPLIT16, S16G, S16G_FOLD, EXACT } sub;
    size_t pack_stride, padded_off, w2_off, ring_off, ring_slab_off, slab_off, aux_rows_off, aux_cols_off, total;
    int ring_len, ksplit, ring_ksplit;
    bool ring, fold, fold16, fold_small;  // exact family, stride-1 reflect: interior + border ring / padded domain + fold; fold16: S16G_FOLD can take it
    int k7_fold;                          // K7_*, reflect: 0 none, 1 inside the kernel / the shift-sum pass, 2 padded-domain gradient + fold pass
    bool want_gy_planes;                  // SPLIT16: hand gy_planes_out to the split pass (whether it writes them is its own decision: Split16Done)
    size_t gy_planes_need;                // ... bytes of the planes it would then write in the default operand format (nemar_conv2d_gy_planes_bytes)
    int split16_ksplit;                   // SPLIT16: reduction runs per tile (1: the fused epilogue takes addend / out_max)
    int mskip;                            // first output row (C0 when gx0 is absent)
    bool narrow;                          // EXACT: <= 4 input channels, the correlation on the narrow VALU kernel (route id stays exact)
    bool split;                           // EXACT: this call's main launch writes ksplit slabs
    bool aux_rows;                        // EXACT, ring: the border may fold into the main launch — if route_ws2 picks the 16-byte-load kernel (operator)
    K7MfPlan k7;                          // K7_MANY_FEW
    S16gProblem q; S16gPlan pl;           // S16G, S16G_FOLD
};
DgradPlan plan_dgrad(const ConvShape& s, const ConvFacts& f) {
    DgradPlan L;
    const int N = s.N, C = s.C(), H = s.H, W = s.W, K = s.K, R = s.R, S = s.S, stride = s.stride, pad = s.pad, OH = s.OH(), OW = s.OW();
    const bool refl = s.refl();
    // -- what the shape could need
    L.ring = refl && stride == 1;
    L.fold = refl && !L.ring;
    L.pack_stride = packed_floats(C, K * R * S);             // upper bound over parity classes and channel skips
    if (wide_candidates(s).dgrad)     // room for either packed image
        grow(L.pack_stride, (nemar_split16_pack_bytes(C, K, R) + 3) / 4);
    // the general 16-bit-pipe kernel's problem of this layer, built here once.  Zero padding: the layer as it is, one class per parity.  Stride-1
    // reflect (<= 9 taps): the data gradient of the PADDED input (a zero-padded full correlation on the (H + 2p) x (W + 2p) domain), then the fold
    bool s16g = false;
    L.fold16 = false;
    if (!refl && OH > 0 && OW > 0 && s16g_dgrad_problem(L.q, L.pl, N, C, 0, H, W, K, OH, OW, R, S, stride, pad, ACT_NONE, 0.f)) {
        s16g = true;
        grow(L.pack_stride, ((nemar_s16g_pack_bytes(L.q, L.pl) + 3) / 4 + stride * stride - 1) / (stride * stride));
    } else if (L.ring && g_s16g_fold && R * S <= 9 && OH > 0 && OW > 0 &&
               s16g_dgrad_problem(L.q, L.pl, N, C, 0, H + 2 * pad, W + 2 * pad, K, OH, OW, R, S, 1, 0, ACT_NONE, 0.f)) {
        L.fold16 = true;
        grow(L.pack_stride, (nemar_s16g_pack_bytes(L.q, L.pl) + 3) / 4);
    }
    // tiny stride-1 reflect layers that stay on the exact-fp32 kernels: the padded-domain form as well — ONE split launch over the padded domain, then
    // ONE pass that sums the slabs and folds the mirrored border (nemar_sum_partials_fold) instead of the ring form's five small launches
    L.fold_small = L.ring && !L.fold16 && g_fold_small && g_ksplit && C > 4 && (H + 2 * pad) * (W + 2 * pad) <= 1296;
    if (L.fold_small) { L.ring = false; L.fold = true; }
    size_t o = L.pack_stride * (size_t)(stride * stride);
    L.padded_off = o;
    if (L.fold || L.fold16) o += (size_t)N * C * (H + 2 * pad) * (W + 2 * pad);
    L.w2_off = o;
    if (C <= 4) o += (size_t)C * K * R * S;
    L.ring_off = o;
    L.ring_len = L.ring ? 2 * pad * (W + 2 * pad) + 2 * pad * H : 0;
    o += (size_t)N * C * L.ring_len;
    // a ring tile is a few pixels deep in a full-length reduction: split it until ~1.5 workgroups per CU exist (each split = one slab, summed in order)
    L.ring_ksplit = 1;
    L.ring_slab_off = o;
    if (L.ring) {
        const int tiles = nemar_cdiv(N * L.ring_len, 64) * nemar_cdiv(C, 64), stages = nemar_cdiv(K * R * S, BK);
        int ks = nemar_cdiv(384, tiles);
        if (ks > nemar_cdiv(stages, 8)) ks = nemar_cdiv(stages, 8);
        L.ring_ksplit = normalize_ksplit(K * R * S, ks < 1 ? 1 : ks);
        if (L.ring_ksplit > 1) o += (size_t)L.ring_ksplit * N * C * L.ring_len;
    }
    // split reductions (stride 1; whether THIS call splits is L.split below): few, deep 128x128 tiles (D's 256->512 k4 layer) get one workgroup
    // per CU; tiny deep problems on the generic kernels ~256 workgroups of >= 4 stages
    L.ksplit = 1;
    const int Hs = L.fold_small ? H + 2 * pad : H, Wsl = L.fold_small ? W + 2 * pad : W;      // the domain the split launch covers
    if (g_ksplit && stride == 1 && (!L.fold || L.fold_small) && C > 4) {
        const int P = N * Hs * Wsl, Kred = K * R * S, stages = nemar_cdiv(Kred, BK);
        if (g_cfg128 == 0 && C > 64 && K % BK == 0) {
            const long long tiles = (long long)nemar_cdiv(C, 128) * nemar_cdiv(P, 128);
            if (tiles < 200 && stages >= 256) {
                int ks = nemar_cdiv(256, (int)tiles);
                if (ks > stages / 128) ks = stages / 128;
                if (ks > 1) L.ksplit = ks;
            }
        }
        if (L.ksplit == 1) L.ksplit = small_problem_split(C, P, Kred);
        L.ksplit = normalize_ksplit(Kred, L.ksplit);
    }
    L.slab_off = o;
    if (L.ksplit > 1) o += (size_t)L.ksplit * N * C * Hs * Wsl;
    // side buffers of the ring-free reflect data gradient (source = gy [N,K,H,W] for a 3x3 / pad 1 layer)
    const bool aux = L.ring && pad == 1 && R == 3 && S == 3;
    L.aux_rows_off = o;
    if (aux) o += 6ull * N * K * W;
    L.aux_cols_off = o;
    if (aux) o += 8ull * N * K * H;
    L.total = o;
    L.k7.ok = false;
    if (k7_mf_eligible(K, C, R, S, stride, pad)) {                       // 7x7 stem (<= 4 input channels): gy through a 3- / 6-texel zero border
        L.k7 = k7_mf_plan(N, K, OH, OW, refl ? 6 : 3, BORDER_ZERO);
        if (L.k7.ok) grow(L.total, L.k7.total);
    }
    const bool k7_fm = C > 4 && nemar_k7_fm_eligible(K, C, R, S, stride, pad);      // 7x7 head (<= 4 output channels)
    if (k7_fm) grow(L.total, ((nemar_k7_fm_pack_floats(C) + 3) & ~(size_t)3) + (refl ? (size_t)N * C * (H + 6) * (W + 6) : 0));
    // -- what this call takes
    const bool one_plain = s.C1 == 0 && f.gx0 && !f.bias && f.act == ACT_NONE;      // one destination, no epilogue
    const int mode = refl ? SPLIT16_DGRAD_REFLECT : SPLIT16_ZERO;
    L.mskip = f.gx0 ? 0 : s.C0;
    // a skipped first destination or a tanh makes another s16g problem than the one above; any other epilogue rides on it (nemar_s16g_plan
    // reads q.act for its tanh refusal only — noted there)
    const bool own_problem = L.mskip != 0 || f.act == ACT_TANH;
    L.k7_fold = 0; L.want_gy_planes = false; L.gy_planes_need = 0; L.split16_ksplit = 0; L.narrow = L.split = L.aux_rows = false;
    if (one_plain && L.k7.ok) {
        L.route = ROUTE_K7; L.sub = DgradPlan::K7_MANY_FEW; L.k7_fold = refl ? 1 : 0;
    } else if (g_k7 && one_plain && k7_fm) {
        L.route = ROUTE_K7; L.sub = DgradPlan::K7_FEW_MANY; L.k7_fold = !refl ? 0 : nemar_k7_fm_fold_ok(H, W) ? 1 : 2;
    } else if (g_split16 && one_plain && split16_worth_it(N, OH, OW, K, C, R, S) &&
               nemar_split16_eligible(N, H, W, C, K, R, S, stride, pad, mode, g_split16_variant) &&
               f.scratch_bytes && f.scratch_bytes >= nemar_split16_scratch_total(N, H, W, C, K, H, W)) {
        L.route = ROUTE_SPLIT16; L.sub = DgradPlan::SPLIT16;
        const size_t gb = nemar_split16_wgrad_g_bytes(N, H, W, K, R);      // (the weight gradient that follows takes its gy planes from this call's split pass)
        L.want_gy_planes = g_dual_gy && R == 3 && f.gy_planes_bytes && f.gy_planes_bytes >= gb && gb > 0 &&
                           nemar_split16_wgrad_eligible(N, C, H, W, K, R, S, stride, pad);
        L.gy_planes_need = L.want_gy_planes && g_split16_variant == 4 ? gb : 0;
        L.split16_ksplit = nemar_split16_ksplit(N, H, W, C, K);
    } else if (!refl && (own_problem ? s16g_dgrad_problem(L.q, L.pl, N, C, L.mskip, H, W, K, OH, OW, R, S, stride, pad, f.act, f.slope) : s16g)) {
        L.route = ROUTE_S16G; L.sub = DgradPlan::S16G;
        L.q.act = f.act; L.q.slope = f.slope;
    } else if (L.fold16 && f.gx0 && !f.gx1 && !f.bias && f.act == ACT_NONE) {
        L.route = ROUTE_S16G; L.sub = DgradPlan::S16G_FOLD;
    } else {
        L.route = ROUTE_EXACT; L.sub = DgradPlan::EXACT;
        L.narrow = g_narrow && stride == 1 && !L.fold && !f.bias && f.act == ACT_NONE && L.mskip == 0 && !f.gx1 && R - 1 - pad >= 0 &&
                   nemar_narrow_eligible(C, 0, R, S, 1, N, H, W);
        L.split = !L.narrow && L.ksplit > 1 && !f.bias && f.act == ACT_NONE && L.mskip == 0 &&
                  (L.fold ? (f.gx0 && !f.gx1) : (!f.gx1 || (f.gx0 && !L.ring)));
        L.aux_rows = !L.narrow && L.ring && g_reflect_aux && pad == 1 && R == 3 && S == 3 && H >= 4 && W >= 8;
    }
    return L;
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------------------
void legacy_wgrad_plan(int K, int J, int P, int* splits_out, int* pix_per_split_out) {
    const bool wide = K > 32;
    const int BM = wide ? 128 : 32, BN = wide ? 128 : 256;
    const int mt = nemar_cdiv(K, BM), jt = nemar_cdiv(J, BN);
    // split the pixel reduction so that ~4 workgroups per CU exist, but keep >= 8 stages per split
    int splits = nemar_cdiv(1024, mt * jt);
    const int max_splits = nemar_cdiv(P, WBK * 8);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    if (splits > 65535) splits = 65535;
    *pix_per_split_out = nemar_cdiv(nemar_cdiv(P, splits), WBK) * WBK;
    *splits_out = nemar_cdiv(P, *pix_per_split_out);
}
// gy planes that are not a multiple of 4 floats (the discriminator's 31x31 / 15x15 maps) cannot be read in aligned 16-byte chunks: gy is copied
// once into planes of OHv >= OH rows with (OHv * OW) % 4 == 0, zero below row OH, and the wave-specialised kernel runs on the virtual OHv x OW map
int padded_rows(int OH, int OW) {
    int ohv = OH;
    while ((ohv * OW) % 4) ++ohv;
    return ohv;
}
bool wgrad_pad_route(int K, int OH, int OW, int pad_mode) {
    return K > 4 && (OH * OW) % 4 != 0 && pad_mode == BORDER_ZERO && g_wgrad != 1;
}

// Workspace (floats): [splits][K * J] slabs of the fixed-order reduction, then what the route keeps behind them (bias_off: [splits][K] bias slabs
// or the partial sums of bias_grad_kernel; gyp_off: the padded copy of gy).  total = the largest over the routes the shape could take.
struct WgradPlan {
    int route;
    enum Sub { K7, NARROW, S16G, SPLIT16, WGRAD2, WGRAD2_PADDED_GY, LEGACY } sub;
    size_t total, bias_off, gyp_off;    // floats
    int splits, pix_per_split, ohv;     // LEGACY: the pixel split; WGRAD2_PADDED_GY: rows of the virtual map
};
WgradPlan plan_wgrad(const ConvShape& s, const ConvFacts& f) {
    WgradPlan P;
    const int N = s.N, C = s.C(), H = s.H, W = s.W, K = s.K, R = s.R, S = s.S, stride = s.stride, pad = s.pad, OH = s.OH(), OW = s.OW();
    const int J = C * R * S, Pix = N * OH * OW, ohv = padded_rows(OH, OW);
    const size_t slab = (size_t)K * J, bias_parts = (size_t)N * nemar_cdiv(OH * OW, BIAS_CHUNK) * K;
    int w2_splits, legacy_splits, pad_splits = 0, pps;
    // -- what the shape could need
    nemar_wgrad2_plan(K, J, Pix, g_wgrad_blocks, &w2_splits, &pps);
    legacy_wgrad_plan(K, J, Pix, &legacy_splits, &P.pix_per_split);
    P.total = (size_t)(w2_splits > legacy_splits ? w2_splits : legacy_splits) * (slab + K);
    if ((OH * OW) % 4 != 0 && K > 4) {          // padded-gy route: slabs of the virtual map + the padded copy of gy
        nemar_wgrad2_plan(K, J, N * ohv * OW, g_wgrad_blocks, &pad_splits, &pps);
        grow(P.total, (size_t)pad_splits * (slab + K) + 4 + (size_t)N * K * ohv * OW);
    }
    if (K <= 4) grow(P.total, (size_t)nemar_narrow_wgrad_splits(N, C, OH, OW) * slab + bias_parts);
    if (nemar_s16g_wgrad_eligible(N, C, 0, H, W, K, OH, OW, R, S, stride, pad, BORDER_ZERO))       // (slab count: same for any channel split)
        grow(P.total, (size_t)nemar_s16g_wgrad_slabs_max(N, C, K, OH, W, stride) * (slab + K));
    const bool k7 = nemar_k7_wgrad_eligible(N, C, H, W, K, R, S, stride, pad);                     // 7x7 stem / head: slabs + max words + bias partials
    if (k7) grow(P.total, nemar_k7_wgrad_floats(N, C, H, W, K) + bias_parts);
    const bool wide = wide_candidates(s).wgrad;              // slabs of the split-16 route + bias partials
    if (wide) grow(P.total, (size_t)nemar_split16_wgrad_splits(N, C, H, W, K, R) * slab + bias_parts);
    // -- what this call takes
    const bool s16g_wg = g_s16g_wgrad && f.part && s16g_worth_it(s.macs()) &&
                         nemar_s16g_wgrad_eligible(N, s.C0, s.C1, H, W, K, OH, OW, R, S, stride, pad, s.pad_mode);
    const bool split16_wg = g_split16 && g_split16_variant == 4 && f.part && s.C1 == 0 && split16_worth_it(N, OH, OW, K, C, R, S) && wide &&
                            (R == 3 || s.pad_mode == BORDER_ZERO) && f.scratch_bytes &&
                            f.scratch_bytes >= nemar_split16_wgrad_scratch_bytes(N, C, H, W, K, R);
    P.bias_off = P.gyp_off = 0; P.splits = 0; P.ohv = ohv;
    if (g_k7 && f.part && s.C1 == 0 && k7) {
        P.route = ROUTE_K7; P.sub = WgradPlan::K7; P.bias_off = nemar_k7_wgrad_floats(N, C, H, W, K);
    } else if (nemar_narrow_eligible(K, s.C1, R, S, stride, N, OH, OW) && g_narrow) {
        P.route = ROUTE_NARROW; P.sub = WgradPlan::NARROW; P.bias_off = (size_t)nemar_narrow_wgrad_splits(N, s.C0, OH, OW) * slab;
    } else if (s16g_wg && (g_s16g_wgrad_first || !split16_wg)) {
        P.route = ROUTE_S16G; P.sub = WgradPlan::S16G;
    } else if (split16_wg) {
        P.route = ROUTE_SPLIT16; P.sub = WgradPlan::SPLIT16; P.bias_off = (size_t)nemar_split16_wgrad_splits(N, C, H, W, K, R) * slab;
    } else {
        P.route = ROUTE_EXACT;
        P.gyp_off = ((size_t)pad_splits * (slab + K) + 3) & ~(size_t)3;       // 16-byte aligned, behind the slabs
        // (the padded copy of gy sits behind the slabs: where the workspace is misaligned it is not made, and the first-generation kernel runs)
        const bool padded_gy = f.part && wgrad_pad_route(K, OH, OW, s.pad_mode) && nemar_wgrad2_eligible(K, ohv, OW, f.part_aligned);
        if (g_wgrad != 1 && nemar_wgrad2_eligible(K, OH, OW, f.gy_aligned)) P.sub = WgradPlan::WGRAD2;
        else if (padded_gy) P.sub = WgradPlan::WGRAD2_PADDED_GY;
        else { P.sub = WgradPlan::LEGACY; P.splits = legacy_splits; P.bias_off = (size_t)legacy_splits * slab; }
    }
    return P;
}

// ---- the arena: bytes of scratch the wide route of ANY of the three operators may want for a layer (nemar_conv2d_scratch; 0: none uses one).
// A per-shape bound the caller sizes its arena with: the candidates above, and the work threshold at the stride-1 output size.
size_t plan_arena_bytes(const ConvShape& s) {
    const int N = s.N, C = s.C(), H = s.H, W = s.W, K = s.K, R = s.R;
    if (!g_split16 || !split16_worth_it(N, H + 2 * s.pad - R + 1, W + 2 * s.pad - s.S + 1, K, C, R, s.S)) return 0;
    const WideCandidates c = wide_candidates(s);
    size_t b = c.fwd ? nemar_split16_scratch_total(N, H, W, K, C, H, W) : 0;
    if (c.dgrad) grow(b, nemar_split16_scratch_total(N, H, W, C, K, H, W));
    if (c.wgrad) grow(b, nemar_split16_wgrad_scratch_bytes(N, C, H, W, K, R));
    return b;
}

}  // namespace
