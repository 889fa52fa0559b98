// Rational-quadratic spline element: the general routine of the stand-alone spline kernels (misc.hip) and the training forward
// (train_spline.hip), the branch-free forward evaluator of the fused GEMM epilogues (gemm_kernel.h, gemm_spline_persistent.hip,
// spline_wide.hip), and the column layout of the spline parameter layer's output.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "common.h"

namespace fc {

// ---------------------------------------------------------------- rational-quadratic spline
// One element: models/spline_coupling.py:24-66 (tails) + :69-169 (spline) + :17-19 (searchsorted).
// u points at 3K+1 parameters [K widths | K heights | K+1 derivative logits] with element stride `us`.
// Quirks reproduced: derivative logits are padded left with log(exp(1-min_d-1)); knot i>=1 uses ud[i-1];
// ud[K] is never used; last knot + 1e-6 only for the bin search; outside [-3,3] identity with logabsdet 0.
constexpr float RQ_BOUND = 3.0f;                                 // tail bound: identity outside [-RQ_BOUND, RQ_BOUND]
constexpr float RQ_MIN_W = 1e-3f, RQ_MIN_H = 1e-3f, RQ_MIN_D = 1e-3f;       // minimum bin width, bin height, knot derivative
constexpr float RQ_PAD_LOGIT = -1e-3f;                           // log(exp(1 - min_derivative - 1)): left pad of the derivative logits
constexpr float RQ_SEARCH_EPS = 1e-6f;                           // added to the last knot, for the bin search only

// v_exp_f32 / v_log_f32 / v_rcp_f32 based helpers (about 1 ulp on the base-2 function): the spline evaluates 16 exponentials,
// 2 softplus, 2 logs and ~10 divisions per element, which made the ocml versions the kernel's dominant VALU cost.
__device__ __forceinline__ float fast_exp(float v) { return __builtin_amdgcn_exp2f(v * 1.4426950408889634f); }
__device__ __forceinline__ float fast_log(float v) { return __builtin_amdgcn_logf(v) * 0.6931471805599453f; }
__device__ __forceinline__ float fast_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }

// Running sums of the spline's softmax terms and bin sizes.  Up to 8 bins: one by one.  16 bins: in blocks of four (a block's terms are added to
// each other, finished blocks to each other, the two once per step).  Fifteen equal bins beside a wide one round the same way at every step of a
// plain chain, which put the knots 8.6 units of 2^-22 from their fp64 places and mid-bin y 3.6e-5 off (tests/test_gpu_spline_edges.py); in
// blocks the same parameters come within 2.5.  K <= 8 keeps the chain and its result bits.  rq_spline_bwd_elem (train_spline.hip) sums the same
// way, so that the training forward and its gradient pick their bins from knots summed alike.
template <int K>
struct rq_prefix {
    float done = 0.f, part = 0.f;
    __device__ __forceinline__ float add(int i, float v) {           // i: position of v (a compile-time constant after unrolling); returns the sum so far
        if (K > 8 && i % 4 == 0) { done += part; part = 0.f; }
        part += v;
        return K > 8 ? done + part : part;
    }
};

// Forward and inverse, with divergent branches for the bin selection.  rq_spline_bwd_elem (train_spline.hip) is the gradient of THIS
// routine's forward direction in its own arithmetic (expf, true division, probabilities kept): merging the two would change training bits.
template <int K>
__device__ __forceinline__ void rq_spline_elem(float x, const float* u, int us, bool inverse, float& y, float& lad) {
    constexpr float B = RQ_BOUND, MIND = RQ_MIN_D;
    if (!(x >= -B && x <= B)) { y = x; lad = 0.f; return; }
    // cumulative knots of the widths (pass 0) and heights (pass 1): c[0] = -B, c[i] = -B + 2B sum_{k<i} (min + (1 - K min) softmax_k), c[K] = B
    float knots[2][K + 1];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float min_size = h ? RQ_MIN_H : RQ_MIN_W;
        float e[K], mx = u[h * K * us];
#pragma unroll
        for (int i = 0; i < K; ++i) { e[i] = u[(h * K + i) * us]; mx = fmaxf(mx, e[i]); }
        float sum = 0.f;
        rq_prefix<K> se;
#pragma unroll
        for (int i = 0; i < K; ++i) { e[i] = fast_exp(e[i] - mx); sum = se.add(i, e[i]); }
        const float rs = __builtin_amdgcn_rcpf(sum);
        knots[h][0] = -B;
        rq_prefix<K> sc;
#pragma unroll
        for (int i = 0; i < K; ++i) { const float c = sc.add(i, min_size + (1.0f - min_size * K) * (e[i] * rs)); knots[h][i + 1] = 2.0f * B * c - B; }
        knots[h][K] = B;
    }
    const float (&cw)[K + 1] = knots[0], (&ch)[K + 1] = knots[1];
    // bin = #{knots <= x} - 1 over the searched knots (last one + 1e-6)
    int bin = 0;
#pragma unroll
    for (int i = 1; i <= K; ++i) {
        const float knot = (inverse ? ch[i] : cw[i]) + (i == K ? RQ_SEARCH_EPS : 0.f);
        bin += (x >= knot) ? 1 : 0;
    }
    float in_cw = cw[0], in_w = cw[1] - cw[0], in_ch = ch[0], in_h = ch[1] - ch[0];
    float ud0 = 0.f, ud1 = u[(2 * K) * us];
#pragma unroll
    for (int i = 1; i < K; ++i) {
        if (bin == i) {
            in_cw = cw[i]; in_w = cw[i + 1] - cw[i]; in_ch = ch[i]; in_h = ch[i + 1] - ch[i];
            ud0 = u[(2 * K + i - 1) * us]; ud1 = u[(2 * K + i) * us];
        }
    }
    const float raw0 = bin == 0 ? RQ_PAD_LOGIT : ud0;
    auto softplus = [](float v) { return v > 20.f ? v : fast_log(1.0f + fast_exp(v)); };
    const float d0 = MIND + softplus(raw0), d1 = MIND + softplus(ud1);
    const float rw = __builtin_amdgcn_rcpf(in_w);
    const float delta = in_h * rw;
    if (!inverse) {
        const float th = (x - in_cw) * rw;
        const float tt = th * (1.0f - th);
        const float num = in_h * (delta * th * th + d0 * tt);
        const float den = delta + (d0 + d1 - 2.0f * delta) * tt;
        y = in_ch + fast_div(num, den);
        const float omt = 1.0f - th;
        const float dnum = delta * delta * (d1 * th * th + 2.0f * delta * tt + d0 * omt * omt);
        lad = fast_log(dnum) - 2.0f * fast_log(den);
    } else {
        const float dy = x - in_ch;
        const float t3 = d0 + d1 - 2.0f * delta;
        const float qa = dy * t3 + in_h * (delta - d0);
        const float qb = in_h * d0 - dy * t3;
        const float qc = -delta * dy;
        const float disc = qb * qb - 4.0f * qa * qc;
        // The root lies in [0, 1].  Where the spline is flat the discriminant is a difference of numbers of order one: fp32 can round it below
        // zero at a bin's upper knot, where it is (h d1)^2 (the root is then 2 qc / -qb to rounding), and can put the root a few 1e-6 beyond 1,
        // so that the point leaves the bin while log|det| still comes from this bin's formula.  Both are held at the bound (a NaN stays a NaN).
        // Below 0 the root cannot fall: dy >= 0 from the bin search, so qc <= 0, and -qb - sqrt(disc) < 0 wherever dy is small (qb ~ h d0 > 0);
        // sign arithmetic is exact.
        const float r0 = fast_div(2.0f * qc, -qb - sqrtf(disc < 0.f ? 0.f : disc));
        const float root = r0 > 1.0f ? 1.0f : r0;
        y = root * in_w + in_cw;
        const float tt = root * (1.0f - root);
        const float den = delta + t3 * tt;
        const float omr = 1.0f - root;
        const float dnum = delta * delta * (d1 * root * root + 2.0f * delta * tt + d0 * omr * omr);
        lad = -(fast_log(dnum) - 2.0f * fast_log(den));
    }
}

// Forward direction only, BRANCH-FREE: the fused GEMM epilogues evaluate 2-5 independent elements per thread as straight-line code, so
// the compiler can interleave their dependency chains (the general routine above compiles to ~14 divergent branches per element for
// its bin selection).  Same algorithm and quirks; differences to it are rounding-level only: exp via one fma + v_exp (log2 e folded into
// the argument), the softmax scale folded into the prefix sums, bin edges picked by running selects instead of knot arrays.
// ONE body serves every caller, so all of them round alike and their results are bit-identical.  u(i) returns parameter i:
//   INDEXED  the two derivative logits of the bin are read at a run-time index after the search (u in memory: the LDS parameter tile,
//            readable at every index 0 .. 3K); otherwise they are picked by running selects along the bin search, so every index is a
//            compile-time constant after unrolling and u may be accumulator registers.
//   os       the parameters arrive SCALED: logical parameter i = u(i) * os with os an exact power of two.  The scale rides inside the
//            softmax's existing fma (fma(u, L2E os, -max u L2E os) is bit for bit fma(u os, L2E, -max(u os) L2E)); the two derivative
//            logits are scaled after their selection: same operations and roundings as os = 1 on u os.
//            rq_unscaled{} in place of os: the parameters arrive as they are.  With no scale to apply behind the pick, the pad logit
//            seeds the select chain of the non-INDEXED form instead of being selected at the end (same value, one select fewer).
struct rq_unscaled { __device__ constexpr operator float() const { return 1.0f; } };
template <int K, bool INDEXED = false, class U, class S>
__device__ __forceinline__ void rq_spline_fwd_regs(float x, const U& u, S os, float& y, float& lad) {
    constexpr float B = RQ_BOUND, MINW = RQ_MIN_W, MINH = RQ_MIN_H, MIND = RQ_MIN_D, L2E = 1.4426950408889634f;
    constexpr bool SEEDED = std::is_same<S, rq_unscaled>::value && !INDEXED;
    const bool inside = x >= -B && x <= B;
    const float l2s = L2E * os;
    float ew[K], eh[K], mw = u(0), mh = u(K);
#pragma unroll
    for (int i = 0; i < K; ++i) { ew[i] = u(i); eh[i] = u(K + i); mw = fmaxf(mw, ew[i]); mh = fmaxf(mh, eh[i]); }
    float sw = 0.f, sh = 0.f;
    rq_prefix<K> sew, seh;
    const float ow = -mw * l2s, oh = -mh * l2s;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        ew[i] = __builtin_amdgcn_exp2f(fmaf(ew[i], l2s, ow)); sw = sew.add(i, ew[i]);
        eh[i] = __builtin_amdgcn_exp2f(fmaf(eh[i], l2s, oh)); sh = seh.add(i, eh[i]);
    }
    const float fw = (1.0f - MINW * K) * __builtin_amdgcn_rcpf(sw), fh = (1.0f - MINH * K) * __builtin_amdgcn_rcpf(sh);
    // widths: bin = #{knots <= x} (last knot + 1e-6), in_cw = largest knot <= x, hi = smallest knot > x
    float in_cw = -B, hi = INFINITY;
    rq_prefix<K> scw, sch;
    float ud0r = SEEDED ? RQ_PAD_LOGIT : 0.f, ud1r = u(2 * K);   // bin 0: the left pad and logit 0
    int bin = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float c = scw.add(i, fmaf(fw, ew[i], MINW));
        const float knot = i == K - 1 ? B : fmaf(2.0f * B, c, -B);
        const bool ge = x >= (i == K - 1 ? knot + RQ_SEARCH_EPS : knot);
        bin += ge ? 1 : 0;
        in_cw = ge ? knot : in_cw;
        hi = ge ? hi : fminf(hi, knot);
        if constexpr (!INDEXED) {
            ud0r = ge ? u(2 * K + i) : ud0r;                     // knots increase: the last `ge` is i = bin - 1
            ud1r = ge ? u(2 * K + i + 1) : ud1r;
        }
    }
    const float in_w = hi - in_cw;
    // heights: knot index bin (lower edge) and bin + 1 (upper edge) of the cumulative heights
    float in_ch = -B, ch_hi = B;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float ch = sch.add(i, fmaf(fh, eh[i], MINH));
        const float knot = i == K - 1 ? B : fmaf(2.0f * B, ch, -B);
        in_ch = (i + 1 == bin) ? knot : in_ch;
        ch_hi = (i == bin) ? knot : ch_hi;
    }
    const float in_h = ch_hi - in_ch;
    if constexpr (INDEXED) { ud0r = u(2 * K + (bin > 0 ? bin - 1 : 0)); ud1r = u(2 * K + bin); }
    const float ud0 = SEEDED ? ud0r : bin == 0 ? RQ_PAD_LOGIT : ud0r * os, ud1 = ud1r * os;
    const float d0 = MIND + (ud0 > 20.f ? ud0 : fast_log(1.0f + fast_exp(ud0)));
    const float d1 = MIND + (ud1 > 20.f ? ud1 : fast_log(1.0f + fast_exp(ud1)));
    const float rw = __builtin_amdgcn_rcpf(in_w);
    const float delta = in_h * rw;
    const float th = (x - in_cw) * rw;
    const float tt = th * (1.0f - th);
    const float num = in_h * (delta * th * th + d0 * tt);
    const float den = delta + (d0 + d1 - 2.0f * delta) * tt;
    const float yy = in_ch + fast_div(num, den);
    const float omt = 1.0f - th;
    const float dnum = delta * delta * (d1 * th * th + 2.0f * delta * tt + d0 * omt * omt);
    const float ll = fast_log(dnum) - 2.0f * fast_log(den);
    y = inside ? yy : x;
    lad = inside ? ll : 0.f;
}

// the same on parameters in memory, element stride `us`
template <int K>
__device__ __forceinline__ void rq_spline_fwd(float x, const float* u, int us, float& y, float& lad) {
    rq_spline_fwd_regs<K, true>(x, [&](int i) { return u[i * us]; }, rq_unscaled{}, y, lad);
}

// The K = 8 spline on its 22 INFORMATIVE parameters [7 width logits | 7 height logits | derivative logits 0..7], scaled as above (the folded
// image of spline_wide.hip).  softmax is shift-invariant, so the parameter layer was folded at pack time to emit w_i - w_7 and h_i - h_7:
// logit 7 of either softmax is the literal 0 and still takes part in the maximum, the exponentials and the sum (today's operation sequence on
// a constant input).  Derivative logit 8 is read by the reference for no bin; the bin search above selects it only where x >= 3 + 1e-6, whose
// result is discarded, so a literal stands in for it as well.
template <class U>
__device__ __forceinline__ void rq_spline_fwd_regs_folded(float x, const U& u, float os, float& y, float& lad) {
    rq_spline_fwd_regs<8>(x, [&](int i) { return i < 7 ? u(i) : i == 7 || i == 15 || i == 24 ? 0.f : i < 15 ? u(i - 1) : u(i - 2); }, os, y, lad);
}

// The bin counts the kernels are instantiated for (host side): calls f(std::integral_constant<int, K>) and returns whether K is one of them.
template <class F>
inline bool spline_bins_dispatch(int K, F&& f) {
    switch (K) {
        case 4: f(std::integral_constant<int, 4>{}); return true;
        case 8: f(std::integral_constant<int, 8>{}); return true;
        case 16: f(std::integral_constant<int, 16>{}); return true;
        default: return false;
    }
}
inline bool spline_bins_ok(int K) { return spline_bins_dispatch(K, [](auto) {}); }
// host entry points: dispatch, or refuse in the caller's words ("<who>: <its name of the bin count>")
template <class F>
inline void spline_bins_require(int K, const char* what, F&& f) {
    if (!spline_bins_dispatch(K, f)) throw Error(FC_ERR_UNSUPPORTED, std::string(what) + " must be 4, 8 or 16");
}
inline void spline_bins_require(int K, const char* what) { spline_bins_require(K, what, [](auto) {}); }

// The device side keeps its own switch over the same three counts: routed through spline_bins_dispatch and a lambda, the kernels that
// call rq_any compile to different code.
__device__ __forceinline__ void rq_any(int K, float x, const float* u, int us, bool inv, float& y, float& lad) {
    switch (K) {
        case 4: rq_spline_elem<4>(x, u, us, inv, y, lad); break;
        case 8: rq_spline_elem<8>(x, u, us, inv, y, lad); break;
        case 16: rq_spline_elem<16>(x, u, us, inv, y, lad); break;
        default: y = x; lad = 0.f; break;     // rejected on the host
    }
}

// Column layout of the spline parameter layer's output ("tile-grouped"): the 3K+1 parameters of DPT = 128 / (3K+1) transformed dims
// share one 128-column GEMM tile (K = 8: 5 dims, 125 of 128 columns used), so the workgroup that produced a 128x128 tile holds every
// parameter of DPT dims of its 128 rows and can evaluate the splines in its epilogue.
//   K = 4, 16: dim-major inside the tile, column(j, p) = (j / DPT) * 128 + (j % DPT) * (3K+1) + p.
//   K = 8: REGISTER-SLOT order of the transposed 32x32 MFMA product (parameters on the accumulator's row index, points on its lanes;
//     gemm.hip VAR 10).  A lane of half h = lane >> 5 owns, for its point, accumulator slot s = 16 * (block of 32 columns) + register
//     v, which is tile column  c(s, h) = (s / 16) * 32 + ((s % 16) / 4) * 8 + 4 h + s % 4.  Dims 0, 1 of the tile live in slots 0..49 of
//     half 0, dims 2, 3 in slots 0..49 of half 1, dim 4 in slots 50..63 of half 0 (parameters 0..13) and slots 50..60 of half 1
//     (parameters 14..24); slots 61..63 of half 1 (columns 125..127) are unused.  A lane pair therefore holds all 25 parameters of
//     each of its 5 dims in registers with compile-time indices, and 11 v_permlane32_swap move dim 4's upper part across.
__host__ __device__ inline int spline_dpt(int K) { return 128 / (3 * K + 1); }
__host__ __device__ inline int spline_slot_col(int s, int h) { return (s / 16) * 32 + ((s % 16) / 4) * 8 + 4 * h + s % 4; }
__host__ __device__ inline int spline_col(int j, int pp, int K) {
    const int dpt = spline_dpt(K), tile = j / dpt, dl = j % dpt;
    if (K != 8) return tile * 128 + dl * (3 * K + 1) + pp;
    if (dl < 4) return tile * 128 + spline_slot_col((dl & 1) * 25 + pp, dl >> 1);
    return tile * 128 + (pp < 14 ? spline_slot_col(50 + pp, 0) : spline_slot_col(50 + pp - 14, 1));
}
// inverse of the above inside one tile: column c -> dim-major position (dim in tile) * (3K+1) + parameter (the LDS-tile epilogues of the
// other GEMM variants store their accumulators there, so their readers see the parameters of a dim contiguously)
__host__ __device__ inline int spline_tile_pos(int c, int K) {
    if (K != 8) return c;
    const int h = (c >> 2) & 1, s = (c >> 5) * 16 + ((c >> 3) & 3) * 4 + (c & 3);
    if (s < 50) return (2 * h + s / 25) * 25 + s % 25;
    return h == 0 ? 100 + (s - 50) : 100 + 14 + (s - 50);          // h = 1, s = 61..63 -> 125..127 (unused)
}
__host__ __device__ inline int spline_ncols(int d2, int K) { return ((d2 + spline_dpt(K) - 1) / spline_dpt(K)) * 128; }

}  // namespace fc
