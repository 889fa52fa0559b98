// ExponentialCoupling beyond d2 = 16: the action of the per-point matrix exponential on the vector, for 17 <= d2 <= 256.
//
// models/exponential_coupling.py:44-75: per point, W = rescale*tanh(scale*raw + shift) + reshift + 1e-8 (d2 x d2),
// y2 = expm(W) x2 + b, ldj = tr W ; inverse x2 = expm(-W)(y2 - b).  Both of the reference's algorithms ('torch' = matrix_exp,
// 'original' = converged truncated series, utils.py:294-327) converge to this value, so only the action e^A v is formed, never e^A:
// Al-Mohy & Higham, "Computing the action of the matrix exponential" (SIAM J. Sci. Comput. 33(2), 2011), Algorithm 3.2 in fp32:
//   * A = sign*W - mu I with mu = tr(sign*W) / d2 (the shift of their section 3.1), e^(sign W) v = e^mu e^A v;
//   * per point, from its own ||A||_1: s steps of an m-term Taylor polynomial, (m, s) = argmin m * ceil(||A||_1 / theta_m) over
//     m <= 55 with the single-precision theta_m (u = 2^-24, the table below);
//   * early exit of a step once two consecutive terms are below u * ||F||_inf.
// The work therefore grows like ||A||_1 / theta_55 + const matrix-vector products, not like the old kernel's 24 ||W||.
//
// One workgroup per point.  The matrix is read and transformed ONCE, straight into registers spread over the workgroup: G lanes form a
// row group; group g owns rows g + NGRP*r (r < R), lane q of the group owns columns q + G*c (c < C), i.e. w[r][c] = A[g + NGRP r][q + G c]
// (a backward can accumulate dA in the same layout).  A product A t is C LDS reads of the term vector + R*C register FMAs + an xor
// reduction over the G lanes of each row group; lane q < R of group g then owns row g + NGRP*q of the result (term and partial sum).
// The trace is summed while the matrix is loaded.  A point whose ||A||_1 needs more than kExpmWideMaxSteps steps raises *status and
// gets NaN outputs: the series is never returned truncated.
#include "common.h"
#include "launch.h"

namespace fc {

// theta_m (m = 1..55) for u = 2^-24: the largest theta with sum_{k>m} |c_k| theta^(k-1) <= u, c_k the Taylor coefficients of
// log(e^-x T_m(x)) (Al-Mohy & Higham 2011, eq. (3.7), Table 3.1 single-precision row: 1.3e-1, 1.0, 2.2, ..., 1.3e1), recomputed in
// 80-digit arithmetic from 200 coefficients.
__constant__ float c_expm_theta[56] = {
    0.f, 1.1921e-07f, 5.9789e-04f, 1.1234e-02f, 5.1166e-02f, 1.3085e-01f, 2.4953e-01f, 4.0146e-01f, 5.8005e-01f, 7.7951e-01f, 9.9518e-01f,
    1.2235e+00f, 1.4617e+00f, 1.7076e+00f, 1.9599e+00f, 2.2170e+00f, 2.4783e+00f, 2.7428e+00f, 3.0101e+00f, 3.2796e+00f, 3.5509e+00f,
    3.8239e+00f, 4.0981e+00f, 4.3735e+00f, 4.6498e+00f, 4.9269e+00f, 5.2047e+00f, 5.4831e+00f, 5.7620e+00f, 6.0414e+00f, 6.3211e+00f,
    6.6011e+00f, 6.8815e+00f, 7.1620e+00f, 7.4428e+00f, 7.7238e+00f, 8.0049e+00f, 8.2862e+00f, 8.5676e+00f, 8.8491e+00f, 9.1307e+00f,
    9.4123e+00f, 9.6940e+00f, 9.9758e+00f, 1.0258e+01f, 1.0539e+01f, 1.0821e+01f, 1.1103e+01f, 1.1385e+01f, 1.1667e+01f, 1.1949e+01f,
    1.2231e+01f, 1.2513e+01f, 1.2795e+01f, 1.3077e+01f, 1.3359e+01f};
constexpr int kExpmWideMmax = 55;

__device__ __forceinline__ float ew_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float ew_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ldj_mode: 0 = none, 1 = ldj[row] = tr W, 2 = ldj[row] += tr W.  y2 may alias x2 (each lane writes only the element it read); columns
// [d2, ypad) of y2 are zeroed (training panels carry zero pad columns).
// info (optional): per row {||A||_1, s, m, matrix-vector products}.
template <int NT, int G, int R, int C>
__global__ __launch_bounds__(NT) void expm_wide_kernel(const float* __restrict__ params, int ldp, const float* x2, int ldx, const float* __restrict__ scal4,
                                                       float* y2, int ldy, int ypad, float* ldj, int ldj_mode, int d2, int inverse, int* status,
                                                       float* __restrict__ info) {
    constexpr int NGRP = NT / G, NW = NT / 64, DC = G * C;
    static_assert(R <= G && NGRP * R == DC && 64 % G == 0, "expm_wide_kernel: bad register layout");
    __shared__ float tb[2][DC];            // term vectors (double-buffered: one LDS barrier per product)
    __shared__ float colp[NGRP][DC];       // per-row-group column sums of |A| (off-diagonal)
    __shared__ float diag[DC];
    __shared__ float red[2][NW][2];
    __shared__ float trp[NW], nrp[NW][2];
    const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = tid / G, q = tid % G;
    const float sc = scal4[0], sh = scal4[1], rs = scal4[2], rsh = scal4[3];
    const float sgn = inverse ? -1.f : 1.f;
    const float* pr = params + (size_t)row * ldp;

    // ---- load + transform W once (natural row-major panel: the G lanes of a group read G consecutive floats of one row)
    float w[R][C];
    float tr_part = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = g + NGRP * r;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = q + G * c;
            float v = 0.f;
            if (i < d2 && j < d2) v = rs * tanhf(sc * pr[(size_t)i * d2 + j] + sh) + rsh + 1e-8f;
            if (i == j && i < d2) { tr_part += v; diag[i] = sgn * v; v = 0.f; }       // the diagonal gets the shift below
            w[r][c] = sgn * v;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) a += fabsf(w[r][c]);
        colp[g][q + G * c] = a;
    }
    const int own = g + NGRP * q;                          // the result row this lane owns (q < R)
    const bool writer = q < R && own < d2;
    float F = 0.f;
    if (writer) {
        F = x2[(size_t)row * ldx + own];
        if (inverse) F -= pr[(size_t)d2 * d2 + own];
        tb[0][own] = F;
    }
    tr_part = ew_wave_sum(tr_part);
    if (lane == 0) trp[wave] = tr_part;
    __syncthreads();

    // ---- trace (fixed order), shift mu, ||A||_1 and ||x||_inf
    float tr = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) tr += trp[k];
    const float mu = sgn * tr / (float)d2;
    float cs = 0.f;
    if (tid < d2) {
        for (int k = 0; k < NGRP; ++k) cs += colp[k][tid];
        cs += fabsf(diag[tid] - mu);
        if (!(cs <= 3.4e38f)) cs = __builtin_inff();      // a NaN column must not vanish in the fmaxf reductions below
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int i = g + NGRP * r, j = q + G * c;
            if (i == j && i < d2) w[r][c] = diag[i] - mu;
        }
    const float cm = ew_wave_max(cs), xm = ew_wave_max(writer ? fabsf(F) : 0.f);
    if (lane == 0) { nrp[wave][0] = cm; nrp[wave][1] = xm; }
    __syncthreads();
    float nrm = 0.f, bnorm = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) { nrm = fmaxf(nrm, nrp[k][0]); bnorm = fmaxf(bnorm, nrp[k][1]); }

    // ---- (m, s): fewest products m * s with ||A||_1 / s <= theta_m.  Uniform over the workgroup (every lane reads the same LDS words).
    if (!(nrm <= (float)kExpmWideMaxSteps * c_expm_theta[kExpmWideMmax])) {        // (also catches a NaN / Inf matrix)
        if (tid == 0) {
            *status = 1;
            if (ldj_mode) ldj[row] = __builtin_nanf("");
            if (info) { info[4 * row] = nrm; info[4 * row + 1] = -1.f; info[4 * row + 2] = 0.f; info[4 * row + 3] = 0.f; }
        }
        if (writer) y2[(size_t)row * ldy + own] = __builtin_nanf("");
        return;
    }
    int m = 1, s = 1;
    {
        float best = 3.4e38f;
        for (int mm = 1; mm <= kExpmWideMmax; ++mm) {
            const float sm = fmaxf(1.f, ceilf(nrm / c_expm_theta[mm]));
            if ((float)mm * sm < best) { best = (float)mm * sm; m = mm; s = (int)sm; }
        }
    }
    const float eta = expf(mu / (float)s);
    const float tol = 5.9604645e-08f;                      // u = 2^-24

    // ---- s steps of F <- eta * T_m(A / s) F with early exit
    int cur = 0, nmv = 0;
    for (int st = 0; st < s; ++st) {
        float c1 = bnorm, fn = bnorm;
        for (int k = 1; k <= m; ++k) {
            float tv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) tv[c] = (q + G * c < d2) ? tb[cur][q + G * c] : 0.f;
            float acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float a = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) a = fmaf(w[r][c], tv[c], a);
                acc[r] = a;
            }
#pragma unroll
            for (int off = G / 2; off >= 1; off >>= 1)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] += __shfl_xor(acc[r], off, 64);
            float mine = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) mine = (r == q) ? acc[r] : mine;
            const float nb = mine * (1.0f / ((float)s * (float)k));
            float cb = 0.f, cf = 0.f;
            if (writer) {
                tb[cur ^ 1][own] = nb;
                F += nb;
                cb = fabsf(nb);
                cf = fabsf(F);
            }
            cb = ew_wave_max(cb);
            cf = ew_wave_max(cf);
            if (lane == 0) { red[k & 1][wave][0] = cb; red[k & 1][wave][1] = cf; }
            __syncthreads();
            float c2 = 0.f;
            fn = 0.f;
#pragma unroll
            for (int v = 0; v < NW; ++v) { c2 = fmaxf(c2, red[k & 1][v][0]); fn = fmaxf(fn, red[k & 1][v][1]); }
            cur ^= 1;
            ++nmv;
            if (c1 + c2 <= tol * fn) break;
            c1 = c2;
        }
        F *= eta;
        bnorm = fn * eta;
        if (st + 1 < s) {
            // the next step starts from b = F: written into the buffer every lane finished reading before the last barrier
            if (writer) tb[cur ^ 1][own] = F;
            cur ^= 1;
            __syncthreads();
        }
    }
    if (writer) y2[(size_t)row * ldy + own] = inverse ? F : F + pr[(size_t)d2 * d2 + own];
    if (tid >= d2 && tid < ypad) y2[(size_t)row * ldy + tid] = 0.f;
    if (tid == 0) {
        if (ldj_mode == 1) ldj[row] = tr;
        else if (ldj_mode == 2) ldj[row] += tr;
        if (info) { info[4 * row] = nrm; info[4 * row + 1] = (float)s; info[4 * row + 2] = (float)m; info[4 * row + 3] = (float)nmv; }
    }
}

template <int NT, int G, int R, int C>
static void launch_ew(const float* params, int ldp, const float* x2, int ldx, const float* scal4, float* y2, int ldy, int ypad, float* ldj, int ldj_mode,
                      int rows, int d2, int inverse, int* status, float* info, hipStream_t s) {
    launch_kernel<expm_wide_kernel<NT, G, R, C>>(nullptr, 0.0, 0.0, dim3(rows), dim3(NT), 0, s, params, ldp, x2, ldx, scal4, y2, ldy, ypad, ldj, ldj_mode, d2,      // (the caller's scope)
                                                 inverse, status, info);
}

void launch_expm_wide(const float* params, int ldp, const float* x2, int ldx, const float* scal4, float* y2, int ldy, int ypad, float* ldj,
                      int ldj_mode, int rows, int d2, int inverse, int* status, float* info, hipStream_t s) {
    if (d2 < 1 || d2 > kExpmWideMaxD2)
        throw Error(FC_ERR_UNSUPPORTED, "ExponentialCoupling: latent_dim - latent_dim/2 > 256 is not supported (the matrix-exponential action kernel holds "
                                        "at most a 256 x 256 matrix per point)");
    if (ldp < d2 * d2 + d2) throw Error(FC_ERR_INVALID, "expm wide: parameter pitch too small");
    if (!status) throw Error(FC_ERR_INVALID, "expm wide: null status word");
    if (ypad > ldy || ypad > round_up(d2, 32)) throw Error(FC_ERR_INVALID, "expm wide: pad width beyond the output pitch");
    if (rows <= 0) return;
    // bytes: the panel row, x2 in, y2 out, ldj; flops: the load-time transform (tanh counted as one) and trace -- the matrix-vector
    // products (2 d2^2 each) depend on each point's norm and are counted by the info output of fc_op_expm_action_f32
    ProfScope ps("fc::expm_wide_kernel", (double)rows * d2 * d2 * 5.0, 4.0 * rows * ((double)d2 * d2 + 3.0 * d2 + (ldj_mode ? 2 : 0)), s);
    if (d2 <= 32) launch_ew<256, 16, 2, 2>(params, ldp, x2, ldx, scal4, y2, ldy, ypad, ldj, ldj_mode, rows, d2, inverse, status, info, s);
    else if (d2 <= 64) launch_ew<256, 16, 4, 4>(params, ldp, x2, ldx, scal4, y2, ldy, ypad, ldj, ldj_mode, rows, d2, inverse, status, info, s);
    else if (d2 <= 128) launch_ew<256, 16, 8, 8>(params, ldp, x2, ldx, scal4, y2, ldy, ypad, ldj, ldj_mode, rows, d2, inverse, status, info, s);
    else if (d2 <= 160) launch_ew<256, 16, 10, 10>(params, ldp, x2, ldx, scal4, y2, ldy, ypad, ldj, ldj_mode, rows, d2, inverse, status, info, s);
    else launch_ew<1024, 32, 8, 8>(params, ldp, x2, ldx, scal4, y2, ldy, ypad, ldj, ldj_mode, rows, d2, inverse, status, info, s);
}

// ---------------------------------------------------------------- training backward, 17 <= d2 <= 160
// Exact reverse mode through the recurrence of expm_wide_kernel above.
//
// Forward (expm_wide_kernel, sign +): W = rs tanh(sc raw + sh) + rsh + 1e-8, mu = tr W / d2, A = W - mu I, (m, s) from ||A||_1 and the theta
// table, F_0 = x2, step st: t_0 = F_{st-1}, t_k = A t_{k-1} / (s k) for k <= K_st (K_st <= m, set by the early exit), F_st = eta sum_k t_k with
// eta = e^(mu / s); y2 = F_s + b, ldj = tr W.
// Backward: mu, eta, m, s, K_st are constants (exact for the true function: e^mu e^(W - mu I) = e^W for any fixed mu).  The forward is
// replayed with the same arithmetic, keeping the step inputs F_0 .. F_{s-2}, every K_st and the last step's terms in LDS.  For st = s .. 1:
// the step's terms t_0 .. t_{K-1} are in LDS (replayed from F_{st-1} for every step but the last), nu = eta lambda_st, mu_K = nu, and for
// k = K .. 1:  dA += (mu_k / (s k)) t_{k-1}^T,  mu_{k-1} = nu + A^T mu_k / (s k);  lambda_{st-1} = mu_0.  dx2 = lambda_0, db = dy2,
// dW = dA + dldj I, then the chain through the tanh rescale as in expm_train_bwd_kernel (train_expm.hip).
//
// One workgroup of 256 lanes per point, the forward's register layout: w[r][c] = A[g + NGRP r][q + G c], and dA in the same layout.  The
// rank-1 update is R C FMAs from R + C LDS reads.  A^T mu gives each lane C partial column sums over its own R rows; the row groups of a
// wave reduce with xor shuffles over lanes 16 and 32 apart, the 4 waves through cred[NW][DC] in fixed order.  No atomics: the same input
// gives the same bytes, and a row's outputs do not depend on the other rows of the launch.  A point beyond the forward's bound
// (||A||_1 > 40 theta_55, or a non-finite matrix) raises *status and gets NaN outputs.

// A t for the term vector t in LDS: lane q < R of group g returns row g + NGRP q of the product (the forward's arithmetic and order)
template <int G, int R, int C>
__device__ __forceinline__ float ewb_matvec(const float (&w)[R][C], const float* t, int q, int d2) {
    float tv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) tv[c] = (q + G * c < d2) ? t[q + G * c] : 0.f;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) a = fmaf(w[r][c], tv[c], a);
        acc[r] = a;
    }
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += __shfl_xor(acc[r], off, 64);
    float mine = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) mine = (r == q) ? acc[r] : mine;
    return mine;
}

// dx2 columns [d2, xpad) and dout columns [d2*d2 + d2, opad) are zeroed.  dscal [rows, 4]: this point's parts of d scale, d shift,
// d rescale, d reshift.
template <int NT, int G, int R, int C>
__global__ __launch_bounds__(NT) void expm_wide_bwd_kernel(const float* __restrict__ x2, int ldx, const float* __restrict__ o, int ldo,
                                                           const float* __restrict__ scal4, const float* __restrict__ dy2, int lddy,
                                                           const float* __restrict__ dldj, float* __restrict__ dx2, int lddx, int xpad,
                                                           float* __restrict__ dout, int lddo, int opad, float* __restrict__ dscal, int d2,
                                                           int* status) {
    constexpr int NGRP = NT / G, NW = NT / 64, DC = G * C;
    constexpr int NTERM = kExpmWideMmax + 1, NSTATE = kExpmWideMaxSteps - 1;
    static_assert(R <= G && NGRP * R == DC && 64 % G == 0 && DC <= NT && NGRP + 1 <= NTERM, "expm_wide_bwd_kernel: bad register layout");
    __shared__ float T[NTERM][DC];         // the terms t_0 .. t_K of one step; before the first step: colp[NGRP][DC] and diag[DC]
    __shared__ float Fs[NSTATE][DC];       // step inputs F_0 .. F_{s-2} (the last step's terms stay in T)
    __shared__ float cred[NW][DC];         // per-wave column sums of A^T mu
    __shared__ float mub[2][DC];           // mu_k
    __shared__ float red[2][NW][2];
    __shared__ float trp[NW], nrp[NW][2], sred[NW][4];
    __shared__ int kst[kExpmWideMaxSteps];
    static_assert(sizeof(float) * (NTERM * DC + NSTATE * DC + NW * DC + 2 * DC + 4 * NW + NW + 2 * NW + 4 * NW) + sizeof(int) * kExpmWideMaxSteps <= 65536,
                  "expm_wide_bwd_kernel: LDS beyond 64 KiB");
    float(*colp)[DC] = T;                  // per-row-group column sums of |A| (off-diagonal): rows 0 .. NGRP-1 of T
    float* diag = T[NGRP];
    const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = tid / G, q = tid % G;
    const float sc = scal4[0], sh = scal4[1], rs = scal4[2], rsh = scal4[3];
    const float* pr = o + (size_t)row * ldo;
    float* dr = dout + (size_t)row * lddo;
    const int np = d2 * d2 + d2;

    // ---- load + transform W once, with the forward's arithmetic.  One wave per SIMD hides no latency, so the loads are unconditional
    //      (pad elements read element 0 of the point's panel row) and all issued ahead of the first tanh; the raw values stay in
    //      registers for the chain at the end.
    float w[R][C], raw[R][C];
    float tr_part = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = g + NGRP * r;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = q + G * c;
            raw[r][c] = pr[(i < d2 && j < d2) ? i * d2 + j : 0];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = g + NGRP * r;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = q + G * c;
            float v = 0.f;
            if (i < d2 && j < d2) v = rs * tanhf(sc * raw[r][c] + sh) + rsh + 1e-8f;
            if (i == j && i < d2) { tr_part += v; diag[i] = v; v = 0.f; }
            w[r][c] = v;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) a += fabsf(w[r][c]);
        colp[g][q + G * c] = a;
    }
    const int own = g + NGRP * q;                          // the result row this lane owns in a product (q < R)
    const bool writer = q < R && own < d2;
    float F = writer ? x2[(size_t)row * ldx + own] : 0.f;
    tr_part = ew_wave_sum(tr_part);
    if (lane == 0) trp[wave] = tr_part;
    __syncthreads();

    float tr = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) tr += trp[k];
    const float mu = tr / (float)d2;
    float cs = 0.f;
    if (tid < d2) {
        for (int k = 0; k < NGRP; ++k) cs += colp[k][tid];
        cs += fabsf(diag[tid] - mu);
        if (!(cs <= 3.4e38f)) cs = __builtin_inff();
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int i = g + NGRP * r, j = q + G * c;
            if (i == j && i < d2) w[r][c] = diag[i] - mu;
        }
    const float cm = ew_wave_max(cs), xm = ew_wave_max(writer ? fabsf(F) : 0.f);
    if (lane == 0) { nrp[wave][0] = cm; nrp[wave][1] = xm; }
    __syncthreads();                                       // colp and diag are dead from here on: T is free
    float nrm = 0.f, bnorm = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) { nrm = fmaxf(nrm, nrp[k][0]); bnorm = fmaxf(bnorm, nrp[k][1]); }

    if (!(nrm <= (float)kExpmWideMaxSteps * c_expm_theta[kExpmWideMmax])) {        // beyond the forward's bound, or a NaN / Inf matrix
        const float nan = __builtin_nanf("");
        if (tid == 0) *status = 1;
        if (tid < 4) dscal[(size_t)row * 4 + tid] = nan;
        if (tid < xpad) dx2[(size_t)row * lddx + tid] = tid < d2 ? nan : 0.f;
        for (int c = tid; c < opad; c += NT) dr[c] = c < np ? nan : 0.f;
        return;
    }
    int m = 1, s = 1;
    {
        float best = 3.4e38f;
        for (int mm = 1; mm <= kExpmWideMmax; ++mm) {
            const float sm = fmaxf(1.f, ceilf(nrm / c_expm_theta[mm]));
            if ((float)mm * sm < best) { best = (float)mm * sm; m = mm; s = (int)sm; }
        }
    }
    const float eta = expf(mu / (float)s);
    const float tol = 5.9604645e-08f;                      // u = 2^-24

    // ---- the forward again: step inputs into Fs, terms into T, K_st into kst
    for (int st = 0; st < s; ++st) {
        if (writer) {
            T[0][own] = F;
            if (st + 1 < s) Fs[st][own] = F;
        }
        __syncthreads();
        float c1 = bnorm, fn = bnorm;
        int K = m;
        for (int k = 1; k <= m; ++k) {
            const float nb = ewb_matvec<G, R, C>(w, T[k - 1], q, d2) * (1.0f / ((float)s * (float)k));
            float cb = 0.f, cf = 0.f;
            if (writer) {
                T[k][own] = nb;
                F += nb;
                cb = fabsf(nb);
                cf = fabsf(F);
            }
            cb = ew_wave_max(cb);
            cf = ew_wave_max(cf);
            if (lane == 0) { red[k & 1][wave][0] = cb; red[k & 1][wave][1] = cf; }
            __syncthreads();
            float c2 = 0.f;
            fn = 0.f;
#pragma unroll
            for (int v = 0; v < NW; ++v) { c2 = fmaxf(c2, red[k & 1][v][0]); fn = fmaxf(fn, red[k & 1][v][1]); }
            if (c1 + c2 <= tol * fn) { K = k; break; }
            c1 = c2;
        }
        if (tid == 0) kst[st] = K;
        F *= eta;
        bnorm = fn * eta;
    }

    // ---- reverse: lane tid < d2 owns element tid of lambda / mu_k
    float lam = tid < d2 ? dy2[(size_t)row * lddy + tid] : 0.f;
    float dA[R][C];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) dA[r][c] = 0.f;
    for (int st = s - 1; st >= 0; --st) {
        __syncthreads();                                   // kst, and T free of the step above
        const int K = kst[st];
        if (st + 1 < s) {                                  // the terms t_0 .. t_{K-1} of this step (t_K is not needed)
            if (writer) T[0][own] = Fs[st][own];
            __syncthreads();
            for (int k = 1; k < K; ++k) {
                const float nb = ewb_matvec<G, R, C>(w, T[k - 1], q, d2) * (1.0f / ((float)s * (float)k));
                if (writer) T[k][own] = nb;
                __syncthreads();
            }
        }
        const float nu = eta * lam;
        if (tid < DC) mub[0][tid] = nu;                    // (lam = 0 beyond d2)
        __syncthreads();
        int cur = 0;
        float mk_own = nu;
        for (int k = K; k >= 1; --k) {
            const float fk = 1.0f / ((float)s * (float)k);
            float mk[R], tv[C], pc[C];
#pragma unroll
            for (int r = 0; r < R; ++r) mk[r] = (g + NGRP * r < d2) ? mub[cur][g + NGRP * r] * fk : 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) tv[c] = (q + G * c < d2) ? T[k - 1][q + G * c] : 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float a = 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    dA[r][c] = fmaf(mk[r], tv[c], dA[r][c]);
                    a = fmaf(w[r][c], mk[r], a);
                }
                pc[c] = a;
            }
#pragma unroll
            for (int off = G; off < 64; off <<= 1)
#pragma unroll
                for (int c = 0; c < C; ++c) pc[c] += __shfl_xor(pc[c], off, 64);
            if (lane < G) {
#pragma unroll
                for (int c = 0; c < C; ++c) cred[wave][q + G * c] = pc[c];
            }
            __syncthreads();
            if (tid < DC) {
                float a = cred[0][tid];
#pragma unroll
                for (int v = 1; v < NW; ++v) a += cred[v][tid];
                mk_own = nu + a;
                mub[cur ^ 1][tid] = mk_own;
            }
            cur ^= 1;
            __syncthreads();
        }
        lam = mk_own;
    }

    // ---- outputs: dx2, the chain through W = rs tanh(sc raw + sh) + rsh + 1e-8 (and ldj = tr W), db, pads
    if (tid < xpad) dx2[(size_t)row * lddx + tid] = tid < d2 ? lam : 0.f;
    const float gl = dldj[row];
    float g_sc = 0.f, g_sh = 0.f, g_rs = 0.f, g_rsh = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = g + NGRP * r;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = q + G * c;
            if (i < d2 && j < d2) {
                const float gw = dA[r][c] + (i == j ? gl : 0.f);
                const float t = tanhf(sc * raw[r][c] + sh);
                const float gt = gw * rs * (1.0f - t * t);
                dr[i * d2 + j] = gt * sc;
                g_sc += gt * raw[r][c]; g_sh += gt; g_rs += gw * t; g_rsh += gw;
            }
        }
    }
    if (tid < d2) dr[(size_t)d2 * d2 + tid] = dy2[(size_t)row * lddy + tid];
    if (np + tid < opad) dr[np + tid] = 0.f;
    g_sc = ew_wave_sum(g_sc); g_sh = ew_wave_sum(g_sh); g_rs = ew_wave_sum(g_rs); g_rsh = ew_wave_sum(g_rsh);
    if (lane == 0) { sred[wave][0] = g_sc; sred[wave][1] = g_sh; sred[wave][2] = g_rs; sred[wave][3] = g_rsh; }
    __syncthreads();
    if (tid < 4) {
        float a = sred[0][tid];
#pragma unroll
        for (int v = 1; v < NW; ++v) a += sred[v][tid];
        dscal[(size_t)row * 4 + tid] = a;
    }
}

template <int NT, int G, int R, int C>
static void launch_ewb(const float* x2, int ldx, const float* o, int ldo, const float* scal4, const float* dy2, int lddy, const float* dldj, float* dx2,
                       int lddx, float* dout, int lddo, float* dscal, int rows, int d2, int* status, hipStream_t s) {
    launch_kernel<expm_wide_bwd_kernel<NT, G, R, C>>(nullptr, 0.0, 0.0, dim3(rows), dim3(NT), 0, s, x2, ldx, o, ldo, scal4, dy2, lddy, dldj, dx2, lddx,      // (the caller's scope)
                                                     round_up(d2, 32), dout, lddo, round_up(d2 * d2 + d2, 32), dscal, d2, status);
}

}  // namespace fc

using namespace fc;

extern "C" {

int fc_train_expm_wide_bwd_f32(const float* x2, int32_t ldx, const float* o, int32_t ldo, const float* scal4, const float* dy2, int32_t lddy,
                               const float* dldj, float* dx2, int32_t lddx, float* dout, int32_t lddo, float* dscal, int32_t rows, int32_t d2,
                               int32_t* status, void* stream) {
    FC_API_BEGIN
    if (!x2 || !o || !scal4 || !dy2 || !dldj || !dx2 || !dout || !dscal || !status || rows < 1 || d2 <= kExpmSmallMaxD2 || d2 > kExpmWideBwdMaxD2 ||
        ldx < d2 || ldo < d2 * d2 + d2 || lddy < d2 || lddx < round_up(d2, 32) || lddo < round_up(d2 * d2 + d2, 32))
        throw Error(FC_ERR_INVALID, "fc_train_expm_wide_bwd_f32: bad argument (17 <= d2 <= 160)");
    hipStream_t s = (hipStream_t)stream;
    // bytes: the panel row read twice (load, chain) and its gradient written once; the products depend on each point's norm
    ProfScope ps("fc::expm_wide_bwd_kernel", (double)rows * d2 * d2 * 12.0, 4.0 * rows * (3.0 * d2 * d2 + 5.0 * d2 + 5.0), s);
    if (d2 <= 32) launch_ewb<256, 16, 2, 2>(x2, ldx, o, ldo, scal4, dy2, lddy, dldj, dx2, lddx, dout, lddo, dscal, rows, d2, (int*)status, s);
    else if (d2 <= 64) launch_ewb<256, 16, 4, 4>(x2, ldx, o, ldo, scal4, dy2, lddy, dldj, dx2, lddx, dout, lddo, dscal, rows, d2, (int*)status, s);
    else if (d2 <= 128) launch_ewb<256, 16, 8, 8>(x2, ldx, o, ldo, scal4, dy2, lddy, dldj, dx2, lddx, dout, lddo, dscal, rows, d2, (int*)status, s);
    else launch_ewb<256, 16, 10, 10>(x2, ldx, o, ldo, scal4, dy2, lddy, dldj, dx2, lddx, dout, lddo, dscal, rows, d2, (int*)status, s);
    FC_API_END
}

}  // extern "C"
