// Training's narrow ExponentialCoupling (d2 <= 16), forward + backward: expm_train_fwd_kernel, expm_train_bwd_kernel and the entries
// fc_train_expm_fwd_f32 / fc_train_expm_bwd_f32.  Larger d2 goes to expm_wide.hip: the forward entry here dispatches to it, the wide
// backward has its own entry there.
// models/exponential_coupling.py:44-58, utils.py:294-327: o = [d2 x d2 raw matrix | d2 shift] per point,
// W = rescale tanh(scale raw + shift) + reshift + 1e-8, y2 = expm(W) x2 + b, ldj = tr W.
// Forward = the inference kernel's arithmetic, the same two functions of expm_narrow.h: A = W 2^-s with |A|_inf <= 1/2, the 12-term Taylor
// ACTION u = sum_k A^k v / k! applied 2^s times.  Backward = exact reverse mode through that recurrence: the intermediate vectors v_rep are
// kept, each action is replayed for its terms t_k and differentiated with mu_12 = lambda, mu_{k-1} = lambda + A^T mu_k / k,
// dA += mu_k t_{k-1}^T / k.  One thread per point with per-thread arrays (scratch): the layer only exists for small d2, like in the reference.
#include <hip/hip_runtime.h>

#include "common.h"
#include "expm_narrow.h"
#include "launch.h"

namespace fc {

constexpr int EX_REP = 64;
// w = W, tr = tr W, nrm = |W|_inf; returns the number of halvings s: |W 2^-s|_inf <= 1/2 where the stored states allow it
__device__ __forceinline__ int expm_prepare(const float* pr, int d2, const float* scal4, float* w, float& tr, float& nrm) {
    nrm = expm_narrow_matrix<EX_D>(pr, d2, scal4, false, w, tr);
    int s = 0;
    for (float h = nrm; h > 0.5f && s < 6; h *= 0.5f) ++s;          // 2^6 = EX_REP stored states at most
    return s;
}
__global__ void expm_train_fwd_kernel(const float* __restrict__ x2, int ldx, const float* __restrict__ o, int ldo, const float* __restrict__ scal4,
                                      float* __restrict__ y2, int ldy, float* __restrict__ ldj, int rows, int d2, int d2_pad, int* __restrict__ status) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const float* pr = o + (size_t)row * ldo;
    float w[EX_D * EX_D], v[EX_D];
    float tr, nrm;
    const int s = expm_prepare(pr, d2, scal4, w, tr, nrm);
    if (ldexpf(nrm, -s) > 0.5f) atomicOr(status, 1);             // |W| too large for the stored-state budget: reported by the host
    const float f = ldexpf(1.0f, -s);
    for (int i = 0; i < d2; ++i) v[i] = x2[(size_t)row * ldx + i];
    for (int rep = 0; rep < (1 << s); ++rep) expm_narrow_action<EX_D, false>(w, d2, f, v, v);
    for (int i = 0; i < d2_pad; ++i) y2[(size_t)row * ldy + i] = i < d2 ? v[i] + pr[d2 * d2 + i] : 0.f;
    ldj[row] = tr;
}

// do [rows, ldo] gets d raw matrix | d shift (pads zero); dscal [rows, 4] the per-point parts of d scale, d shift, d rescale, d reshift
__global__ void expm_train_bwd_kernel(const float* __restrict__ x2, int ldx, const float* __restrict__ o, int ldo, const float* __restrict__ scal4,
                                      const float* __restrict__ dy2, int lddy, const float* __restrict__ dldj, float* __restrict__ dx2, int lddx,
                                      float* __restrict__ dout, int lddo, float* __restrict__ dscal, int rows, int d2, int d2_pad, int no_pad) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const float* pr = o + (size_t)row * ldo;
    float w[EX_D * EX_D], dA[EX_D * EX_D], V[EX_REP + 1][EX_D], T[13][EX_D], lam[EX_D], mu[EX_D];
    float tr, nrm;
    const int s = expm_prepare(pr, d2, scal4, w, tr, nrm);
    const float f = ldexpf(1.0f, -s);
    const int R = 1 << s;
    for (int i = 0; i < d2; ++i) V[0][i] = x2[(size_t)row * ldx + i];
    for (int rep = 0; rep < R; ++rep) expm_narrow_action<EX_D, false>(w, d2, f, V[rep], V[rep + 1]);      // forward again, keeping every state
    for (int i = 0; i < d2 * EX_D; ++i) dA[i] = 0.f;
    for (int i = 0; i < d2; ++i) lam[i] = dy2[(size_t)row * lddy + i];
    for (int rep = R - 1; rep >= 0; --rep) {
        expm_narrow_action<EX_D, true>(w, d2, f, V[rep], nullptr, T);          // terms of this action: t_0 = v, t_k = (f / k) W t_{k-1}
        for (int i = 0; i < d2; ++i) mu[i] = lam[i];              // mu_12
        for (int k = 12; k >= 1; --k) {
            const float fk = f / (float)k;
            // d W += (f / k) mu_k t_{k-1}^T ; mu_{k-1} = lambda + (f / k) W^T mu_k
            float nm[EX_D];
            for (int j = 0; j < d2; ++j) nm[j] = lam[j];
            for (int i = 0; i < d2; ++i) {
                const float mi = mu[i] * fk;
                for (int j = 0; j < d2; ++j) {
                    dA[i * EX_D + j] = fmaf(mi, T[k - 1][j], dA[i * EX_D + j]);
                    nm[j] = fmaf(w[i * EX_D + j], mi, nm[j]);
                }
            }
            for (int j = 0; j < d2; ++j) mu[j] = nm[j];
        }
        for (int i = 0; i < d2; ++i) lam[i] = mu[i];              // adjoint of this action's input
    }
    for (int i = 0; i < d2_pad; ++i) dx2[(size_t)row * lddx + i] = i < d2 ? lam[i] : 0.f;
    // through W = rescale tanh(scale raw + shift) + reshift + 1e-8 (and ldj = tr W)
    const float sc = scal4[0], sh = scal4[1], rs = scal4[2];
    const float gl = dldj[row];
    float g_sc = 0.f, g_sh = 0.f, g_rs = 0.f, g_rsh = 0.f;
    float* dr = dout + (size_t)row * lddo;
    for (int i = 0; i < d2; ++i)
        for (int j = 0; j < d2; ++j) {
            const float gw = dA[i * EX_D + j] + (i == j ? gl : 0.f);
            const float raw = pr[i * d2 + j];
            const float t = tanhf(sc * raw + sh);
            const float gt = gw * rs * (1.0f - t * t);
            dr[i * d2 + j] = gt * sc;
            g_sc += gt * raw; g_sh += gt; g_rs += gw * t; g_rsh += gw;
        }
    for (int i = 0; i < d2; ++i) dr[d2 * d2 + i] = dy2[(size_t)row * lddy + i];
    for (int c = d2 * d2 + d2; c < no_pad; ++c) dr[c] = 0.f;
    dscal[(size_t)row * 4 + 0] = g_sc; dscal[(size_t)row * 4 + 1] = g_sh; dscal[(size_t)row * 4 + 2] = g_rs; dscal[(size_t)row * 4 + 3] = g_rsh;
}

}  // namespace fc

using namespace fc;


extern "C" {

int fc_train_expm_fwd_f32(const float* x2, int32_t ldx, const float* o, int32_t ldo, const float* scal4, float* y2, int32_t ldy, float* ldj, int32_t rows,
                          int32_t d2, int32_t* status, void* stream) {
    FC_API_BEGIN
    if (!x2 || !o || !scal4 || !y2 || !ldj || !status || rows < 1 || d2 < 1 || d2 > kExpmWideMaxD2 || ldx < d2 || ldo < d2 * d2 + d2 || ldy < round_up(d2, 32))
        throw Error(FC_ERR_INVALID, "fc_train_expm_fwd_f32: bad argument (d2 <= 256)");
    hipStream_t s = (hipStream_t)stream;
    if (d2 > EX_D) {      // the inference engine's matrix-exponential action kernel (expm_wide.hip); its bound raises the same status word
        launch_expm_wide(o, ldo, x2, ldx, scal4, y2, ldy, round_up(d2, 32), ldj, 1, rows, d2, 0, (int*)status, nullptr, s);
        return FC_OK;
    }
    launch_kernel<expm_train_fwd_kernel>("fc::expm_train_fwd_kernel", 0.0, 0.0, dim3((rows + 63) / 64), dim3(64), 0, s, x2, ldx, o, ldo, scal4, y2, ldy, ldj, rows, d2,
                                         round_up(d2, 32), (int*)status);
    FC_API_END
}

int fc_train_expm_bwd_f32(const float* x2, int32_t ldx, const float* o, int32_t ldo, const float* scal4, const float* dy2, int32_t lddy, const float* dldj,
                          float* dx2, int32_t lddx, float* dout, int32_t lddo, float* dscal, int32_t rows, int32_t d2, void* stream) {
    FC_API_BEGIN
    if (!x2 || !o || !scal4 || !dy2 || !dldj || !dx2 || !dout || !dscal || rows < 1 || d2 < 1 || d2 > EX_D || ldx < d2 || ldo < d2 * d2 + d2 || lddy < d2 ||
        lddx < round_up(d2, 32) || lddo < round_up(d2 * d2 + d2, 32))
        throw Error(FC_ERR_INVALID, "fc_train_expm_bwd_f32: bad argument (d2 <= 16)");
    launch_kernel<expm_train_bwd_kernel>("fc::expm_train_bwd_kernel", 0.0, 0.0, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, x2, ldx, o, ldo, scal4, dy2, lddy, dldj,
                                         dx2, lddx, dout, lddo, dscal, rows, d2, round_up(d2, 32), round_up(d2 * d2 + d2, 32));
    FC_API_END
}

}  // extern "C"
