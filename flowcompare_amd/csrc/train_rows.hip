// Training's row-wise element operators other than the spline (train_spline.hip) and the ExponentialCoupling (train_expm.hip), forward +
// backward, with their ten entries fc_train_{layernorm,affine,gauss,normlp,base}_{fwd,bwd}_f32:
//   layernorm  torch.nn.LayerNorm(width, eps 1e-5) of PreNorm (models/perceiver.py:18-27), one wave per row; backward returns dx and the
//            panel dy * xhat whose column sums are d gamma (d beta = column sums of dy), reduced by fc_train_colsum_f32 in a fixed order.
//   affine, gauss, normlp, base   the flow's per-element closures, one workgroup per point: the affine coupling, the augmenter's Gauss
//            draw, the Slice's Normal log-probability and the base density; row sums by block_sum_256 (device.h).
#include <hip/hip_runtime.h>

#include "common.h"
#include "device.h"
#include "launch.h"

namespace fc {

// ---------------------------------------------------------------- LayerNorm: one wave per row
__global__ __launch_bounds__(256) void layernorm_train_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* __restrict__ y, int ldy,
                                                                  float* __restrict__ stats, int rows, int width, int width_pad, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * ldx;
    float s = 0.f;
    for (int c = lane; c < width; c += 64) s += xr[c];
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    const float mean = s / width;
    float v = 0.f;
    for (int c = lane; c < width; c += 64) { const float d = xr[c] - mean; v += d * d; }
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    const float rstd = 1.0f / sqrtf(v / width + eps);
    for (int c = lane; c < width_pad; c += 64) y[(size_t)row * ldy + c] = c < width ? (xr[c] - mean) * rstd * gamma[c] + beta[c] : 0.f;
    if (lane == 0) { stats[2 * (size_t)row] = mean; stats[2 * (size_t)row + 1] = rstd; }
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma ; t = dy xhat (column sums = d gamma)
__global__ __launch_bounds__(256) void layernorm_train_bwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                                  const float* __restrict__ dy, int lddy, const float* __restrict__ stats,
                                                                  float* __restrict__ dx, int lddx, float* __restrict__ t, int ldt, int rows,
                                                                  int rows_pad, int width, int width_pad) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows_pad) return;
    if (row >= rows) {
        for (int c = lane; c < width_pad; c += 64) { dx[(size_t)row * lddx + c] = 0.f; t[(size_t)row * ldt + c] = 0.f; }
        return;
    }
    const float mean = stats[2 * (size_t)row], rstd = stats[2 * (size_t)row + 1];
    const float* xr = x + (size_t)row * ldx;
    const float* gr = dy + (size_t)row * lddy;
    float a = 0.f, b = 0.f;
    for (int c = lane; c < width; c += 64) {
        const float g = gr[c] * gamma[c], xh = (xr[c] - mean) * rstd;
        a += g; b += g * xh;
    }
    for (int m = 1; m < 64; m <<= 1) { a += __shfl_xor(a, m, 64); b += __shfl_xor(b, m, 64); }
    a /= width; b /= width;
    for (int c = lane; c < width_pad; c += 64) {
        float o = 0.f, tv = 0.f;
        if (c < width) {
            const float xh = (xr[c] - mean) * rstd;
            o = rstd * (gr[c] * gamma[c] - a - xh * b);
            tv = gr[c] * xh;
        }
        dx[(size_t)row * lddx + c] = o;
        t[(size_t)row * ldt + c] = tv;
    }
}


// ---------------------------------------------------------------- the three per-element closures of the flow, one workgroup per point
// affine coupling (models/affine_coupling.py:23-46): st = [raw scale d2 | shift d2];  y2 = x2 s + t,  ldj = sum log s
__device__ __forceinline__ float affine_scale(float raw, int scale_fn, float& ds) {
    if (scale_fn == FC_SCALE_EXP) { const float s = expf(raw); ds = s; return s; }
    const float sg = 1.0f / (1.0f + expf(-raw));
    ds = 2.0f * sg * (1.0f - sg) * (float)(1.0 - 1e-8);
    return (2.0f * sg - 1.0f) * (float)(1.0 - 1e-8) + 1.0f;
}
__global__ __launch_bounds__(256) void affine_train_fwd_kernel(const float* __restrict__ x2, int ldx, const float* __restrict__ st, int ldst,
                                                               float* __restrict__ y2, int ldy, float* __restrict__ ldj, int d2, int d2_pad, int scale_fn) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    float part = 0.f;
    for (int j = threadIdx.x; j < d2_pad; j += 256) {
        float y = 0.f;
        if (j < d2) {
            float ds;
            const float s = affine_scale(st[row * ldst + j], scale_fn, ds);
            y = x2[row * ldx + j] * s + st[row * ldst + d2 + j];
            part += logf(s);
        }
        y2[row * ldy + j] = y;
    }
    const float tot = block_sum_256(part, red);
    if (threadIdx.x == 0) ldj[row] = tot;
}
__global__ __launch_bounds__(256) void affine_train_bwd_kernel(const float* __restrict__ x2, int ldx, const float* __restrict__ st, int ldst,
                                                               const float* __restrict__ dy2, int lddy, const float* __restrict__ dldj,
                                                               float* __restrict__ dx2, int lddx, float* __restrict__ dst, int lddst, int d2,
                                                               int d2_pad, int nst_pad, int scale_fn) {
    const size_t row = blockIdx.x;
    const float gl = dldj[row];
    for (int j = threadIdx.x; j < d2_pad; j += 256) {
        float gx = 0.f;
        if (j < d2) {
            float ds;
            const float s = affine_scale(st[row * ldst + j], scale_fn, ds);
            const float gy = dy2[row * lddy + j];
            gx = gy * s;
            dst[row * lddst + j] = (gy * x2[row * ldx + j] + gl / s) * ds;
            dst[row * lddst + d2 + j] = gy;
        }
        dx2[row * lddx + j] = gx;
    }
    for (int c = 2 * d2 + threadIdx.x; c < nst_pad; c += 256) dst[row * lddst + c] = 0.f;
}

// augmenter draw (models/augmenter.py:49-63, distributions.py:128-153): p = [mean nz | log std nz];  z = mean + eps exp(log std),
// ldj = -log N(z; mean, std) summed = sum (eps^2 / 2 + log std + log(2 pi) / 2)
__global__ __launch_bounds__(256) void gauss_train_fwd_kernel(const float* __restrict__ p, int ldp, const float* __restrict__ eps, float* __restrict__ z,
                                                              int ldz, float* __restrict__ ldj, int nz, int nz_pad, float clamp) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    float part = 0.f;
    for (int j = threadIdx.x; j < nz_pad; j += 256) {
        float v = 0.f;
        if (j < nz) {
            const float e = eps[row * nz + j], ls = p[row * ldp + nz + j];
            float sc = expf(ls), lsc = ls;
            if (clamp > 0.f && sc > clamp) { sc = clamp; lsc = logf(clamp); }          // distributions.py:134-137 (clamp_max on the std)
            v = p[row * ldp + j] + e * sc;
            part += 0.5f * e * e + lsc + 0.91893853320467274178f;
        }
        z[row * ldz + j] = v;
    }
    const float tot = block_sum_256(part, red);
    if (threadIdx.x == 0) ldj[row] = tot;
}
__global__ __launch_bounds__(256) void gauss_train_bwd_kernel(const float* __restrict__ p, int ldp, const float* __restrict__ eps,
                                                              const float* __restrict__ dz, int lddz, const float* __restrict__ dldj,
                                                              float* __restrict__ dp, int lddp, int nz, int np_pad, float clamp) {
    const size_t row = blockIdx.x;
    const float gl = dldj[row];
    for (int j = threadIdx.x; j < nz; j += 256) {
        const float g = dz[row * lddz + j];
        const float sc = expf(p[row * ldp + nz + j]);
        dp[row * lddp + j] = g;
        dp[row * lddp + nz + j] = (clamp > 0.f && sc > clamp) ? 0.f : g * eps[row * nz + j] * sc + gl;
    }
    for (int c = 2 * nz + threadIdx.x; c < np_pad; c += 256) dp[row * lddp + c] = 0.f;
}

// Slice (models/slice.py:31-44 + distributions.py:140-142): out[row] = sum_j log N(v_j; mean_j, std_j), p = [mean nz | log std nz]
__global__ __launch_bounds__(256) void normlp_train_fwd_kernel(const float* __restrict__ v, int ldv, const float* __restrict__ p, int ldp,
                                                               float* __restrict__ out, int nz, float clamp) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    float part = 0.f;
    for (int j = threadIdx.x; j < nz; j += 256) {
        const float ls = p[row * ldp + nz + j];
        float sc = expf(ls), lsc = ls;
        if (clamp > 0.f && sc > clamp) { sc = clamp; lsc = logf(clamp); }
        const float d = (v[row * ldv + j] - p[row * ldp + j]) / sc;
        part += -0.5f * d * d - lsc - 0.91893853320467274178f;
    }
    const float tot = block_sum_256(part, red);
    if (threadIdx.x == 0) out[row] = tot;
}
__global__ __launch_bounds__(256) void normlp_train_bwd_kernel(const float* __restrict__ v, int ldv, const float* __restrict__ p, int ldp,
                                                               const float* __restrict__ g, float* __restrict__ dv, int lddv, float* __restrict__ dp,
                                                               int lddp, int nz, int nz_pad, int np_pad, float clamp) {
    const size_t row = blockIdx.x;
    const float gr = g[row];
    for (int j = threadIdx.x; j < nz_pad; j += 256) {
        float gv = 0.f;
        if (j < nz) {
            const float sc0 = expf(p[row * ldp + nz + j]);
            const bool cl = clamp > 0.f && sc0 > clamp;
            const float sc = cl ? clamp : sc0;
            const float d = (v[row * ldv + j] - p[row * ldp + j]) / sc;
            gv = -gr * d / sc;
            dp[row * lddp + j] = -gv;
            dp[row * lddp + nz + j] = cl ? 0.f : gr * (d * d - 1.0f);
        }
        dv[row * lddv + j] = gv;
    }
    for (int c = 2 * nz + threadIdx.x; c < np_pad; c += 256) dp[row * lddp + c] = 0.f;
}

// base density (models/distributions.py:192-195): out[row] = sum_c (-x^2 / 2 - log(2 pi) / 2) over `width` columns
__global__ __launch_bounds__(256) void base_train_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int width) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    float part = 0.f;
    for (int j = threadIdx.x; j < width; j += 256) { const float v = x[row * ldx + j]; part -= 0.5f * v * v; }
    const float tot = block_sum_256(part, red);
    if (threadIdx.x == 0) out[row] = tot - 0.91893853320467274178f * width;
}
__global__ __launch_bounds__(256) void base_train_bwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ g, float* __restrict__ dx,
                                                             int lddx, int width, int width_pad) {
    const size_t row = blockIdx.x;
    const float gr = g[row];
    for (int j = threadIdx.x; j < width_pad; j += 256) dx[row * lddx + j] = j < width ? -x[row * ldx + j] * gr : 0.f;
}

}  // namespace fc

using namespace fc;


extern "C" {

int fc_train_layernorm_fwd_f32(const float* x, int32_t ldx, const float* gamma, const float* beta, float* y, int32_t ldy, float* stats,
                               int32_t rows, int32_t width, float eps, void* stream) {
    FC_API_BEGIN
    if (!x || !gamma || !beta || !y || !stats || rows < 1 || width < 1 || ldx < width || ldy < round_up(width, 32))
        throw Error(FC_ERR_INVALID, "fc_train_layernorm_fwd_f32: bad argument");
    launch_kernel<layernorm_train_fwd_kernel>("fc::layernorm_train_fwd_kernel", 0.0, (double)rows * width * 8.0, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx,
                                              gamma, beta, y, ldy, stats, rows, width, round_up(width, 32), eps);
    FC_API_END
}

int fc_train_layernorm_bwd_f32(const float* x, int32_t ldx, const float* gamma, const float* dy, int32_t lddy, const float* stats, float* dx,
                               int32_t lddx, float* dy_xhat, int32_t ldt, int32_t rows_pad, int32_t rows, int32_t width, void* stream) {
    FC_API_BEGIN
    if (!x || !gamma || !dy || !stats || !dx || !dy_xhat || rows < 1 || rows_pad < rows || width < 1 || ldx < width || lddy < width ||
        lddx < round_up(width, 32) || ldt < round_up(width, 32))
        throw Error(FC_ERR_INVALID, "fc_train_layernorm_bwd_f32: bad argument");
    launch_kernel<layernorm_train_bwd_kernel>("fc::layernorm_train_bwd_kernel", 0.0, (double)rows * width * 16.0, dim3((rows_pad + 3) / 4), dim3(256), 0, (hipStream_t)stream, x,
                                              ldx, gamma, dy, lddy, stats, dx, lddx, dy_xhat, ldt, rows, rows_pad, width, round_up(width, 32));
    FC_API_END
}

int fc_train_affine_fwd_f32(const float* x2, int32_t ldx, const float* st, int32_t ldst, float* y2, int32_t ldy, float* ldj, int32_t rows, int32_t d2,
                            int32_t scale_fn, void* stream) {
    FC_API_BEGIN
    if (!x2 || !st || !y2 || !ldj || rows < 1 || d2 < 1 || ldx < d2 || ldst < 2 * d2 || ldy < round_up(d2, 32)) throw Error(FC_ERR_INVALID, "fc_train_affine_fwd_f32: bad argument");
    launch_kernel<affine_train_fwd_kernel>("fc::affine_train_fwd_kernel", 0.0, (double)rows * d2 * 16.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, x2, ldx, st, ldst, y2, ldy,
                                           ldj, d2, round_up(d2, 32), scale_fn);
    FC_API_END
}

int fc_train_affine_bwd_f32(const float* x2, int32_t ldx, const float* st, int32_t ldst, const float* dy2, int32_t lddy, const float* dldj, float* dx2,
                            int32_t lddx, float* dst, int32_t lddst, int32_t rows, int32_t d2, int32_t scale_fn, void* stream) {
    FC_API_BEGIN
    if (!x2 || !st || !dy2 || !dldj || !dx2 || !dst || rows < 1 || d2 < 1 || ldx < d2 || ldst < 2 * d2 || lddy < d2 || lddx < round_up(d2, 32) ||
        lddst < round_up(2 * d2, 32))
        throw Error(FC_ERR_INVALID, "fc_train_affine_bwd_f32: bad argument");
    launch_kernel<affine_train_bwd_kernel>("fc::affine_train_bwd_kernel", 0.0, (double)rows * d2 * 28.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, x2, ldx, st, ldst, dy2, lddy,
                                           dldj, dx2, lddx, dst, lddst, d2, round_up(d2, 32), round_up(2 * d2, 32), scale_fn);
    FC_API_END
}

int fc_train_gauss_fwd_f32(const float* p, int32_t ldp, const float* eps, float* z, int32_t ldz, float* ldj, int32_t rows, int32_t nz, float clamp,
                           void* stream) {
    FC_API_BEGIN
    if (!p || !eps || !z || !ldj || rows < 1 || nz < 1 || ldp < 2 * nz || ldz < round_up(nz, 32)) throw Error(FC_ERR_INVALID, "fc_train_gauss_fwd_f32: bad argument");
    launch_kernel<gauss_train_fwd_kernel>("fc::gauss_train_fwd_kernel", 0.0, (double)rows * nz * 16.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, p, ldp, eps, z, ldz, ldj, nz,
                                          round_up(nz, 32), clamp);
    FC_API_END
}

int fc_train_gauss_bwd_f32(const float* p, int32_t ldp, const float* eps, const float* dz, int32_t lddz, const float* dldj, float* dp, int32_t lddp,
                           int32_t rows, int32_t nz, float clamp, void* stream) {
    FC_API_BEGIN
    if (!p || !eps || !dz || !dldj || !dp || rows < 1 || nz < 1 || ldp < 2 * nz || lddz < nz || lddp < round_up(2 * nz, 32))
        throw Error(FC_ERR_INVALID, "fc_train_gauss_bwd_f32: bad argument");
    launch_kernel<gauss_train_bwd_kernel>("fc::gauss_train_bwd_kernel", 0.0, (double)rows * nz * 24.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, p, ldp, eps, dz, lddz, dldj,
                                          dp, lddp, nz, round_up(2 * nz, 32), clamp);
    FC_API_END
}

int fc_train_normlp_fwd_f32(const float* v, int32_t ldv, const float* p, int32_t ldp, float* out, int32_t rows, int32_t nz, float clamp, void* stream) {
    FC_API_BEGIN
    if (!v || !p || !out || rows < 1 || nz < 1 || ldv < nz || ldp < 2 * nz) throw Error(FC_ERR_INVALID, "fc_train_normlp_fwd_f32: bad argument");
    launch_kernel<normlp_train_fwd_kernel>("fc::normlp_train_fwd_kernel", 0.0, (double)rows * nz * 12.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, v, ldv, p, ldp, out, nz, clamp);
    FC_API_END
}

int fc_train_normlp_bwd_f32(const float* v, int32_t ldv, const float* p, int32_t ldp, const float* g, float* dv, int32_t lddv, float* dp, int32_t lddp,
                            int32_t rows, int32_t nz, float clamp, void* stream) {
    FC_API_BEGIN
    if (!v || !p || !g || !dv || !dp || rows < 1 || nz < 1 || ldv < nz || ldp < 2 * nz || lddv < round_up(nz, 32) || lddp < round_up(2 * nz, 32))
        throw Error(FC_ERR_INVALID, "fc_train_normlp_bwd_f32: bad argument");
    launch_kernel<normlp_train_bwd_kernel>("fc::normlp_train_bwd_kernel", 0.0, (double)rows * nz * 24.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, v, ldv, p, ldp, g, dv, lddv,
                                           dp, lddp, nz, round_up(nz, 32), round_up(2 * nz, 32), clamp);
    FC_API_END
}

int fc_train_base_fwd_f32(const float* x, int32_t ldx, float* out, int32_t rows, int32_t width, void* stream) {
    FC_API_BEGIN
    if (!x || !out || rows < 1 || width < 1 || ldx < width) throw Error(FC_ERR_INVALID, "fc_train_base_fwd_f32: bad argument");
    launch_kernel<base_train_fwd_kernel>("fc::base_train_fwd_kernel", 0.0, (double)rows * width * 4.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, ldx, out, width);
    FC_API_END
}

int fc_train_base_bwd_f32(const float* x, int32_t ldx, const float* g, float* dx, int32_t lddx, int32_t rows, int32_t width, void* stream) {
    FC_API_BEGIN
    if (!x || !g || !dx || rows < 1 || width < 1 || ldx < width || lddx < round_up(width, 32)) throw Error(FC_ERR_INVALID, "fc_train_base_bwd_f32: bad argument");
    launch_kernel<base_train_bwd_kernel>("fc::base_train_bwd_kernel", 0.0, (double)rows * width * 8.0, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, ldx, g, dx, lddx, width,
                                         round_up(width, 32));
    FC_API_END
}

}  // extern "C"
