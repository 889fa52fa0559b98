// Training's rational-quadratic spline coupling element, forward + backward: spline_train_fwd_kernel,
// rq_spline_bwd_elem, spline_train_bwd_kernel and the entries fc_train_rqspline_fwd_f32 / fc_train_rqspline_bwd_f32.
//   models/spline_coupling.py:24-169 in the REFERENCE's parameter layout: the coupling MLP's output row is [d2][3K+1] =
//   per transformed dim [K width logits | K height logits | K+1 derivative logits] (spline_coupling.py:196-203).  One
//   workgroup per point; forward = the inference element function (spline.h), backward = its analytic gradient w.r.t. x and
//   all 3K+1 logits (through the softmax of the bin widths / heights, the cumulative knots and the softplus derivatives).
#include <hip/hip_runtime.h>

#include "common.h"
#include "device.h"
#include "launch.h"
#include "spline.h"

namespace fc {

// One workgroup per point.  The point's d2 (3K+1) logits are staged through LDS with coalesced 16-byte loads (a thread evaluating one
// dim reads 3K+1 consecutive floats: straight from HBM that is a 100-byte stride across the wave); 3K+1 is odd, so the per-thread
// reads from LDS are conflict-free.
template <int K>
__global__ __launch_bounds__(256) void spline_train_fwd_kernel(const float* __restrict__ x2, int ldx, const float* __restrict__ params, int ldp,
                                                               float* __restrict__ y2, int ldy, float* __restrict__ ldj, int d2, int d2_pad) {
    extern __shared__ float sp[];                        // [d2 (3K+1)] rounded up to 4
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    const int np = d2 * (3 * K + 1), np4 = (np + 3) >> 2;
    const float4* src = reinterpret_cast<const float4*>(params + row * ldp);          // panel rows are 16-byte aligned, ldp >= round_up(np, 32)
    for (int i = threadIdx.x; i < np4; i += 256) reinterpret_cast<float4*>(sp)[i] = src[i];
    __syncthreads();
    float part = 0.f;
    for (int dim = threadIdx.x; dim < d2_pad; dim += 256) {
        float y = 0.f, lad = 0.f;
        if (dim < d2) rq_spline_elem<K>(x2[row * ldx + dim], sp + dim * (3 * K + 1), 1, false, y, lad);
        y2[row * ldy + dim] = y;
        part += lad;
    }
    const float s = block_sum_256(part, red);
    if (threadIdx.x == 0) ldj[row] = s;
}

// gradient of (y, lad) of ONE spline element: gx = dL/dx, gu[3K+1] = dL/d logits, given gy = dL/dy and gl = dL/dlad
template <int K>
__device__ __forceinline__ void rq_spline_bwd_elem(float x, const float* __restrict__ u, float gy, float gl, float& gx, float* __restrict__ gu) {
    constexpr float B = RQ_BOUND, MINW = RQ_MIN_W, MINH = RQ_MIN_H, MIND = RQ_MIN_D;
    if (!(x >= -B && x <= B)) {
        gx = gy;
#pragma unroll
        for (int i = 0; i < 3 * K + 1; ++i) gu[i] = 0.f;
        return;
    }
    // softmax probabilities and cumulative knots of the widths (pass 0) and heights (pass 1), as in rq_spline_elem (spline.h) but in this
    // routine's own arithmetic (expf, true division) and with the probabilities kept: sharing that block would change training bits
    float probs[2][K], knots[2][K + 1];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const float min_size = hh ? MINH : MINW;
        float* p = probs[hh];
        float mx = u[hh * K];
#pragma unroll
        for (int i = 0; i < K; ++i) { p[i] = u[hh * K + i]; mx = fmaxf(mx, p[i]); }
        float sum = 0.f;
        rq_prefix<K> se, sc;                 // the forward's summation order (spline.h): blocks of four at 16 bins, so both pick their bins from knots summed alike
#pragma unroll
        for (int i = 0; i < K; ++i) { p[i] = expf(p[i] - mx); sum = se.add(i, p[i]); }
        knots[hh][0] = -B;
#pragma unroll
        for (int i = 0; i < K; ++i) { p[i] = p[i] / sum; const float c = sc.add(i, min_size + (1.0f - min_size * K) * p[i]); knots[hh][i + 1] = 2.0f * B * c - B; }
        knots[hh][K] = B;
    }
    const float (&pw)[K] = probs[0], (&ph)[K] = probs[1], (&cw)[K + 1] = knots[0], (&ch)[K + 1] = knots[1];
    int bin = 0;
#pragma unroll
    for (int i = 1; i <= K; ++i) bin += (x >= cw[i] + (i == K ? RQ_SEARCH_EPS : 0.f)) ? 1 : 0;
    float in_cw = cw[0], w = cw[1] - cw[0], in_ch = ch[0], h = ch[1] - ch[0];
    float raw0 = RQ_PAD_LOGIT, raw1 = u[2 * K];
#pragma unroll
    for (int i = 1; i < K; ++i)
        if (bin == i) { in_cw = cw[i]; w = cw[i + 1] - cw[i]; in_ch = ch[i]; h = ch[i + 1] - ch[i]; raw0 = u[2 * K + i - 1]; raw1 = u[2 * K + i]; }
    auto softplus = [](float v) { return v > 20.f ? v : log1pf(expf(v)); };
    auto sigmoid = [](float v) { return 1.0f / (1.0f + expf(-v)); };
    const float d0 = MIND + softplus(raw0), d1 = MIND + softplus(raw1);
    const float s = h / w;
    const float th = (x - in_cw) / w, omt = 1.0f - th, tt = th * omt;
    const float A = s * th * th + d0 * tt;
    const float E = d0 + d1 - 2.0f * s;
    const float den = s + E * tt;
    const float G = d1 * th * th + 2.0f * s * tt + d0 * omt * omt;
    const float rden = 1.0f / den, rG = 1.0f / G;
    const float dtt = 1.0f - 2.0f * th;
    // y = ch + h A / den ; lad = 2 log s + log G - 2 log den
    const float y_A = h * rden, y_den = -h * A * rden * rden;
    const float g_th = gy * (y_A * (2.0f * s * th + d0 * dtt) + y_den * (E * dtt)) +
                       gl * ((2.0f * d1 * th + 2.0f * s * dtt - 2.0f * d0 * omt) * rG - 2.0f * E * dtt * rden);
    const float g_s = gy * (y_A * th * th + y_den * (1.0f - 2.0f * tt)) + gl * (2.0f / s + 2.0f * tt * rG - 2.0f * (1.0f - 2.0f * tt) * rden);
    const float g_d0 = gy * (y_A * tt + y_den * tt) + gl * (omt * omt * rG - 2.0f * tt * rden);
    const float g_d1 = gy * (y_den * tt) + gl * (th * th * rG - 2.0f * tt * rden);
    const float g_h = gy * A * rden + g_s / w;                              // direct + through s = h / w
    const float g_w = -g_s * s / w - g_th * th / w;                         // through s and through th = (x - cw) / w
    const float g_cw = -g_th / w;
    gx = g_th / w;
    // widths: bin b owns w_b = 2B p_b and its left knot cw_b = -B + sum_{k<b} w_k ; p = MIN + (1 - K MIN) softmax(u)
    {
        float gs[K], dot = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float gwk = (k < bin ? g_cw : 0.f) + (k == bin ? g_w : 0.f);
            gs[k] = 2.0f * B * (1.0f - MINW * K) * gwk;
            dot += pw[k] * gs[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) gu[k] = pw[k] * (gs[k] - dot);
    }
    {
        float gs[K], dot = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float ghk = (k < bin ? gy : 0.f) + (k == bin ? g_h : 0.f);       // d y / d ch_b = 1
            gs[k] = 2.0f * B * (1.0f - MINH * K) * ghk;
            dot += ph[k] * gs[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) gu[K + k] = ph[k] * (gs[k] - dot);
    }
    // derivative logits: knot j >= 1 uses logit j-1 (knot 0 is the padded constant, the last logit is never read)
    const float gr0 = g_d0 * sigmoid(raw0), gr1 = g_d1 * sigmoid(raw1);
#pragma unroll
    for (int j = 0; j <= K; ++j) gu[2 * K + j] = (j == bin - 1 ? gr0 : 0.f) + (j == bin ? gr1 : 0.f);
}

template <int K>
__global__ __launch_bounds__(256) void spline_train_bwd_kernel(const float* __restrict__ x2, int ldx, const float* __restrict__ params, int ldp,
                                                               const float* __restrict__ dy2, int lddy, const float* __restrict__ dldj,
                                                               float* __restrict__ dx2, int lddx, float* __restrict__ dparams, int lddp, int d2,
                                                               int d2_pad, int np_pad, float* __restrict__ rowmax) {
    extern __shared__ float sp[];                        // logits in, their gradients out (in place): [round_up(d2 (3K+1), 32)]
    const size_t row = blockIdx.x;
    const int np = d2 * (3 * K + 1), np4 = (np + 3) >> 2;
    const float4* src = reinterpret_cast<const float4*>(params + row * ldp);
    for (int i = threadIdx.x; i < np4; i += 256) reinterpret_cast<float4*>(sp)[i] = src[i];
    __syncthreads();
    const float gl = dldj[row];
    for (int dim = threadIdx.x; dim < d2_pad; dim += 256) {
        float gx = 0.f;
        if (dim < d2) {
            float gu[3 * K + 1];
            float* u = sp + dim * (3 * K + 1);
            rq_spline_bwd_elem<K>(x2[row * ldx + dim], u, dy2[row * lddy + dim], gl, gx, gu);
#pragma unroll
            for (int i = 0; i < 3 * K + 1; ++i) u[i] = gu[i];                  // this thread's own logits: nobody else reads them
        }
        dx2[row * lddx + dim] = gx;
    }
    for (int c = np + threadIdx.x; c < np_pad; c += 256) sp[c] = 0.f;
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(dparams + row * lddp);
    float m = 0.f;
    for (int i = threadIdx.x; i < (np_pad >> 2); i += 256) {
        const float4 v = reinterpret_cast<const float4*>(sp)[i];
        dst[i] = v;
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        if (!(v.x == v.x && v.y == v.y && v.z == v.z && v.w == v.w)) m = INFINITY;      // (fmaxf drops a NaN: the consumer must see it)
    }
    if (rowmax) {
        // max |row| for the data-gradient GEMM of the parameter layer (the caller's buffer, fc_train_rqspline_bwd_f32)
        __shared__ float red[4];
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) rowmax[row] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
}

template <int K>
static void spline_fwd_k(const float* x2, int ldx, const float* params, int ldp, float* y2, int ldy, float* ldj, int rows, int d2, hipStream_t s) {
    const size_t lds = (size_t)round_up(d2 * (3 * K + 1), 32) * sizeof(float);
    if (lds > 60 * 1024) throw Error(FC_ERR_UNSUPPORTED, "training spline: more than 15360 logits per point");
    launch_kernel<spline_train_fwd_kernel<K>>("fc::spline_train_fwd_kernel", 0.0, (double)rows * d2 * (3 * K + 3) * 4.0, dim3(rows), dim3(256), lds, s, x2, ldx, params, ldp,
                                              y2, ldy, ldj, d2, round_up(d2, 32));
}
template <int K>
static void spline_bwd_k(const float* x2, int ldx, const float* params, int ldp, const float* dy2, int lddy, const float* dldj, float* dx2, int lddx,
                         float* dparams, int lddp, int rows, int d2, float* rowmax, hipStream_t s) {
    // rows beyond `rows` of the row-maximum buffer (the GEMM reads a multiple of 256) are zero: scale 1 on zero rows
    const int rows_pad = round_up(rows, ROW_PAD);
    if (rowmax && rows_pad > rows) FC_HIP(hipMemsetAsync(rowmax + rows, 0, (size_t)(rows_pad - rows) * 4, s));
    const size_t lds = (size_t)round_up(d2 * (3 * K + 1), 32) * sizeof(float);
    if (lds > 60 * 1024) throw Error(FC_ERR_UNSUPPORTED, "training spline: more than 15360 logits per point");
    launch_kernel<spline_train_bwd_kernel<K>>("fc::spline_train_bwd_kernel", 0.0, (double)rows * d2 * (6 * K + 5) * 4.0, dim3(rows), dim3(256), lds, s, x2, ldx, params, ldp,
                                              dy2, lddy, dldj, dx2, lddx, dparams, lddp, d2, round_up(d2, 32), round_up(d2 * (3 * K + 1), 32), rowmax);
}

}  // namespace fc

using namespace fc;


extern "C" {

int fc_train_rqspline_fwd_f32(const float* x2, int32_t ldx, const float* params, int32_t ldp, float* y2, int32_t ldy, float* ldj, int32_t rows,
                              int32_t d2, int32_t K, void* stream) {
    FC_API_BEGIN
    if (!x2 || !params || !y2 || !ldj || rows < 1 || d2 < 1 || ldx < d2 || ldy < round_up(d2, 32) || ldp < round_up(d2 * (3 * K + 1), 4) || ldp % 4 != 0 ||
        ((uintptr_t)params & 15))
        throw Error(FC_ERR_INVALID, "fc_train_rqspline_fwd_f32: bad argument (params: 16-byte aligned rows, pitch a multiple of 4)");
    hipStream_t s = (hipStream_t)stream;
    spline_bins_require(K, "fc_train_rqspline_fwd_f32: num_bins", [&](auto k) { spline_fwd_k<decltype(k)::value>(x2, ldx, params, ldp, y2, ldy, ldj, rows, d2, s); });
    FC_API_END
}

int fc_train_rqspline_bwd_f32(const float* x2, int32_t ldx, const float* params, int32_t ldp, const float* dy2, int32_t lddy, const float* dldj,
                              float* dx2, int32_t lddx, float* dparams, int32_t lddp, int32_t rows, int32_t d2, int32_t K, float* row_absmax,
                              void* stream) {
    FC_API_BEGIN
    if (!x2 || !params || !dy2 || !dldj || !dx2 || !dparams || rows < 1 || d2 < 1 || ldx < d2 || lddy < d2 || lddx < round_up(d2, 32) ||
        ldp < round_up(d2 * (3 * K + 1), 4) || ldp % 4 != 0 || lddp < round_up(d2 * (3 * K + 1), 32) || lddp % 4 != 0 || (((uintptr_t)params | (uintptr_t)dparams) & 15))
        throw Error(FC_ERR_INVALID, "fc_train_rqspline_bwd_f32: bad argument (params / dparams: 16-byte aligned rows, pitches multiples of 4)");
    hipStream_t s = (hipStream_t)stream;
    spline_bins_require(K, "fc_train_rqspline_bwd_f32: num_bins", [&](auto k) {
        spline_bwd_k<decltype(k)::value>(x2, ldx, params, ldp, dy2, lddy, dldj, dx2, lddx, dparams, lddp, rows, d2, row_absmax, s);
    });
    FC_API_END
}

}  // extern "C"
