// HBM-bound helper kernels of the flow engine: layout packing, LayerNorm, base density, the
// rational-quadratic spline, DGCNN gather-max and global pooling.  All are one-wave-per-row streaming
// kernels (coalesced row reads, wave reductions via DPP shuffles); none of them is reshaped into a GEMM.
#include "common.h"
#include "device.h"
#include "expm_narrow.h"
#include "launch.h"
#include "spline.h"

namespace fc {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// ---------------------------------------------------------------- limb images of a packed weight matrix (fc_*_create)
// One thread per (row, k16 block, element): W3 [rows][K/16][3][16] bf16 limbs (hi, mid, lo: x = hi + mid + lo to 24 bits), W2
// [rows][K/16][2][16] fp16 limbs (hi, lo' = (x - hi) * 2048) -- the roundings of hostpack.cpp make_bf16_limbs / make_f16_limbs.
__global__ void limb_images_kernel(const float* __restrict__ W, size_t n, int K_pad, unsigned short* __restrict__ W3, unsigned short* __restrict__ W2) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t row = t / K_pad;
    const int k = (int)(t - row * K_pad);
    const float x = W[t];
    const size_t blk = row * (K_pad / 16) + k / 16;
    const int e = k & 15;
    const __bf16 h = (__bf16)x;
    const float r1 = x - (float)h;
    const __bf16 m = (__bf16)r1;
    const __bf16 l = (__bf16)(r1 - (float)m);
    W3[blk * 48 + e] = __builtin_bit_cast(unsigned short, h);
    W3[blk * 48 + 16 + e] = __builtin_bit_cast(unsigned short, m);
    W3[blk * 48 + 32 + e] = __builtin_bit_cast(unsigned short, l);
    if (W2) {
        const _Float16 h16 = (_Float16)x;
        const _Float16 l16 = (_Float16)((x - (float)h16) * 2048.0f);
        W2[blk * 32 + e] = __builtin_bit_cast(unsigned short, h16);
        W2[blk * 32 + 16 + e] = __builtin_bit_cast(unsigned short, l16);
    }
}
void launch_limb_images(const float* W, int rows, int K_pad, unsigned short* W3, unsigned short* W2, hipStream_t s) {
    const size_t n = (size_t)rows * K_pad;
    if (!n) return;
    launch_kernel<limb_images_kernel>(nullptr, 0.0, 0.0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, n, K_pad, W3, W2);
}

// ---------------------------------------------------------------- pack / fill
// dst[row, dst_col0 + c] = src[row, c] for c < src_cols ; zero for src_cols <= c < zero_to
__global__ void pack_rows_kernel(const float* __restrict__ src, int src_ld, int src_cols, float* __restrict__ dst, int dst_ld,
                                 int dst_col0, int zero_to, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    for (int c = lane; c < zero_to; c += 64)
        dst[(size_t)row * dst_ld + dst_col0 + c] = c < src_cols ? src[(size_t)row * src_ld + c] : 0.f;
}
void launch_pack_rows(const float* src, int src_ld, int src_cols, float* dst, int dst_ld, int dst_col0, int zero_to, int rows,
                      hipStream_t s) {
    if (rows <= 0) return;
    launch_kernel<pack_rows_kernel>("fc::pack_rows_kernel", 0.0, 4.0 * rows * ((double)src_cols + zero_to), dim3((rows + 3) / 4), dim3(256), 0, s, src, src_ld, src_cols,
                                    dst, dst_ld, dst_col0, zero_to, rows);
}

__global__ void fill_kernel(float* p, float v, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) p[i] = v;
}
void launch_fill(float* p, float v, size_t n, hipStream_t s) {
    if (!n) return;
    size_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    launch_kernel<fill_kernel>("fc::fill_kernel", 0.0, 4.0 * n, dim3((unsigned)blocks), dim3(256), 0, s, p, v, n);
}

// Per-scene context point counts (fcflow_context_counts.h): rows >= the scene's count of a [B][M][ld] panel := 0, so that what a caller left in
// its pad rows (a NaN, a value beyond fp16's range) reaches neither a limb image's range flag nor the K|V projection.  blockIdx.y = scene,
// one 16-byte store per thread; the count is clamped like the attention kernels clamp it.
__global__ __launch_bounds__(256) void zero_pad_rows_kernel(float* __restrict__ panel, int ld4, const int* __restrict__ m_counts, int M) {
    const int b = blockIdx.y;
    const int Mb = attn_scene_keys(m_counts, b, M);
    const long i = (long)blockIdx.x * 256 + threadIdx.x + (long)Mb * ld4;      // float4 index inside the scene, starting at its first pad row
    if (i < (long)M * ld4) reinterpret_cast<float4*>(panel)[(size_t)b * M * ld4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
void launch_zero_pad_rows(float* panel, int ld, const int32_t* m_counts, int B, int M, hipStream_t s) {
    if (!m_counts || B <= 0 || M <= 1) return;                                  // (a count is at least 1: one key has no pad row)
    if (ld % 4 != 0 || ((uintptr_t)panel & 15)) throw Error(FC_ERR_INVALID, "zero_pad_rows: the panel must be 16-byte aligned with a pitch that is a multiple of 4 floats");
    const long n4 = (long)(M - 1) * (ld / 4);                                   // the most pad a scene can have
    launch_kernel<zero_pad_rows_kernel>("fc::zero_pad_rows_kernel", 0.0, 16.0 * (double)n4 * B, dim3((unsigned)((n4 + 255) / 256), B), dim3(256), 0, s, panel, ld / 4, m_counts, M);
}

// extra context [B, X] -> per-point scalar rowscal[b*N + i] = extra[b, 0]   (inner_loop's einops.repeat, X == 1)
__global__ void repeat_extra_kernel(const float* extra, int X, float* rowscal, int B, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B * N) rowscal[i] = extra[(size_t)(i / N) * X];
}
void launch_repeat_extra(const float* extra, int X, float* rowscal, int B, int N, hipStream_t s) {
    launch_kernel<repeat_extra_kernel>(nullptr, 0.0, 0.0, dim3((B * N + 255) / 256), dim3(256), 0, s, extra, X, rowscal, B, N);
}

// ---------------------------------------------------------------- LayerNorm (no affine: gamma/beta are folded into the q projection)
// models/perceiver.py:18-26 -> torch.nn.LayerNorm(width), biased variance, eps 1e-5.  In place.
__global__ void layernorm_kernel(float* h, int ld, int width, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* p = h + (size_t)row * ld;
    float v[16];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < width ? p[c] : 0.f;
        sum += v[i];
    }
    const float mean = wave_sum(sum) / (float)width;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        const float d = c < width ? v[i] - mean : 0.f;
        sq += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)width + 1e-5f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < width) p[c] = (v[i] - mean) * rstd;
    }
}
void launch_layernorm(float* h, int ld, int width, int rows, hipStream_t s) {
    if (width > 1024) throw Error(FC_ERR_UNSUPPORTED, "layernorm: width > 1024");
    launch_kernel<layernorm_kernel>("fc::layernorm_kernel(float*, int, int, int)", 0.0, 8.0 * rows * width, dim3((rows + 3) / 4), dim3(256), 0, s, h, ld, width, rows);
}

// q[row, :] = q_unnorm[row, :] * rsqrt(sum_blocks(sumsq[b][row]) / width + 1e-5) + q_bias   (LayerNorm -> q fold, common.h EPI_LNQ)
__global__ __launch_bounds__(256) void lnq_finalize_kernel(float* __restrict__ q, int ldq, const float* __restrict__ sumsq, int nslots, size_t pitch,
                                                           float inv_width, const float* __restrict__ q_bias, int rows) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;          // 16 threads per row, one float4 of the 64 q columns each
    const int row = (int)(t >> 4), c4 = ((int)t & 15) * 4;
    if (row >= rows) return;
    float ss = 0.f;
    for (int b = 0; b < nslots; ++b) ss += sumsq[(size_t)b * pitch + row];
    const float rstd = 1.0f / sqrtf(ss * inv_width + 1e-5f);
    float4* qp = reinterpret_cast<float4*>(q + (size_t)row * ldq + c4);
    const float4 v = *qp, bq = *reinterpret_cast<const float4*>(q_bias + c4);
    *qp = make_float4(v.x * rstd + bq.x, v.y * rstd + bq.y, v.z * rstd + bq.z, v.w * rstd + bq.w);
}
void launch_lnq_finalize(float* q, int ldq, const float* sumsq, int nslots, size_t pitch, int width, const float* q_bias, int rows, hipStream_t s) {
    launch_kernel<lnq_finalize_kernel>("fc::lnq_finalize_kernel", 0.0, 4.0 * rows * (128.0 + nslots), dim3((unsigned)(((long)rows * 16 + 255) / 256)), dim3(256), 0, s, q, ldq,
                                       sumsq, nslots, pitch, 1.0f / (float)width, q_bias, rows);
}

// ---------------------------------------------------------------- base density + latent export
// logprob[row] += sum_d(-0.5 log 2pi - 0.5 x_d^2) + log_const   (models/distributions.py:192-195)
// x is in the engine layout [x1 (d1) | pad | x2 (d2) | pad]; z_out (optional) gets the dense [rows, D] latent.
__global__ void base_density_kernel(const float* __restrict__ x, int ldx, int d1, int d1_pad, int d2, float* logprob, float log_const,
                                    float* z_out, int D, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* p = x + (size_t)row * ldx;
    float acc = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float v = c < d1 ? p[c] : p[d1_pad + (c - d1)];
        acc += -0.91893853320467274178f - 0.5f * v * v;
        if (z_out) z_out[(size_t)row * D + c] = v;
    }
    acc = wave_sum(acc);
    if (lane == 0) logprob[row] += acc + log_const;
}
void launch_base_density(const float* x, int ldx, int d1, int d1_pad, int d2, float* logprob, float log_const, float* z_out, int D,
                         int rows, hipStream_t s) {
    launch_kernel<base_density_kernel>("fc::base_density_kernel", 0.0, 4.0 * rows * (D + 2.0 + (z_out ? D : 0)), dim3((rows + 3) / 4), dim3(256), 0, s, x, ldx, d1, d1_pad, d2,
                                       logprob, log_const, z_out, D, rows);
}

// One wave per point row; lane j handles dims j, j+64, ...  Parameters arrive in the tile-grouped dim-major layout of spline.h
// (the producing GEMM normally evaluates the spline in its own epilogue; this kernel serves the inverse direction and the
// non-split GEMM variants).  y2 overwrites x2 in place; forward adds the row's sum of logabsdet to logprob.
__global__ __launch_bounds__(256) void spline_rows_kernel(const float* __restrict__ params, int ldp, float* xbuf, int ldx, int x2_col0,
                                                          int d2, int K, float* logprob, int rows, int inverse) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float* pr = params + (size_t)row * ldp;
    float acc = 0.f;
    float* xr = xbuf + (size_t)row * ldx + x2_col0;
    for (int j = lane; j < d2; j += 64) {
        float y, lad;
        if (K == 8) {                                            // K = 8: register-slot column order (spline.h), gathered per dim
            float u[25];
#pragma unroll
            for (int pp = 0; pp < 25; ++pp) u[pp] = pr[spline_col(j, pp, 8)];
            rq_spline_elem<8>(xr[j], u, 1, inverse != 0, y, lad);
        } else {
            rq_any(K, xr[j], pr + spline_col(j, 0, K), 1, inverse != 0, y, lad);
        }
        xr[j] = y;
        acc += lad;
    }
    acc = wave_sum(acc);
    if (lane == 0 && !inverse) logprob[row] += acc;
}
void launch_spline(const float* params, int ldp, float* xbuf, int ldx, int x2_col0, int d2, int K, float* logprob, int rows, int inverse,
                   hipStream_t s) {
    spline_bins_require(K, "spline: num_bins_spline");
    if (ldp < spline_ncols(d2, K)) throw Error(FC_ERR_INVALID, "spline: parameter pitch too small");
    launch_kernel<spline_rows_kernel>("fc::spline_rows_kernel", 0.0, 4.0 * rows * ((3.0 * K + 1) * d2 + 2.0 * d2 + 2.0), dim3((rows + 3) / 4), dim3(256), 0, s, params, ldp, xbuf,
                                      ldx, x2_col0, d2, K, logprob, rows, inverse);
}

// logprob[row] += sum over the column tiles of the fused spline epilogue's per-tile log-det partials (fixed order: reproducible)
__global__ __launch_bounds__(256) void ldj_reduce_kernel(const float* __restrict__ part, int ntiles, size_t pitch, float* __restrict__ logprob, int rows) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    float s = 0.f;
    for (int t = 0; t < ntiles; ++t) s += part[(size_t)t * pitch + row];
    logprob[row] += s;
}
void launch_ldj_reduce(const float* part, int ntiles, size_t pitch, float* logprob, int rows, hipStream_t s) {
    launch_kernel<ldj_reduce_kernel>("fc::ldj_reduce_kernel", 0.0, 4.0 * rows * (ntiles + 2.0), dim3((rows + 255) / 256), dim3(256), 0, s, part, ntiles, pitch, logprob, rows);
}

__global__ void spline_flat_kernel(const float* x, const float* params, float* y, float* lad, int64_t n, int K, int inverse) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float yy, ll;
    rq_any(K, x[i], params + i * (3 * K + 1), 1, inverse != 0, yy, ll);
    y[i] = yy;
    lad[i] = ll;
}
void launch_spline_flat(const float* x, const float* params, float* y, float* lad, int64_t n, int K, int inverse, hipStream_t s) {
    spline_bins_require(K, "spline: num_bins_spline");
    if (n <= 0) return;
    launch_kernel<spline_flat_kernel>(nullptr, 0.0, 0.0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, params, y, lad, n, K, inverse);
}

// ---------------------------------------------------------------- exponential coupling
// models/exponential_coupling.py:44-75: per point, W = rescale*tanh(scale*raw + shift) + reshift + 1e-8 (d2 x d2),
// y2 = expm(W) x2 + b, ldj = tr W ; inverse x2 = expm(-W)(y2 - b).  expm acts on the vector directly (expm_narrow.h: scaling by 2^-s so
// that |W|_inf <= 1/2, 12-term Taylor action applied 2^s times): both of the reference's algorithms ('torch' = matrix_exp,
// 'original' = truncated series with a batch-global stopping rule, utils.py:294-327) converge to this value.
// One thread per point; only feasible for small d2 (the layer emits d2^2 + d2 numbers per point), like in the reference.
template <int DMAX>
__global__ void expm_coupling_kernel(const float* __restrict__ params, int ldp, float* xbuf, int ldx, int x2_col0, int d2,
                                     const float* __restrict__ scal4, float* logprob, int rows, int inverse) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const float* pr = params + (size_t)row * ldp;
    float w[DMAX * DMAX], v[DMAX];
    float tr;
    float nrm = expm_narrow_matrix<DMAX>(pr, d2, scal4, inverse != 0, w, tr);
    float* xr = xbuf + (size_t)row * ldx + x2_col0;
    for (int i = 0; i < d2; ++i) v[i] = inverse ? xr[i] - pr[d2 * d2 + i] : xr[i];
    int s = 0;
    while (nrm > 0.5f && s < 24) { nrm *= 0.5f; ++s; }
    const float f = ldexpf(1.0f, -s);
    for (int rep = 0; rep < (1 << s); ++rep) expm_narrow_action<DMAX, false>(w, d2, f, v, v);
    for (int i = 0; i < d2; ++i) xr[i] = inverse ? v[i] : v[i] + pr[d2 * d2 + i];
    if (!inverse) logprob[row] += tr;
}
void launch_expm_coupling(const float* params, int ldp, float* xbuf, int ldx, int x2_col0, int d2, const float* scal4, float* logprob,
                          int rows, int inverse, hipStream_t s) {
    if (d2 > 16) throw Error(FC_ERR_UNSUPPORTED, "ExponentialCoupling: latent_dim - latent_dim/2 > 16 is not supported (the layer emits d2^2 numbers per point)");
    if (ldp < d2 * d2 + d2) throw Error(FC_ERR_INVALID, "expm coupling: parameter pitch too small");
    launch_kernel<expm_coupling_kernel<EX_D>>("fc::expm_coupling_kernel", 0.0, 4.0 * rows * (d2 * d2 + 3.0 * d2), dim3((rows + 63) / 64), dim3(64), 0, s, params, ldp, xbuf, ldx,
                                              x2_col0, d2, scal4, logprob, rows, inverse);
}

// ---------------------------------------------------------------- DGCNN edge-conv tail
// out[p, c] = LeakyReLU_0.2( max_j u[idx[p, j], c] + v[p, c] ), uv rows = [u (c_out) | v (c_out)].
// Equals conv(cat(nbr - x, x)) -> BN -> LeakyReLU -> max_k of models/pytorch_gcn.py:23-47,85-99 because the 1x1 conv is
// linear (W1 nbr + (W2 - W1) x), eval BN is a per-channel affine map folded into u and v, and LeakyReLU is monotone.
// The body is shared with the counted kernel (fcflow_embed_counts.h): CNT = with per-scene counts, Mb = the points of row p's scene; the uniform
// kernel's instantiation has no pad-row test at all.
template <bool CNT>
__device__ __forceinline__ void gather_max_row(const float* __restrict__ uv, int lduv, int c_out, const int32_t* __restrict__ idx, int k, float* out, int ldo, int out_col0,
                                               int M, int m_stride, int b, int i, int Mb, int lane) {
    const size_t base = (size_t)b * m_stride;
    if (CNT && i >= Mb) {                               // a pad row: no index is read, and the next level's GEMM finds zeros, not stale workspace bytes
        for (int c = lane; c < c_out; c += 64) out[(base + i) * ldo + out_col0 + c] = 0.0f;
        return;
    }
    const int32_t* ip = idx + ((size_t)b * M + i) * k;
    for (int c = lane; c < c_out; c += 64) {
        float mx = -INFINITY;
        for (int j = 0; j < k; ++j) mx = fmaxf(mx, uv[(base + ip[j]) * lduv + c]);
        const float t = mx + uv[(base + i) * lduv + c_out + c];
        out[(base + i) * ldo + out_col0 + c] = t > 0.f ? t : 0.2f * t;
    }
}
__global__ void gather_max_kernel(const float* __restrict__ uv, int lduv, int c_out, const int32_t* __restrict__ idx, int k,
                                  float* out, int ldo, int out_col0, int M, int m_stride, int total) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= total) return;
    const int b = p / M, i = p - b * M;
    gather_max_row<false>(uv, lduv, c_out, idx, k, out, ldo, out_col0, M, m_stride, b, i, M, lane);
}
__global__ void gather_max_counts_kernel(const float* __restrict__ uv, int lduv, int c_out, const int32_t* __restrict__ idx, int k,
                                         float* out, int ldo, int out_col0, int M, int m_stride, int total, const int32_t* __restrict__ m_counts, int count_min,
                                         int count_max) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= total) return;
    const int b = p / M, i = p - b * M;                 // (one wave per row: b is wave-uniform)
    gather_max_row<true>(uv, lduv, c_out, idx, k, out, ldo, out_col0, M, m_stride, b, i, scene_count(m_counts, b, count_min, count_max), lane);
}
void launch_gather_max(const float* uv, int lduv, int c_out, const int32_t* idx, int k, float* out, int ldo, int out_col0, int B, int M,
                       int m_stride_rows, hipStream_t s) {
    const int total = B * M;
    launch_kernel<gather_max_kernel>("fc::gather_max_kernel", 0.0, 4.0 * total * ((double)k * c_out + 2.0 * c_out + k), dim3((total + 3) / 4), dim3(256), 0, s, uv, lduv, c_out, idx, k,
                                     out, ldo, out_col0, M, m_stride_rows, total);
}
void launch_gather_max_counts(const float* uv, int lduv, int c_out, const int32_t* idx, int k, float* out, int ldo, int out_col0, int B, int M, int m_stride_rows,
                              const SceneCounts& cnt, hipStream_t s) {
    const int total = B * M;
    launch_kernel<gather_max_counts_kernel>("fc::gather_max_counts_kernel", 0.0, 4.0 * total * ((double)k * c_out + 2.0 * c_out + k), dim3((total + 3) / 4), dim3(256), 0, s, uv, lduv,
                                            c_out, idx, k, out, ldo, out_col0, M, m_stride_rows, total, cnt.counts, cnt.lo, cnt.hi);
}

// global embedder pooling: out[b] = [max_i t[b,i,:] | mean_i t[b,i,:]]  (models/pytorch_gcn.py:178-182)
// (M: the rows pooled; the counted kernel passes its scene's count: the same partial sums in the same order as for the scene alone)
__device__ __forceinline__ void pool_max_mean_scene(const float* __restrict__ t, int ldt, int width, float* out, int ldo, int M, int m_stride) {
    const int b = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;   // 4 row-partitions per block
    __shared__ float smx[4][64], ssum[4][64];
    float mx = -INFINITY, sum = 0.f;
    if (c < width)
        for (int i = part; i < M; i += 4) {
            const float v = t[((size_t)b * m_stride + i) * ldt + c];
            mx = fmaxf(mx, v);
            sum += v;
        }
    smx[part][threadIdx.x & 63] = mx;
    ssum[part][threadIdx.x & 63] = sum;
    __syncthreads();
    if (part == 0 && c < width) {
        const int l = threadIdx.x;
        out[(size_t)b * ldo + c] = fmaxf(fmaxf(smx[0][l], smx[1][l]), fmaxf(smx[2][l], smx[3][l]));
        out[(size_t)b * ldo + width + c] = ((ssum[0][l] + ssum[1][l]) + (ssum[2][l] + ssum[3][l])) / (float)M;
    }
}
__global__ void pool_max_mean_kernel(const float* __restrict__ t, int ldt, int width, float* out, int ldo, int M, int m_stride) {
    pool_max_mean_scene(t, ldt, width, out, ldo, M, m_stride);
}
__global__ void pool_max_mean_counts_kernel(const float* __restrict__ t, int ldt, int width, float* out, int ldo, int m_stride, const int32_t* __restrict__ m_counts,
                                            int count_min, int count_max) {
    pool_max_mean_scene(t, ldt, width, out, ldo, scene_count(m_counts, blockIdx.y, count_min, count_max), m_stride);
}
void launch_pool_max_mean(const float* t, int ldt, int width, float* out, int ldo, int B, int M, int m_stride_rows, hipStream_t s) {
    launch_kernel<pool_max_mean_kernel>(nullptr, 0.0, 0.0, dim3((width + 63) / 64, B), dim3(256), 0, s, t, ldt, width, out, ldo, M, m_stride_rows);
}
void launch_pool_max_mean_counts(const float* t, int ldt, int width, float* out, int ldo, int B, int M, int m_stride_rows, const SceneCounts& cnt, hipStream_t s) {
    (void)M;
    launch_kernel<pool_max_mean_counts_kernel>(nullptr, 0.0, 0.0, dim3((width + 63) / 64, B), dim3(256), 0, s, t, ldt, width, out, ldo, m_stride_rows, cnt.counts, cnt.lo, cnt.hi);
}

// rows >= the scene's count of a dense [B][M][width] tensor := 0.0f (the per-point output of a counted embed call: callers allocate it
// uninitialised and its width need not be a multiple of 4, so the 16-byte stores of zero_pad_rows_kernel do not fit).  blockIdx.y = scene.
__global__ __launch_bounds__(256) void zero_tail_rows_kernel(float* __restrict__ out, int width, int M, const int32_t* __restrict__ m_counts, int count_min, int count_max) {
    const int b = blockIdx.y;
    const int Mb = scene_count(m_counts, b, count_min, count_max);
    const long i = (long)blockIdx.x * 256 + threadIdx.x + (long)Mb * width;       // element inside the scene, starting at its first pad row
    if (i < (long)M * width) out[(size_t)b * M * width + i] = 0.0f;
}
void launch_zero_tail_rows(float* out, int width, int B, int M, const SceneCounts& cnt, hipStream_t s) {
    const long n = (long)(M - cnt.lo) * width;                                    // the most pad a scene can have
    if (B <= 0 || n <= 0) return;
    launch_kernel<zero_tail_rows_kernel>("fc::zero_tail_rows_kernel", 0.0, 4.0 * (double)n * B, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, out, width, M, cnt.counts,
                                         cnt.lo, cnt.hi);
}

}  // namespace fc
