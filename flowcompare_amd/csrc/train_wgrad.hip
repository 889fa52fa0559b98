// Training Linear, the parameter gradients (train_linear.hip has the rest of the step): dW = du^T x per input panel and db = column sums
// of du, and the column sums on their own (fc_train_colsum_f32: d gamma / d beta of the norms, bias-only Linears).  Rows are split over
// workgroups and the partial results added in a fixed order, so every gradient is bit-reproducible.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "activations.h"
#include "launch.h"
#include "train_linear.h"

namespace fc {

// ---------------------------------------------------------------- weight gradient  dW[n][k] = sum_p du[p][n] x[p][k]
// Both operands are row-major with the contraction index p as the slow one, which is exactly the operand order of
// v_mfma_f32_32x32x2_f32 (lane l supplies A[m = l % 32][k = l / 32] and B[k = l / 32][n = l % 32]): 32 consecutive floats of one row
// per half-wave, no transposition anywhere.  Workgroup = 4 waves, tile 128 (n) x 128 (k), each wave 64 x 64; grid.y splits the rows.

constexpr int WG_PS = 16;                  // rows per staged slab
constexpr int WG_LD = 128 + 4;             // LDS pitch in floats

__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ du, int ldu, int du_cols, const float* __restrict__ x, int ldx,
                                                    int x_cols, int rows_valid, int chunk_rows, int tiles_k, float* __restrict__ part,
                                                    int part_rows, int part_ld, float* __restrict__ colpart, int colpart_ld) {
    __shared__ float sA[WG_PS * WG_LD];
    __shared__ float sB[WG_PS * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x / tiles_k, tk = blockIdx.x % tiles_k;
    const int n0 = tn * 128, k0 = tk * 128;
    const int wn = wave >> 1, wk = wave & 1;
    const int p_begin = blockIdx.y * chunk_rows, p_end = min(rows_valid, p_begin + chunk_rows);
    // staging: thread t moves 2 float4 per operand per slab: rows (t / 32) and (t / 32) + 8, columns 4 (t % 32) ...
    const int lr = tid >> 5, lc = (tid & 31) * 4;
    const bool a_ok = n0 + lc < du_cols, b_ok = k0 + lc < x_cols;
    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float4 ra[2], rb[2];
    auto gload = [&](int p0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = p0 + lr + 8 * h;
            const bool ok = p < p_end;
            ra[h] = (ok && a_ok) ? *reinterpret_cast<const float4*>(du + (size_t)p * ldu + n0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
            rb[h] = (ok && b_ok) ? *reinterpret_cast<const float4*>(x + (size_t)p * ldx + k0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // bias gradient for free: the du slab is in LDS anyway, so the workgroups of the first k tile also sum its columns
    // (thread t < 128 owns column n0 + t; rows beyond the chunk were staged as zeros)
    const bool do_cols = colpart != nullptr && tk == 0 && tid < 128;
    float csum = 0.f;
    if (p_begin < p_end) gload(p_begin);
    for (int p0 = p_begin; p0 < p_end; p0 += WG_PS) {
        __syncthreads();                                  // the previous slab's reads are done
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(&sA[(lr + 8 * h) * WG_LD + lc]) = ra[h];
            *reinterpret_cast<float4*>(&sB[(lr + 8 * h) * WG_LD + lc]) = rb[h];
        }
        __syncthreads();
        if (p0 + WG_PS < p_end) gload(p0 + WG_PS);
        if (do_cols) {
            float t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int r = 0; r < WG_PS; r += 2) { t0 += sA[r * WG_LD + tid]; t1 += sA[(r + 1) * WG_LD + tid]; }
            csum += t0 + t1;
        }
#pragma unroll
        for (int kk = 0; kk < WG_PS / 2; ++kk) {
            const int row = 2 * kk + (lane >> 5);
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = sA[row * WG_LD + wn * 64 + i * 32 + (lane & 31)];
                b[i] = sB[row * WG_LD + wk * 64 + i * 32 + (lane & 31)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    if (do_cols && n0 + tid < du_cols) colpart[(size_t)blockIdx.y * colpart_ld + n0 + tid] = csum;
    float* out = part + (size_t)blockIdx.y * part_rows * part_ld;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int k = k0 + wk * 64 + j * 32 + (lane & 31);
                out[(size_t)n * part_ld + k] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------- the same product on the split-fp16 loop (default inside a guard scope)
// Operands go global -> registers (fp32) -> fp16 limbs (hi, lo' = (x - hi) 2048, gemm.hip) -> LDS row-major [p][hi 128 | lo' 128];
// the MFMA operands (8 consecutive-in-p halfs of one column per lane) come out of LDS through ds_read_b64_tr_b16, the transposing
// read the forward attention uses for P.V: a 16-lane group reads a [4 rows][16 columns] block and lane i receives column i.  Each
// lane's k-group therefore holds rows {4h .. 4h+3, 8+4h .. 8+4h+3} of the 16-row step -- the same permutation for both operands, so
// the contraction is unchanged.  3 MFMAs (v_mfma_f32_32x32x16_f16) per block and step: hi.hi into `main`, hi.lo' + lo'.hi into `cross`.
typedef short v4i16 __attribute__((ext_vector_type(4)));

constexpr int W16_ROWS = 32;               // rows per staged slab (two MFMA k-steps)
constexpr int W16_PITCH = 512 + 64;        // bytes per LDS row: [hi 128 halfs | lo' 128 halfs] + pad.  144 words = 16 banks (of the 64 a ds_read_b64_tr_b16 sees) from
                                           // row to row: the 32 lanes of one read cycle -- 4 rows x 2 column halves x 4 lanes of 8 bytes -- then cover all 64 banks once
                                           // (with 512 + 32 a row advanced 8 banks, the distance of the column halves: 2-way conflicts, SQ_LDS_BANK_CONFLICT 33 % of the LDS cycles)

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void wgrad16_kernel(const float* __restrict__ du, int ldu, int du_cols, const float* __restrict__ x, int ldx,
                                                      int x_cols, int rows_valid, int chunk_rows, int tiles_k, float* __restrict__ part,
                                                      int part_rows, int part_ld, float* __restrict__ colpart, int colpart_ld, int* __restrict__ ovf) {
    __shared__ __attribute__((aligned(16))) char sA[2 * W16_ROWS * W16_PITCH];      // two stages each
    __shared__ __attribute__((aligned(16))) char sB[2 * W16_ROWS * W16_PITCH];
    constexpr int STAGE = W16_ROWS * W16_PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lh = lane >> 5;
    const int tn = blockIdx.x / tiles_k, tk = blockIdx.x % tiles_k;
    const int n0 = tn * 128, k0 = tk * 128;
    const int wn = wave >> 1, wk = wave & 1;
    const int p_begin = blockIdx.y * chunk_rows, p_end = min(rows_valid, p_begin + chunk_rows);
    const int lr = tid >> 5, lc = (tid & 31) * 4;
    const bool a_ok = n0 + lc < du_cols, b_ok = k0 + lc < x_cols;
    const bool do_cols = colpart != nullptr && tk == 0;
    floatx16 om[2][2], oc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { om[i][j][r] = 0.f; oc[i][j][r] = 0.f; }
    float4 ra[4], rb[4];
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
    float amax = 0.f;
    // Operand loads through buffer descriptors (round 3: the SQ counters showed this loop bound by VALU issue, 11 VALU + 1.5 SALU per MFMA, and
    // ~5 of them were the bounds branches and 64-bit address arithmetic of eight `ok ? load : 0` per slab).  A slab's descriptor starts at its
    // first row and ends behind row p_end - 1, so rows past the chunk read as zero through the hardware range check; a lane whose four columns
    // lie beyond the panel's width carries an offset no descriptor reaches.  Per-lane offsets are loop constants: a load is ONE instruction.
    unsigned va[4], vb[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        va[h] = a_ok ? (unsigned)(((lr + 8 * h) * ldu + n0 + lc) * 4) : 0x80000000u;
        vb[h] = b_ok ? (unsigned)(((lr + 8 * h) * ldx + k0 + lc) * 4) : 0x80000000u;
    }
    auto gload = [&](int p0) {
        const int left = p_end - p0;                      // > 0 at every call
        const __amdgpu_buffer_rsrc_t ra_d = __builtin_amdgcn_make_buffer_rsrc((void*)(du + (size_t)p0 * ldu), 0, left * ldu * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb_d = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)p0 * ldx), 0, left * ldx * 4, 0x00020000);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            ra[h] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(ra_d, va[h], 0, 0));
            rb[h] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rb_d, vb[h], 0, 0));
        }
    };
    auto split_store = [&](char* base, const float4& v) {
        asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(v.x), "v"(v.y));
        asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(v.z), "v"(v.w));
        uint2 hi, lo;                                       // five VALU per pair of values (activations.h limb_split2)
        limb_split2(v.x, v.y, hi.x, lo.x);
        limb_split2(v.z, v.w, hi.y, lo.y);
        *reinterpret_cast<uint2*>(base) = hi;
        *reinterpret_cast<uint2*>(base + 256) = lo;
    };
    // transposed-read address of this lane inside a [4 rows][16 columns] block (attention.hip): lane 4q+c of a 16-lane group supplies
    // row q, columns 4c .. 4c+3; the group's columns are 16 ((lane >> 4) & 1) .. +15 of the 32-column block, its rows start at 4 lh
    const int tr_off = (4 * lh + ((lane & 15) >> 2)) * W16_PITCH + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    // (the bias-gradient column sums exist in the workgroups of the first k tile only: two copies of the loop instead of a select per value)
    auto run = [&](auto cols_tag) {
        constexpr bool COLS = decltype(cols_tag)::value;
        auto lstore = [&](int st) {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                if constexpr (COLS) { csum.x += ra[h].x; csum.y += ra[h].y; csum.z += ra[h].z; csum.w += ra[h].w; }
                split_store(sA + st * STAGE + (lr + 8 * h) * W16_PITCH + lc * 2, ra[h]);
                split_store(sB + st * STAGE + (lr + 8 * h) * W16_PITCH + lc * 2, rb[h]);
            }
        };
        // software pipeline: slab t is multiplied out of LDS stage t & 1 while slab t + 1 (already in registers) is converted and stored
        // into the other stage and slab t + 2 is fetched from HBM; one barrier per slab
        if (p_begin < p_end) { gload(p_begin); lstore(0); }
        if (p_begin + W16_ROWS < p_end) gload(p_begin + W16_ROWS);
        int st = 0;
        for (int p0 = p_begin; p0 < p_end; p0 += W16_ROWS, st ^= 1) {
            __syncthreads();                                  // stage st is complete; every wave has finished reading stage st ^ 1
#pragma unroll
            for (int ks = 0; ks < W16_ROWS / 16; ++ks) {
                f16x8 ah[2], al[2], bh[2], bl[2];
#define FC_TR(PTR_) __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)(PTR_))
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const char* pa = sA + st * STAGE + (16 * ks) * W16_PITCH + (wn * 64 + i * 32) * 2 + tr_off;
                    const char* pb = sB + st * STAGE + (16 * ks) * W16_PITCH + (wk * 64 + i * 32) * 2 + tr_off;
                    ah[i] = __builtin_bit_cast(f16x8, __builtin_shufflevector(FC_TR(pa), FC_TR(pa + 8 * W16_PITCH), 0, 1, 2, 3, 4, 5, 6, 7));
                    al[i] = __builtin_bit_cast(f16x8, __builtin_shufflevector(FC_TR(pa + 256), FC_TR(pa + 256 + 8 * W16_PITCH), 0, 1, 2, 3, 4, 5, 6, 7));
                    bh[i] = __builtin_bit_cast(f16x8, __builtin_shufflevector(FC_TR(pb), FC_TR(pb + 8 * W16_PITCH), 0, 1, 2, 3, 4, 5, 6, 7));
                    bl[i] = __builtin_bit_cast(f16x8, __builtin_shufflevector(FC_TR(pb + 256), FC_TR(pb + 256 + 8 * W16_PITCH), 0, 1, 2, 3, 4, 5, 6, 7));
                }
#undef FC_TR
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        om[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], om[i][j], 0, 0, 0);
                        oc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], oc[i][j], 0, 0, 0);
                        oc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], oc[i][j], 0, 0, 0);
                    }
                if (ks == 0 && p0 + W16_ROWS < p_end) lstore(st ^ 1);        // the next slab's limbs, under this slab's MFMAs
                if (ks == 0 && p0 + 2 * W16_ROWS < p_end) gload(p0 + 2 * W16_ROWS);      // ... and the slab after it requested at once: a whole slab to land
            }
        }
    };
    if (do_cols) run(std::true_type{}); else run(std::false_type{});
    if (amax >= 65504.0f || amax != amax) atomicOr(ovf, 1);
    if (do_cols) {
        // the 8 thread rows (tid >> 5) of the staging grid each summed their own rows of the chunk: add them in a fixed order
        __syncthreads();
        float* red = reinterpret_cast<float*>(sA);
        *reinterpret_cast<float4*>(red + lr * 128 + lc) = csum;
        __syncthreads();
        if (tid < 128 && n0 + tid < du_cols) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) t += red[r * 128 + tid];
            colpart[(size_t)blockIdx.y * colpart_ld + n0 + tid] = t;
        }
    }
    float* out = part + (size_t)blockIdx.y * part_rows * part_ld;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int k = k0 + wk * 64 + j * 32 + (lane & 31);
                out[(size_t)n * part_ld + k] = om[i][j][r] + oc[i][j][r] * (1.0f / 2048.0f);
            }
}

// src[0] + src[stride] + ... + src[(S - 1) stride], the S row-chunk partials of one output: added in chunk order, 8 independent loads in
// flight.  The ORDER of the additions is the contract of every reduce below (bit-reproducible gradients): do not reassociate it.
__device__ __forceinline__ float sum_partials(const float* __restrict__ src, size_t stride, int S) {
    float s = 0.f;
    int c = 0;
    for (; c + 8 <= S; c += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(c + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < S; ++c) s += src[(size_t)c * stride];
    return s;
}

// dW[n][k_off + k] (=|+=) sum_s part[s][n][k]   for n < N, k < k_true: fixed summation order
__global__ void wgrad_reduce_kernel(const float* __restrict__ part, int S, int part_rows, int part_ld, float* __restrict__ dW, int N, int K,
                                    int k_off, int k_true, int accumulate, const float* __restrict__ colpart, int colpart_ld, float* __restrict__ db) {
    // entries [0, N k_true) are dW, entries [N k_true, N k_true + N) the bias gradient (column partials of the same launch)
    const size_t nw = (size_t)N * k_true, total = nw + (db ? N : 0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float* src;
        size_t stride;
        float* dst;
        if (i < nw) {
            const int n = (int)(i / k_true), k = (int)(i % k_true);
            src = part + (size_t)n * part_ld + k; stride = (size_t)part_rows * part_ld; dst = dW + (size_t)n * K + k_off + k;
        } else {
            const int n = (int)(i - nw);
            src = colpart + n; stride = colpart_ld; dst = db + n;
        }
        const float s = sum_partials(src, stride, S);
        *dst = accumulate ? *dst + s : s;
    }
}

// column sums over rows [0, rows_valid): part[s][col] then a fixed-order reduce (bias gradients).  One float4 of 4 columns per lane,
// 4 rows in flight per workgroup step; grid.y = row chunks.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ a, int lda, int cols, int rows_valid, int chunk_rows,
                                                     float* __restrict__ part, int part_ld) {
    __shared__ float4 red[4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 4;
    const int p_begin = blockIdx.y * chunk_rows, p_end = min(rows_valid, p_begin + chunk_rows);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < cols) {
        if (c + 3 < cols && (lda & 3) == 0 && (((uintptr_t)a) & 15) == 0) {
#pragma unroll 8
            for (int p = p_begin + q; p < p_end; p += 4) {
                const float4 v = *reinterpret_cast<const float4*>(a + (size_t)p * lda + c);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        } else {
            for (int p = p_begin + q; p < p_end; p += 4) {
                const float* r = a + (size_t)p * lda + c;
                s.x += r[0];
                if (c + 1 < cols) s.y += r[1];
                if (c + 2 < cols) s.z += r[2];
                if (c + 3 < cols) s.w += r[3];
            }
        }
    }
    red[q][lane] = s;
    __syncthreads();
    if (q == 0 && c < cols) {
        const float4 t0 = red[0][lane], t1 = red[1][lane], t2 = red[2][lane], t3 = red[3][lane];
        float* o = part + (size_t)blockIdx.y * part_ld + c;
        o[0] = (t0.x + t1.x) + (t2.x + t3.x);
        if (c + 1 < cols) o[1] = (t0.y + t1.y) + (t2.y + t3.y);
        if (c + 2 < cols) o[2] = (t0.z + t1.z) + (t2.z + t3.z);
        if (c + 3 < cols) o[3] = (t0.w + t1.w) + (t2.w + t3.w);
    }
}
__global__ void colsum_reduce_kernel(const float* __restrict__ part, int S, int part_ld, float* __restrict__ out, int n, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const float s = sum_partials(part + c, part_ld, S);
    out[c] = accumulate ? out[c] + s : s;
}

// ---------------------------------------------------------------- host side
static int colsum_chunks(int rows) { return std::max(1, std::min(256, rows / 128)); }

// out[c] (=|+=) sum over rows [0, rows) of a[row][c] for c < cols; ws: colsum_chunks(rows) partial rows of round_up(cols, 32) floats
static void launch_colsum(const float* a, int lda, int cols, int rows, float* out, int accumulate, float* ws, hipStream_t s) {
    const int S = colsum_chunks(rows), chunk = (rows + S - 1) / S, ld = round_up(cols, 32);
    ProfScope ps("fc::colsum_kernel", 0.0, (double)rows * cols * 4.0, s);      // one scope over the partial sums and their reduction
    launch_kernel<colsum_kernel>(nullptr, 0.0, 0.0, dim3((cols + 255) / 256, S), dim3(256), 0, s, a, lda, cols, rows, chunk, ws, ld);
    launch_kernel<colsum_reduce_kernel>(nullptr, 0.0, 0.0, dim3((cols + 255) / 256), dim3(256), 0, s, (const float*)ws, S, ld, out, cols, accumulate);
}

struct WgradPlan { int S, chunk, n128, k128max; size_t part_floats, colsum_floats, bytes; };
static WgradPlan wgrad_plan(const TrainLinearLayout& L, int rows) {
    WgradPlan w{};
    w.n128 = round_up(L.N_pad, 128);
    int tiles_max = 1;
    for (int i = 0; i < L.nseg; ++i) {
        w.k128max = std::max(w.k128max, round_up(L.seg_pad[i], 128));
        tiles_max = std::max(tiles_max, (w.n128 / 128) * (round_up(L.seg_pad[i], 128) / 128));
    }
    // enough workgroups for 256 CUs x 2, slabs of at least 512 rows
    w.S = std::max(1, std::min(std::max(1, 512 / tiles_max), std::max(1, rows / 512)));
    w.chunk = round_up((rows + w.S - 1) / w.S, W16_ROWS);
    w.part_floats = (size_t)w.S * w.n128 * w.k128max;
    w.colsum_floats = (size_t)std::max(w.S, colsum_chunks(rows)) * round_up(L.N_pad, 128);      // wgrad's column partials, or launch_colsum's
    w.bytes = round_up_sz(w.part_floats * 4, 256) + round_up_sz(w.colsum_floats * 4, 256);
    return w;
}

}  // namespace fc


using namespace fc;

extern "C" {

size_t fc_train_linear_wgrad_ws_bytes(int32_t N, const int32_t* seg_widths, int32_t nseg, int32_t rows) {
    try { return wgrad_plan(train_layout(N, seg_widths, nseg), rows).bytes; } catch (const std::exception& e) { set_last_error(e.what()); return 0; }
}

int fc_train_linear_wgrad_f32(int32_t N, const int32_t* seg_widths, int32_t nseg, const float* du, int32_t ldu, const float* const* x,
                              const int32_t* ldx, int32_t rows, float* dW, float* db, int32_t accumulate, void* ws, size_t ws_bytes, int32_t* ovf,
                              void* stream) {
    FC_API_BEGIN
    const TrainLinearLayout L = train_layout(N, seg_widths, nseg);
    if (!x || !ldx || rows < 1 || (!dW && !db)) throw Error(FC_ERR_INVALID, "fc_train_linear_wgrad_f32: bad argument");
    check_panel(du, ldu, L.N_pad, "du");
    const WgradPlan w = wgrad_plan(L, rows);
    if (!ws || ws_bytes < w.bytes || ((uintptr_t)ws & 255)) throw Error(FC_ERR_WORKSPACE, "fc_train_linear_wgrad_f32: workspace too small (fc_train_linear_wgrad_ws_bytes) or not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)ws;
    float* cpart = (float*)((char*)ws + round_up_sz(w.part_floats * 4, 256));
    if (dW) {
        int k_off = 0;
        for (int i = 0; i < L.nseg; ++i) {
            check_panel(x[i], ldx[i], L.seg_pad[i], "x");
            const int k128 = round_up(L.seg_pad[i], 128), tiles_k = k128 / 128, tiles_n = w.n128 / 128;
            if (ovf && g_knobs.train_wgrad16) {                   // (knob 11)
                launch_kernel<wgrad16_kernel>("fc::wgrad16_kernel", 2.0 * rows * (double)L.N * L.seg[i], 0.0, dim3(tiles_n * tiles_k, w.S), dim3(256), 0, s, du, ldu, L.N_pad, x[i],
                                              ldx[i], L.seg_pad[i], rows, w.chunk, tiles_k, part, w.n128, k128, (db && i == 0) ? cpart : nullptr, w.n128, (int*)ovf);
            } else {
                launch_kernel<wgrad_kernel>("fc::wgrad_kernel", 2.0 * rows * (double)L.N * L.seg[i], 0.0, dim3(tiles_n * tiles_k, w.S), dim3(256), 0, s, du, ldu, L.N_pad, x[i], ldx[i],
                                            L.seg_pad[i], rows, w.chunk, tiles_k, part, w.n128, k128, (db && i == 0) ? cpart : nullptr, w.n128);
            }
            const size_t total = (size_t)L.N * L.seg[i];
            launch_kernel<wgrad_reduce_kernel>("fc::wgrad_reduce_kernel", 0.0, (double)total * 4.0 * (w.S + 1), dim3(grid_for(total + L.N, 256)), dim3(256), 0, s, part, w.S, w.n128,
                                               k128, dW, L.N, L.K, k_off, L.seg[i], accumulate, cpart, w.n128, (db && i == 0) ? db : nullptr);
            k_off += L.seg[i];
        }
    }
    if (db && !dW) launch_colsum(du, ldu, L.N, rows, db, accumulate, cpart, s);
    FC_API_END
}

size_t fc_train_colsum_ws_bytes(int32_t cols, int32_t rows) {
    return (size_t)colsum_chunks(std::max(rows, 1)) * round_up(std::max(cols, 1), 32) * 4 + 256;
}

/* out[c] (=|+=) sum over rows [0, rows) of a[row][c], fixed summation order */
int fc_train_colsum_f32(const float* a, int32_t lda, int32_t cols, int32_t rows, float* out, int32_t accumulate, void* ws, size_t ws_bytes,
                        void* stream) {
    FC_API_BEGIN
    if (!a || !out || cols < 1 || rows < 1 || lda < cols) throw Error(FC_ERR_INVALID, "fc_train_colsum_f32: bad argument");
    if (!ws || ws_bytes < fc_train_colsum_ws_bytes(cols, rows)) throw Error(FC_ERR_WORKSPACE, "fc_train_colsum_f32: workspace too small (fc_train_colsum_ws_bytes)");
    launch_colsum(a, lda, cols, rows, out, accumulate, (float*)ws, (hipStream_t)stream);
    FC_API_END
}

}  // extern "C"
