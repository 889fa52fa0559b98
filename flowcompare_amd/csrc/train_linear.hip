// Training primitives: the backward of the hot path, first slice = the residual GELU MLP (models/nets.py:19-30),
// which is ~61 % of the reference's forward time and two thirds of its backward FLOPs.
//
// The training path keeps parameters as ordinary dense fp32 tensors (they change every optimiser step), so nothing is folded at
// create time as in the inference engine.  Per step and per Linear the caller
//   * packs  W [N, K] -> the operand images of the split-fp16 GEMM loop (gemm.hip), for W and for W^T           (train_pack_kernel)
//   * forward   u = x W^T + b (+ residual),  y = act(u)             launch_gemm on the packed W   + act kernel
//   * backward  du = dy . act'(u)                                    act_bwd_kernel
//               dx = du W                                            launch_gemm on the packed W^T (same split-fp16 tile as the forward)
//               dW = du^T x ,  db = column sums of du                train_wgrad.hip (rows split over workgroups, partial tiles
//                                                                    reduced in a fixed order: bit-reproducible)
// This file: the pack, the two activation passes, the forward and the data gradient (layout of the pack: train_linear.h).
// Activations are "panels": row-major fp32 [rows_pad, width_pad], rows padded to ROW_PAD, widths to 32 with ZERO pad columns.
// An input may be up to three panels side by side (the coupling MLP reads cat(x1, attention output), models/affine_coupling.py:33),
// exactly like launch_gemm's A segments.
//
// Range: the split-fp16 loop needs |operand| < 65504.  The caller owns ONE device flag per optimisation step (forward and backward
// run on different host threads under torch.autograd, so no thread-local scope can span them); every primitive ORs into it and the
// caller repeats the step with flag == NULL (fp32-input MFMA loop, any range) if it came back set.
#include <hip/hip_runtime.h>

#include "activations.h"
#include "launch.h"
#include "train_linear.h"

namespace fc {

__device__ __forceinline__ int padded_to_true_k(const TrainLinearLayout& d, int kp) {
    int pad0 = 0, true0 = 0;
    for (int i = 0; i < d.nseg; ++i) {
        if (kp < pad0 + d.seg_pad[i]) {
            const int l = kp - pad0;
            return l < d.seg[i] ? true0 + l : -1;
        }
        pad0 += d.seg_pad[i]; true0 += d.seg[i];
    }
    return -1;
}

constexpr float kTrainWideWScale = (float)(1 << kTrainWideWExp);

// x as two fp16 limbs at [row][k / 16][hi 16 | lo 16] of `image`.  ONE_ACC false: x = hi + lo'/2048 (gemm.hip); true, the one-accumulator
// form (spline_wide.hip): x 2^kTrainWideWExp = hi + lo with lo = rn16(x 2^e - hi) unscaled
template <bool ONE_ACC>
__device__ __forceinline__ void store_limbs(unsigned short* image, size_t row, int kt16, int k, float x, int* ovf) {
    float v = x;
    if constexpr (ONE_ACC) v = x * kTrainWideWScale;
    if (x != 0.f && !(fabsf(v) < 65504.0f) && ovf) atomicOr(ovf, 1);
    const _Float16 h = (_Float16)v;
    float r = v - (float)h;
    if constexpr (!ONE_ACC) r *= 2048.0f;
    const _Float16 l = (_Float16)r;
    unsigned short* dst = image + (row * kt16 + (k >> 4)) * 32 + (k & 15);
    dst[0] = __builtin_bit_cast(unsigned short, h);
    dst[16] = __builtin_bit_cast(unsigned short, l);
}

// One [rows][cols] image of the pack: entry (r, c) is W[n = r][k = c], TRANSPOSED W[n = c][k = r], zero outside W.  The GEMM images
// (ONE_ACC false) come as zero-padded fp32 `dense` plus limbs, their k counted in padded segment columns; the one-accumulator images of a
// wide layer are limbs alone, and such a layer has one segment, so padded k = true k.  stride: threads of the grid
template <bool ONE_ACC, bool TRANSPOSED>
__device__ __forceinline__ void pack_image(const float* __restrict__ W, const TrainLinearLayout& d, float* dense, unsigned short* limbs, int rows,
                                           int cols, int* ovf, size_t stride) {
    const size_t total = (size_t)rows * cols;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int r = (int)(i / cols), c = (int)(i % cols);
        const int n = TRANSPOSED ? c : r, kp = TRANSPOSED ? r : c;
        int k = -1;                                                     // (kp beyond the padded segments maps to -1 as well)
        if (n < d.N) k = ONE_ACC ? (kp < d.K ? kp : -1) : padded_to_true_k(d, kp);
        const float x = k >= 0 ? W[(size_t)n * d.K + k] : 0.f;
        if constexpr (!ONE_ACC) dense[i] = x;
        store_limbs<ONE_ACC>(limbs, r, cols >> 4, c, x, ovf);
    }
}

// W [N, K] dense -> zero-padded fp32 + fp16 limb images of W ([n_alloc][K_pad]) and of W^T ([k_alloc][N_pad]), padded bias; for a wide
// layer also the one-accumulator images of both ([n256][K_pad], [k256][N_pad]) and the bias scaled for that loop
__global__ void train_pack_kernel(const float* __restrict__ W, const float* __restrict__ bias, TrainLinearLayout d, char* pack, int* ovf) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    pack_image<false, false>(W, d, (float*)(pack + d.off_W), (unsigned short*)(pack + d.off_W2), d.n_alloc, d.K_pad, ovf, stride);
    pack_image<false, true>(W, d, (float*)(pack + d.off_WT), (unsigned short*)(pack + d.off_WT2), d.k_alloc, d.N_pad, ovf, stride);
    float* bp = (float*)(pack + d.off_bias);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)d.n_alloc; i += stride)
        bp[i] = (bias && (int)i < d.N) ? bias[i] : 0.f;
    if (d.wide) {
        pack_image<true, false>(W, d, nullptr, (unsigned short*)(pack + d.off_W1), d.n256, d.K_pad, ovf, stride);
        pack_image<true, true>(W, d, nullptr, (unsigned short*)(pack + d.off_WT1), d.k256, d.N_pad, ovf, stride);
        float* b1 = (float*)(pack + d.off_bias1);
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)d.n256; i += stride)
            b1[i] = (bias && (int)i < d.N) ? bias[i] * (kOneAccActScale * kTrainWideWScale) : 0.f;
    }
}

// ---------------------------------------------------------------- activations (models/nets.py:21-29; GELU = exact erf form)
__device__ __forceinline__ float act_grad(float u, int act) { return fc_act_grad(u, act); }      // (activations.h: shared with the GEMM epilogue)

__global__ void act_fwd_kernel(const float4* __restrict__ u, float4* __restrict__ y, size_t n4, int act) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 v = u[i];
        v.x = act_apply(v.x, act); v.y = act_apply(v.y, act); v.z = act_apply(v.z, act); v.w = act_apply(v.w, act);
        y[i] = v;
    }
}

// du = dy * act'(u) on a dense [rows_pad, ld] panel; rows >= rows_valid come out as zeros (they must not reach weight gradients)
__global__ void act_bwd_kernel(const float4* __restrict__ dy, const float4* __restrict__ u, float4* __restrict__ du, size_t n4, size_t valid4,
                               int act) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < valid4) {
            const float4 a = dy[i], b = u[i];
            g.x = a.x * act_grad(b.x, act); g.y = a.y * act_grad(b.y, act); g.z = a.z * act_grad(b.z, act); g.w = a.w * act_grad(b.w, act);
        }
        du[i] = g;
    }
}

// ---------------------------------------------------------------- host side
// The wide layers run on the 256 x 256 one-accumulator loop (forward: constant activation scale; data gradient: per-row scales) where that
// loop can take the call (train_wide, knob 31); everything else on launch_gemm.  `who`: the public entry, for the error texts.
static bool train_wide_ok(const TrainLinearLayout& L, int rows_pad, const int32_t* ovf) {
    return g_knobs.train_wide && L.wide && ovf && rows_pad % 256 == 0 && gemm_fp16_enabled();
}

// u = cat(x) W^T + b (+ residual); with an activation (GELU / RELU / ELU) also y = act(u), from the same launch
static void train_linear_forward(const char* who, const void* pack, int N, const int32_t* seg_widths, int nseg, const float* const* x, const int32_t* ldx,
                                 int rows_pad, const float* residual, int ldr, float* u, float* y, int ldu, int act, int32_t* ovf, hipStream_t s) {
    const TrainLinearLayout L = train_layout(N, seg_widths, nseg);
    if (!pack || !x || !ldx || rows_pad < 1 || rows_pad % ROW_PAD != 0) throw Error(FC_ERR_INVALID, std::string(who) + ": bad argument (rows_pad must be a multiple of 256)");
    ASeg a[3] = {};
    for (int i = 0; i < L.nseg; ++i) { check_panel(x[i], ldx[i], L.seg_pad[i], "x"); a[i] = ASeg{x[i], ldx[i]}; }
    check_panel(u, ldu, L.N_pad, "u");
    if (act != FC_ACT_NONE) check_panel(y, ldu, L.N_pad, "y");
    if (residual) check_panel(residual, ldr, L.N_pad, "residual");
    if (train_wide_ok(L, rows_pad, ovf) && act == FC_ACT_NONE && !residual) {
        TrainWideArgs w;
        w.A = x[0]; w.lda = ldx[0]; w.W1 = (const unsigned short*)((const char*)pack + L.off_W1); w.bias1 = (const float*)((const char*)pack + L.off_bias1);
        w.K_pad = L.K_pad; w.rows_pad = rows_pad; w.n_cols = L.N_pad; w.C = u; w.ldc = ldu; w.ovf = (int*)ovf;
        w.flops = 2.0 * rows_pad * (double)L.N * (double)L.K;
        launch_train_wide(w, s);
        return;
    }
    const PackedLinear P = packed_view(L, pack, false, ovf != nullptr);
    GemmEpi e{};
    e.C = u; e.ldc = ldu; e.residual = residual; e.ldr = ldr; e.rows_valid = rows_pad;
    if (act != FC_ACT_NONE) { e.C = y; e.Cpre = u; e.act = act; }
    Fp16FlagScope scope((int*)ovf);
    launch_gemm(P, a, rows_pad, e, EPI_LINEAR, s);
}

// dx = du W, or with an activation dx = (du . W + addend) * act'(u_prev): the data gradient of a hidden Linear together with the backward of
// the activation in front of it (and the residual branch's gradient, `addend`): the result is the PRE-activation gradient of the previous
// layer, what its weight and data gradients consume -- no separate fc_train_act_bwd_f32 pass over the panel (6 % of a C2 training step
// went into the activation passes).  u_prev and addend are [rows_pad, lddx] panels like dx.  On the one-accumulator loop every row of du is
// scaled by an exact power of two from `row_absmax` ([rows_pad], each >= max |du[row, :]|, written by the kernel that produced du --
// fc_train_rqspline_bwd_f32); without it the fp32-A loop runs
static void train_linear_dgrad(const char* who, const void* pack, int N, const int32_t* seg_widths, int nseg, const float* du, int ldu, int rows_pad,
                               float* dx, int lddx, const float* addend, const float* u_prev, int act, const float* row_absmax, int32_t* ovf,
                               hipStream_t s) {
    const TrainLinearLayout L = train_layout(N, seg_widths, nseg);
    if (!pack || rows_pad < 1 || rows_pad % ROW_PAD != 0) throw Error(FC_ERR_INVALID, std::string(who) + ": bad argument (rows_pad must be a multiple of 256)");
    check_panel(du, ldu, L.N_pad, "du");
    check_panel(dx, lddx, L.K_pad, "dx");
    if (act != FC_ACT_NONE) check_panel(u_prev, lddx, L.K_pad, "u_prev");
    if (addend) check_panel(addend, lddx, L.K_pad, "addend");
    if (train_wide_ok(L, rows_pad, ovf) && row_absmax && (act == FC_ACT_NONE || act == FC_ACT_GELU)) {
        TrainWideArgs w;
        w.A = du; w.lda = ldu; w.W1 = (const unsigned short*)((const char*)pack + L.off_WT1); w.K_pad = L.N_pad; w.rows_pad = rows_pad; w.n_cols = L.K_pad;
        w.row_absmax = row_absmax; w.C = dx; w.ldc = lddx; w.ovf = (int*)ovf;
        if (act != FC_ACT_NONE) { w.addend = addend; w.gradu = u_prev; w.ldgu = lddx; w.gact = act; }
        w.flops = 2.0 * rows_pad * (double)L.N * (double)L.K;
        launch_train_wide(w, s);
        return;
    }
    const PackedLinear P = packed_view(L, pack, true, ovf != nullptr);
    ASeg a{du, ldu};
    GemmEpi e{};
    e.C = dx; e.ldc = lddx; e.rows_valid = rows_pad;
    if (act != FC_ACT_NONE) { e.residual = addend; e.ldr = lddx; e.gradu = u_prev; e.ldgu = lddx; e.gact = act; }
    Fp16FlagScope scope((int*)ovf);
    launch_gemm(P, &a, rows_pad, e, EPI_LINEAR, s);
}

static bool act_is_gelu_relu_or_elu(int act) { return act == FC_ACT_GELU || act == FC_ACT_RELU || act == FC_ACT_ELU; }

}  // namespace fc


using namespace fc;

extern "C" {

size_t fc_train_linear_pack_bytes(int32_t N, const int32_t* seg_widths, int32_t nseg) {
    try { return train_layout(N, seg_widths, nseg).bytes; } catch (const std::exception& e) { set_last_error(e.what()); return 0; }
}

int fc_train_linear_pack_f32(const float* W, const float* bias, int32_t N, const int32_t* seg_widths, int32_t nseg, void* pack, size_t pack_bytes,
                             int32_t* ovf, void* stream) {
    FC_API_BEGIN
    const TrainLinearLayout L = train_layout(N, seg_widths, nseg);
    if (!W || !pack || pack_bytes < L.bytes || ((uintptr_t)pack & 255)) throw Error(FC_ERR_INVALID, "fc_train_linear_pack_f32: bad argument (pack must be 256-byte aligned, fc_train_linear_pack_bytes long)");
    size_t n = std::max((size_t)L.n_alloc * L.K_pad, (size_t)L.k_alloc * L.N_pad);
    if (L.wide) n = std::max(n, std::max((size_t)L.n256 * L.K_pad, (size_t)L.k256 * L.N_pad));
    launch_kernel<train_pack_kernel>("fc::train_pack_kernel", 0.0, (double)n * 16.0, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, W, bias, L, (char*)pack, (int*)ovf);
    FC_API_END
}

int fc_train_linear_fwd_f32(const void* pack, int32_t N, const int32_t* seg_widths, int32_t nseg, const float* const* x, const int32_t* ldx,
                            int32_t rows_pad, const float* residual, int32_t ldr, float* u, int32_t ldu, int32_t* ovf, void* stream) {
    FC_API_BEGIN
    train_linear_forward(__func__, pack, N, seg_widths, nseg, x, ldx, rows_pad, residual, ldr, u, nullptr, ldu, FC_ACT_NONE, ovf, (hipStream_t)stream);
    FC_API_END
}

// the same with the activation in the GEMM's epilogue: u = cat(x) W^T + b (+ residual) AND y = act(u) from one launch (the separate
// fc_train_act_fwd_f32 pass re-read u: 6 % of a C2 training step went into the activation passes)
int fc_train_linear_act_fwd_f32(const void* pack, int32_t N, const int32_t* seg_widths, int32_t nseg, const float* const* x, const int32_t* ldx,
                                int32_t rows_pad, const float* residual, int32_t ldr, float* u, float* y, int32_t ldu, int32_t act, int32_t* ovf,
                                void* stream) {
    FC_API_BEGIN
    if (!act_is_gelu_relu_or_elu(act)) throw Error(FC_ERR_INVALID, "fc_train_linear_act_fwd_f32: act must be GELU, RELU or ELU");
    train_linear_forward(__func__, pack, N, seg_widths, nseg, x, ldx, rows_pad, residual, ldr, u, y, ldu, act, ovf, (hipStream_t)stream);
    FC_API_END
}

int fc_train_linear_dgrad_f32(const void* pack, int32_t N, const int32_t* seg_widths, int32_t nseg, const float* du, int32_t ldu, int32_t rows_pad,
                              float* dx, int32_t lddx, const float* row_absmax, int32_t* ovf, void* stream) {
    FC_API_BEGIN
    train_linear_dgrad(__func__, pack, N, seg_widths, nseg, du, ldu, rows_pad, dx, lddx, nullptr, nullptr, FC_ACT_NONE, row_absmax, ovf, (hipStream_t)stream);
    FC_API_END
}

// (one input segment: dx is a single panel beside u_prev and addend)
int fc_train_linear_dgrad_act_f32(const void* pack, int32_t N, const int32_t* seg_widths, int32_t nseg, const float* du, int32_t ldu, int32_t rows_pad,
                                  float* dx, int32_t lddx, const float* addend, const float* u_prev, int32_t act, const float* row_absmax, int32_t* ovf,
                                  void* stream) {
    FC_API_BEGIN
    if (!pack || rows_pad < 1 || rows_pad % ROW_PAD != 0 || nseg != 1) throw Error(FC_ERR_INVALID, "fc_train_linear_dgrad_act_f32: bad argument (one input segment, rows_pad a multiple of 256)");
    if (!act_is_gelu_relu_or_elu(act)) throw Error(FC_ERR_INVALID, "fc_train_linear_dgrad_act_f32: act must be GELU, RELU or ELU");
    train_linear_dgrad(__func__, pack, N, seg_widths, nseg, du, ldu, rows_pad, dx, lddx, addend, u_prev, act, row_absmax, ovf, (hipStream_t)stream);
    FC_API_END
}

int fc_train_act_fwd_f32(const float* u, float* y, int32_t rows_pad, int32_t ld, int32_t act, void* stream) {
    FC_API_BEGIN
    if (!u || !y || rows_pad < 1 || ld < 4 || ld % 4 != 0 || (((uintptr_t)u | (uintptr_t)y) & 15)) throw Error(FC_ERR_INVALID, "fc_train_act_fwd_f32: bad argument");
    const size_t n4 = (size_t)rows_pad * ld / 4;
    launch_kernel<act_fwd_kernel>("fc::act_fwd_kernel", 0.0, (double)n4 * 32.0, dim3(grid_for(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)u, (float4*)y, n4, act);
    FC_API_END
}

int fc_train_act_bwd_f32(const float* dy, const float* u, float* du, int32_t rows_pad, int32_t rows, int32_t ld, int32_t act, void* stream) {
    FC_API_BEGIN
    if (!dy || !u || !du || rows_pad < 1 || rows < 0 || rows > rows_pad || ld < 4 || ld % 4 != 0 || (((uintptr_t)u | (uintptr_t)dy | (uintptr_t)du) & 15))
        throw Error(FC_ERR_INVALID, "fc_train_act_bwd_f32: bad argument");
    const size_t n4 = (size_t)rows_pad * ld / 4, v4 = (size_t)rows * ld / 4;
    launch_kernel<act_bwd_kernel>("fc::act_bwd_kernel", 0.0, (double)n4 * 48.0, dim3(grid_for(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)dy, (const float4*)u,
                                  (float4*)du, n4, v4, act);
    FC_API_END
}

}  // extern "C"
