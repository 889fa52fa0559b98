// Softmax rows of the flow's cross attention for selected queries (fc_flow_attention_weights_f32, fc_op_attention_weights_f32):
//   w[b, p, j] = softmax_j( q[b, sel[b,p], :] . k[b, j, :] )      j < M          (models/perceiver.py:108-111, `attn_weights`)
// The forward's kernels (attention.hip) stream the softmax and never form a row; this kernel is launched next to them, only at the layers a
// caller asks about, and reads the operands in the forms the forward leaves them in:
//   K  KF 0: an fp32 panel (head dims 128 and 256, the range-fallback pass, fc_op_*);  KF 1: columns of the stacked K|V GEMM's one-accumulator limb image
//      (GemmEpi::C16 with c16_scale = kOneAccActScale: [16 columns: hi 16 | lo 16] tiles, k 16 = hi + lo) -- joined back to fp32 while the tile
//      is staged, which is exact: hi + lo spans at most 22 significant bits; with k16_rows the folded engine's context image instead, packed rows
//      [key][hi DH | lo DH] of the same form (launch_context_limbs: the keys of EVERY layer, with q carrying the layer's Wk);
//   q  final, or the un-normalised projection of the LayerNorm -> q fold, finished on load with rstd and the bias exactly as attn16_kernel does.
// Arithmetic: fp32 operands on v_mfma_f32_32x32x2_f32, fp32 everywhere (DESIGN.md section 11b says why not the limb products).
//
// One workgroup = 128 selected queries of one scene (4 waves x 32), key tiles of 64 staged in LDS and shared by the waves.  S^T = K Q^T in the
// swapped form of attn_kernel: the query sits on the LANE, its 32 keys of a block in the 16 accumulator registers x 2 half-waves, so a row's
// maximum and sum are in-lane reductions plus one cross-half exchange -- and a row's bits depend on its own query and the keys only, never
// on which other queries share the wave.  Two passes over the key tiles: pass 1 keeps the running maximum m and sum l, pass 2 recomputes S
// and stores exp2(S - m) * (1 / l).  A wave's 32 x 64 block of weights goes through LDS so that every store instruction writes one row's 64
// consecutive floats (a per-lane store at the row pitch would touch 32 lines per instruction).  Keys beyond M are clamped on load, masked to
// -inf before the maximum and never stored; the pad rows of the K panel are never read.
#include "common.h"
#include <cstdio>

namespace fc {

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct AttnWParams {
    const float* q; int ldq;
    const float* k; int ldk;             // KF 0
    const unsigned short* k16; int ld16; // KF 1: first half-word of this layer's K columns, half-words per image row
    int k16_rows;                        // KF 1: 0 = [16 columns: hi 16 | lo 16] tiles of a GEMM limb image, 1 = packed rows [hi DH | lo DH]
    float* out;                          // [B][P][M]
    const int* sel; int sel_stride;      // null = query p; else sel[b * sel_stride + p]  (sel_stride 0: one table for all scenes)
    int P, N, n_stride, M, m_stride;
    float qscale;
    const float* q_sumsq; int q_slots; size_t q_pitch; float q_inv_width; const float* q_bias;    // LayerNorm -> q fold (Attn16Params)
};

template <int DH, int KF>
__global__ __launch_bounds__(256) void attn_weights_kernel(const AttnWParams p) {
    constexpr int NG = DH / 8, LD = DH + 4, PL = 65;
    extern __shared__ float smem[];
    float* const sK = smem;                                   // [64][LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const sP = smem + 64 * LD + wave * 32 * PL;        // [32 queries][PL] of this wave
    const int li = lane & 31, lh = lane >> 5;
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * 128 + wave * 32;

    // ---- Q fragment of this lane's query (B operand of S^T = K Q^T): q[8g + 4h + e]
    float4 qf[NG];
    {
        int pi = p0 + li;
        pi = pi < p.P ? pi : p.P - 1;
        int qi = p.sel ? p.sel[(size_t)b * p.sel_stride + pi] : pi;
        qi = qi < 0 ? 0 : (qi < p.N ? qi : p.N - 1);          // (the host wrappers validate the table; this keeps a bad one inside the panel)
        const size_t qrow = (size_t)b * p.n_stride + qi;
        const float* qp = p.q + qrow * p.ldq + 4 * lh;
        float rstd = 1.0f;
        if (p.q_sumsq) {
            float ss = 0.f;
            for (int sb = 0; sb < p.q_slots; ++sb) ss += p.q_sumsq[(size_t)sb * p.q_pitch + qrow];
            rstd = 1.0f / sqrtf(ss * p.q_inv_width + 1e-5f);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float4 t = *reinterpret_cast<const float4*>(qp + 8 * g);
            float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.q_bias) bq = *reinterpret_cast<const float4*>(p.q_bias + 8 * g + 4 * lh);
            if (p.q_sumsq) qf[g] = make_float4((t.x * rstd + bq.x) * p.qscale, (t.y * rstd + bq.y) * p.qscale, (t.z * rstd + bq.z) * p.qscale, (t.w * rstd + bq.w) * p.qscale);
            else qf[g] = make_float4(t.x * p.qscale, t.y * p.qscale, t.z * p.qscale, t.w * p.qscale);
        }
    }

    // ---- one key tile into LDS as fp32 rows (rows beyond M repeat key M - 1 and are masked below)
    auto stage = [&](int t) {
        if constexpr (KF == 0) {
            constexpr int F4R = DH / 4;
            for (int i = tid; i < 64 * F4R; i += 256) {
                const int row = i / F4R, c4 = (i - row * F4R) * 4;
                int key = t * 64 + row;
                key = key < p.M ? key : p.M - 1;
                *reinterpret_cast<float4*>(sK + row * LD + c4) = *reinterpret_cast<const float4*>(p.k + ((size_t)b * p.m_stride + key) * p.ldk + c4);
            }
        } else {
            constexpr int G8 = DH / 8;
            for (int i = tid; i < 64 * G8; i += 256) {
                const int row = i / G8, w8 = i - row * G8;
                int key = t * 64 + row;
                key = key < p.M ? key : p.M - 1;
                const unsigned short* src = p.k16 + ((size_t)b * p.m_stride + key) * p.ld16 + (p.k16_rows ? 8 * w8 : (w8 >> 1) * 32 + (w8 & 1) * 8);
                const uint4 hu = *reinterpret_cast<const uint4*>(src), lu = *reinterpret_cast<const uint4*>(src + (p.k16_rows ? DH : 16));
                const unsigned hw[4] = {hu.x, hu.y, hu.z, hu.w}, lw[4] = {lu.x, lu.y, lu.z, lu.w};
                float x[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float h0 = (float)__builtin_bit_cast(_Float16, (unsigned short)(hw[e] & 0xffffu)), h1 = (float)__builtin_bit_cast(_Float16, (unsigned short)(hw[e] >> 16));
                    const float l0 = (float)__builtin_bit_cast(_Float16, (unsigned short)(lw[e] & 0xffffu)), l1 = (float)__builtin_bit_cast(_Float16, (unsigned short)(lw[e] >> 16));
                    x[2 * e] = (h0 + l0) * (1.0f / kOneAccActScale);
                    x[2 * e + 1] = (h1 + l1) * (1.0f / kOneAccActScale);
                }
                *reinterpret_cast<float4*>(sK + row * LD + 8 * w8) = make_float4(x[0], x[1], x[2], x[3]);
                *reinterpret_cast<float4*>(sK + row * LD + 8 * w8 + 4) = make_float4(x[4], x[5], x[6], x[7]);
            }
        }
    };
    // ---- S^T = K Q^T for the two 32-key halves of the staged tile, tail keys masked
    auto scores = [&](int t, floatx16 (&s)[2]) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[h2][r] = 0.f;
            const float* kr = sK + (32 * h2 + li) * LD + 4 * lh;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float4 kf = *reinterpret_cast<const float4*>(kr + 8 * g);
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[g].x, s[h2], 0, 0, 0);
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[g].y, s[h2], 0, 0, 0);
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[g].z, s[h2], 0, 0, 0);
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[g].w, s[h2], 0, 0, 0);
            }
        }
        if (t * 64 + 64 > p.M) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= p.M) s[h2][r] = -INFINITY;
                }
        }
    };

    const int ntiles = (p.M + 63) / 64;
    // ---- pass 1: running maximum and sum of this lane's query (the other half of its keys lives in lane ^ 32)
    float m_run = -INFINITY, l_run = 0.f;
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        stage(t);
        __syncthreads();
        floatx16 s[2];
        scores(t, s);
        float mt = s[0][0];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[h2][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);          // 0 on the first tile (m_run = -inf)
        float lt = 0.f;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) lt += __builtin_amdgcn_exp2f(s[h2][r] - m_new);
        lt += __shfl_xor(lt, 32, 64);
        l_run = l_run * alpha + lt;
        m_run = m_new;
    }
    const float inv_l = 1.0f / l_run;

    // ---- pass 2: the weights, a wave's [32 queries][64 keys] block through LDS, one row segment per store instruction
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        stage(t);
        __syncthreads();
        floatx16 s[2];
        scores(t, s);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                sP[li * PL + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh] = __builtin_amdgcn_exp2f(s[h2][r] - m_run) * inv_l;
        __syncthreads();
        const int key = t * 64 + lane;
        if (key < p.M) {
            const int nrow = p.P - p0 < 32 ? p.P - p0 : 32;                 // (wave-uniform; <= 0 for a wave beyond the selection)
            float* op = p.out + ((size_t)b * p.P + p0) * p.M + key;
            for (int rr = 0; rr < nrow; ++rr) op[(size_t)rr * p.M] = sP[rr * PL + lane];
        }
    }
}

template <int DH, int KF>
static void launch_attnw_dh(const AttnWParams& p, int B, hipStream_t s) {
    constexpr size_t lds = (64 * (size_t)(DH + 4) + 4 * 32 * 65) * sizeof(float);      // 67 KB at head dim 128, 100 KB at 256
    static PerDeviceOnce attr_once;
    auto kern = attn_weights_kernel<DH, KF>;
    attr_once.run([&](int) { FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); return 0; });
    char name[80];
    snprintf(name, sizeof name, "void fc::attn_weights_kernel<%d, %d>(fc::AttnWParams)", DH, KF);
    ProfScope ps(name, 4.0 * B * (double)p.P * (double)p.M * DH, 4.0 * B * (double)p.P * (double)p.M, s);      // two passes of Q K^T; the output bytes
    hipLaunchKernelGGL(kern, dim3((p.P + 127) / 128, B), dim3(256), lds, s, p);
    FC_HIP(hipGetLastError());
}

void launch_attention_weights(const AttnQuery& qy, const AttnKeys& kv, const AttnProblem& pb, const int32_t* sel, int P, int sel_per_scene,
                              float* out, hipStream_t s) {
    const int B = pb.B, dh_pad = pb.dh_pad;
    const bool limbs = kv.form != AttnKeys::PANELS;
    if (B <= 0 || pb.N <= 0 || pb.M <= 0 || P <= 0) throw Error(FC_ERR_INVALID, "attention weights: empty problem");
    if (!qy.q || !out || (limbs ? !kv.img : !kv.k)) throw Error(FC_ERR_INVALID, "attention weights: null pointer");
    if (!sel && P != pb.N) throw Error(FC_ERR_INVALID, "attention weights: without a selection table P must equal N");
    if (qy.ldq % 4 != 0 || ((uintptr_t)qy.q & 15)) throw Error(FC_ERR_INVALID, "attention weights: q must be 16-byte aligned with a pitch that is a multiple of 4 floats");
    AttnWParams p{};
    p.q = qy.q; p.ldq = qy.ldq; p.out = out; p.sel = sel; p.sel_stride = sel && sel_per_scene ? P : 0;
    p.P = P; p.N = pb.N; p.n_stride = pb.n_stride_rows; p.M = pb.M; p.m_stride = pb.m_stride_rows; p.qscale = qy.qscale;
    if (const AttnLnq* l = qy.lnq) { p.q_sumsq = l->sumsq; p.q_slots = l->slots; p.q_pitch = l->pitch; p.q_inv_width = l->inv_width; p.q_bias = l->bias; }
    if (limbs) {
        if (kv.form == AttnKeys::CONTEXT) {
            if (((uintptr_t)kv.img & 15)) throw Error(FC_ERR_INVALID, "attention weights: the context limb image must be 16-byte aligned");
            p.k16 = kv.img;
            p.ld16 = 2 * dh_pad;
            p.k16_rows = 1;
        } else {
            if (kv.col0 % 16 != 0 || kv.n_pad % 16 != 0 || dh_pad > 64) throw Error(FC_ERR_INVALID, "attention weights: limb-image K needs 16-column tiles and head dim <= 64");
            p.k16 = kv.img + (size_t)(kv.col0 / 16) * 32;
            p.ld16 = kv.n_pad * 2;
        }
        if (dh_pad == 32) launch_attnw_dh<32, 1>(p, B, s);
        else if (dh_pad == 64) launch_attnw_dh<64, 1>(p, B, s);
        else throw Error(FC_ERR_UNSUPPORTED, "attention weights: inner dim (padded) must be 32 or 64 with a limb-image K");
        return;
    }
    if (kv.ldk % 4 != 0 || ((uintptr_t)kv.k & 15)) throw Error(FC_ERR_INVALID, "attention weights: k must be 16-byte aligned with a pitch that is a multiple of 4 floats");
    p.k = kv.k; p.ldk = kv.ldk;
    switch (dh_pad) {
        case 32: launch_attnw_dh<32, 0>(p, B, s); break;
        case 64: launch_attnw_dh<64, 0>(p, B, s); break;
        case 128: launch_attnw_dh<128, 0>(p, B, s); break;
        case 256: launch_attnw_dh<256, 0>(p, B, s); break;
        default: throw Error(FC_ERR_UNSUPPORTED, "attention weights: inner dim (padded) must be 32, 64, 128 or 256");
    }
}

}  // namespace fc
