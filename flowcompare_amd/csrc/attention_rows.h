// The part the two softmax-row kernels share (attention_weights.hip: the rows themselves; attention_mass.hip: their weighted column sums):
// the operands, the q fragment of a lane's query, one staged key tile, S^T = K Q^T of the tile, and pass 1 (running maximum and sum).
// attention_weights.hip's header comment describes the layout; the code below is that kernel's, moved here unchanged, so that a row's
// probabilities exp2(S - m) * (1 / l) are the same bits in both kernels.
#pragma once
#include "common.h"
#include "device.h"

namespace fc {


struct AttnRowParams {
    const float* q; int ldq;
    const float* k; int ldk;             // KF 0
    const unsigned short* k16; int ld16; // KF 1: first half-word of this layer's K columns, half-words per image row
    int k16_rows;                        // KF 1: 0 = [16 columns: hi 16 | lo 16] tiles of a GEMM limb image, 1 = packed rows [hi DH | lo DH]
    const int* sel; int sel_stride;      // null = query p; else sel[b * sel_stride + p]  (sel_stride 0: one table for all scenes)
    int P, N, n_stride, M, m_stride;
    float qscale;
    const float* q_sumsq; int q_slots; size_t q_pitch; float q_inv_width; const float* q_bias;    // LayerNorm -> q fold (Attn16Params)
    const int* m_counts;                 // optional [B] per-scene key counts (AttnProblem::m_counts); null: every scene has M keys
};

// LDS of a 256-thread workgroup: the key tile [64][DH + 4] and one [32 queries][65] slab per wave (+ `extra` floats of the kernel's own)
template <int DH>
constexpr size_t attn_rows_lds_bytes(int extra = 0) { return (64 * (size_t)(DH + 4) + 4 * 32 * 65 + extra) * sizeof(float); }

template <int DH, int KF>
struct AttnRows {
    static constexpr int NG = DH / 8, LD = DH + 4, PL = 65;
    const AttnRowParams& p;
    float* const sK;                     // [64][LD]
    float* const sP;                     // [32 queries][PL] of this wave
    const int tid, lane, wave, li, lh, b, p0;
    const int Mb;                        // keys of this scene, from the kernel: p.M, or its count (attn_scene_keys); tiles, clamp and mask follow it
    float4 qf[NG];                       // Q fragment of this lane's query (B operand of S^T = K Q^T): q[8g + 4h + e]

    __device__ __forceinline__ AttnRows(const AttnRowParams& p_, float* smem, int scene_keys)
        : p(p_), sK(smem), sP(smem + 64 * LD + (threadIdx.x >> 6) * 32 * PL), tid(threadIdx.x), lane(threadIdx.x & 63), wave(threadIdx.x >> 6),
          li(threadIdx.x & 31), lh((threadIdx.x & 63) >> 5), b(blockIdx.y), p0(blockIdx.x * 128 + (threadIdx.x >> 6) * 32),
          Mb(scene_keys) {}

    __device__ __forceinline__ void load_q() {
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

    // ---- one key tile into LDS as fp32 rows (rows beyond the scene's keys repeat its last key and are masked below)
    __device__ __forceinline__ void stage(int t) {
        if constexpr (KF == 0) {
            constexpr int F4R = DH / 4;
            for (int i = tid; i < 64 * F4R; i += 256) {
                const int row = i / F4R, c4 = (i - row * F4R) * 4;
                int key = t * 64 + row;
                key = key < Mb ? key : Mb - 1;
                *reinterpret_cast<float4*>(sK + row * LD + c4) = *reinterpret_cast<const float4*>(p.k + ((size_t)b * p.m_stride + key) * p.ldk + c4);
            }
        } else {
            constexpr int G8 = DH / 8;
            for (int i = tid; i < 64 * G8; i += 256) {
                const int row = i / G8, w8 = i - row * G8;
                int key = t * 64 + row;
                key = key < Mb ? key : Mb - 1;
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
    }

    // ---- S^T = K Q^T for the two 32-key halves of the staged tile, tail keys masked
    __device__ __forceinline__ void scores(int t, floatx16 (&s)[2]) const {
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
        if (t * 64 + 64 > Mb) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= Mb) s[h2][r] = -INFINITY;
                }
        }
    }

    // key of accumulator register r of half h2 within the tile (this lane's half-wave): where scores() left S[key][query li]
    __device__ __forceinline__ int tile_key(int h2, int r) const { return 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh; }

    // ---- pass 1: running maximum and sum of this lane's query (the other half of its keys lives in lane ^ 32)
    __device__ __forceinline__ void pass1(int ntiles, float& m_run, float& l_run) {
        m_run = -INFINITY;
        l_run = 0.f;
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
    }
};

// the operand half of a launch: checks and AttnRowParams of (query, keys, problem), shared by launch_attention_weights / launch_attention_mass.
// `what` prefixes the error texts.  Returns the K form: 0 = fp32 panel, 1 = limb image.
int attn_rows_params(const char* what, const AttnQuery& qy, const AttnKeys& kv, const AttnProblem& pb, AttnRowParams& p);

}  // namespace fc
