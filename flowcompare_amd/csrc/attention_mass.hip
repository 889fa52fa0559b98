// Attention mass per context point (fc_flow_attention_mass_f32, fc_op_attention_mass_f32): weighted column sums of the cross-attention softmax,
//   mass[b, j] = sum_p g[b, p] * softmax_j( q[b, p, :] . k[b, j, :] )      j < M,   g null = ones
// without the [B, N, M] map that attention_weights.hip would have to write first (4 B N M bytes per layer; the result here is 4 B M).
// Same grid, operand forms and pass 1 as attn_weights_kernel (attention_rows.h; that file's header comment describes the layout): one
// workgroup = 128 queries of one scene (4 waves x 32), key tiles of 64, the query on the lane.  Pass 2: the lane forms its query's
// probabilities exp2(S - m) * (1 / l) -- the bits the weight kernel stores for that row -- and multiplies them by g[b, p]; a lane whose
// query index was clamped (p >= N) and a lane with g = 0 contribute exact zeros, whatever their q row holds.  The wave's 32 x 64 block goes
// through its LDS slab, lane `key` adds the 32 rows of its column in ascending row order, and the four waves' column sums are added through
// LDS in wave order.
// No float atomics: every workgroup writes its partial of the tile to its own row of a slab [B][ceil(N / 128)][M] in caller-provided scratch,
// and attn_mass_reduce_kernel adds the rows of a scene in ascending workgroup order, so the result is the same bytes on every run.
// Keys beyond M are masked and never written.
#include "attention_rows.h"
#include "launch.h"
#include <cstdio>

namespace fc {

struct AttnMassParams : AttnRowParams {
    const float* g;                      // [B][N] row weights, or null = ones
    float* slab;                         // [B][gridDim.x][M]
};

template <int DH, int KF>
__global__ __launch_bounds__(256) void attn_mass_kernel(const AttnMassParams p) {
    extern __shared__ float smem[];
    AttnRows<DH, KF> rows(p, smem, attn_scene_keys(p.m_counts, blockIdx.y, p.M));
    constexpr int PL = AttnRows<DH, KF>::PL, LD = AttnRows<DH, KF>::LD;
    float* const sP = rows.sP;
    float* const sC = smem + 64 * LD + 4 * 32 * PL;           // [4 waves][64 keys] column sums of the tile
    const int lane = rows.lane, wave = rows.wave, li = rows.li, b = rows.b;
    rows.load_q();
    float gp = 0.f;                                           // a clamped lane repeats query N - 1: it must not be counted again
    if (rows.p0 + li < p.P) gp = p.g ? p.g[(size_t)b * p.P + rows.p0 + li] : 1.0f;

    const int Mb = rows.Mb, ntiles = (Mb + 63) / 64;          // (per-scene key counts: a scene with few keys runs few tiles)
    float m_run, l_run;
    rows.pass1(ntiles, m_run, l_run);
    const float inv_l = 1.0f / l_run;

    // ---- pass 2: g x the weights of the tile through the wave's LDS slab, column sums over its 32 rows, then over the 4 waves
    float* const op = p.slab + ((size_t)b * gridDim.x + blockIdx.x) * p.M;
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        rows.stage(t);
        __syncthreads();
        floatx16 s[2];
        rows.scores(t, s);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float w = __builtin_amdgcn_exp2f(s[h2][r] - m_run) * inv_l;
                sP[li * PL + rows.tile_key(h2, r)] = gp == 0.f ? 0.f : w * gp;      // (zero weight = zero contribution, also for a non-finite row)
            }
        __syncthreads();
        float acc = sP[lane];
        for (int rr = 1; rr < 32; ++rr) acc += sP[rr * PL + lane];
        sC[wave * 64 + lane] = acc;
        __syncthreads();
        const int key = t * 64 + lane;
        if (wave == 0 && key < Mb) op[key] = ((sC[lane] + sC[64 + lane]) + sC[128 + lane]) + sC[192 + lane];
    }
}

// out[b, j] = sum over the scene's workgroups, in ascending order
// (per-scene key counts: the slab holds columns below the scene's count only; the dense row's other columns are exact zeros)
__global__ __launch_bounds__(256) void attn_mass_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, int B, int nwg, int M,
                                                               const int* __restrict__ m_counts) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const size_t i = (size_t)b * M + j;
    if (j >= attn_scene_keys(m_counts, b, M)) { out[i] = 0.f; return; }
    const float* sp = slab + (size_t)b * nwg * M + j;
    float acc = sp[0];
    for (int w = 1; w < nwg; ++w) acc += sp[(size_t)w * M];
    out[i] = acc;
}

template <int DH, int KF>
static void launch_attn_mass_dh(const AttnMassParams& p, int B, hipStream_t s) {
    constexpr size_t lds = attn_rows_lds_bytes<DH>(4 * 64);
    char name[80];
    snprintf(name, sizeof name, "void fc::attn_mass_kernel<%d, %d>(fc::AttnMassParams)", DH, KF);
    const int nwg = (p.P + 127) / 128;
    launch_kernel<attn_mass_kernel<DH, KF>, (int)lds>(name, 4.0 * B * (double)p.P * (double)p.M * DH, 4.0 * B * (double)nwg * (double)p.M,      // two passes of Q K^T; the slab bytes
                                                      dim3(nwg, B), dim3(256), lds, s, p);
}

size_t attention_mass_slab_bytes(int B, int N, int M) { return sizeof(float) * (size_t)B * (size_t)((N + 127) / 128) * (size_t)M; }

void launch_attention_mass(const AttnQuery& qy, const AttnKeys& kv, const AttnProblem& pb, const float* row_weight, float* slab, float* out,
                           hipStream_t s) {
    const int B = pb.B;
    if (!slab || !out) throw Error(FC_ERR_INVALID, "attention mass: null pointer");
    AttnMassParams p{};
    const int kf = attn_rows_params("attention mass", qy, kv, pb, p);
    p.P = pb.N; p.g = row_weight; p.slab = slab;
    if (kf) {
        if (pb.dh_pad == 32) launch_attn_mass_dh<32, 1>(p, B, s);
        else launch_attn_mass_dh<64, 1>(p, B, s);
    } else {
        switch (pb.dh_pad) {
            case 32: launch_attn_mass_dh<32, 0>(p, B, s); break;
            case 64: launch_attn_mass_dh<64, 0>(p, B, s); break;
            case 128: launch_attn_mass_dh<128, 0>(p, B, s); break;
            default: launch_attn_mass_dh<256, 0>(p, B, s); break;
        }
    }
    const int nwg = (pb.N + 127) / 128;
    const size_t n = (size_t)B * pb.M;
    launch_kernel<attn_mass_reduce_kernel>("void fc::attn_mass_reduce_kernel(const float*, float*, int, int, int, const int*)", 0.0, 4.0 * (double)n * (nwg + 1),
                                           dim3((unsigned)((pb.M + 255) / 256), B), dim3(256), 0, s, slab, out, B, nwg, pb.M, pb.m_counts);
}

}  // namespace fc
