// Single-head cross attention of the flow's pre-conditioner, flash style.  Two kernels: attn16_kernel (split-fp16 operands on
// the 16-bit matrix cores, the default for head dims <= 64 inside an Fp16Guard scope; further down) and attn_kernel (fp32-input
// MFMA; head dims 128 and 256, the range-fallback pass, and the first build's kernel), described here:
//   out[b, i, :] = softmax_j( q[b,i,:] . k[b,j,:] ) v[b,j,:]        (models/perceiver.py:106-113)
// q arrives PRE-SCALED by inner_dim^-0.5 * log2(e) (folded into the packed q projection), so the softmax
// is exp2(S - max).  The [N, M] score matrix is never materialised (the reference materialises [B,N,M]).
//
// One workgroup = 128 queries of one scene (4 waves x 32 queries); K/V tiles of 64 keys (32 at head dim 256) are staged in LDS
// (register prefetch, double buffered) and shared by the 4 waves.
//   S^T tile = K Q^T   (A = K rows from LDS via ds_read_b128, B = Q held in registers for the whole kernel);
//     its C layout puts the query on the LANE and the 32 keys in the 16 registers x 2 half-waves, so the
//     softmax max/sum are in-lane reductions + one cross-half exchange, and
//   O tile  = P V      consumes those registers DIRECTLY as the A operand (lane (q,h) supplies key
//     (r&3)+8(r>>2)+4h of step r), with B = V[key][d] read row-wise from LDS (conflict-free ds_read_b32).
// No LDS round trip for P, no transposed V image.
// Per-scene key counts (AttnProblem::m_counts): both kernels read Mb = clamp(m_counts[b], 1, M) once per workgroup
// (attn_scene_keys) and run ceil(Mb / tile) tiles with the index clamp and the mask at Mb; strides stay.  Null m_counts: Mb = M.
#include "common.h"
#include "activations.h"
#include "launch.h"
#include <cstdio>

namespace fc {


struct AttnParams {
    const float* q; int ldq;
    const float* k; int ldk;
    const float* v; int ldv;
    float* out; int ldo;
    int N, n_stride, M, m_stride;
    float qscale;     // extra multiplier applied to q at load (1 when the projection is pre-scaled)
    const int* m_counts;   // optional [B] per-scene key counts (AttnProblem::m_counts); null: every scene attends over M keys
};

template <int DH>
__global__ __launch_bounds__(256) void attn_kernel(const AttnParams p) {
    constexpr int NG = DH / 8, DT = DH / 32, LD = DH + 4;
    // keys per staged tile: 64 up to head dim 128; 32 at 256, where two stages of 64 keys of K and V (266 KB) exceed a CU's 160 KiB of LDS
    constexpr int KT = DH > 128 ? 32 : 64, NH2 = KT / 32;
    constexpr int F4R = DH / 4, RPP = 256 / F4R, PASSES = KT / RPP;
    constexpr int STAGE = 2 * KT * LD;
    extern __shared__ float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int b = blockIdx.y;
    const int Mb = attn_scene_keys(p.m_counts, b, p.M);       // this scene's keys: tile count, index clamp and mask below; strides stay p.m_stride
    const int q0 = blockIdx.x * 128 + wave * 32;

    // ---- Q fragment of this lane's query (B operand of S^T = K Q^T): q[8g + 4h + e]
    float4 qf[NG];
    {
        int qi = q0 + li;
        qi = qi < p.N ? qi : p.N - 1;
        const float* qp = p.q + ((size_t)b * p.n_stride + qi) * p.ldq + 4 * lh;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float4 t = *reinterpret_cast<const float4*>(qp + 8 * g);
            qf[g] = make_float4(t.x * p.qscale, t.y * p.qscale, t.z * p.qscale, t.w * p.qscale);
        }
    }

    floatx16 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- staging: thread t moves float4 (t % F4R) of key rows (t / F4R) + RPP*pass, for K and for V.
    //      Straight-line macros on plain register arrays (lambdas / conditionals here sent the tile through scratch memory).
    const int srow = tid / F4R, sc4 = (tid % F4R) * 4;
    float4 rk[PASSES], rv[PASSES];
    const float* kb = p.k + (size_t)b * p.m_stride * p.ldk + sc4;
    const float* vb = p.v + (size_t)b * p.m_stride * p.ldv + sc4;
    float* const sKst = smem + srow * LD + sc4;
#define FC_GLOAD(T_)                                                                          \
    _Pragma("unroll") for (int i = 0; i < PASSES; ++i) {                                      \
        int key_ = (T_) * KT + srow + RPP * i;                                                \
        key_ = key_ < Mb ? key_ : Mb - 1; /* clamped rows are masked to -inf below */       \
        rk[i] = *reinterpret_cast<const float4*>(kb + (size_t)key_ * p.ldk);                  \
        rv[i] = *reinterpret_cast<const float4*>(vb + (size_t)key_ * p.ldv);                  \
    }
#define FC_LSTORE(ST_)                                                                        \
    _Pragma("unroll") for (int i = 0; i < PASSES; ++i) {                                      \
        *reinterpret_cast<float4*>(sKst + (ST_) * STAGE + RPP * i * LD) = rk[i];              \
        *reinterpret_cast<float4*>(sKst + (ST_) * STAGE + KT * LD + RPP * i * LD) = rv[i];    \
    }

    const int ntiles = (Mb + KT - 1) / KT;
    FC_GLOAD(0)
    FC_LSTORE(0)
    __syncthreads();

    for (int t = 0; t < ntiles; ++t) {
        const int tn = t + 1 < ntiles ? t + 1 : t;          // the last iteration re-loads its own tile: branch-free loop
        FC_GLOAD(tn)
        const float* sK = smem + (t & 1) * STAGE;
        const float* sV = sK + KT * LD;

        // ---- S^T = K Q^T for the 32-key blocks of the tile
        floatx16 s[NH2];
#pragma unroll
        for (int h2 = 0; h2 < NH2; ++h2) {
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
        // ---- mask the tail keys of the last tile
        if (t * KT + KT > Mb) {
#pragma unroll
            for (int h2 = 0; h2 < NH2; ++h2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * KT + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= Mb) s[h2][r] = -INFINITY;
                }
        }
        // ---- online softmax (this lane's query = lane&31; the other half of its keys lives in lane^32)
        float mt = s[0][0];
#pragma unroll
        for (int h2 = 0; h2 < NH2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[h2][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);          // 0 on the first tile (m_run = -inf)
        float lt = 0.f;
#pragma unroll
        for (int h2 = 0; h2 < NH2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(s[h2][r] - m_new);   // raw v_exp_f32: arguments are <= 0, results below 2^-126 may flush to 0
                s[h2][r] = pv;
                lt += pv;
            }
        lt += __shfl_xor(lt, 32, 64);
        l_run = l_run * alpha + lt;
        m_run = m_new;
        // ---- rescale O: its rows are queries (r&3)+8(r>>2)+4h, whose alpha lives in that LANE
        if (!__all(alpha == 1.0f)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ar = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * lh, 64);
#pragma unroll
                for (int d = 0; d < DT; ++d) o[d][r] *= ar;
            }
        }
        // ---- O += P V : A = P registers (query on the lane, key per step), B = V[key][d] from LDS
#pragma unroll
        for (int h2 = 0; h2 < NH2; ++h2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* vr = sV + (32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh) * LD + li;
#pragma unroll
                for (int d = 0; d < DT; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[h2][r], vr[32 * d], o[d], 0, 0, 0);
            }
        }
        FC_LSTORE((t + 1) & 1)
        __syncthreads();
    }
#undef FC_GLOAD
#undef FC_LSTORE

    // ---- normalise and store: O rows are queries (r&3)+8(r>>2)+4h of this wave, columns d = 32*dt + lane&31
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qr = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float lr = __shfl(l_run, qr, 64);
        const int qi = q0 + qr;
        if (qi < p.N) {
            float* op = p.out + ((size_t)b * p.n_stride + qi) * p.ldo + li;
#pragma unroll
            for (int d = 0; d < DT; ++d) op[32 * d] = o[d][r] / lr;
        }
    }
}

// =====================================================================================================================
// Split-fp16 attention (the default when the caller is inside an Fp16Guard scope, DH <= 64).
// Same flash structure, but every product runs on the 16-bit matrix cores with fp32-equivalent operands in the ONE-ACCUMULATOR limb
// form of spline_wide.hip (round 4; rounds 2-3 kept x = hi + lo'/2048 with separate main / cross-product accumulators): q, k, v are
// x * 16 = hi + lo with lo = rn16(x 16 - hi) unscaled, the probabilities p * 2^12 = hi + lo, a*b ~= ah*bh + ah*bl + al*bh in one fp32
// accumulator.  12 MFMAs (32 cycles) per 32x32 score block instead of 32 fp32-input MFMAs (64 cycles); against the two-accumulator
// form: no fold per score, 3 instead of 5 VALU per pair of probabilities in the limb split, 64 fewer accumulator registers.
//   * K and V of the layer are split ONCE by kv_limbs_kernel into row images [key][hi DH | lo DH] (the fp32 kernel above
//     re-reads them per 128-query workgroup; here 32 workgroups per scene would redo the same conversion);
//   * S^T = K Q^T: A = K rows (ds_read_b128 per limb), B = Q limbs held in registers for the whole kernel;
//   * P: the S^T accumulator has the query on the lane and 32 keys in its registers, so registers 8s..8s+7 split into limbs
//     ARE the A operand of k-step s of O += P V; element j of lane half h is key 16s + 8(j>>2) + 4h + (j&3) of the block;
//   * V: B operand wants, per lane (column d), those same 8 keys: two ds_read_b64_tr_b16 (hardware transposing read of a
//     4-key x 16-column block per 16-lane group) on the row-major V image.  Row pitches: K 4*DH+16 B (conflict-free b128 reads),
//     V 4*DH+64 B (the 4 rows x 64 B a half-wave's transposed read touches land on 64 distinct banks).
typedef short v4i16 __attribute__((__vector_size__(4 * sizeof(short))));

struct Attn16Params {
    const float* q; int ldq;
    const unsigned short* k16;      // [B * m_stride][2][DH] halves
    const unsigned short* v16;
    float* out; int ldo;
    int N, n_stride, M, m_stride;
    float qscale;
    int* ovf;
    // optional LayerNorm -> q fold (common.h EPI_LNQ): q holds the UN-normalised projection; the kernel applies
    // q * rsqrt(sum_b q_sumsq[b][row] * q_inv_width + 1e-5) + q_bias while it loads its query (no separate finalize pass)
    const float* q_sumsq; int q_slots; size_t q_pitch; float q_inv_width; const float* q_bias;
    int kv_pitch;                   // row pitch of the k16 / v16 images in 16-byte chunks (DH / 4 for the packed images)
    int c16;                        // 1: rows are slices of a GEMM's limb-image output ([16 columns: hi 16 | lo' 16] tiles, GemmEpi::C16)
    float* lse = nullptr;           // optional [B * n_stride]: natural-log sum-exp of every query's scaled scores (training: the backward reuses it)
    const int* m_counts = nullptr;  // optional [B] per-scene key counts (AttnProblem::m_counts); null: every scene attends over M keys
};

// fp32 K / V columns of the projected context -> limb row images in the ONE-ACCUMULATOR form (common.h kOneAccActScale): x s = hi + lo with
// lo = rn16(x s - hi) unscaled; raises *ovf when |x s| leaves fp16's range.  With a null v16 only the K image is made (the folded engine's
// context panel, which is the keys AND the values of every layer: launch_context_limbs).
__global__ __launch_bounds__(256) void kv_limbs_kernel(const float* k, int ldk, const float* v, int ldv, unsigned short* k16, unsigned short* v16,
                                                       long rows, int DH, int* ovf) {
    const int c4 = DH / 4;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    float amax = 0.f;
    if (t < rows * c4) {
        const long row = t / c4;
        const int c = (int)(t - row * c4) * 4;
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            if (which && !v16) break;
            const float4 x = *reinterpret_cast<const float4*>((which ? v + row * ldv : k + row * ldk) + c);
            const float xs[4] = {x.x, x.y, x.z, x.w};
            uint2 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(xs[e]));
            limb_split2s(xs[0], xs[1], kOneAccActScale, 1.0f, h.x, l.x);
            limb_split2s(xs[2], xs[3], kOneAccActScale, 1.0f, h.y, l.y);
            unsigned short* dst = (which ? v16 : k16) + row * 2 * DH + c;
            *reinterpret_cast<uint2*>(dst) = h;
            *reinterpret_cast<uint2*>(dst + DH) = l;
        }
    }
    if (!(amax * kOneAccActScale < 65504.0f)) atomicOr(ovf, 1);
}

// SH = 1 (the folded engine, flow_engine.cpp: K and V of every layer ARE the context panel, head dim 64): k16 is that one packed row image and
// a tile is staged ONCE -- half the global loads and LDS stores per tile, 16 KB per stage instead of 37 -- into plain 256-byte rows whose
// 16-byte chunks are XOR-swizzled, chunk ch of row r at 256 r + 16 (ch ^ swz(r)), swz(r) = ((r & 3) << 2) | ((r >> 2) & 3):
//   * the S phase's ds_read_b128 (lane = row, 16 rows per lane group {0-3, 12-15, 20-27} ...) sees 16 distinct swz values = 16 distinct slots;
//   * the PV phase's ds_read_b64_tr_b16 (per 32-lane half: 4 rows q x 4 chunks x 2 halves of a chunk) sees slots const ^ (q << 2 | 2-bit chunk):
//     16 distinct slots x 2 = all 64 banks;
//   * the staging ds_write_b128 (8 consecutive lanes = 8 consecutive chunks of one row) keeps 8 distinct slots under the XOR.
// The XOR only touches address bits 4-7, so every read is (lane constant ^ compile-time constant) + immediate.
template <int DH, int SH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn16_kernel(const Attn16Params p) {
    static_assert(!SH || DH == 64, "the shared K / V tile is laid out for 256-byte rows");
    constexpr int KS = DH / 16, DT = DH / 32;
    constexpr int KP = SH ? 4 * DH : 4 * DH + 16, VP = SH ? 4 * DH : 4 * DH + 64;          // LDS row pitches in bytes
    constexpr int VOFF = SH ? 0 : 64 * KP;
    constexpr int STAGE = SH ? 64 * KP : 64 * (KP + VP);
    constexpr int CPR = DH / 4;                                // 16-byte chunks per image row
    constexpr int NCH = 64 * CPR / 256;                        // chunks per thread, tile and image
    extern __shared__ float smem[];
    char* smc = reinterpret_cast<char*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int b = blockIdx.y;
    const int Mb = attn_scene_keys(p.m_counts, b, p.M);       // this scene's keys: tile count, index clamp and mask below; strides stay p.m_stride
    const int q0 = blockIdx.x * 128 + wave * 32;

    // ---- Q limbs of this lane's query (B operand of S^T = K Q^T): element j of k-step s is q[16 s + 8 h + j]
    f16x8 qh[KS], ql[KS];
    float amax = 0.f;
    {
        int qi = q0 + li;
        qi = qi < p.N ? qi : p.N - 1;
        const size_t qrow = (size_t)b * p.n_stride + qi;
        const float* qp = p.q + qrow * p.ldq + 8 * lh;
        float rstd = 1.0f;
        if (p.q_sumsq) {
            float ss = 0.f;
            for (int sb = 0; sb < p.q_slots; ++sb) ss += p.q_sumsq[(size_t)sb * p.q_pitch + qrow];
            rstd = 1.0f / sqrtf(ss * p.q_inv_width + 1e-5f);
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const float4 t0 = *reinterpret_cast<const float4*>(qp + 16 * s), t1 = *reinterpret_cast<const float4*>(qp + 16 * s + 4);
            const float xs[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float bq = p.q_bias ? p.q_bias[16 * s + 8 * lh + e] : 0.f;
                const float x = (xs[e] * rstd + bq) * (p.qscale * kOneAccActScale);
                amax = fmaxf(amax, fabsf(x));
                qh[s][e] = (_Float16)x;
                ql[s][e] = (_Float16)(x - (float)qh[s][e]);
            }
        }
    }
    if (!(amax < 65504.0f)) atomicOr(p.ovf, 1);

    // ONE accumulator per output (round 4, the limb form of spline_wide.hip): q, k, v are held as hi + lo of x * 16 with lo UNSCALED and the
    // probabilities as hi + lo of p * 2^12, so that the three limb products hi.hi + hi.lo + lo.hi land at one scale in one fp32 accumulator:
    // no cross-product accumulator sets (64 registers) and no fold of S per score.  The scales cancel exactly: scores are read as
    // S / 256 inside the exponent's fma, 2^12 rides in the exponent's offset (row sums carry it too), the output divides by 16 l.
    floatx16 om[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) om[d][r] = 0.f;
    // LAZY reference (round 4, second half): m_run follows the running maximum of the true scores only when a tile's maximum exceeds it by more
    // than TAU (log2 domain), so p = exp2(s - m_run) <= 2^TAU and the probabilities are held as hi + lo of p 2^12 <= 2^15 (fp16's range).  The
    // result is the same quotient -- numerator and row sum carry the same reference -- but the rescaling of O (16 cross-lane reads + 32
    // multiplies per lane, taken in ~60 % of the tiles of a 4096-key scene with the exact running maximum) happens a handful of times per query.
    constexpr float S_INV = 1.0f / (kOneAccActScale * kOneAccActScale), P_EXP = 12.0f, TAU = 3.0f;
    float m_run = -INFINITY, l_run = 0.f;                      // m_run: the reference (log2 domain, within TAU of the running maximum of the true scores); l_run: sum of p 2^12

    // ---- staging: plain 16-byte copies of the limb images (whole-vector register values: arrays went through scratch)
    typedef unsigned int u32xs __attribute__((ext_vector_type(4 * NCH)));
    u32xs rk, rv;
    const uint4* kb = reinterpret_cast<const uint4*>(p.k16) + (size_t)b * p.m_stride * p.kv_pitch;
    const uint4* vb = reinterpret_cast<const uint4*>(p.v16) + (size_t)b * p.m_stride * p.kv_pitch;
    // shared tile: thread tid stores chunk tid & 15 of rows (tid >> 4) + 16 i, whose swizzle does not depend on i (16 i keeps r & 3, adds 4 i to r >> 2)
    const int st_sh = (tid >> 4) * KP + 16 * ((tid & 15) ^ ((((tid >> 4) & 3) << 2) | ((tid >> 6) & 3)));
#define FC_GLOAD_SH(T_)                                                                       \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i) {                                         \
        int key_ = (T_) * 64 + (tid >> 4) + 16 * i;                                           \
        key_ = key_ < Mb ? key_ : Mb - 1; /* clamped rows are masked to -inf below */       \
        const uint4 a_ = kb[(size_t)key_ * CPR + (tid & 15)];                                 \
        rk[4 * i] = a_.x; rk[4 * i + 1] = a_.y; rk[4 * i + 2] = a_.z; rk[4 * i + 3] = a_.w;     \
    }
#define FC_LSTORE_SH(ST_)                                                                     \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i)                                           \
        *reinterpret_cast<uint4*>(smc + (ST_) * STAGE + 16 * i * KP + st_sh) =                \
            make_uint4(rk[4 * i], rk[4 * i + 1], rk[4 * i + 2], rk[4 * i + 3]);
#define FC_GLOAD(T_)                                                                          \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i) {                                         \
        const int c_ = tid + 256 * i, kr_ = c_ / CPR, part_ = c_ - kr_ * CPR;                 \
        int key_ = (T_) * 64 + kr_;                                                           \
        key_ = key_ < Mb ? key_ : Mb - 1; /* clamped rows are masked to -inf below */       \
        /* chunk part_ of the [hi DH | lo' DH] row = limb part_/(CPR/2), columns 8 w .. 8 w + 7; in a C16 slice that is chunk   */ \
        /* (w >> 1) * 4 + limb * 2 + (w & 1)                                                                                    */ \
        const int w_ = part_ % (CPR / 2), lb_ = part_ / (CPR / 2);                             \
        const int sp_ = p.c16 ? (w_ >> 1) * 4 + lb_ * 2 + (w_ & 1) : part_;                    \
        const uint4 a_ = kb[(size_t)key_ * p.kv_pitch + sp_], b_ = vb[(size_t)key_ * p.kv_pitch + sp_];  \
        rk[4 * i] = a_.x; rk[4 * i + 1] = a_.y; rk[4 * i + 2] = a_.z; rk[4 * i + 3] = a_.w;     \
        rv[4 * i] = b_.x; rv[4 * i + 1] = b_.y; rv[4 * i + 2] = b_.z; rv[4 * i + 3] = b_.w;     \
    }
#define FC_LSTORE(ST_)                                                                        \
    _Pragma("unroll") for (int i = 0; i < NCH; ++i) {                                         \
        const int c_ = tid + 256 * i, kr_ = c_ / CPR, part_ = c_ - kr_ * CPR;                 \
        *reinterpret_cast<uint4*>(smc + (ST_) * STAGE + kr_ * KP + part_ * 16) =              \
            make_uint4(rk[4 * i], rk[4 * i + 1], rk[4 * i + 2], rk[4 * i + 3]);               \
        *reinterpret_cast<uint4*>(smc + (ST_) * STAGE + VOFF + kr_ * VP + part_ * 16) =       \
            make_uint4(rv[4 * i], rv[4 * i + 1], rv[4 * i + 2], rv[4 * i + 3]);               \
    }

    // transposed-read address of this lane inside a [4 keys][16 columns] block: lane 4q+p of a 16-lane group supplies row q,
    // columns 4p..4p+3; the group's 16 columns are 16*((lane>>4)&1) .. +15 of the 32-column block, its keys start at 4*lh
    const int tr_off = (4 * lh + ((lane & 15) >> 2)) * VP + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    // shared tile: the lane parts of the swizzled addresses.  S phase: row li, chunk (2 ks | lh) + 8 limb, swz = ((li & 3) << 2) | ((li >> 2) & 3);
    // PV phase: row 4 lh + q (+ 32 h2 + 16 s2 + 8 j), q = (lane & 15) >> 2, chunk (4 d + 8 limb) | (tr_off's 16-byte chunk), swz = (q << 2) | lh, ^ 2 j
    const int kr_sh = li * KP + 16 * (lh ^ (((li & 3) << 2) | ((li >> 2) & 3)));
    const int tr_sh = tr_off ^ (16 * ((((lane & 15) >> 2) << 2) | lh));

    const int ntiles = (Mb + 63) / 64;
    if constexpr (SH) { FC_GLOAD_SH(0) FC_LSTORE_SH(0) } else { FC_GLOAD(0) FC_LSTORE(0) }
    __syncthreads();

    for (int t = 0; t < ntiles; ++t) {
        const int tn = t + 1 < ntiles ? t + 1 : t;          // the last iteration re-loads its own tile: branch-free loop
        if constexpr (SH) { FC_GLOAD_SH(tn) } else { FC_GLOAD(tn) }
        const char* sK = smc + (t & 1) * STAGE;
        const char* sV = sK + VOFF;

        // ---- S^T = K Q^T for the two 32-key halves of the tile
        floatx16 s[2];                                          // 256 x the scores
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[h2][r] = 0.f;
            const char* kr = sK + (32 * h2 + li) * KP + 16 * lh;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const f16x8 kh = *reinterpret_cast<const f16x8*>(SH ? sK + 32 * h2 * KP + (kr_sh ^ (32 * ks)) : kr + 32 * ks);
                const f16x8 kl = *reinterpret_cast<const f16x8*>(SH ? sK + 32 * h2 * KP + (kr_sh ^ (32 * ks + 2 * DH)) : kr + 2 * DH + 32 * ks);
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], s[h2], 0, 0, 0);
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], s[h2], 0, 0, 0);
                s[h2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], s[h2], 0, 0, 0);
            }
        }
        // ---- mask the tail keys of the last tile
        if (t * 64 + 64 > Mb) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= Mb) s[h2][r] = -INFINITY;
                }
        }
        // ---- online softmax (this lane's query = lane&31; the other half of its keys lives in lane^32)
        float mt = s[0][0];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[h2][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mts = mt * S_INV;
        const float m_new = mts > m_run + TAU ? mts : m_run;                 // (first tile: m_run = -inf; a fully masked tail keeps the reference)
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);          // 0 on the first tile (m_run = -inf), 1 while the reference stands
        const float off = P_EXP - m_new;                                     // p 2^12 = exp2(S / 256 - m + 12)
        float lt = 0.f;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(s[h2][r], S_INV, off));   // raw v_exp_f32: arguments are <= 15, tiny results may flush to 0
                s[h2][r] = pv;
                lt += pv;
            }
        lt += __shfl_xor(lt, 32, 64);
        l_run = l_run * alpha + lt;
        m_run = m_new;
        // ---- rescale O: its rows are queries (r&3)+8(r>>2)+4h, whose alpha lives in that LANE
        if (!__all(alpha == 1.0f)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ar = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * lh, 64);
#pragma unroll
                for (int d = 0; d < DT; ++d) om[d][r] *= ar;
            }
        }
        // ---- O += P V, 16 keys per MFMA k-step: A = limbs of P registers 8 s2 .. 8 s2 + 7, B = V via transposed reads
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                f16x8 ph, pl;
                {
                    const float x8[8] = {s[h2][8 * s2], s[h2][8 * s2 + 1], s[h2][8 * s2 + 2], s[h2][8 * s2 + 3],
                                         s[h2][8 * s2 + 4], s[h2][8 * s2 + 5], s[h2][8 * s2 + 6], s[h2][8 * s2 + 7]};
                    limb_split8_unscaled(x8, ph, pl);             // (3 VALU per pair of probabilities: this kernel is VALU-bound on exactly this)
                }
                const char* vr = sV + (32 * h2 + 16 * s2) * VP + tr_off;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    // (assembled with one shufflevector + whole-vector bit_cast: element-wise extraction of the read's result made hipcc
                    //  emit v_perm/v_mov sequences that duplicated its first dword)
                    // FC_TR(j, col): keys 8 j .. 8 j + 7 of this k-step, byte column col of a row (32 columns of block d at 64 d, the low limb at
                    // + 2 DH).  Shared tile: the rows ride in the offset, the lane's swizzle in tr_sh, and 8 j more rows add 2 j to swz (^ 32 bytes)
#define FC_TR(J_, COL_) __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)( \
        SH ? sV + (32 * h2 + 16 * s2 + 8 * (J_)) * VP + (tr_sh ^ (COL_) ^ (32 * (J_))) : vr + 8 * (J_) * VP + (COL_)))
                    const f16x8 vh = __builtin_bit_cast(f16x8, __builtin_shufflevector(FC_TR(0, 64 * d), FC_TR(1, 64 * d), 0, 1, 2, 3, 4, 5, 6, 7));
                    const f16x8 vl = __builtin_bit_cast(f16x8, __builtin_shufflevector(FC_TR(0, 64 * d + 2 * DH), FC_TR(1, 64 * d + 2 * DH),
                                                                                      0, 1, 2, 3, 4, 5, 6, 7));
#undef FC_TR
                    om[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vh, om[d], 0, 0, 0);
                    om[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph, vl, om[d], 0, 0, 0);
                    om[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pl, vh, om[d], 0, 0, 0);
                }
            }
        }
        if constexpr (SH) { FC_LSTORE_SH((t + 1) & 1) } else { FC_LSTORE((t + 1) & 1) }
        __syncthreads();
    }
#undef FC_GLOAD
#undef FC_LSTORE
#undef FC_GLOAD_SH
#undef FC_LSTORE_SH

    if (p.lse && lane < 32 && q0 + lane < p.N)                   // scores are in the log2 domain (qscale carries log2 e); l_run carries 2^12 and the reference m_run
        p.lse[(size_t)b * p.n_stride + q0 + lane] = (m_run - P_EXP + __builtin_amdgcn_logf(l_run)) * 0.6931471805599453f;
    // ---- normalise and store: O rows are queries (r&3)+8(r>>2)+4h of this wave, columns d = 32*dt + lane&31
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qr = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float lr = __shfl(l_run, qr, 64);
        const int qi = q0 + qr;
        if (qi < p.N) {
            float* op = p.out + ((size_t)b * p.n_stride + qi) * p.ldo + li;
#pragma unroll
            for (int d = 0; d < DT; ++d) op[32 * d] = om[d][r] / (lr * kOneAccActScale);      // (v carries 16, p and l carry 2^12)
        }
    }
}

// (Round 4 also tried this attention as ONE 512-thread workgroup of two wave groups that run S / softmax / P V one slot apart -- the
//  explicit matrix | vector alternation of the fused spline GEMM.  Bit-identical and no faster, 26.6 against 26.2 ms per C2 step: the
//  softmax is VALU issue time that two waves per SIMD need more of than of MFMA time under any interleaving.  The kernel was removed when
//  this one went to a single accumulator; its measurements stay in DESIGN.md section 9 and profiles/r04q_*, r04r_attn_stamps.log.)

template <int DH, int SH = 0>
static void launch_attn16_dh(const Attn16Params& p, int B, hipStream_t s) {
    constexpr size_t lds = SH ? 2 * 64 * (size_t)(4 * DH) : 2 * 64 * (size_t)(8 * DH + 80);
    char name[64];
    if (SH) snprintf(name, sizeof name, "void fc::attn16_kernel<%d, 1>(fc::Attn16Params)", DH);
    else snprintf(name, sizeof name, "void fc::attn16_kernel<%d>(fc::Attn16Params)", DH);
    launch_kernel<attn16_kernel<DH, SH>, (int)lds>(name, 4.0 * B * (double)p.N * (double)p.M * DH, 0.0, dim3((p.N + 127) / 128, B), dim3(256), lds, s, p);
}

template <int DH>
static void launch_attn_dh(const AttnParams& p, int B, hipStream_t s) {
    constexpr size_t lds = 2 * 2 * (size_t)(DH > 128 ? 32 : 64) * (DH + 4) * sizeof(float);      // 135 KB at head dim 128, 133 KB at 256 (32-key tiles)
    char name[64];
    snprintf(name, sizeof name, "void fc::attn_kernel<%d>(fc::AttnParams)", DH);
    launch_kernel<attn_kernel<DH>, (int)lds>(name, 4.0 * B * (double)p.N * (double)p.M * DH, 0.0, dim3((p.N + 127) / 128, B), dim3(256), lds, s, p);
}

size_t attention_limb_ws_bytes(long kv_rows, int dh_pad) { return dh_pad <= 64 ? (size_t)kv_rows * dh_pad * 8 : 0; }

// The folded engine (flow_engine.cpp, fc_debug_set 33): keys and values of every attention are the context panel itself.  Its limb image
// [row][hi dh_pad | lo dh_pad] (kv_limbs_kernel's K image alone) is made once per forward; every layer then attends over it (AttnKeys::CONTEXT)
void launch_context_limbs(const float* ctx, int ldc, unsigned short* img, long rows, int dh_pad, hipStream_t s) {
    int* flag = gemm_fp16_flag();
    if (!flag || dh_pad > 64 || dh_pad % 4 != 0 || ldc % 4 != 0 || ldc < dh_pad || (((uintptr_t)ctx | (uintptr_t)img) & 15))
        throw Error(FC_ERR_INVALID, "context limb image: needs a guard scope, a head dim <= 64 within the row pitch and 16-byte aligned operands");
    const long n = rows * (dh_pad / 4);
    launch_kernel<kv_limbs_kernel>("fc::kv_limbs_kernel", 0.0, (double)rows * dh_pad * 8.0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ctx, ldc, nullptr, 0, img, nullptr,
                                   rows, dh_pad, flag);
}

// the split-fp16 kernel's parameters over limb images k16 / v16 of row pitch kv_pitch (16-byte chunks); c16: 1 = slices of a GEMM limb-image output
static Attn16Params attn16_params(const AttnQuery& qy, const AttnProblem& pb, const unsigned short* k16, const unsigned short* v16, float* out, int ldo,
                                  int* flag, int kv_pitch, int c16) {
    const AttnLnq* l = qy.lnq;
    return Attn16Params{qy.q, qy.ldq, k16, v16, out, ldo, pb.N, pb.n_stride_rows, pb.M, pb.m_stride_rows, qy.qscale, flag, l ? l->sumsq : nullptr,
                        l ? l->slots : 0, l ? l->pitch : 0, l ? l->inv_width : 0.f, l ? l->bias : nullptr, kv_pitch, c16, nullptr, pb.m_counts};
}

bool launch_attention(const AttnQuery& qy, const AttnKeys& kv, const AttnProblem& pb, float* out, int ldo, hipStream_t s, float* lse) {
    const int B = pb.B, dh_pad = pb.dh_pad;
    if (kv.form == AttnKeys::SLICE && (kv.col0 % 16 != 0 || kv.n_pad % 16 != 0 || dh_pad % 16 != 0))
        throw Error(FC_ERR_INVALID, "attention: limb-image slices must start on 16-column tiles");
    if (B <= 0 || pb.N <= 0 || pb.M <= 0) throw Error(FC_ERR_INVALID, "attention: empty problem");
    int* flag = gemm_fp16_flag();
    if (kv.form == AttnKeys::SLICE) {
        // K / V arrive as slices of the projection GEMM's limb-image output: no fp32 K / V, no conversion pass
        if (!flag || dh_pad > 64 || !kv.img || kv.n_pad / 4 <= 0 || (qy.ldq % 4) != 0)
            throw Error(FC_ERR_INVALID, "attention: limb-image K / V need a guard scope, head dim <= 64 and a pitch");
        const unsigned short* kp = kv.img + (size_t)(kv.col0 / 16) * 32;
        const Attn16Params p = attn16_params(qy, pb, kp, kp + (size_t)(dh_pad / 16) * 32, out, ldo, flag, kv.n_pad / 4, 1);
        if (dh_pad == 32) launch_attn16_dh<32>(p, B, s); else launch_attn16_dh<64>(p, B, s);
        return false;
    }
    if (kv.form == AttnKeys::PANELS) {
        if ((qy.ldq | kv.ldk | kv.ldv) % 4 != 0 || (((uintptr_t)qy.q | (uintptr_t)kv.k | (uintptr_t)kv.v) & 15))
            throw Error(FC_ERR_INVALID, "attention: q/k/v must be 16-byte aligned with pitches that are multiples of 4 floats");
        if (flag && kv.limb_ws && dh_pad <= 64 && g_knobs.attn_fp16) {      // (knob 5)
            // split-fp16 path (needs the caller's Fp16Guard scope for its range check and limb_ws for the K/V limb images)
            const long rows = (long)(B - 1) * pb.m_stride_rows + pb.M;
            unsigned short* k16 = (unsigned short*)kv.limb_ws;
            unsigned short* v16 = k16 + (size_t)rows * 2 * dh_pad;
            const long n = rows * (dh_pad / 4);
            launch_kernel<kv_limbs_kernel>("fc::kv_limbs_kernel", 0.0, (double)rows * dh_pad * 16.0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kv.k, kv.ldk, kv.v, kv.ldv,
                                           k16, v16, rows, dh_pad, flag);
            Attn16Params p = attn16_params(qy, pb, k16, v16, out, ldo, flag, dh_pad / 4, 0);
            p.lse = lse;
            if (dh_pad == 32) launch_attn16_dh<32>(p, B, s); else launch_attn16_dh<64>(p, B, s);
            return lse != nullptr;
        }
        AttnParams p{qy.q, qy.ldq, kv.k, kv.ldk, kv.v, kv.ldv, out, ldo, pb.N, pb.n_stride_rows, pb.M, pb.m_stride_rows, qy.qscale, pb.m_counts};
        switch (dh_pad) {
            case 32: launch_attn_dh<32>(p, B, s); break;
            case 64: launch_attn_dh<64>(p, B, s); break;
            case 128: launch_attn_dh<128>(p, B, s); break;
            case 256: launch_attn_dh<256>(p, B, s); break;
            default: throw Error(FC_ERR_UNSUPPORTED, "attention: inner dim (padded) must be 32, 64, 128 or 256");
        }
        return false;
    }
    // CONTEXT: at head dim 64 with ONE staged tile per 64 keys (attn16_kernel<64, 1>), at 32 with the two-image kernel reading the same image twice
    if (!flag || !kv.img || (dh_pad != 32 && dh_pad != 64) || (qy.ldq % 4) != 0 || (((uintptr_t)qy.q | (uintptr_t)kv.img) & 15))
        throw Error(FC_ERR_INVALID, "attention: the context limb image needs a guard scope, head dim 32 or 64 and 16-byte aligned operands");
    const Attn16Params p = attn16_params(qy, pb, kv.img, kv.img, out, ldo, flag, dh_pad / 4, 0);
    if (dh_pad == 32) launch_attn16_dh<32>(p, B, s); else launch_attn16_dh<64, 1>(p, B, s);
    return false;
}

}  // namespace fc
