// k nearest neighbours in feature space for the DGCNN edge convolutions (models/pytorch_gcn.py:13-20).
//
// Ranking value, same expansion and fp32 operation order as the reference:
//     pd[i][j] = fl( fl(-|xj|^2 + 2 xi.xj) - |xi|^2 ),   top-k LARGEST over j (self included)
// The M x M matrix is never written (the reference materialises it; at 16384 points it is 1 GiB per
// scene per level): distances are produced tile by tile from LDS-staged candidate features and consumed
// immediately by a streaming top-k.
//
// Workgroup = 16 queries of one scene (4 waves x 4 queries).  Per 64-candidate tile each lane owns one
// candidate: it reads its feature row from LDS (ds_read_b128, padded rows -> conflict free) and the four
// query rows as LDS broadcasts.  Selection keeps, per query, an unordered candidate set in LDS:
// values above the current k-th best (tau) are appended with a ballot/popcount compaction; when the set
// exceeds 64 entries it is pruned back to k with a 32-step radix select over the two entries each lane holds.
// Output is the unordered SET of k indices (only max-pooling consumes it).
#include "common.h"
#include "device.h"
#include "launch.h"
#include <climits>
#include <cstdio>

namespace fc {

__device__ __forceinline__ uint32_t sortable_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}
__device__ __forceinline__ int popc64(unsigned long long m) { return __popcll(m); }

// prune the wave-private set (vals/idxs in LDS, cnt entries <= 128) down to its k largest; returns the k-th largest value
__device__ __forceinline__ float prune_set(float* vals, int32_t* idxs, int cnt, int k, int lane) {
    const bool h0 = lane < cnt, h1 = 64 + lane < cnt;
    const float v0 = h0 ? vals[lane] : 0.f, v1 = h1 ? vals[64 + lane] : 0.f;
    const int32_t i0 = h0 ? idxs[lane] : 0, i1 = h1 ? idxs[64 + lane] : 0;
    const uint32_t k0 = h0 ? sortable_key(v0) : 0u, k1 = h1 ? sortable_key(v1) : 0u;
    uint32_t prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t t = prefix | (1u << bit);
        const int c = popc64(__ballot(k0 >= t)) + popc64(__ballot(k1 >= t));
        if (c >= k) prefix = t;
    }
    // keep everything above the k-th key, and the first ties (slot order) to fill up to k
    const unsigned long long gt0 = __ballot(k0 > prefix), gt1 = __ballot(k1 > prefix);
    const unsigned long long eq0 = __ballot(h0 && k0 == prefix), eq1 = __ballot(h1 && k1 == prefix);
    const int n_gt = popc64(gt0) + popc64(gt1);
    const int need_eq = k - n_gt;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int eq_rank0 = popc64(eq0 & lt), eq_rank1 = popc64(eq0) + popc64(eq1 & lt);
    const bool keep0 = (k0 > prefix) || (h0 && k0 == prefix && eq_rank0 < need_eq);
    const bool keep1 = (k1 > prefix) || (h1 && k1 == prefix && eq_rank1 < need_eq);
    const unsigned long long m0 = __ballot(keep0), m1 = __ballot(keep1);
    if (keep0) { const int p = popc64(m0 & lt); vals[p] = v0; idxs[p] = i0; }
    if (keep1) { const int p = popc64(m0) + popc64(m1 & lt); vals[p] = v1; idxs[p] = i1; }
    return key_to_float(prefix);
}

constexpr int KNN_Q = 4;        // queries per wave
constexpr int KNN_CAP = 128;    // set capacity per query

// knn_kernel and knn_counts_kernel are the same statements, csrc/knn_lane_body.h, included in both.  In them M is the scene's points in every
// role the key count has (tiles, clamps, masks, the store's guard), m_rows the rows per scene of idx_out, [B][m_rows][k], and m_stride the
// rows per scene of f; the uniform kernel has M for both.  (Why an include and not a function: knn_lane_body.h.)
__global__ __launch_bounds__(256) void knn_kernel(const float* __restrict__ f, int ldf, int Cp, int32_t* __restrict__ idx_out, int M,
                                                  int m_stride, int k) {
    const int m_rows = M;
#include "knn_lane_body.h"
}

// Per-scene point counts (fcflow_embed_counts.h): scene b is searched as if it had been passed alone with its first M_b rows, M_b =
// scene_count(m_counts, b, count_min, count_max); idx_out keeps its [B][M][k] shape and rows >= M_b of it are written by nobody.  The grid
// covers count_max queries: a workgroup whose first query is past its scene's end leaves before any LDS write or barrier, and so does every
// workgroup of a scene that the other kernel owns (M_b >= mfma_from, the count from which a scene alone takes the matrix-core kernel).
__global__ __launch_bounds__(256) void knn_counts_kernel(const float* __restrict__ f, int ldf, int Cp, int32_t* __restrict__ idx_out, int M,
                                                         int m_stride, int k, const int32_t* __restrict__ m_counts, int count_min, int count_max,
                                                         int mfma_from) {
    const int Mb = scene_count(m_counts, blockIdx.y, count_min, count_max);
    if (Mb >= mfma_from || (int)blockIdx.x * 16 >= Mb) return;
    const int m_rows = M;
    M = Mb;
#include "knn_lane_body.h"
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same selection on the matrix cores (round 3).  The reference literally computes the Gram matrix with `matmul`
// (models/pytorch_gcn.py:13-16); here a wave owns 32 queries and produces a 32 x 32 tile of inner products per step with
// v_mfma_f32_32x32x2_f32 -- exact fp32 products and sums, the fp32-input matrix rate is twice the scalar FMA rate and needs ONE LDS
// read per 4 products where the lane-per-candidate loop above needs five per 16 -- queries as the A operand (held in registers for the
// whole launch), candidates as B (staged through LDS in blocks of 64, double-buffered, one barrier per block, shared by the four waves
// of a workgroup).  The accumulator of a lane then holds 16 QUERIES of ONE candidate (column = lane & 31, rows 8 (r / 4) + 4 (lane >>
// 5) + r % 4), so `pd > tau` is one compare per register and a ballot tells which of the 32 candidates beat the current k-th best of the
// two queries a register stands for (lower / upper half-wave).
// The per-query top-k lives in REGISTERS, sorted: query (r, half) owns one value VGPR and one index VGPR, entry e on lane e (k <= 64).
// A hit is inserted with one whole-wave lane shift (v_mov_b32_dpp wave_shr:1): lanes holding smaller entries take min(left neighbour,
// new value), so the list stays sorted, the k-th best (lane k - 1) is always exact -- tau never lags, which keeps the hits at
// k (1 + ln(M / k)) per query instead of the ~2x of the lazily pruned LDS set above -- and nothing of it touches LDS.
// Ranking value as above: pd = fl( fl(2 xi.xj - |xj|^2) - |xi|^2 ), largest first, strict `>` against the k-th best (earlier candidates
// win ties); norms are summed per half-row and then across the two halves, queries and candidates alike.

__device__ __forceinline__ float knn_wave_shr1(float v, float edge) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ int knn_wave_shr1(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }

// inserts (v, ci) into the descending list (sv, si): entry e on lane e; what falls off lane 63 is lost (k <= 64 entries matter)
__device__ __forceinline__ void knn_insert(float& sv, int& si, float v, int ci) {
    const bool smaller = sv < v;                                  // a suffix of the lanes
    const float shv = knn_wave_shr1(sv, INFINITY);                // lane e <- entry e - 1; lane 0 <- +inf
    const int shi = knn_wave_shr1(si, 0);
    const bool moved = shv < v;                                   // lanes behind the insertion point
    const float nv = moved ? shv : v;
    const int ni = moved ? shi : ci;
    sv = smaller ? nv : sv;
    si = smaller ? ni : si;
}

constexpr int KM_TC = 64;       // candidates per LDS block

// (knn_mfma_kernel and knn_mfma_counts_kernel: the statements of csrc/knn_mfma_body.h, included in both; M, m_rows and m_stride as in the
// lane kernels, and `warm` is [B][m_rows][k] like idx_out)
template <int CP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void knn_mfma_kernel(const float* __restrict__ f, int ldf, int C, int32_t* idx_out, int M, int m_stride,
                                                       int k, const int32_t* warm) {
    const int m_rows = M;
#include "knn_mfma_body.h"
}

// (with per-scene counts, as knn_counts_kernel: the scenes below mfma_from belong to that kernel, and a workgroup's first query is blockIdx.x * 128)
template <int CP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void knn_mfma_counts_kernel(const float* __restrict__ f, int ldf, int C, int32_t* idx_out, int M,
                                                       int m_stride, int k, const int32_t* warm, const int32_t* __restrict__ m_counts, int count_min, int count_max, int mfma_from) {
    const int Mb = scene_count(m_counts, blockIdx.y, count_min, count_max);
    if (Mb < mfma_from || (int)blockIdx.x * 128 >= Mb) return;
    const int m_rows = M;
    M = Mb;
#include "knn_mfma_body.h"
}

// cnt: null for the uniform launch, or the per-scene counts of a counted one (grid over cnt->hi queries; mfma_from as in the kernels)
template <int CP>
static void launch_knn_mfma(const float* f, int ldf, int C, int32_t* idx, int B, int M, int m_stride_rows, int k, hipStream_t s, const int32_t* warm,
                            const SceneCounts* cnt = nullptr, int mfma_from = 0) {
    constexpr size_t lds = (2 * (size_t)KM_TC * (CP + 4) + 256) * sizeof(float);
    char name[160];
    if (cnt) {
        snprintf(name, sizeof name, "void fc::knn_mfma_counts_kernel<%d>(float const*, int, int, int*, int, int, int, int const*, int const*, int, int, int)", CP);
        launch_kernel<knn_mfma_counts_kernel<CP>, (int)lds>(name, 2.0 * B * (double)cnt->hi * cnt->hi * C, 4.0 * B * (double)cnt->hi * (C + k), dim3((cnt->hi + 127) / 128, B),
                                                            dim3(256), lds, s, f, ldf, C, idx, M, m_stride_rows, k, warm, cnt->counts, cnt->lo, cnt->hi, mfma_from);
        return;
    }
    snprintf(name, sizeof name, "void fc::knn_mfma_kernel<%d>(float const*, int, int, int*, int, int, int, int const*)", CP);
    launch_kernel<knn_mfma_kernel<CP>, (int)lds>(name, 2.0 * B * (double)M * M * C, 4.0 * B * (double)M * (C + k), dim3((M + 127) / 128, B), dim3(256), lds, s,
                                                 f, ldf, C, idx, M, m_stride_rows, k, warm);
}

// The kernel choice in two parts.  The shape part: the padded feature width of the matrix-core kernel where it takes features of this shape,
// 0 where it does not (wider features, a pitch that does not cover the padded row, knob 24 = 0) ...
static int knn_mfma_shape(int ldf, int C) {
    if (!g_knobs.knn_mfma) return 0;                                // (knob 24)
    const int Cp8 = C <= 8 ? 8 : (C <= 16 ? 16 : (C <= 32 ? 32 : (C <= 64 ? 64 : (C <= 128 ? 128 : 0))));
    return Cp8 && ldf >= Cp8 ? Cp8 : 0;
}
// ... and the count from which a scene of such a shape takes it.  Small scenes take the lane-per-candidate kernel -- a workgroup of the MFMA
// kernel owns 128 queries for ALL M candidates, which takes as long with two scenes in the batch as with sixteen, so the choice depends on
// M alone (a scene's neighbour sets, near-ties included, must not depend on the batch it sits in); at M = 1024 the 16-query
// workgroups of the lane-per-candidate kernel finish a C1 batch in 0.37 ms against 2.7.  A counted search asks per scene (launch_knn_counts).
static int knn_mfma_from() { return g_knobs.knn_mfma == 2 ? 1 : 2048; }
// the padded feature width of the matrix-core kernel where a search of this shape takes it, 0 where it takes the lane-per-candidate kernel
static int knn_mfma_width(int ldf, int C, int M) { return M >= knn_mfma_from() ? knn_mfma_shape(ldf, C) : 0; }
static size_t knn_lane_lds(int Cp) { return ((size_t)(64 + 16) * (Cp + 4) + 16 + 16 * KNN_CAP) * sizeof(float) + 16 * KNN_CAP * sizeof(int32_t); }

// every refusal of launch_knn that the shape alone decides (an operator entry asks before it launches anything of its own)
void knn_check_shape(int ldf, int C, int M, int k) {
    if (k > 64 || k < 1) throw Error(FC_ERR_UNSUPPORTED, "knn: k must be in [1, 64]");
    if (M < k) throw Error(FC_ERR_INVALID, "knn: fewer points than neighbours (torch.topk would raise as well)");
    if (!knn_mfma_width(ldf, C, M) && knn_lane_lds(round_up(C, 4)) > 160 * 1024)
        throw Error(FC_ERR_UNSUPPORTED, "knn: feature dimension too large for the LDS tile");
}

// warm: k neighbours per query of the same cloud from another feature space (may alias idx: a workgroup reads its own queries' sets before it
// writes them), or null; used by the matrix-core kernel only -- the result is the exact top-k set either way
void launch_knn(const float* f, int ldf, int C, int32_t* idx, int B, int M, int m_stride_rows, int k, hipStream_t s, const int32_t* warm) {
    if (!g_knobs.knn_warm) warm = nullptr;                          // (knob 32)
    knn_check_shape(ldf, C, M, k);
    const int Cp = round_up(C, 4);
    if (ldf < Cp || ldf % 4 != 0 || ((uintptr_t)f & 15)) throw Error(FC_ERR_INVALID, "knn: feature pitch must cover round_up(C,4) and be 16-byte aligned");
    switch (knn_mfma_width(ldf, C, M)) {
        case 0: break;
        case 8: return launch_knn_mfma<8>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm);
        case 16: return launch_knn_mfma<16>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm);
        case 32: return launch_knn_mfma<32>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm);
        case 64: return launch_knn_mfma<64>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm);
        default: return launch_knn_mfma<128>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm);
    }
    launch_kernel<knn_kernel, 160 * 1024>("fc::knn_kernel(float const*, int, int, int*, int, int, int)", 2.0 * B * (double)M * M * C, 4.0 * B * (double)M * (C + k),
                                          dim3((M + 15) / 16, B), dim3(256), knn_lane_lds(Cp), s, f, ldf, Cp, idx, M, m_stride_rows, k);
}

// ---- per-scene counts (fcflow_embed_counts.h): scene b is searched over its first clamp(counts[b], lo, hi) rows, by the kernel it takes alone.
// the refusals of launch_knn_counts that shape and bounds decide: k <= lo <= hi <= M, and the lane kernel's LDS tile where a scene can take it
void knn_check_counts(int ldf, int C, int M, int k, const SceneCounts& cnt) {
    if (k > 64 || k < 1) throw Error(FC_ERR_UNSUPPORTED, "knn: k must be in [1, 64]");
    if (!cnt.counts) throw Error(FC_ERR_INVALID, "knn: null counts (the search without counts is launch_knn)");
    if (cnt.lo < k) throw Error(FC_ERR_INVALID, "knn: count_min: fewer points than neighbours (torch.topk would raise as well)");
    if (cnt.lo > cnt.hi || cnt.hi > M) throw Error(FC_ERR_INVALID, "knn: counts must satisfy k <= count_min <= count_max <= M");
    const int from = knn_mfma_shape(ldf, C) ? knn_mfma_from() : INT_MAX;
    if (cnt.lo < from && knn_lane_lds(round_up(C, 4)) > 160 * 1024) throw Error(FC_ERR_UNSUPPORTED, "knn: feature dimension too large for the LDS tile");
}

// idx (and warm) stay [B][M][k]; rows >= a scene's count are not written.  The lane kernel is launched iff some scene can lie below the
// threshold, the matrix-core kernel iff some scene can lie at or above it: a batch on both sides costs two launches, each scene's workgroups
// leave the launch that is not theirs at once, and every scene gets exactly the sets it gets alone.
void launch_knn_counts(const float* f, int ldf, int C, int32_t* idx, int B, int M, int m_stride_rows, int k, hipStream_t s, const int32_t* warm, const SceneCounts& cnt) {
    if (!g_knobs.knn_warm) warm = nullptr;                          // (knob 32)
    knn_check_counts(ldf, C, M, k, cnt);
    const int Cp = round_up(C, 4);
    if (ldf < Cp || ldf % 4 != 0 || ((uintptr_t)f & 15)) throw Error(FC_ERR_INVALID, "knn: feature pitch must cover round_up(C,4) and be 16-byte aligned");
    const int width = knn_mfma_shape(ldf, C), from = width ? knn_mfma_from() : INT_MAX;
    if (cnt.lo < from)
        launch_kernel<knn_counts_kernel, 160 * 1024>("fc::knn_counts_kernel(float const*, int, int, int*, int, int, int, int const*, int, int, int)",
                                                     2.0 * B * (double)cnt.hi * cnt.hi * C, 4.0 * B * (double)cnt.hi * (C + k), dim3((cnt.hi + 15) / 16, B), dim3(256),
                                                     knn_lane_lds(Cp), s, f, ldf, Cp, idx, M, m_stride_rows, k, cnt.counts, cnt.lo, cnt.hi, from);
    if (cnt.hi < from) return;
    switch (width) {
        case 8: return launch_knn_mfma<8>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm, &cnt, from);
        case 16: return launch_knn_mfma<16>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm, &cnt, from);
        case 32: return launch_knn_mfma<32>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm, &cnt, from);
        case 64: return launch_knn_mfma<64>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm, &cnt, from);
        default: return launch_knn_mfma<128>(f, ldf, C, idx, B, M, m_stride_rows, k, s, warm, &cnt, from);
    }
}

}  // namespace fc
