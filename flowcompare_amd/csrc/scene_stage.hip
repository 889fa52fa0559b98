// Staging of whole scene pairs: what the voxel loader does per item (dataloaders/ams_voxel_loader.py:291-307),
// for every voxel centre of a scene at once.
//   * box membership (utils.get_voxel, utils.py:135-142) of every cloud row in every box, counted and then selected into a CSR
//     list in ASCENDING row order, without atomics: the same input gives the same bytes, and farthest point sampling, which
//     starts at a voxel's first row and breaks ties to the lowest position, sees the rows in the reference's order;
//   * farthest point sampling of every voxel's rows, voxels of different sizes in one launch, one workgroup per voxel, with the
//     distance arithmetic of fps_nd_kernel (fps_dist.h).
#include "common.h"
#include "launch.h"
#include "fps_dist.h"
#include "block_reduce.h"

#include <algorithm>

namespace fc {

// ---------------------------------------------------------------- box membership
// A wave owns kVoxChunk = 512 consecutive cloud rows (8 per lane, row = chunk * 512 + it * 64 + lane, held in registers), a workgroup
// of 4 waves 2048 rows and a tile of kVoxTile boxes whose bounds sit in LDS.  Ascending row order inside a chunk is (it, lane): the
// rank of a member is the popcount of the earlier ballots plus the popcount of the lower lanes of its own ballot.  The count pass
// writes one int per (chunk, box) into table[chunk * K + box]; voxel_scan_kernel turns every box's column into an exclusive prefix
// over the chunks (and its total into counts[box]); the select pass repeats the tests and writes row numbers at
// offsets[box] + table[chunk * K + box] + rank.  No wave needs another wave's result inside a launch, so there is no barrier
// after the tile load and nothing is appended atomically.
constexpr int kVoxChunk = 512, kVoxWaves = 4, kVoxTile = 256, kVoxPerLane = kVoxChunk / 64;

__device__ __forceinline__ unsigned lanes_below(unsigned long long mask, int lane) {
    return (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

// SELECT = false: table[chunk * K + k] = members of box k among the chunk's rows.
// SELECT = true : rows[offsets[k] + table[chunk * K + k] + rank] = row number, for every member (table already scanned).
template <bool SELECT>
__global__ __launch_bounds__(64 * kVoxWaves) void voxel_member_kernel(const float* __restrict__ cloud, int ld, int P, const float* __restrict__ centers, int K,
                                                                      float hx, float hy, float hz, int* __restrict__ table,
                                                                      const int64_t* __restrict__ offsets, int32_t* __restrict__ rows, int64_t rows_cap) {
    __shared__ float lo[3][kVoxTile], hi[3][kVoxTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k0 = blockIdx.y * kVoxTile;
    // lo = c - d/2, hi = c + d/2 in fp32, one rounding each (d/2 is exact), as torch rounds `center - dimensions / 2`
    for (int j = threadIdx.x; j < kVoxTile; j += 64 * kVoxWaves) {
        const int k = k0 + j;
        const float cx = k < K ? centers[3 * (size_t)k] : NAN, cy = k < K ? centers[3 * (size_t)k + 1] : NAN, cz = k < K ? centers[3 * (size_t)k + 2] : NAN;
        lo[0][j] = cx - hx; lo[1][j] = cy - hy; lo[2][j] = cz - hz;
        hi[0][j] = cx + hx; hi[1][j] = cy + hy; hi[2][j] = cz + hz;
    }
    __syncthreads();
    const int chunk = blockIdx.x * kVoxWaves + wave;
    const long row0 = (long)chunk * kVoxChunk;
    if (row0 >= P) return;                                   // whole wave; after the only barrier
    float x[kVoxPerLane], y[kVoxPerLane], z[kVoxPerLane];
#pragma unroll
    for (int it = 0; it < kVoxPerLane; ++it) {
        const long r = row0 + it * 64 + lane;
        const bool in = r < P;                               // rows beyond the cloud are NaN: in no box
        x[it] = in ? cloud[(size_t)r * ld] : NAN;
        y[it] = in ? cloud[(size_t)r * ld + 1] : NAN;
        z[it] = in ? cloud[(size_t)r * ld + 2] : NAN;
    }
    const int kend = min(kVoxTile, K - k0);
    for (int g = 0; g < kend; g += 64) {                     // 64 boxes at a time: lane j keeps box g + j's count / write base
        const int kb = k0 + g + lane;
        int mine = 0;
        long long base = 0;
        if (SELECT && g + lane < kend) base = (long long)offsets[kb] + table[(size_t)chunk * K + kb];
        const int jend = min(64, kend - g);
        for (int j = 0; j < jend; ++j) {
            const int t = g + j;
            const float lx = lo[0][t], ly = lo[1][t], lz = lo[2][t], ux = hi[0][t], uy = hi[1][t], uz = hi[2][t];
            const long long wbase = SELECT ? __shfl(base, j, 64) : 0;
            unsigned run = 0;
#pragma unroll
            for (int it = 0; it < kVoxPerLane; ++it) {
                const bool in = x[it] >= lx && x[it] <= ux && y[it] >= ly && y[it] <= uy && z[it] >= lz && z[it] <= uz;
                const unsigned long long b = __ballot(in);
                if (SELECT && in) {
                    const long long pos = wbase + run + lanes_below(b, lane);
                    if (pos >= 0 && pos < rows_cap) rows[pos] = (int32_t)(row0 + it * 64 + lane);    // cap: offsets that do not belong to this table
                }
                run += (unsigned)__popcll(b);
            }
            if (!SELECT && lane == j) mine = (int)run;
        }
        if (!SELECT && g + lane < kend) table[(size_t)chunk * K + kb] = mine;
    }
}

// One thread per box: exclusive prefix of its column over the chunks, total -> counts.  Consecutive threads read consecutive ints.
__global__ __launch_bounds__(64) void voxel_scan_kernel(int* __restrict__ table, int n_chunks, int K, int32_t* __restrict__ counts) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    int run = 0;
    int c = 0;
    for (; c + 8 <= n_chunks; c += 8) {                      // 8 independent loads in flight
        int t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = table[(size_t)(c + u) * K + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) { table[(size_t)(c + u) * K + k] = run; run += t[u]; }
    }
    for (; c < n_chunks; ++c) { const int t = table[(size_t)c * K + k]; table[(size_t)c * K + k] = run; run += t; }
    counts[k] = run;
}

static int voxel_chunks(long P) { return (int)((P + kVoxChunk - 1) / kVoxChunk); }

size_t voxel_ws_bytes(long P, int K) { return (size_t)std::max(voxel_chunks(std::max(P, 1L)), 1) * (size_t)std::max(K, 1) * sizeof(int); }

static void check_voxel_args(const float* cloud, int ld, long P, const float* centers, int K, const void* ws, size_t ws_bytes) {
    if (!cloud || !centers || !ws) throw Error(FC_ERR_INVALID, "voxel membership: null pointer");
    if (ld < 3 || P < 1 || P > 0x7fffffffL - kVoxChunk || K < 1) throw Error(FC_ERR_INVALID, "voxel membership: bad shape");
    if ((K + kVoxTile - 1) / kVoxTile > 65535) throw Error(FC_ERR_UNSUPPORTED, "voxel membership: more than 16 776 960 boxes");
    if (ws_bytes < voxel_ws_bytes(P, K)) throw Error(FC_ERR_WORKSPACE, "voxel membership: workspace smaller than fc_stage_voxel_ws_bytes");
}

static dim3 voxel_grid(long P, int K) { return dim3((voxel_chunks(P) + kVoxWaves - 1) / kVoxWaves, (K + kVoxTile - 1) / kVoxTile); }

// algorithmic bytes of one membership pass: the cloud's xyz once per box tile, one table entry per (chunk, box)
static double voxel_pass_bytes(long P, int K) { return (double)((K + kVoxTile - 1) / kVoxTile) * P * 12.0 + 4.0 * voxel_chunks(P) * (double)K; }

void launch_voxel_count(const float* cloud, int ld, long P, const float* centers, int K, float dx, float dy, float dz, int32_t* counts, void* ws,
                        size_t ws_bytes, hipStream_t s) {
    check_voxel_args(cloud, ld, P, centers, K, ws, ws_bytes);
    if (!counts) throw Error(FC_ERR_INVALID, "voxel count: null pointer");
    launch_kernel<voxel_member_kernel<false>>("fc::voxel_member_kernel<false>", 0.0, voxel_pass_bytes(P, K), voxel_grid(P, K), dim3(64 * kVoxWaves), 0, s, cloud, ld, (int)P, centers, K,
                                              dx * 0.5f, dy * 0.5f, dz * 0.5f, (int*)ws, (const int64_t*)nullptr, (int32_t*)nullptr, (int64_t)0);
    launch_kernel<voxel_scan_kernel>("fc::voxel_scan_kernel", 0.0, 8.0 * voxel_chunks(P) * (double)K, dim3((K + 63) / 64), dim3(64), 0, s, (int*)ws, voxel_chunks(P), K, counts);
}

void launch_voxel_select(const float* cloud, int ld, long P, const float* centers, int K, float dx, float dy, float dz, const int64_t* offsets,
                         int32_t* rows, int64_t rows_cap, const void* ws, size_t ws_bytes, hipStream_t s) {
    check_voxel_args(cloud, ld, P, centers, K, ws, ws_bytes);
    if (!offsets || rows_cap < 0 || (rows_cap > 0 && !rows)) throw Error(FC_ERR_INVALID, "voxel select: bad argument");
    if (rows_cap == 0) return;
    launch_kernel<voxel_member_kernel<true>>("fc::voxel_member_kernel<true>", 0.0, voxel_pass_bytes(P, K) + 4.0 * rows_cap, voxel_grid(P, K), dim3(64 * kVoxWaves), 0, s, cloud, ld, (int)P,
                                             centers, K, dx * 0.5f, dy * 0.5f, dz * 0.5f, (int*)const_cast<void*>(ws), offsets, rows, rows_cap);
}

// ---------------------------------------------------------------- ragged farthest point sampling
// One workgroup per listed voxel v: n = offsets[v + 1] - offsets[v] rows of the cloud, named by rows[offsets[v] ...] in ascending
// order.  Same algorithm, reduction order and tie rule as fps_nd_kernel on the cropped voxel (first pick = position 0, running
// distances min'ed in place, first maximum wins); positions are translated to cloud row numbers on output.
//   PTS_LDS : the voxel's rows are gathered ONCE into LDS (n * C floats behind the n running distances) and every pass reads them
//             there; the values are the cloud's own floats, so the selection cannot differ from reading them in place;
//   otherwise the rows are read through the index list on every pass; the running distances live in LDS up to kFpsLdsDist rows
//   and in dist_scratch[offsets[v] ...] beyond (as in fps_nd_kernel).
constexpr int kFpsLdsDist = 24576;                           // fps_nd_kernel's limit
constexpr int kFpsLdsFloats = 36864;                         // 144 KB of gfx950's 160 KB per workgroup

template <bool PTS_LDS>
__device__ __forceinline__ void fps_ragged_body(const float* __restrict__ cloud, int ld, int C, int P, const int32_t* __restrict__ vr, int n, int m,
                                                int64_t* __restrict__ out, float* __restrict__ dist, float* __restrict__ pts, float* red_v, int* red_i,
                                                int* s_last) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto cloud_row = [&](int k) { return cloud + (size_t)min(max(vr[k], 0), P - 1) * ld; };    // clamped: a bad list cannot read outside the cloud
    for (int k = tid; k < n; k += 1024) {
        dist[k] = INFINITY;
        if (PTS_LDS) {
            const float* r = cloud_row(k);
            for (int c = 0; c < C; ++c) pts[(size_t)k * C + c] = r[c];
        }
    }
    if (tid == 0) { out[0] = vr[0]; *s_last = 0; }
    __syncthreads();
    for (int j = 1; j < m; ++j) {
        const int last = *s_last;
        const float* lr = PTS_LDS ? pts + (size_t)last * C : cloud_row(last);
        float ref[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) ref[c] = c < C ? lr[c] : 0.f;
        float best = -1.f;
        int besti = 0x7fffffff;
        for (int k = tid; k < n; k += 1024) {
            const float d2 = fminf(fps_row_dist2(PTS_LDS ? pts + (size_t)k * C : cloud_row(k), ref, C), dist[k]);
            dist[k] = d2;
            if (d2 > best) { best = d2; besti = k; }          // ascending k: keeps this thread's lowest position among equals
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(besti, off, 64);
            if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
        }
        if (lane == 0) { red_v[wave] = best; red_i[wave] = besti; }
        __syncthreads();
        if (wave == 0) {
            float v = lane < 16 ? red_v[lane] : -2.f;
            int i = lane < 16 ? red_i[lane] : 0x7fffffff;
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(v, off, 64);
                const int oi = __shfl_xor(i, off, 64);
                if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
            }
            if (lane == 0) { *s_last = i; out[j] = vr[i]; }
        }
        __syncthreads();
    }
}

// One voxel's sampling on the residency path its size asks for, the choice fps_ragged_kernel makes; false when no path holds the voxel
// (refused by the host beforehand).  fps_ragged_kernel keeps its own three lines: routed through this helper hipcc gives it 32 VGPRs, not 30.
__device__ __forceinline__ bool fps_ragged_voxel(const float* __restrict__ cloud, int ld, int C, int P, const int32_t* __restrict__ vr, int n, int m,
                                                 int64_t* __restrict__ out, float* sm, int lds_floats, float* __restrict__ dist_scratch, int64_t off, float* red_v,
                                                 int* red_i, int* s_last) {
    if ((int64_t)n * (C + 1) <= lds_floats)
        fps_ragged_body<true>(cloud, ld, C, P, vr, n, m, out, sm, sm + n, red_v, red_i, s_last);
    else if (n <= min(lds_floats, kFpsLdsDist))
        fps_ragged_body<false>(cloud, ld, C, P, vr, n, m, out, sm, nullptr, red_v, red_i, s_last);
    else if (dist_scratch)
        fps_ragged_body<false>(cloud, ld, C, P, vr, n, m, out, dist_scratch + off, nullptr, red_v, red_i, s_last);
    else
        return false;
    return true;
}

__global__ __launch_bounds__(1024) void fps_ragged_kernel(const float* __restrict__ cloud, int ld, int C, int P, const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ rows, const int32_t* __restrict__ voxel_ids,
                                                          int64_t* __restrict__ idx, int m, int lds_floats, float* __restrict__ dist_scratch) {
    extern __shared__ float sm[];
    __shared__ float red_v[16];
    __shared__ int red_i[16];
    __shared__ int s_last;
    const int v = voxel_ids ? voxel_ids[blockIdx.x] : (int)blockIdx.x;
    const int64_t off = offsets[v];
    const int64_t n64 = offsets[v + 1] - off;
    if (n64 < m || n64 > 0x7fffffff) return;                  // refused by the host beforehand; uniform over the workgroup
    const int n = (int)n64;
    const int32_t* vr = rows + off;
    int64_t* out = idx + (size_t)blockIdx.x * m;
    if ((int64_t)n * (C + 1) <= lds_floats)
        fps_ragged_body<true>(cloud, ld, C, P, vr, n, m, out, sm, sm + n, red_v, red_i, &s_last);
    else if (n <= min(lds_floats, kFpsLdsDist))
        fps_ragged_body<false>(cloud, ld, C, P, vr, n, m, out, sm, nullptr, red_v, red_i, &s_last);
    else if (dist_scratch)
        fps_ragged_body<false>(cloud, ld, C, P, vr, n, m, out, dist_scratch + off, nullptr, red_v, red_i, &s_last);
}

// The same with a sample count per voxel: a listed voxel with n rows takes m_v = min(n, m) picks -- fps_ragged_voxel
// with m_v in place of m, so idx[v, :m_v] is what the kernel above gives for m_v samples -- and the workgroup itself writes the literal -1 into
// idx[v, m_v:] and m_v into sample_counts[v]: the outputs need no initialisation.  A voxel without rows (or one no residency path holds)
// writes count 0 and a row of -1.
__global__ __launch_bounds__(1024) void fps_ragged_counts_kernel(const float* __restrict__ cloud, int ld, int C, int P, const int64_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ rows, const int32_t* __restrict__ voxel_ids,
                                                                 int64_t* __restrict__ idx, int32_t* __restrict__ sample_counts, int m, int lds_floats,
                                                                 float* __restrict__ dist_scratch) {
    extern __shared__ float sm[];
    __shared__ float red_v[16];
    __shared__ int red_i[16];
    __shared__ int s_last;
    const int v = voxel_ids ? voxel_ids[blockIdx.x] : (int)blockIdx.x;
    const int64_t off = offsets[v];
    const int64_t n64 = offsets[v + 1] - off;
    int64_t* out = idx + (size_t)blockIdx.x * m;
    int m_v = n64 < 1 || n64 > 0x7fffffff ? 0 : (int)min(n64, (int64_t)m);      // uniform over the workgroup
    if (m_v > 0 && !fps_ragged_voxel(cloud, ld, C, P, rows + off, (int)n64, m_v, out, sm, lds_floats, dist_scratch, off, red_v, red_i, &s_last))
        m_v = 0;
    for (int j = m_v + (int)threadIdx.x; j < m; j += 1024) out[j] = -1;
    if (threadIdx.x == 0) sample_counts[blockIdx.x] = m_v;
}

// sample_counts null: fps_ragged_kernel (every listed voxel has at least m rows); otherwise fps_ragged_counts_kernel, where m may exceed max_rows
// (every listed voxel is sparse).
void launch_fps_ragged(const float* cloud, int ld, int C, long P, const int64_t* offsets, const int32_t* rows, const int32_t* voxel_ids, int n_voxels,
                       int max_rows, int m, int64_t* idx, int32_t* sample_counts, float* dist_scratch, hipStream_t s) {
    if (n_voxels <= 0 || m <= 0) return;
    if (!cloud || !offsets || !rows || !idx) throw Error(FC_ERR_INVALID, "ragged fps: null pointer");
    if (C < 1 || C > 8 || ld < C) throw Error(FC_ERR_UNSUPPORTED, "fps: 1..8 feature columns supported");
    if (P < 1 || P > 0x7fffffffL) throw Error(FC_ERR_INVALID, "ragged fps: bad cloud size");
    if (max_rows < 0) throw Error(FC_ERR_INVALID, "ragged fps: bad max_rows");
    if (!sample_counts && m > max_rows) throw Error(FC_ERR_INVALID, "fps: more samples than points");
    if (max_rows > kFpsLdsDist && !dist_scratch)
        throw Error(FC_ERR_WORKSPACE, "ragged fps: voxels above 24576 rows need a float scratch as long as the row list");
    const long want = (long)max_rows * (C + 1);
    const int lds_floats = want <= kFpsLdsFloats ? (int)want : kFpsLdsFloats;          // >= min(max_rows, 24576) either way
    const double bytes = 4.0 * n_voxels * ((double)max_rows * (C + 1) + 2.0 * m);
    if (!sample_counts)
        launch_kernel<fps_ragged_kernel, kFpsLdsFloats * 4>("fc::fps_ragged_kernel", 0.0, bytes, dim3(n_voxels), dim3(1024), (size_t)lds_floats * sizeof(float), s, cloud, ld, C,
                                                            (int)P, offsets, rows, voxel_ids, idx, m, lds_floats, dist_scratch);
    else
        launch_kernel<fps_ragged_counts_kernel, kFpsLdsFloats * 4>("fc::fps_ragged_counts_kernel", 0.0, bytes, dim3(n_voxels), dim3(1024), (size_t)lds_floats * sizeof(float), s,
                                                                   cloud, ld, C, (int)P, offsets, rows, voxel_ids, idx, sample_counts, m, lds_floats, dist_scratch);
}

// ---------------------------------------------------------------- gather + joint normalisation with a context count per pair
// One workgroup per pair k: its context cloud is the c = clamp(counts_0[k], 1, M) rows of cloud_0 named by index_0[k, :c], its target cloud the
// N rows of cloud_1 named by index_1[k] (the lists the ragged FPS kernels write; -1 behind c is never read).  The rows are read straight through
// the lists -- no gathered intermediate -- and normalised with co_unit_sphere_kernel's operations in that kernel's order (staging.hip: strided
// sums over the joint index, block_sum / block_max of block_reduce.h, subtract then divide), so the result is bit for bit what that kernel gives
// for the pair (cloud_0[index_0[k, :c]], cloud_1[index_1[k]]).  Rows c .. M-1 of out_0[k] are written as 0.0f: the outputs need no initialisation.
// stage_pair_body is one pair.  TARGET_COUNTS = false is the entry above as it was (counts_1 unused, every one of the N target rows real);
// TARGET_COUNTS = true gives the target its own count n = clamp(counts_1[k], 1, N) -- the -1 behind it in index_1[k] is
// never read, rows n .. N-1 of out_1[k] are written as 0.0f -- and lets counts_0 be null (every context row real).  The flag is a template
// parameter, so the first instantiation holds the statements it always held, in their order.
template <bool TARGET_COUNTS>
__device__ __forceinline__ void stage_pair_body(const float* __restrict__ cloud_0, int P0, const float* __restrict__ cloud_1, int P1, int ld,
                                                const int64_t* __restrict__ index_0, const int64_t* __restrict__ index_1,
                                                const int32_t* __restrict__ counts_0, const int32_t* __restrict__ counts_1, int M, int N,
                                                float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ inverse, float* red) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n0 = TARGET_COUNTS && !counts_0 ? M : min(max(counts_0[b], 1), M);
    const int n1 = TARGET_COUNTS ? min(max(counts_1[b], 1), N) : N;
    const int n = n0 + n1;
    const int64_t* i0 = index_0 + (size_t)b * M;
    const int64_t* i1 = index_1 + (size_t)b * N;
    auto row = [&](int k) {                                    // clamped: a bad list cannot read outside the clouds
        return k < n0 ? cloud_0 + (size_t)min(max(i0[k], (int64_t)0), (int64_t)P0 - 1) * ld
                      : cloud_1 + (size_t)min(max(i1[k - n0], (int64_t)0), (int64_t)P1 - 1) * ld;
    };
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int k = tid; k < n; k += 1024) {
        const float* r = row(k);
        sx += r[0]; sy += r[1]; sz += r[2];
    }
    const float mx = block_sum(sx, red) / (float)n, my = block_sum(sy, red) / (float)n, mz = block_sum(sz, red) / (float)n;
    float far2 = 0.f;
    for (int k = tid; k < n; k += 1024) {
        const float* r = row(k);
        const float x = r[0] - mx, y = r[1] - my, z = r[2] - mz;
        far2 = fmaxf(far2, sqrtf((x * x + y * y) + z * z));
    }
    const float far = block_max(far2, red);
    float* w0 = o0 + (size_t)b * M * ld;
    float* w1 = o1 + (size_t)b * N * ld;
    for (int k = tid; k < n; k += 1024) {
        const float* r = row(k);
        float* w = k < n0 ? w0 + (size_t)k * ld : w1 + (size_t)(k - n0) * ld;
        w[0] = (r[0] - mx) / far; w[1] = (r[1] - my) / far; w[2] = (r[2] - mz) / far;
        for (int col = 3; col < ld; ++col) w[col] = r[col];
    }
    for (int e = n0 * ld + tid; e < M * ld; e += 1024) w0[e] = 0.0f;
    if (TARGET_COUNTS)
        for (int e = n1 * ld + tid; e < N * ld; e += 1024) w1[e] = 0.0f;
    if (tid == 0) { inverse[4 * b] = far; inverse[4 * b + 1] = mx; inverse[4 * b + 2] = my; inverse[4 * b + 3] = mz; }
}

__global__ __launch_bounds__(1024) void stage_pairs_counts_kernel(const float* __restrict__ cloud_0, int P0, const float* __restrict__ cloud_1, int P1, int ld,
                                                                  const int64_t* __restrict__ index_0, const int64_t* __restrict__ index_1,
                                                                  const int32_t* __restrict__ counts_0, int M, int N, float* __restrict__ o0,
                                                                  float* __restrict__ o1, float* __restrict__ inverse) {
    __shared__ float red[16];
    stage_pair_body<false>(cloud_0, P0, cloud_1, P1, ld, index_0, index_1, counts_0, nullptr, M, N, o0, o1, inverse, red);
}

// A count on both sides: pair k = (cloud_0[index_0[k, :c_k]], cloud_1[index_1[k, :n_k]]), counts_0 null = every c_k is M.
__global__ __launch_bounds__(1024) void stage_pairs_counts2_kernel(const float* __restrict__ cloud_0, int P0, const float* __restrict__ cloud_1, int P1, int ld,
                                                                   const int64_t* __restrict__ index_0, const int64_t* __restrict__ index_1,
                                                                   const int32_t* __restrict__ counts_0, const int32_t* __restrict__ counts_1, int M, int N,
                                                                   float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ inverse) {
    __shared__ float red[16];
    stage_pair_body<true>(cloud_0, P0, cloud_1, P1, ld, index_0, index_1, counts_0, counts_1, M, N, o0, o1, inverse, red);
}

// counts_1 null: stage_pairs_counts_kernel (counts_0 required, N >= 0); otherwise stage_pairs_counts2_kernel (counts_0 may be null, N >= 1).
void launch_stage_pairs_counts(const float* cloud_0, long P0, const float* cloud_1, long P1, int ld, const int64_t* index_0, const int64_t* index_1,
                               const int32_t* counts_0, const int32_t* counts_1, int n_pairs, int M, int N, float* out_0, float* out_1, float* inverse,
                               hipStream_t s) {
    if (n_pairs <= 0) return;
    if (!cloud_0 || !cloud_1 || !index_0 || !index_1 || (!counts_0 && !counts_1) || !out_0 || !out_1 || !inverse) throw Error(FC_ERR_INVALID, "stage pairs: null pointer");
    if (ld < 3 || ld > 8) throw Error(FC_ERR_UNSUPPORTED, "stage pairs: 3..8 columns supported (xyz first)");
    if (P0 < 1 || P0 > 0x7fffffffL || P1 < 1 || P1 > 0x7fffffffL) throw Error(FC_ERR_INVALID, "stage pairs: bad cloud size");
    if (M < 1 || N < (counts_1 ? 1 : 0) || (long)M * ld > 0x7fffffffL || (long)N * ld > 0x7fffffffL || (long)M + N > 0x7fffffffL)
        throw Error(FC_ERR_INVALID, "stage pairs: bad sample counts");
    const double bytes = 4.0 * n_pairs * ((double)(M + N) * (2.0 * ld + 2.0));
    if (!counts_1)
        launch_kernel<stage_pairs_counts_kernel>("fc::stage_pairs_counts_kernel", 0.0, bytes, dim3(n_pairs), dim3(1024), 0, s,
                                                 cloud_0, (int)P0, cloud_1, (int)P1, ld, index_0, index_1, counts_0, M, N, out_0, out_1, inverse);
    else
        launch_kernel<stage_pairs_counts2_kernel>("fc::stage_pairs_counts2_kernel", 0.0, bytes, dim3(n_pairs), dim3(1024), 0, s,
                                                  cloud_0, (int)P0, cloud_1, (int)P1, ld, index_0, index_1, counts_0, counts_1, M, N, out_0, out_1, inverse);
}

// ---------------------------------------------------------------- dense blocks: ALL members of the staged voxels
// Block b of the i-th listed voxel holds its members b * block ... min((b + 1) * block, count) - 1 in the list's ascending order, xyz as
// (x - mean) / furthest_distance with co_unit_sphere_kernel's operations (staging.hip), the other columns as they are.  A slot of a
// voxel's last block beyond its count repeats the voxel's FIRST member (a real point: nothing downstream sees garbage) with index -1.
// One workgroup per block; the number of blocks is block_offsets[n_voxels] on the device, so a launch of fixed width strides over the
// blocks and the host needs neither that number nor a synchronisation.  Member rows ascend, so a block's gather walks forward through the
// cloud; consecutive threads take consecutive floats of `out`.  Nothing is accumulated: the same input gives the same bytes.
constexpr int kDenseThreads = 256, kDenseGrid = 4096;

__global__ __launch_bounds__(kDenseThreads) void dense_blocks_kernel(const float* __restrict__ cloud, int ld, int C, int P, const int64_t* __restrict__ offsets,
                                                                     const int32_t* __restrict__ rows, const int32_t* __restrict__ voxel_ids, int n_voxels,
                                                                     const float* __restrict__ inverse, const int64_t* __restrict__ block_offsets, int block,
                                                                     float* __restrict__ out, int64_t* __restrict__ index, int32_t* __restrict__ block_voxel) {
    const int64_t n_blocks = block_offsets[n_voxels];
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        int lo = 0, hi = n_voxels;                            // the last i with block_offsets[i] <= b: voxels without blocks are stepped over
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (block_offsets[mid] <= b) lo = mid; else hi = mid;
        }
        const int i = lo;
        const int v = voxel_ids ? voxel_ids[i] : i;
        const int64_t off = offsets[v], count = offsets[v + 1] - off;
        const int64_t first = (b - block_offsets[i]) * block;
        if (count < 1 || first >= count) continue;            // block_offsets that do not belong to this list; uniform over the workgroup
        const float far = inverse[4 * (size_t)i], mx = inverse[4 * (size_t)i + 1], my = inverse[4 * (size_t)i + 2], mz = inverse[4 * (size_t)i + 3];
        const int32_t* vr = rows + off;
        float* ob = out + (size_t)b * block * C;
        for (int e = threadIdx.x; e < block * C; e += kDenseThreads) {
            const int slot = e / C, col = e - slot * C;
            const bool member = first + slot < count;
            const int r = min(max(vr[member ? first + slot : 0], 0), P - 1);       // clamped: a bad list cannot read outside the cloud
            const float x = cloud[(size_t)r * ld + col];
            ob[e] = col == 0 ? (x - mx) / far : col == 1 ? (x - my) / far : col == 2 ? (x - mz) / far : x;
            if (col == 0) index[(size_t)b * block + slot] = member ? (int64_t)r : (int64_t)-1;
        }
        if (threadIdx.x == 0) block_voxel[b] = i;
    }
}

void launch_dense_blocks(const float* cloud, int ld, int C, long P, const int64_t* offsets, const int32_t* rows, const int32_t* voxel_ids, int n_voxels,
                         const float* inverse, const int64_t* block_offsets, int block, float* out, int64_t* index, int32_t* block_voxel, hipStream_t s) {
    if (n_voxels <= 0) return;
    if (!cloud || !offsets || !rows || !inverse || !block_offsets || !out || !index || !block_voxel) throw Error(FC_ERR_INVALID, "dense blocks: null pointer");
    if (C < 3 || C > 8 || ld < C) throw Error(FC_ERR_UNSUPPORTED, "dense blocks: 3..8 columns supported (xyz first)");
    if (P < 1 || P > 0x7fffffffL) throw Error(FC_ERR_INVALID, "dense blocks: bad cloud size");
    if (block < 1 || (long)block * C > 0x7fffffffL) throw Error(FC_ERR_INVALID, "dense blocks: bad block size");
    // (no byte figure: the traffic depends on block_offsets, which the host does not read)
    launch_kernel<dense_blocks_kernel>("fc::dense_blocks_kernel", 0.0, 0.0, dim3(kDenseGrid), dim3(kDenseThreads), 0, s,
                                       cloud, ld, C, (int)P, offsets, rows, voxel_ids, n_voxels, inverse, block_offsets, block, out, index, block_voxel);
}

}  // namespace fc

extern "C" {

size_t fc_stage_voxel_ws_bytes(int64_t P, int32_t K) { return fc::voxel_ws_bytes((long)P, K); }

int fc_stage_voxel_count_f32(const float* cloud, int32_t ld, int64_t P, const float* centers, int32_t K, float dx, float dy, float dz, int32_t* counts,
                             void* ws, size_t ws_bytes, void* stream) {
    FC_API_BEGIN
    fc::launch_voxel_count(cloud, ld, (long)P, centers, K, dx, dy, dz, counts, ws, ws_bytes, (hipStream_t)stream);
    FC_API_END
}

int fc_stage_voxel_select_f32(const float* cloud, int32_t ld, int64_t P, const float* centers, int32_t K, float dx, float dy, float dz,
                              const int64_t* offsets, int32_t* rows, int64_t rows_capacity, const void* ws, size_t ws_bytes, void* stream) {
    FC_API_BEGIN
    fc::launch_voxel_select(cloud, ld, (long)P, centers, K, dx, dy, dz, offsets, rows, rows_capacity, ws, ws_bytes, (hipStream_t)stream);
    FC_API_END
}

int fc_stage_fps_ragged_f32(const float* cloud, int32_t ld, int32_t C, int64_t P, const int64_t* offsets, const int32_t* rows, const int32_t* voxel_ids,
                            int32_t n_voxels, int32_t max_rows, int32_t m, int64_t* idx, float* dist_scratch, void* stream) {
    FC_API_BEGIN
    if (n_voxels < 0 || m < 1) throw fc::Error(FC_ERR_INVALID, "fc_stage_fps_ragged_f32: bad argument");
    fc::launch_fps_ragged(cloud, ld, C, (long)P, offsets, rows, voxel_ids, n_voxels, max_rows, m, idx, nullptr, dist_scratch, (hipStream_t)stream);
    FC_API_END
}

/* include/fcflow_sparse_stage.h */
int fc_stage_fps_ragged_counts_f32(const float* cloud, int32_t ld, int32_t C, int64_t P, const int64_t* offsets, const int32_t* rows,
                                   const int32_t* voxel_ids, int32_t n_voxels, int32_t max_rows, int32_t m, int64_t* idx, int32_t* sample_counts,
                                   float* dist_scratch, void* stream) {
    FC_API_BEGIN
    if (n_voxels < 0 || m < 1 || !sample_counts) throw fc::Error(FC_ERR_INVALID, "fc_stage_fps_ragged_counts_f32: bad argument");
    fc::launch_fps_ragged(cloud, ld, C, (long)P, offsets, rows, voxel_ids, n_voxels, max_rows, m, idx, sample_counts, dist_scratch, (hipStream_t)stream);
    FC_API_END
}

int fc_stage_pairs_counts_f32(const float* cloud_0, int64_t P0, const float* cloud_1, int64_t P1, int32_t ld, const int64_t* index_0,
                              const int64_t* index_1, const int32_t* counts_0, int32_t n_pairs, int32_t M, int32_t N, float* out_0, float* out_1,
                              float* inverse, void* stream) {
    FC_API_BEGIN
    if (n_pairs < 0) throw fc::Error(FC_ERR_INVALID, "fc_stage_pairs_counts_f32: bad argument");
    if (n_pairs > 0 && !counts_0) throw fc::Error(FC_ERR_INVALID, "stage pairs: null pointer");
    fc::launch_stage_pairs_counts(cloud_0, (long)P0, cloud_1, (long)P1, ld, index_0, index_1, counts_0, nullptr, n_pairs, M, N, out_0, out_1, inverse,
                                  (hipStream_t)stream);
    FC_API_END
}

/* include/fcflow_sparse_target.h */
int fc_stage_pairs_counts2_f32(const float* cloud_0, int64_t P0, const float* cloud_1, int64_t P1, int32_t ld, const int64_t* index_0,
                               const int64_t* index_1, const int32_t* counts_0, const int32_t* counts_1, int32_t n_pairs, int32_t M, int32_t N,
                               float* out_0, float* out_1, float* inverse, void* stream) {
    FC_API_BEGIN
    if (n_pairs < 0) throw fc::Error(FC_ERR_INVALID, "fc_stage_pairs_counts2_f32: bad argument");
    if (n_pairs > 0 && !counts_1) throw fc::Error(FC_ERR_INVALID, "stage pairs: null pointer");
    fc::launch_stage_pairs_counts(cloud_0, (long)P0, cloud_1, (long)P1, ld, index_0, index_1, counts_0, counts_1, n_pairs, M, N, out_0, out_1, inverse,
                                  (hipStream_t)stream);
    FC_API_END
}

int fc_stage_dense_blocks_f32(const float* cloud, int32_t ld, int32_t C, int64_t P, const int64_t* offsets, const int32_t* rows, const int32_t* voxel_ids,
                              int32_t n_voxels, const float* inverse, const int64_t* block_offsets, int32_t block, float* out, int64_t* index,
                              int32_t* block_voxel, void* stream) {
    FC_API_BEGIN
    if (n_voxels < 0) throw fc::Error(FC_ERR_INVALID, "fc_stage_dense_blocks_f32: bad argument");
    fc::launch_dense_blocks(cloud, ld, C, (long)P, offsets, rows, voxel_ids, n_voxels, inverse, block_offsets, block, out, index, block_voxel,
                            (hipStream_t)stream);
    FC_API_END
}

}  // extern "C"
