// Training Linear, host side: the layout of its per-step weight pack and what train_linear.hip and train_wgrad.hip both need of it.
#pragma once
#include <algorithm>

#include "common.h"

namespace fc {

struct TrainLinearLayout {
    int N, N_pad, n_alloc;                 // output features: true, padded to 32, rows of the packed W (column-tile grid)
    int nseg, seg[3], seg_pad[3];          // input panels: true and padded widths
    int K, K_pad, k_alloc;                 // sums; rows of the packed W^T
    size_t off_W, off_W2, off_bias, off_WT, off_WT2, bytes;
    // wide layers (one input panel, at least 1024 outputs, K and N multiples of 64: the spline parameter layer): one-accumulator images of
    // W and W^T for the 256 x 256 loop of spline_wide.hip (EPI 3) and the bias pre-scaled for it
    int wide, n256, k256;
    size_t off_W1, off_bias1, off_WT1;
};

inline TrainLinearLayout train_layout(int N, const int32_t* seg, int nseg) {
    if (N < 1 || nseg < 1 || nseg > 3 || !seg) throw Error(FC_ERR_INVALID, "training Linear: need N >= 1 and 1..3 input segments");
    TrainLinearLayout L{};
    L.N = N; L.N_pad = round_up(N, 32); L.n_alloc = gemm_n_alloc(L.N_pad);
    L.nseg = nseg;
    for (int i = 0; i < nseg; ++i) {
        if (seg[i] < 1) throw Error(FC_ERR_INVALID, "training Linear: empty input segment");
        L.seg[i] = seg[i]; L.seg_pad[i] = round_up(seg[i], 32);
        L.K += seg[i]; L.K_pad += L.seg_pad[i];
    }
    L.k_alloc = gemm_n_alloc(L.K_pad);
    size_t o = 0;
    auto take = [&](size_t b) { const size_t r = o; o = round_up_sz(o + b, 256); return r; };
    L.off_W = take((size_t)L.n_alloc * L.K_pad * 4);
    L.off_W2 = take((size_t)L.n_alloc * L.K_pad * 4);          // [n_alloc][K_pad/16][hi 16 | lo' 16] halfs
    L.off_bias = take((size_t)L.n_alloc * 4);
    L.off_WT = take((size_t)L.k_alloc * L.N_pad * 4);
    L.off_WT2 = take((size_t)L.k_alloc * L.N_pad * 4);
    L.wide = nseg == 1 && L.N_pad >= 1024 && L.N_pad % 64 == 0 && L.K_pad % 64 == 0;
    L.n256 = round_up(L.N_pad, 256); L.k256 = round_up(L.K_pad, 256);
    if (L.wide) {
        L.off_W1 = take((size_t)L.n256 * L.K_pad * 4);             // [n256][K_pad/16][hi 16 | lo 16] halfs of w 2^kTrainWideWExp
        L.off_bias1 = take((size_t)L.n256 * 4);
        L.off_WT1 = take((size_t)L.k256 * L.N_pad * 4);            // [k256][N_pad/16][hi 16 | lo 16]
    }
    L.bytes = o;
    return L;
}

// what launch_gemm reads of a pack: W with its bias and the input segments (forward), or W^T as one segment of N_pad columns without a
// bias (data gradient); f16: with the fp16 limb image (split-fp16 loop), else the fp32-input loop
inline PackedLinear packed_view(const TrainLinearLayout& L, const void* pack, bool transposed, bool f16) {
    const char* b = (const char*)pack;
    PackedLinear P;
    P.W = (float*)(b + (transposed ? L.off_WT : L.off_W));
    P.W2 = f16 ? (unsigned short*)(b + (transposed ? L.off_WT2 : L.off_W2)) : nullptr;
    if (transposed) {
        P.N_pad = L.K_pad; P.K_pad = L.N_pad; P.nseg = 1; P.seg_k[0] = L.N_pad;
        P.n_true = L.K; P.k_true = L.N; P.n_alloc = L.k_alloc;
    } else {
        P.bias = (float*)(b + L.off_bias);
        P.N_pad = L.N_pad; P.K_pad = L.K_pad; P.nseg = L.nseg;
        for (int i = 0; i < L.nseg; ++i) P.seg_k[i] = L.seg_pad[i];
        P.n_true = L.N; P.k_true = L.K; P.n_alloc = L.n_alloc;
    }
    return P;
}

inline void check_panel(const void* p, int ld, int width_pad, const char* what) {
    if (!p || ld < width_pad || ld % 4 != 0 || ((uintptr_t)p & 15)) throw Error(FC_ERR_INVALID, std::string("training Linear: bad panel for ") + what);
}

// grid of the element-wise kernels (grid-stride loops over n items)
inline int grid_for(size_t n, int block) { return (int)std::min<size_t>((n + block - 1) / block, 256 * 16); }

}  // namespace fc
