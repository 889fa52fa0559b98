// The narrow ExponentialCoupling arithmetic (d2 <= 16, one thread per point with per-thread arrays), stated once for the inference kernel
// (misc.hip) and the training forward / backward (train_expm.hip); expm_wide.hip handles larger d2 with an algorithm of its own.
// models/exponential_coupling.py:44-75, utils.py:294-327: W = rescale tanh(scale raw + shift) + reshift + 1e-8 (d2 x d2), y2 = expm(W) x2 + b,
// ldj = tr W.  expm acts on the vector directly: A = W 2^-s with |A|_inf <= 1/2, the 12-term Taylor ACTION u = sum_k A^k v / k! applied 2^s times.
// The caller picks s from the norm returned here under its own cap (24 in inference; 6 in training, where every state is stored).
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

constexpr int EX_D = 16;      // largest d2 of these kernels: the row stride of W and the length of the per-thread vectors

// w [d2][LD] = W (negated for the inverse; tr is the trace of W itself either way); returns the unhalved row-sum norm |w|_inf
template <int LD>
__device__ __forceinline__ float expm_narrow_matrix(const float* pr, int d2, const float* scal4, bool negate, float* w, float& tr) {
    const float sc = scal4[0], sh = scal4[1], rs = scal4[2], rsh = scal4[3];
    float nrm = 0.f;
    tr = 0.f;
    for (int i = 0; i < d2; ++i) {
        float rsum = 0.f;
        for (int j = 0; j < d2; ++j) {
            float wij = rs * tanhf(sc * pr[i * d2 + j] + sh) + rsh + 1e-8f;
            if (i == j) tr += wij;
            if (negate) wij = -wij;
            w[i * LD + j] = wij;
            rsum += fabsf(wij);
        }
        nrm = fmaxf(nrm, rsum);
    }
    return nrm;
}

// out = sum_{k=0..12} t_k with t_0 = in, t_k = (f / k) w t_{k-1}; out may be in, or null when only the terms are wanted.
// KEEP_TERMS: T[k] = t_k for k = 0 .. 12 (the backward's reverse sweep reads them).
template <int LD, bool KEEP_TERMS>
__device__ __forceinline__ void expm_narrow_action(const float* w, int d2, float f, const float* in, float* out, float (*T)[LD] = nullptr) {
    float acc[LD], two[2][LD];            // the terms live in T when they are kept, else in two alternating vectors
    for (int i = 0; i < d2; ++i) {
        acc[i] = in[i];
        if constexpr (KEEP_TERMS) T[0][i] = in[i];
    }
    const float* term = in;
    for (int k = 1; k <= 12; ++k) {
        float* nt;
        if constexpr (KEEP_TERMS) nt = T[k]; else nt = two[k & 1];
        const float fk = f / (float)k;
        for (int i = 0; i < d2; ++i) {
            float a = 0.f;
            for (int j = 0; j < d2; ++j) a = fmaf(w[i * LD + j], term[j], a);
            nt[i] = a * fk;
        }
        if (out)
            for (int i = 0; i < d2; ++i) acc[i] += nt[i];
        term = nt;
    }
    if (out)
        for (int i = 0; i < d2; ++i) out[i] = acc[i];
}

}  // namespace fc
