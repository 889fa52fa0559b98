// The statements of knn_kernel and knn_counts_kernel (knn.hip), included inside both: no include guard, no declarations of its own.
// Expects f, ldf, Cp, idx_out, m_stride, k as the kernels take them, M = the scene's points and m_rows = the rows per scene of idx_out.
// Not a __forceinline__ function on purpose: with the statements moved into one, verbatim, hipcc gives the uniform kernel 112 VGPRs for the
// parent's 114 and another schedule (and moves instructions of the matrix-core kernels, knn_mfma_body.h); included, the uniform kernels
// compile to the instructions they had before the counted ones existed (device assembly of both commits compared).
    extern __shared__ float smem[];
    const int LDC = Cp + 4;
    float* s_cand = smem;                                   // [64][LDC]
    float* s_qry = s_cand + 64 * LDC;                       // [16][LDC]
    float* s_qxx = s_qry + 16 * LDC;                        // [16]
    float* s_vals = s_qxx + 16;                             // [16][CAP]
    int32_t* s_idx = reinterpret_cast<int32_t*>(s_vals + 16 * KNN_CAP);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, q_base = blockIdx.x * 16;
    const float* fb = f + (size_t)b * m_stride * ldf;
    const int f4r = Cp / 4;

    // ---- stage the 16 query rows, then |xq|^2 with the SAME fma order used for candidates
    for (int e = tid; e < 16 * f4r; e += 256) {
        const int r = e / f4r, c4 = (e - r * f4r) * 4;
        int qi = q_base + r;
        qi = qi < M ? qi : M - 1;
        *reinterpret_cast<float4*>(s_qry + r * LDC + c4) = *reinterpret_cast<const float4*>(fb + (size_t)qi * ldf + c4);
    }
    __syncthreads();
    if (tid < 16) {
        float xx = 0.f;
        for (int c = 0; c < Cp; ++c) { const float v = s_qry[tid * LDC + c]; xx = fmaf(v, v, xx); }
        s_qxx[tid] = xx;
    }
    float tau[KNN_Q];
    int cnt[KNN_Q];
#pragma unroll
    for (int qq = 0; qq < KNN_Q; ++qq) { tau[qq] = -INFINITY; cnt[qq] = 0; }
    __syncthreads();
    float qxx[KNN_Q];
#pragma unroll
    for (int qq = 0; qq < KNN_Q; ++qq) qxx[qq] = s_qxx[wave * KNN_Q + qq];

    const int ntiles = (M + 63) / 64;
    for (int t = 0; t < ntiles; ++t) {
        for (int e = tid; e < 64 * f4r; e += 256) {
            const int r = e / f4r, c4 = (e - r * f4r) * 4;
            int ci = t * 64 + r;
            ci = ci < M ? ci : M - 1;
            *reinterpret_cast<float4*>(s_cand + r * LDC + c4) = *reinterpret_cast<const float4*>(fb + (size_t)ci * ldf + c4);
        }
        __syncthreads();
        // ---- lane = candidate: dot with the wave's 4 queries + own squared norm
        float dot[KNN_Q] = {0.f, 0.f, 0.f, 0.f};
        float cxx = 0.f;
        const float* cr = s_cand + lane * LDC;
        const float* qr = s_qry + wave * KNN_Q * LDC;
        for (int c4 = 0; c4 < Cp; c4 += 4) {
            const float4 cv = *reinterpret_cast<const float4*>(cr + c4);
            cxx = fmaf(cv.x, cv.x, cxx); cxx = fmaf(cv.y, cv.y, cxx); cxx = fmaf(cv.z, cv.z, cxx); cxx = fmaf(cv.w, cv.w, cxx);
#pragma unroll
            for (int qq = 0; qq < KNN_Q; ++qq) {
                const float4 qv = *reinterpret_cast<const float4*>(qr + qq * LDC + c4);
                float d = dot[qq];
                d = fmaf(qv.x, cv.x, d); d = fmaf(qv.y, cv.y, d); d = fmaf(qv.z, cv.z, d); d = fmaf(qv.w, cv.w, d);
                dot[qq] = d;
            }
        }
        const int cand = t * 64 + lane;
        const bool cvalid = cand < M;
#pragma unroll
        for (int qq = 0; qq < KNN_Q; ++qq) {
            // pairwise_distance = -xx - inner - xx^T with inner = -2 x^T x   (pytorch_gcn.py:14-16)
            const float pd = (-cxx + 2.0f * dot[qq]) - qxx[qq];
            const bool hit = cvalid && pd > tau[qq];
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                float* vals = s_vals + (wave * KNN_Q + qq) * KNN_CAP;
                int32_t* idxs = s_idx + (wave * KNN_Q + qq) * KNN_CAP;
                if (hit) {
                    const int pos = cnt[qq] + popc64(mask & ((1ull << lane) - 1ull));
                    vals[pos] = pd;
                    idxs[pos] = cand;
                }
                cnt[qq] += popc64(mask);
                if (cnt[qq] > 64) {
                    tau[qq] = prune_set(vals, idxs, cnt[qq], k, lane);
                    cnt[qq] = k;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int qq = 0; qq < KNN_Q; ++qq) {
        float* vals = s_vals + (wave * KNN_Q + qq) * KNN_CAP;
        int32_t* idxs = s_idx + (wave * KNN_Q + qq) * KNN_CAP;
        if (cnt[qq] > k) { prune_set(vals, idxs, cnt[qq], k, lane); cnt[qq] = k; }
        const int qi = q_base + wave * KNN_Q + qq;
        // fewer than k finite candidates (NaN / -inf features, e.g. in a pass whose fp16 range flag is already up and whose results
        // will be discarded): the open slots get the query itself, never an uninitialised index (the gathers downstream trust them)
        if (qi < M && lane < k) idx_out[((size_t)b * m_rows + qi) * k + lane] = lane < cnt[qq] ? idxs[lane] : qi;
    }
