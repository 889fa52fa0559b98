// The statements of knn_mfma_kernel<CP> and knn_mfma_counts_kernel<CP> (knn.hip), included inside both: no include guard, no declarations of
// its own (why an include: knn_lane_body.h).  Expects f, ldf, C, idx_out, m_stride, k, warm and the template parameter CP as the kernels
// take them, M = the scene's points and m_rows = the rows per scene of idx_out and warm.
    extern __shared__ float smem[];
    constexpr int LDC = CP + 4, H = CP / 2, NLD = (KM_TC * CP / 4 + 255) / 256;
    float* s_qxx = smem + 2 * KM_TC * LDC;                        // [4 waves][32]
    float* s_tau = s_qxx + 128;                                   // [4 waves][32]: warm-start thresholds
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int b = blockIdx.y, q0 = blockIdx.x * 128 + wave * 32;
    const float* fb = f + (size_t)b * m_stride * ldf;

    // ---- this wave's 32 queries as the A operand: lane (i, kh) holds features kh * H + 0 .. H - 1 of query i
    float aq[H];
    {
        int qi = q0 + li;
        qi = qi < M ? qi : M - 1;
        const float* src = fb + (size_t)qi * ldf + lh * H;
        float nrm = 0.f;
#pragma unroll
        for (int u = 0; u < H; u += 4) {
            float4 v = *reinterpret_cast<const float4*>(src + u);
            if (CP != C) {                                        // columns C .. CP - 1 are padding, whatever the memory holds
                const int c0 = lh * H + u;
                v.x = c0 < C ? v.x : 0.f; v.y = c0 + 1 < C ? v.y : 0.f; v.z = c0 + 2 < C ? v.z : 0.f; v.w = c0 + 3 < C ? v.w : 0.f;
            }
            aq[u] = v.x; aq[u + 1] = v.y; aq[u + 2] = v.z; aq[u + 3] = v.w;
            nrm = fmaf(v.x, v.x, nrm); nrm = fmaf(v.y, v.y, nrm); nrm = fmaf(v.z, v.z, nrm); nrm = fmaf(v.w, v.w, nrm);
        }
        nrm += __shfl_xor(nrm, 32);
        if (lh == 0) s_qxx[wave * 32 + li] = nrm;
        // ---- warm start (round 4): `warm` holds k neighbours of every query from the PREVIOUS DGCNN level (models/pytorch_gcn.py:43-60: the four
        // edge convolutions search the same cloud in successive feature spaces).  Any k distinct candidates bound the k-th best from below, so
        // the stream starts with tau0 = min_j pd(query, warm_j) instead of -inf and the ~k ln(M / k) insertions that only serve to raise the
        // threshold never happen (the previous level's neighbours are mostly near in this level's space too).  The selection stays EXACT:
        // tau0 is lowered by a bound on the rounding difference between this scalar fmaf chain and the MFMA's sums, every candidate above it
        // goes through the same sorted insertion in the same order, and tau only ever rises.  A set that holds an index twice (e.g. through the
        // "open slots get the query itself" rule below), an index outside the cloud or a non-finite value gives no bound: tau0 = -inf, the
        // plain stream.  Distinctness is checked for real (a wave looks at its 32 sets one after the other, entry j on lane j, against the
        // entries 1 .. k / 2 places further round the set: every unordered pair once).
        float tau0 = -INFINITY;
        if (warm) {
            unsigned dup_mask = 0;                                     // bit q: the set of this wave's query q repeats an index
            for (int q = 0; q < 32; ++q) {
                int qq = q0 + q;
                qq = qq < M ? qq : M - 1;
                const int mine = lane < k ? warm[((size_t)b * m_rows + qq) * k + lane] : -1 - lane;
                bool dup = false;
                for (int d = 1; d <= k / 2; ++d) {
                    int o = lane + d;
                    o = o >= k ? o - k : o;
                    dup |= lane < k && __shfl(mine, o, 64) == mine;
                }
                dup_mask |= __ballot(dup) ? (1u << q) : 0u;
            }
            const int32_t* wl = warm + ((size_t)b * m_rows + qi) * k;
            float tmin = INFINITY, cmax = 0.f;
            bool bad = ((dup_mask >> li) & 1u) != 0;
            for (int j = 0; j < k; ++j) {
                int ci = wl[j];
                bad |= ci < 0 || ci >= M;
                ci = ci < 0 ? 0 : (ci >= M ? M - 1 : ci);
                const float* row = fb + (size_t)ci * ldf + lh * H;
                float dot = 0.f, cx = 0.f;
#pragma unroll
                for (int u = 0; u < H; u += 4) {
                    float4 v = *reinterpret_cast<const float4*>(row + u);
                    if (CP != C) {
                        const int c0 = lh * H + u;
                        v.x = c0 < C ? v.x : 0.f; v.y = c0 + 1 < C ? v.y : 0.f; v.z = c0 + 2 < C ? v.z : 0.f; v.w = c0 + 3 < C ? v.w : 0.f;
                    }
                    dot = fmaf(aq[u], v.x, dot); dot = fmaf(aq[u + 1], v.y, dot); dot = fmaf(aq[u + 2], v.z, dot); dot = fmaf(aq[u + 3], v.w, dot);
                    cx = fmaf(v.x, v.x, cx); cx = fmaf(v.y, v.y, cx); cx = fmaf(v.z, v.z, cx); cx = fmaf(v.w, v.w, cx);
                }
                dot += __shfl_xor(dot, 32);
                cx += __shfl_xor(cx, 32);
                const float pd = fmaf(2.0f, dot, -cx) - nrm;
                bad |= !(pd == pd);
                tmin = fminf(tmin, pd);
                cmax = fmaxf(cmax, cx);
            }
            // |2 x.y computed two ways| differs by at most ~2 C eps |x| |y| <= C eps (|x|^2 + |y|^2); 2^-21 = 4 eps covers the two subtractions as well
            const float margin = (float)CP * 4.76837158e-7f * (nrm + cmax + fabsf(tmin));
            tau0 = tmin - margin;
            // The bound above is a RELATIVE one: it holds while no product or partial sum leaves the normal range.  Where it does (norms
            // below ~2^-40: a term that rounds in the subnormal range is off by up to 2^-150, 2 CP + 2 of them by < 2^-141) or where the
            // margin is plain zero (query and warm neighbours all zero: every candidate ties at pd = 0 and `pd > tau0` would turn all of
            // them away), tau0 would not lie strictly below the k-th best as the stream computes it.  A margin of at least 2^-100 is normal
            // itself and covers 2^-141 many times over; anything smaller gives no bound: tau0 = -inf, the plain stream.
            if (bad || !(margin >= 7.88860905e-31f) || !(tau0 < tmin)) tau0 = -INFINITY;
        }
        if (lh == 0) s_tau[wave * 32 + li] = tau0;
    }
    // ---- block loader: thread e covers float4 e of the 64 x CP block (register-staged, written to the other buffer after the block's products)
    // in two parts (one per 32-candidate tile of the block in flight), so that only half of a block's float4s are live at a time
    constexpr int NPART = NLD >= 2 ? 2 : 1, NPP = NLD / NPART;
    float4 stg[NPP];
    auto gload = [&](int blk, int part) {
#pragma unroll
        for (int i = 0; i < NPP; ++i) {
            const int e = tid + 256 * (part * NPP + i);
            if (NLD * 256 == KM_TC * CP / 4 || e < KM_TC * CP / 4) {
                const int r = e / (CP / 4), c4 = (e - r * (CP / 4)) * 4;
                int ci = blk * KM_TC + r;
                ci = ci < M ? ci : M - 1;
                float4 v = *reinterpret_cast<const float4*>(fb + (size_t)ci * ldf + c4);
                if (CP != C) { v.x = c4 < C ? v.x : 0.f; v.y = c4 + 1 < C ? v.y : 0.f; v.z = c4 + 2 < C ? v.z : 0.f; v.w = c4 + 3 < C ? v.w : 0.f; }
                stg[i] = v;
            }
        }
    };
    auto lstore = [&](float* dst, int part) {
#pragma unroll
        for (int i = 0; i < NPP; ++i) {
            const int e = tid + 256 * (part * NPP + i);
            if (NLD * 256 == KM_TC * CP / 4 || e < KM_TC * CP / 4) {
                const int r = e / (CP / 4), c4 = (e - r * (CP / 4)) * 4;
                *reinterpret_cast<float4*>(dst + r * LDC + c4) = stg[i];
            }
        }
    };
    float qxx[16], tau[16];
    float setv[16][2];
    int seti[16][2];
#pragma unroll
    for (int part = 0; part < NPART; ++part) { gload(0, part); lstore(smem, part); }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        qxx[r] = s_qxx[wave * 32 + 8 * (r >> 2) + 4 * lh + (r & 3)];
        tau[r] = s_tau[wave * 32 + 8 * (r >> 2) + 4 * lh + (r & 3)];
        setv[r][0] = setv[r][1] = -INFINITY;
        seti[r][0] = seti[r][1] = 0;
    }

    const int nblk = (M + KM_TC - 1) / KM_TC;
    for (int blk = 0; blk < nblk; ++blk) {
        const float* cur = smem + (blk & 1) * (KM_TC * LDC);
        float* nxt = smem + ((blk + 1) & 1) * (KM_TC * LDC);
        const bool more = blk + 1 < nblk;
#pragma unroll 1
        for (int t = 0; t < KM_TC / 32; ++t) {
            const int cbase = blk * KM_TC + t * 32;
            if (more && t < NPART) gload(blk + 1, t);            // (the next block is complete: cbase < M for both of this block's tiles)
            if (cbase >= M) break;
            const float* brow = cur + (t * 32 + li) * LDC + lh * H;
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            float cxx = 0.f;
#pragma unroll
            for (int u = 0; u < H; u += 4) {
                const float4 bv = *reinterpret_cast<const float4*>(brow + u);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[u], bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[u + 1], bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[u + 2], bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[u + 3], bv.w, acc, 0, 0, 0);
                cxx = fmaf(bv.x, bv.x, cxx); cxx = fmaf(bv.y, bv.y, cxx); cxx = fmaf(bv.z, bv.z, cxx); cxx = fmaf(bv.w, bv.w, cxx);
            }
            cxx += __shfl_xor(cxx, 32);
            if (cbase + li >= M) cxx = INFINITY;                  // candidates past the end: pd = -inf, never a hit
            // tau is refreshed once per register, behind its hits: a value below the true k-th best lands behind lane k - 1, where it is
            // ignored.  (Measured: inserting the hits of four lists side by side -- two registers x two half-waves, dummies of -inf for lists
            // without a pending hit -- is no faster, 5.4 vs 5.2 ms per C2 forward: the second wave of the SIMD already fills the gaps of
            // one insertion's dependent chain, so the dummy work costs what the interleaving gains.)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pd = fmaf(2.0f, acc[r], -cxx) - qxx[r];
                unsigned long long mask = __ballot(pd > tau[r]);
                if (mask) {                                       // (wave-uniform)
                    do {
                        const int bpos = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pd), bpos));
                        const int ci = cbase + (bpos & 31);
                        if (bpos < 32) knn_insert(setv[r][0], seti[r][0], v, ci);
                        else knn_insert(setv[r][1], seti[r][1], v, ci);
                    } while (mask);
                    const float t0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, setv[r][0]), k - 1));
                    const float t1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, setv[r][1]), k - 1));
                    tau[r] = fmaxf(tau[r], lh ? t1 : t0);        // (never below the warm-start threshold; without one the list's k-th entry only rises anyway)
                }
            }
            if (more && t < NPART) lstore(nxt, t);
        }
        __syncthreads();
    }
    // ---- entry e of query (r, half) sits on lane e.  Fewer than k finite candidates (NaN / -inf features in a pass whose range flag is
    // already up): the open slots get the query itself, never an uninitialised index (the gathers downstream trust them)
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int qi = q0 + 8 * (r >> 2) + 4 * h + (r & 3);
            if (qi < M && lane < k) idx_out[((size_t)b * m_rows + qi) * k + lane] = setv[r][h] > -INFINITY ? seti[r][h] : qi;
        }
