// cov4_evd_kernel.inc.h -- the text of cov4_evd_kernel (music_kernels.hip.h, section 2a), included there TWICE: BAZ_EVD_ORDER 0
// defines cov4_evd_kernel as it has always been, BAZ_EVD_ORDER 1 its twin cov4_evd_order_kernel with the per-item emitter
// count (OrderArgs; baz_music_set_order_mode).  See evd_lds_kernel.inc.h for why the text is shared this way.
#if BAZ_EVD_ORDER
__global__ __launch_bounds__(256) void cov4_evd_order_kernel(const float* __restrict__ in, double* __restrict__ Qs,
                                                             double* __restrict__ Gs, double2* __restrict__ Rdbg,
                                                             uint32_t batch, uint32_t K, uint32_t n, uint32_t qstride,
                                                             uint32_t task_items, const OrderArgs oa)
{
#else
__global__ __launch_bounds__(256) void cov4_evd_kernel(const float* __restrict__ in, double* __restrict__ Qs,
                                                       double* __restrict__ Gs, double2* __restrict__ Rdbg,
                                                       uint32_t batch, uint32_t K, uint32_t n, uint32_t qstride,
                                                       uint32_t task_items = 64)
{
#endif
    // task_items (64, 32 or 16; round 5): items per wave task.  64 fills the lane-per-item EVD; a SMALL batch -- a host-fed work() call of
    // 1,024 items is 16 tasks of 64 = 16 waves with 8 KiB in flight each, too little to keep a PCIe link (or HBM) busy -- is cut into more,
    // shorter tasks (the EVD then runs on fewer lanes: its latency is what it was).  Items are independent: no result depends on it.
    constexpr int RSD = 34;                       // see cov4_x4_kernel
    constexpr int RING = 8;                       // chunk loads in flight per wave (8 KiB)
    __shared__ double stage[4][2][8 * RSD];       // per wave, double-buffered
    __shared__ double gram[4][2][64];             // per wave: D1, D2
    __shared__ double rtab[4][16][64];            // per wave: R of 64 items, [slot][item]: 4 diagonals, 6 x (re, im)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t chunks = K >> 5;               // 1-KiB chunks per item (multiple of 8)
    const int wcol = lane >> 1, wrow = 4 * (lane & 1);
    const int ri = lane & 3, rh = (lane >> 2) & 1, rw = (lane >> 3) & 1, rk = lane >> 4;
    const int p_off = (4 * rh + ri) * RSD + 8 * rk + 4 * rw;
    const int q_off = (4 * (1 - rh) + ri) * RSD + 8 * rk + 4 * rw;
    double* const g1 = gram[wave][0];
    double* const g2 = gram[wave][1];
    double(*const rt)[64] = rtab[wave];
    const double dK = (double)K;
    const uint32_t ntasks = (batch + task_items - 1) / task_items;
    const uint32_t tstride = gridDim.x * 4;
    // slot of the upper-triangle entry this lane (< 16: a = lane>>2, b = lane&3) produces: diagonal a -> a;
    // pair (a < b) -> 4 + 2p (re), 5 + 2p (im), p = index of (a, b) in (0,1)(0,2)(0,3)(1,2)(1,3)(2,3)
    const int ea = (lane >> 2) & 3, eb = lane & 3;
    const int pidx = (ea == 0) ? eb - 1 : (ea == 1 ? eb + 1 : 5);

    for (uint32_t task = blockIdx.x * 4 + wave; task < ntasks; task += tstride) {
        __builtin_amdgcn_s_setprio(3);
        const uint32_t item0 = task * task_items;
        const uint32_t nit = (batch - item0 < task_items) ? batch - item0 : task_items;
        // the stream of this task: nit items x chunks, contiguous in HBM; ring slot u holds the chunks q = u (mod 8)
        const v4f32* __restrict__ src = reinterpret_cast<const v4f32*>(in + (size_t)item0 * K * 8) + lane;
        const uint32_t total = nit * chunks;                 // multiple of 8
        v4f32 pf[RING];
#pragma unroll
        for (int u = 0; u < RING; ++u) pf[u] = __builtin_nontemporal_load(src + (size_t)u * 64);
        uint32_t q = 0;                                      // chunk index inside the task
        for (uint32_t it = 0; it < nit; ++it) {
            double a1 = 0.0, b1 = 0.0, a2 = 0.0, b2 = 0.0;
            for (uint32_t cg = 0; cg < chunks; cg += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    double* __restrict__ T = stage[wave][u & 1];
#pragma unroll
                    for (int j = 0; j < 4; ++j) T[(wrow + j) * RSD + wcol] = (double)pf[u][j];   // exact widening (.cc:77)
                    // re-arm the slot only after its values are consumed (see cov4_x4_kernel); past the end of the
                    // task the loads repeat its last chunk, so that they stay unconditional
                    asm volatile("" ::: "memory");
                    const uint32_t qn = q + u + RING;
                    pf[u] = __builtin_nontemporal_load(src + (size_t)(qn < total ? qn : total - 1) * 64);
                    wave_lds_fence();
                    const v4f64 P = *reinterpret_cast<const v4f64*>(T + p_off);
                    const v4f64 Q = *reinterpret_cast<const v4f64*>(T + q_off);
                    a1 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[0], P[0], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[0], Q[0], a2, 0, 0, 0);
                    b1 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[1], P[1], b1, 0, 0, 0);
                    b2 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[1], Q[1], b2, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[2], P[2], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[2], Q[2], a2, 0, 0, 0);
                    b1 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[3], P[3], b1, 0, 0, 0);
                    b2 = __builtin_amdgcn_mfma_f64_4x4x4f64(P[3], Q[3], b2, 0, 0, 0);
                    wave_lds_fence();
                }
                q += 8;
            }
            // Gram blocks -> R (see cov4_x4_kernel), upper triangle into the wave's table
            g1[lane] = a1 + b1;
            g2[lane] = a2 + b2;
            wave_lds_fence();
            if (lane < 16) {
                auto G = [&](int x, int y) -> double {
                    if ((x >> 2) == (y >> 2)) {
                        const int hh = x >> 2, o = (y & 3) + 4 * hh + 16 * (x & 3);
                        return g1[o] + g1[o + 8];
                    }
                    if (x > y) { const int t = x; x = y; y = t; }
                    const int o = (y - 4) + 16 * x;
                    return g2[o] + g2[o + 8];
                };
                const double re = (G(2 * ea, 2 * eb) + G(2 * ea + 1, 2 * eb + 1)) / dK;     // .cc:85
                const double im = (G(2 * ea + 1, 2 * eb) - G(2 * ea, 2 * eb + 1)) / dK;
                if (ea == eb) rt[ea][it] = re;
                else if (ea < eb) { rt[4 + 2 * pidx][it] = re; rt[5 + 2 * pidx][it] = im; }
                if (Rdbg) Rdbg[(size_t)(item0 + it) * 16 + lane] = make_double2(re, im);
            }
            wave_lds_fence();
        }
        // EVD of the task's items, one per lane (lanes beyond nit redo the last item and write nothing), at low priority
        __builtin_amdgcn_s_setprio(0);
        {
            const int li = ((uint32_t)lane < nit) ? lane : (int)nit - 1;
            auto getR = [&](int i, int j) -> double2 {
                if (i == j) return make_double2(rt[i][li], 0.0);
                const int lo = i < j ? i : j, hi2 = i < j ? j : i;
                const int p = (lo == 0) ? hi2 - 1 : (lo == 1 ? hi2 + 1 : 5);
                const double re = rt[4 + 2 * p][li], im = rt[5 + 2 * p][li];
                return make_double2(re, i < j ? im : -im);
            };
#if BAZ_EVD_ORDER
            evd_project_lane<4, decltype(getR), true>(getR, (uint32_t)lane < nit, item0 + lane, n, qstride, Qs, Gs, oa);
#else
            evd_project_lane<4>(getR, (uint32_t)lane < nit, item0 + lane, n, qstride, Qs, Gs);
#endif
        }
        wave_lds_fence();
    }
}
