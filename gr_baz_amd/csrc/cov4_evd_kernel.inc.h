// cov4_evd_kernel.inc.h -- the text of cov4_evd_kernel (music_kernels.hip.h, section 2a), included there TWICE: BAZ_EVD_ORDER 0
// defines cov4_evd_kernel as it has always been, BAZ_EVD_ORDER 1 its twin cov4_evd_order_kernel with the per-item emitter
// count (OrderArgs; baz_music_set_order_mode).  See evd_lds_kernel.inc.h for why the text is shared this way.
#if BAZ_EVD_ORDER
__global__ __launch_bounds__(256) void cov4_evd_order_kernel(const float* __restrict__ in, double* __restrict__ Qs,
                                                             double* __restrict__ Gs, double2* __restrict__ Rdbg,
                                                             uint32_t batch, uint32_t K, uint32_t n, uint32_t qstride,
                                                             uint32_t task_items, uint32_t park, const OrderArgs oa)
{
#else
__global__ __launch_bounds__(256) void cov4_evd_kernel(const float* __restrict__ in, double* __restrict__ Qs,
                                                       double* __restrict__ Gs, double2* __restrict__ Rdbg,
                                                       uint32_t batch, uint32_t K, uint32_t n, uint32_t qstride,
                                                       uint32_t task_items, uint32_t park)
{
#endif
    // task_items (64, 32 or 16; round 5): items per wave task.  64 fills the lane-per-item EVD; a SMALL batch -- a host-fed work() call of
    // 1,024 items is 16 tasks of 64 = 16 waves with 8 KiB in flight each, too little to keep a PCIe link (or HBM) busy -- is cut into more,
    // shorter tasks (the EVD then runs on fewer lanes: its latency is what it was).  Items are independent: no result depends on it.
    //
    // park (<= COVEVD_PARK; deferred rotation, lab: BAZ_MUSIC_COVEVD_DEFER=1): how many streamed tasks a wave may HOLD -- each lane its
    // item's R, 16 doubles in registers -- while it goes straight on to its next task.  The rotation passes of the held tasks and of
    // the task still in rtab then run back to back where the wave's work ends (or where the held set is full), so a wave with T tasks
    // stops its read stream ceil(T / (park + 1)) times instead of T times.  0 = one rotation phase per task: what the product launches
    // (the deferred form gained nothing that clears a step's spread, music_kernels.hip.h 2a).  Only the globally last task can be
    // short, and it is always some wave's last task: a held task is therefore always full (task_items items).  Same function on the
    // same values: no result depends on park.
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
    // getR of evd_project_lane over 16 values in rtab's slot order
    auto slotR = [](auto slot, int i, int j) -> double2 {
        if (i == j) return make_double2(slot(i), 0.0);
        const int lo = i < j ? i : j, hi2 = i < j ? j : i;
        const int p = (lo == 0) ? hi2 - 1 : (lo == 1 ? hi2 + 1 : 5);
        const double re = slot(4 + 2 * p), im = slot(5 + 2 * p);
        return make_double2(re, i < j ? im : -im);
    };
    auto rotate = [&](auto getR, const bool valid, const uint32_t item) {
#if BAZ_EVD_ORDER
        evd_project_lane<4, decltype(getR), true>(getR, valid, item, n, qstride, Qs, Gs, oa);
#else
        evd_project_lane<4>(getR, valid, item, n, qstride, Qs, Gs);
#endif
    };

    // streams one task: the covariances of its nit items into the wave's rtab (and the Rdbg tap)
    auto stream = [&](const uint32_t item0, const uint32_t nit) {
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
    };

    uint32_t task = blockIdx.x * 4 + wave;
    while (task < ntasks) {
        // one group: up to `park` tasks streamed and held, one more streamed into rtab, then their rotation passes back to back
        __builtin_amdgcn_s_setprio(3);
        double held[COVEVD_PARK][16];                 // R of this lane's item of each held task, in rtab's slot order
        uint32_t held_item0[COVEVD_PARK];             // (wave-uniform)
        uint32_t nheld = 0;
        const int lfull = ((uint32_t)lane < task_items) ? lane : (int)task_items - 1;
#pragma unroll
        for (int h = 0; h < COVEVD_PARK; ++h) {
            held_item0[h] = 0;
#pragma unroll
            for (int s = 0; s < 16; ++s) held[h][s] = 0.0;
            // more to stream and room to hold: the task's R moves from rtab (the next task rewrites it) into registers and the
            // wave streams on at once -- no rotation phase, no Q/G burst in the middle of its read stream.  (Not the wave's last
            // task, so not the globally last one: it is full.)
            if (nheld == (uint32_t)h && (uint32_t)h < park && task + tstride < ntasks) {
                held_item0[h] = task * task_items;
                stream(held_item0[h], task_items);
#pragma unroll
                for (int s = 0; s < 16; ++s) held[h][s] = rt[s][lfull];
                wave_lds_fence();
                nheld = h + 1;
                task += tstride;
            }
        }
        const uint32_t item0 = task * task_items;
        const uint32_t nit = (batch - item0 < task_items) ? batch - item0 : task_items;
        stream(item0, nit);
        const int li = ((uint32_t)lane < nit) ? lane : (int)nit - 1;     // lanes beyond nit redo the last item and write nothing
        // EVD of the held tasks' items and then of this task's, one item per lane, at low priority
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int h = 0; h < COVEVD_PARK; ++h)
            if ((uint32_t)h < nheld) {
                const double(&hr)[16] = held[h];
                rotate([&](int i, int j) { return slotR([&](int s) { return hr[s]; }, i, j); }, (uint32_t)lane < task_items,
                       held_item0[h] + lane);
            }
        rotate([&](int i, int j) { return slotR([&](int s) { return rt[s][li]; }, i, j); }, (uint32_t)lane < nit, item0 + lane);
        wave_lds_fence();
        task += tstride;
    }
}
