// evd_lds_kernel.inc.h -- the text of evd_proj_lds_kernel (music_kernels.hip.h, section 2b), included there TWICE: with
// BAZ_EVD_ORDER 0 it defines evd_proj_lds_kernel, the reference's kernel -- a __global__ function of its own with the
// signature and the statements it has always had, so that the code a context runs with the emitter-count mode off does not
// depend on the mode's existence --, with BAZ_EVD_ORDER 1 its twin evd_proj_lds_order_kernel with the per-item emitter count
// (OrderArgs; baz_music_set_order_mode): n is then the LARGEST count, and every item takes this Jacobi (the orthogonal
// iteration of 2c yields only the signal eigenvalues).  No include guard, no namespace of its own.
template <int M>
#if BAZ_EVD_ORDER
__global__ __launch_bounds__(64) void evd_proj_lds_order_kernel(const double2* __restrict__ R,
                                                                 double* __restrict__ Qs,
                                                                 uint32_t batch, uint32_t n, uint32_t qstride,
                                                                 double* __restrict__ Gs,
                                                                 double* __restrict__ Ss, const OrderArgs oa)
{
    const uint8_t* const only = nullptr;
#else
__global__ __launch_bounds__(64) void evd_proj_lds_kernel(const double2* __restrict__ R,
                                                           double* __restrict__ Qs,
                                                           uint32_t batch, uint32_t n, uint32_t qstride,
                                                           double* __restrict__ Gs,
                                                           const uint8_t* __restrict__ only = nullptr,
                                                           double* __restrict__ Ss = nullptr)
{
#endif
    constexpr int MM = M * M;
    constexpr int IPW = 64 / M;           // items per wave
    constexpr int MAX_SWEEPS = 24;
    constexpr int ME = M + (M & 1);       // even size of the round-robin schedule (odd M: one phantom index)
    // A lives in LDS (index space, dynamically addressed); V stays in REGISTERS: lane j holds row j of V with its
    // columns kept in tournament-position order, so the column pair of round-pair k is always registers 2k, 2k+1
    // (static), and is re-ordered between rounds by register moves.  V enters LDS only for the final projector
    // (it reuses A's storage).  Halving the LDS footprint doubles the resident waves at m >= 9.
    __shared__ double2 sA[IPW][M][M + 1]; // +1: rows of different lanes start on different banks
    __shared__ double sPart[IPW][M];
    __shared__ double sPar[IPW][ME / 2][6];
    __shared__ int sSel[IPW][M];          // eigenvalue index by ascending rank

    const int lane = threadIdx.x;
    const int slot = lane / M;            // item within the wave
    const int j = lane - slot * M;        // this lane's row (phase 1) / column (phase 2)
    const bool lane_used = slot < IPW;
    const int sl = lane_used ? slot : 0;
    const uint32_t item = blockIdx.x * IPW + sl;
    const uint32_t itc = (item < batch) ? item : (batch - 1);
    // `only` (the pass behind evd_sub_kernel): just the items that kernel handed back; a wave with none of them leaves
    const bool wanted = !only || only[itc] != 0;
    if (only && !__any(wanted && lane_used && item < batch)) return;
    const bool valid = lane_used && item < batch && wanted;
    double2(*A)[M + 1] = sA[sl];

    double2 Vrow[ME];
#pragma unroll
    for (int k = 0; k < ME; ++k) Vrow[k] = make_double2(k == j ? 1.0 : 0.0, 0.0);
    if (lane_used) {
        const double2* Rp = R + (size_t)itc * MM + j * M;
        double rsum = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            double2 v = Rp[k];
            rsum += v.x + v.y;
            if (k == j) v.y = 0.0;
            A[j][k] = v;
        }
        sPart[sl][j] = rsum * 0.0;      // NaN iff this row holds a NaN / Inf
    }
    wave_lds_fence();
    // non-finite covariance -> poisoned projector (see evd_proj_kernel)
    double poison = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) poison += sPart[sl][k];
    // exact power-of-two normalisation (see evd_proj_kernel)
    double dmax = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) dmax = fmax(dmax, fabs(A[k][k].x));
    int ex = 0;
    (void)frexp(dmax, &ex);
    const double scl = (dmax > 0.0 && dmax < __builtin_huge_val()) ? ldexp(1.0, -ex) : 1.0;
    wave_lds_fence();
    if (lane_used) {
#pragma unroll
        for (int k = 0; k < M; ++k) {
            double2 v = A[j][k];
            v.x *= scl; v.y *= scl;
            A[j][k] = v;
        }
    }
    wave_lds_fence();

    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        double off = 0.0;
        if (lane_used) {
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const double2 v = A[j][k];
                if (k != j) off += v.x * v.x + v.y * v.y;
            }
            sPart[sl][j] = off;
        }
        wave_lds_fence();
        double offsum = 0.0, dia = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) { offsum += sPart[sl][k]; const double a = A[k][k].x; dia += a * a; }
        const bool done = !(offsum > 2e-33 * dia);   // offsum counts every off-diagonal twice
        wave_lds_fence();
        if (__all(done || !lane_used)) break;

        // One sweep = ME-1 rounds of the round-robin (tournament) ordering; the <= ME/2 pairs of a round are disjoint,
        // so their rotations commute and read only their own 2x2 block: parameters of all pairs are computed at once
        // (lane k of the item takes pair k), then every lane applies ALL column operations of the round to its row
        // of A (LDS) and V (registers), then ALL row operations to its column of A.  3 LDS hand-overs per round
        // instead of 2 per rotation, one parameter evaluation per lane per round instead of one per lane per
        // rotation.  (Row-cyclic form: 2.05 ms per 16,384 16x16 items, 57 % of the config-5 step.)
        for (int r = 0; r < ME - 1; ++r) {
            if (lane_used && j < ME / 2) {
                const int k = j;
                const int pp = tour_idx<ME>(r, 2 * k), qq = tour_idx<ME>(r, 2 * k + 1);
                double c = 1.0, sn = 0.0, ur = 1.0, ui = 0.0;
                if (pp < M && qq < M) {                  // (a pair with the phantom index of an odd M idles)
                    const double2 apq = A[pp][qq];
                    const double app = A[pp][pp].x, aqq = A[qq][qq].x;
                    const double g2 = apq.x * apq.x + apq.y * apq.y;
                    const bool rot = !done && g2 > 1e-40;   // a converged item freezes (exact identity) while wave-mates sweep
                    const double gg = sqrt(g2);
                    const double ig = rot ? 1.0 / gg : 0.0;
                    ur = rot ? apq.x * ig : 1.0;
                    ui = rot ? apq.y * ig : 0.0;
                    const double tau = (aqq - app) * 0.5 * ig;
                    double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    t = rot ? t : 0.0;
                    c = 1.0 / sqrt(1.0 + t * t);
                    sn = t * c;
                }
                double* par = sPar[sl][k];
                par[0] = c; par[1] = sn; par[2] = sn * ur; par[3] = sn * ui; par[4] = c * ur; par[5] = c * ui;
            }
            wave_lds_fence();
            // phase 1: this lane's row j of A and V, columns p_k and q_k of every pair  (A J, V J).  All operands of
            // the round are fetched before the first result is stored (the pairs touch disjoint columns, which the
            // compiler cannot know): one LDS round trip per phase instead of one per pair.
            if (lane_used) {
                constexpr int HB = (ME / 2 + 1) / 2;          // two operand batches: bounds the live registers
#pragma unroll
                for (int h = 0; h < ME / 2; h += HB) {
                    double2 ax[HB], ay[HB];
#pragma unroll
                    for (int kk = 0; kk < HB; ++kk) {
                        const int k = h + kk;
                        if (k < ME / 2) {
                            const int pp = tour_idx<ME>(r, 2 * k), qq = tour_idx<ME>(r, 2 * k + 1);
                            if (pp < M && qq < M) { ax[kk] = A[j][pp]; ay[kk] = A[j][qq]; }
                        }
                    }
#pragma unroll
                    for (int kk = 0; kk < HB; ++kk) {
                        const int k = h + kk;
                        if (k >= ME / 2) continue;
                        const int pp = tour_idx<ME>(r, 2 * k), qq = tour_idx<ME>(r, 2 * k + 1);
                        if (pp >= M || qq >= M) continue;
                        const double* par = sPar[sl][k];
                        const double c = par[0], s = par[1], sur = par[2], sui = par[3], cur = par[4], cui = par[5];
                        const double2 x = ax[kk], y = ay[kk], vx = Vrow[2 * k], vy = Vrow[2 * k + 1];
                        A[j][pp] = make_double2(c * x.x - (sur * y.x + sui * y.y), c * x.y - (sur * y.y - sui * y.x));
                        A[j][qq] = make_double2(s * x.x + (cur * y.x + cui * y.y), s * x.y + (cur * y.y - cui * y.x));
                        Vrow[2 * k] = make_double2(c * vx.x - (sur * vy.x + sui * vy.y), c * vx.y - (sur * vy.y - sui * vy.x));
                        Vrow[2 * k + 1] = make_double2(s * vx.x + (cur * vy.x + cui * vy.y), s * vx.y + (cur * vy.y - cui * vy.x));
                    }
                }
            }
            wave_lds_fence();
            // phase 2: this lane's column j of A, rows p_k and q_k of every pair  (J^H (A J))
            if (lane_used) {
                double2 ax[ME / 2], ay[ME / 2];
#pragma unroll
                for (int k = 0; k < ME / 2; ++k) {
                    const int pp = tour_idx<ME>(r, 2 * k), qq = tour_idx<ME>(r, 2 * k + 1);
                    if (pp < M && qq < M) { ax[k] = A[pp][j]; ay[k] = A[qq][j]; }
                }
#pragma unroll
                for (int k = 0; k < ME / 2; ++k) {
                    const int pp = tour_idx<ME>(r, 2 * k), qq = tour_idx<ME>(r, 2 * k + 1);
                    if (pp >= M || qq >= M) continue;
                    const double* par = sPar[sl][k];
                    const double c = par[0], s = par[1], sur = par[2], sui = par[3], cur = par[4], cui = par[5];
                    const double2 x = ax[k], y = ay[k];
                    double2 np = make_double2(c * x.x - (sur * y.x - sui * y.y), c * x.y - (sur * y.y + sui * y.x));
                    double2 nq = make_double2(s * x.x + (cur * y.x - cui * y.y), s * x.y + (cur * y.y + cui * y.x));
                    if (j == qq) np = make_double2(0.0, 0.0);                    // a_pq := 0
                    if (j == pp) { nq = make_double2(0.0, 0.0); np.y = 0.0; }    // a_qp := 0, real diagonal
                    if (j == qq) nq.y = 0.0;
                    A[pp][j] = np;
                    A[qq][j] = nq;
                }
            }
            wave_lds_fence();
            // tournament movement of V's columns (registers): position pos now holds what tour_src(pos) held
            {
                double2 t[ME];
#pragma unroll
                for (int k = 0; k < ME; ++k) t[k] = Vrow[tour_src<ME>(k)];
#pragma unroll
                for (int k = 0; k < ME; ++k) Vrow[k] = t[k];
            }
        }
    }
    // (sweeps are whole periods of the tournament: position == original index again)

    // Ascending rank of the eigenvalues (ties -> lower column first; the noise space is rank < m-n, .cc:93): lane j
    // ranks eigenvalue j and publishes sSel[rank] = j.  The projector is then summed over the SMALLER of the two sets:
    // Q = sum_noise v v^H  or  Q = I - sum_signal v v^H  (V is unitary) -- n = 2 of 16 columns at config 5, which
    // takes the epilogue from ~m^3/2 to ~m^2 n complex MACs per item.
    if (lane_used) sSel[sl][j] = j;
    wave_lds_fence();
    if (lane_used) {
        const double wj = A[j][j].x;
        int rank = 0;
#pragma unroll
        for (int l = 0; l < M; ++l) {
            const double wl = A[l][l].x;
            rank += (wl < wj || (wl == wj && l < j)) ? 1 : 0;
        }
        sSel[sl][rank] = j;                    // (NaN eigenvalues: every rank is 0; the projector is poisoned anyway)
    }
#if BAZ_EVD_ORDER
    int nsig;
    {
        // the item's own count: its first lane walks the diagonal in ascending order (one lane per item; m logarithms) and
        // publishes the count through sSel's neighbour sKhat.  A non-finite covariance counts no emitter.
        __shared__ int sKhat[IPW];
        wave_lds_fence();
        if (lane_used && j == 0) {
            const double2(*Ad)[M + 1] = sA[sl];
            const int* sel = sSel[sl];
            int khat = bazorder::order_decide<0>((int)M, (int)n, oa.nsnap, oa.crit, [&](int i) { return Ad[sel[i] & 15][sel[i] & 15].x; });
            khat = (poison == poison) ? khat : 0;
            sKhat[sl] = khat;
            if (valid) oa.ord[item] = (uint8_t)khat;
        }
        wave_lds_fence();
        nsig = sKhat[sl];
    }
    const int nnoise = (int)M - nsig;
    const bool use_noise = nnoise <= nsig;
    const int cnt = use_noise ? nnoise : nsig;
#else
    const int nnoise = (int)M - (int)n;
    const bool use_noise = nnoise <= (int)n;
    const int cnt = use_noise ? nnoise : (int)n;
#endif
    const int base = use_noise ? 0 : nnoise;
    // V rows go to LDS (A's storage) for the cross-lane projector
    wave_lds_fence();
    double2(*V)[M + 1] = sA[sl];
    if (lane_used) {
#pragma unroll
        for (int k = 0; k < M; ++k) V[j][k] = Vrow[k];
    }
    wave_lds_fence();
    // the noise eigenvectors themselves (see evd_proj_kernel): lane j writes component j of every noise vector
    if (valid && Gs) {
        for (int r = 0; r < nnoise; ++r) {
            const double2 v = V[j][sSel[sl][r] & 15];
            Gs[(size_t)((r * M + j) * 2) * qstride + item] = v.x;
            Gs[(size_t)((r * M + j) * 2 + 1) * qstride + item] = v.y;
        }
#if BAZ_EVD_ORDER
        {
            // the scan's literal form runs over the uniform m rows: those at or beyond this item's m - k are zeros (exact zeros
            // in ||G^H a||^2)
            for (int r = nnoise; r < M; ++r) {
                Gs[(size_t)((r * M + j) * 2) * qstride + item] = 0.0;
                Gs[(size_t)((r * M + j) * 2 + 1) * qstride + item] = 0.0;
            }
        }
#endif
    }
    // the two signal eigenvectors as the coefficient vectors of the scan's short form (scan_mfma_kernel, SIG): output
    // 2c = Re s_c^H a, 2c+1 = Im s_c^H a over the real coordinates (re a_0, im a_0, re a_1, ...)
    if (valid && Ss && n <= 2) {
        for (int cI = 0; cI < (int)n; ++cI) {
#if BAZ_EVD_ORDER                              // the short form keeps its n vectors: those below the item's signal set are zeros
            double2 v = V[j][sSel[sl][(int)M - (int)n + cI] & 15];
            if ((int)M - (int)n + cI < nnoise) v = make_double2(0.0, 0.0);
#else
            const double2 v = V[j][sSel[sl][nnoise + cI] & 15];
#endif
            const double vr = v.x + poison, vi = v.y + poison;
            Ss[(size_t)((2 * cI) * 2 * M + 2 * j) * qstride + item] = vr;
            Ss[(size_t)((2 * cI) * 2 * M + 2 * j + 1) * qstride + item] = vi;
            Ss[(size_t)((2 * cI + 1) * 2 * M + 2 * j) * qstride + item] = -vi;
            Ss[(size_t)((2 * cI + 1) * 2 * M + 2 * j + 1) * qstride + item] = vr;
        }
    }
    // lane j emits row j of Q (upper part): Q_jl = sum_{k in set} V[j][k] conj(V[l][k])
    // (Qs == nullptr: the scan runs the short form from Ss and never reads the projector)
    if (valid && Qs) {
        for (int l = j; l < M; ++l) {
            double re = 0.0, im = 0.0;
            for (int i = 0; i < cnt; ++i) {
                const int k = sSel[sl][base + i] & 15;
                const double2 vj = V[j][k], vl = V[l][k];
                re += vj.x * vl.x + vj.y * vl.y;
                im += vj.y * vl.x - vj.x * vl.y;
            }
            if (!use_noise) { re = ((l == j) ? 1.0 : 0.0) - re; im = -im; }
            if (l == j) {
                Qs[(size_t)(j * M + j) * qstride + item] = re + poison;
            } else {
                Qs[(size_t)(j * M + l) * qstride + item] = 2.0 * re + poison;
                Qs[(size_t)(l * M + j) * qstride + item] = -2.0 * im + poison;
            }
        }
    }
}
