// baz_music_hip.hip -- C-ABI (include/baz_music_hip.h) over the gfx950 MUSIC-DoA kernels.
//
// Host-side counterpart of baz_music_doa's state and work() body
// (/root/reference/lib/baz_music_doa.cc:35-53, 60-70, 72-161).  No torch / GNU Radio types
// cross this boundary; no CPU arithmetic fallback exists: without a usable gfx950 device
// baz_music_create() fails with BAZ_MUSIC_E_NODEVICE / BAZ_MUSIC_E_HIP.
#include "../../include/baz_music_hip.h"
#include "music_kernels.hip.h"
#include "music_wide_kernels.hip.h"
#include "scan_coarse_kernels.hip.h"
#include "scan_i8_kernels.hip.h"
#ifdef BAZ_MUSIC_LAB       // measured and NOT shipped (profiles/r05_i8p_negative.txt, r05_sort_negative.txt): the release library has none of their kernels
#include "scan_i8p_kernels.hip.h"
#include "sort_kernels.hip.h"
#endif
#include "table_kernels.hip.h"
#include "smoothing_kernels.hip.h"
#include "refine_kernels.hip.h"
#include "power_kernels.hip.h"
#include "beam_kernels.hip.h"
#include "calib_kernels.hip.h"
#include "whiten_kernels.hip.h"
#include "beamspace_kernels.hip.h"
#include "subband_kernels.hip.h"
#include "average_kernels.hip.h"
#include "spectrum_kernels.hip.h"
#include "device_buffer.hip.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include <mutex>
#include <thread>
#include <new>
#include <string>
#include <vector>

using namespace bazmusic;

// Environment switches.  The RELEASE library reads only the documented tuning knobs: BAZ_MUSIC_EXACT,
// BAZ_MUSIC_COARSE, BAZ_MUSIC_CHUNK_MIB, BAZ_MUSIC_PIN_LIMIT_MIB, BAZ_MUSIC_ZERO_COPY, BAZ_MUSIC_SINGLE_MIB -- none of them
// can make a result wrong.  Everything else (ablations, older kernels, geometry overrides, dumps) exists only in the lab
// build, -DBAZ_MUSIC_LAB = libbaz_music_hip_lab.so, which tests/lab and the A/B tests load explicitly
// (tests/test_abi.py::test_release_library_reads_only_the_documented_knobs lists the strings of the release .so).
#ifdef BAZ_MUSIC_LAB
#define BAZ_LAB_ENV(NAME) getenv(NAME)
#else
#define BAZ_LAB_ENV(NAME) (static_cast<const char*>(nullptr))
#endif

// ---- device allocations ---------------------------------------------------------------------------------------------------------
// Every device buffer of this library comes from dev_malloc / dev_free.  Release build: hipMalloc / hipFree.  Lab build with
// BAZ_MUSIC_GUARD=1 (round 6, after a GPU memory fault the driver saw and no test did): every buffer lies between two 64-KiB guard
// zones filled with a pattern; baz_music_debug_guard_check() -- and every dev_free -- compares the zones with the pattern, so a
// kernel that writes outside its buffer is caught at the buffer it ran over, not at whatever was allocated next to it.
namespace {
#ifdef BAZ_MUSIC_LAB
constexpr size_t GUARD_BYTES = 64u << 10;
constexpr int GUARD_PATTERN = 0xA5;
struct GuardRec { void* base; size_t bytes; };
std::mutex g_guard_mtx;
std::vector<std::pair<void*, GuardRec>> g_guards;     // user pointer -> allocation (a handful of buffers per context)
unsigned long long g_guard_damaged = 0;               // zones found overwritten so far (at a free or at a check)
int guard_level()
{
    static const int level = [] { const char* v = getenv("BAZ_MUSIC_GUARD"); return v ? atoi(v) : 0; }();
    return level;
}
bool guard_on() { return guard_level() != 0; }
// compares both zones of one allocation with the pattern (synchronises the device); returns the damaged zones (0 .. 2)
int guard_check_one(void* user, const GuardRec& g)
{
    static thread_local std::vector<unsigned char> host(GUARD_BYTES);
    int bad = 0;
    (void)hipDeviceSynchronize();
    for (int z = 0; z < 2; ++z) {
        const unsigned char* zone = static_cast<const unsigned char*>(g.base) + (z ? GUARD_BYTES + ((g.bytes + 255) & ~(size_t)255) : 0);
        if (hipMemcpy(host.data(), zone, GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); ++bad; continue; }
        size_t first = GUARD_BYTES;
        for (size_t i = 0; i < GUARD_BYTES; ++i)
            if (host[i] != (unsigned char)GUARD_PATTERN) { first = i; break; }
        if (first != GUARD_BYTES) {
            ++bad;
            fprintf(stderr, "[baz_music_hip] GUARD ZONE DAMAGED: buffer %p (%zu bytes), zone %s it, first damaged byte at %+lld from the buffer's %s\n",
                    user, g.bytes, z ? "behind" : "in front of", z ? (long long)first : (long long)first - (long long)GUARD_BYTES, z ? "end (rounded up to 256)" : "start");
        }
    }
    return bad;
}
#endif

hipError_t dev_malloc(void** p, size_t bytes)
{
#ifdef BAZ_MUSIC_LAB
    if (guard_on()) {
        const size_t body = (bytes + 255) & ~(size_t)255;
        void* base = nullptr;
        hipError_t e = hipMalloc(&base, body + 2 * GUARD_BYTES);
        if (e != hipSuccess) return e;
        e = hipMemset(base, GUARD_PATTERN, body + 2 * GUARD_BYTES);     // (the body too: a read of an uninitialised buffer shows up as 0xA5A5...)
        // The fill runs on the null stream and the library's streams are non-blocking ones: a buffer allocated INSIDE a launch sequence (the peak
        // picker's private spectrum) was still being filled while the scan wrote it -- seen as a fuzz failure under the guard only.  Wait for it.
        // (BAZ_MUSIC_GUARD=2: without the wait, to show that.)
        if (e == hipSuccess && guard_level() != 2) e = hipDeviceSynchronize();
        if (e != hipSuccess) { (void)hipFree(base); return e; }
        *p = static_cast<unsigned char*>(base) + GUARD_BYTES;
        std::lock_guard<std::mutex> lk(g_guard_mtx);
        g_guards.emplace_back(*p, GuardRec{base, bytes});
        return hipSuccess;
    }
#endif
    return hipMalloc(p, bytes);
}

hipError_t dev_free(void* p)
{
#ifdef BAZ_MUSIC_LAB
    if (guard_on() && p) {
        std::lock_guard<std::mutex> lk(g_guard_mtx);
        for (size_t i = 0; i < g_guards.size(); ++i)
            if (g_guards[i].first == p) {
                const GuardRec g = g_guards[i].second;
                g_guard_damaged += (unsigned long long)guard_check_one(p, g);
                g_guards.erase(g_guards.begin() + (long)i);
                return hipFree(g.base);
            }
    }
#endif
    return hipFree(p);
}

// ... through their owners (device_buffer.hip.h): a buffer is freed when its owner goes or regrows, nowhere else
struct GuardedDevice {
    using status = hipError_t;
    static hipError_t alloc(void** p, size_t bytes) { return dev_malloc(p, bytes); }
    static void release(void* p) { (void)dev_free(p); }
};
template <typename T> using DevBuf = bazbuf::Buffer<T, bazbuf::Counted<GuardedDevice, &bazbuf::LiveCounts::device>>;
template <typename T> using PinBuf = bazbuf::PinnedBuffer<T>;
using bazbuf::DeviceGuard;
using bazbuf::drain;
}  // namespace

namespace {


struct StageProf {
    std::vector<hipEvent_t> ev;   // pairs (start, stop)
    size_t used = 0;
    double total_ms = 0.0;
    uint64_t launches = 0;
};

}  // namespace

// device-side slots of the host-fed path's pipelined copies: two when the host waits for a slot's outputs before it reuses the slot
// (pageable caller memory: the runtime blocks in those copies anyway), all four when the whole call is enqueued without the host
// waiting for anything (page-locked caller memory, round 6)
constexpr int BAZ_MUSIC_NSLOT = 4;

// The per-call side output of one opt-in mode: what the mode's kernels leave per item of a whole process*() call, all chunks in call
// order, for its baz_music_last_*() reader.  One or two buffers behind one count (the beam mode: beams and weights).  Nothing is
// allocated while the mode is off.  The steps -- open a call, refuse / place a chunk, reserve, read back -- are the side_*()
// functions below; every mode goes through them.
struct SideOut {
    struct Buf {
        DevBuf<uint8_t> p;
        size_t item_bytes = 0;       // bytes per item of a call (baz_music_create); 0: this mode has no such buffer
    } buf[2];
    uint32_t count = 0;              // items of the call in flight / the last call recorded so far (the next chunk's offset)
    bool on = false;                 // whether the last process*() call ran with the mode on (else the reader reports a constant)
    const char* what = "";           // the name a refused chunk reports
    // where the chunk at `count` goes in buffer k
    template <typename T>
    T* chunk(int k = 0) const { return reinterpret_cast<T*>(buf[k].p + (size_t)count * buf[k].item_bytes); }
};

struct baz_music_ctx {
    uint32_t m = 0, n = 0, nsamples = 0, res = 0, K = 0;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;      // the stream process_device() launches on (own or caller's)
    uint32_t fb_steps = 0;   // 64-bin steps
    size_t fb_step_elems = 0;   // double2 elements per step of FB (2 * KS * 64)
    uint32_t nclass = 1;     // row classes of the spectrum port: 64 / gcd(res, 64) when res % 4 == 0, else 1
    uint32_t keep_mask = 0;  // low-word mask of the top-n key (bin index lives in the cleared bits)
    // per-range top-n candidate keys (scan_mfma_kernel -> topn_merge_kernel)
    DevBuf<double> dCand;
    // workspace
    DevBuf<double2> dR;
    DevBuf<double> dQ;
    uint32_t cap = 0;   // items
    // host-fed path (baz_music_process): two device-side slots so that the H2D copy of chunk i+1, the kernels
    // of chunk i and the D2H copy of chunk i-1 overlap on three streams
    struct Slot {
        DevBuf<float> in;
        DevBuf<float> al;            // ang then lvl of the chunk in flight, back to back (2 * cap * n floats)
        PinBuf<float> h_al;          // page-locked host image of `al`: ONE small D2H per chunk, then a CPU copy to the caller
        DevBuf<float> spec;
        hipEvent_t h2d = nullptr, comp = nullptr, d2h = nullptr;
        bool busy = false;
        uint32_t pend_done = 0, pend_nb = 0;   // the chunk whose ang / lvl still sit in h_al
    } slot[BAZ_MUSIC_NSLOT];
    uint32_t s_cap = 0;
    bool s_has_spec = false;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;   // baz_music_process_device_on: ordering against the caller's stream
    std::mutex mtx;   // serialises process* against the table SWAP of set_table, like d_mutex (.cc:67,101)
    // Every device image of one steering table and the parameters derived from it.  The context holds two: `tab`, the set in force,
    // which every launch site reads, and `shadow`.  Retune without stalling the stream (round 5): baz_music_set_table builds every
    // image of the new table with the kernels of table_kernels.hip.h on `s_tab` into the SHADOW set and takes `mtx` only to exchange
    // the two sets (retune())
    struct TableSet {
        // steering table as the real bilinear-form table F[bin][m*m] (fp64) in MFMA B-operand order:
        // FB[step][chunk][lane] (double2), see build_FB; one padded step in front of step 0 and one behind the last
        // (the scan's row classes read shifted windows), dFB points at the allocation, step 0 is dFB + fb_step_elems
        DevBuf<double2> dFB;
        DevBuf<double2> dTB;             // raw steering table as fp64 MFMA B-operand image (build_TB), padded like dFB
        DevBuf<uint4> dCS;               // coarse-gated scan, per 16-bin tile: f16 hi/lo pieces of the scaled table (B32, B16) + the fp64 B operand (X)
        DevBuf<uint4> dIB;               // int8-matrix-core scan: digit image of the table (build_i8_image)
        DevBuf<double> dA2p;             // short_form_applies(): ||a||^2 per bin, padded like dFB (fb_steps + 2 steps of 64)
        DevBuf<float2> dTA;              // wide arrays: steering table transposed, [m][res] complex64
        DevBuf<double> dA2;              // wide arrays: ||a||^2 per bin
        DevBuf<float2> dRW;              // the raw table as delivered, [res][m] complex64: what refine_kernel gathers its steering rows from
                                         // (dRaw is the upload staging buffer: the next set_table overwrites it under batches in flight)
#ifdef BAZ_MUSIC_LAB
        DevBuf<uint4> dIP;               // level-packed int8 operands (m <= 4; shares i8 / i8_ok with dIB: a configuration has one of the two)
        DevBuf<float> dKT;               // float32 table at the sort key's sample bins (sort_kernels.hip.h; m <= 8)
#endif
        CoarseParams cs = {0.0f, 0.0f, 0.0, 0.0, 1};
        I8Params i8 = {};
        bool cs_ok = false;              // coarse image built and its scales representable
        bool i8_ok = false;              // digit image built (finite table, scale representable, size within I8_IMAGE_LIMIT)
        double refine_below = 0.0;       // literal-form refinement: threshold on d = a^H Q a
        // opt-in noise pre-whitening (whiten_kernels.hip.h): the W this set's images were built under, m x m row-major.  It lives here so
        // that the swap of a retune exchanges (images, W) together: a batch whitens with the W its table was whitened with.
        DevBuf<double2> dWh;             // allocated by the first build with the mode on
        bool wh_on = false;              // the whiten stage runs for batches that read this set
    } tab, shadow;
    std::mutex tab_mtx;              // retunes among themselves (held for a whole baz_music_set_table; never while `mtx` is wanted by work())
    hipStream_t s_tab = nullptr;     // side stream of the table builders (highest priority: they are tiny)
    hipEvent_t ev_swap = nullptr;    // recorded on the launch stream at every swap: batches that still read the retired set
    bool swap_recorded = false;
    DevBuf<float> dRaw;              // the raw fp32 table on the device (resolution x m complex64)
    PinBuf<float> hRaw;              // its page-locked staging copy (the caller's vector may be pageable and short-lived)
    DevBuf<baztab::TableStats> dTabStats;
    PinBuf<baztab::TableStats> hTabStats;   // ... page-locked
    PinBuf<float> h_al_big;                             // host-fed zero-copy calls: page-locked ang / lvl image of a whole call
    double last_retune_ms = 0.0;     // wall time of the last baz_music_set_table, of which ...
    double last_swap_wait_ms = 0.0;  // ... waiting for and holding `mtx`
    int profiling = 0;      // 0 off, 1 every stage, 2 only the dominant (scan) stage
    int lab_variant = 0;
    // literal-form refinement of near-null tiles (literal_tile() inside the scan)
    DevBuf<double> dG;             // noise eigenvectors, item-minor like dQ (cap * m*m * 2 doubles)
    size_t tb_step_elems = 0;      // double2 elements per step of TB (2 * ceil(2m/4) * 64)
    DevBuf<unsigned long long> dRefined;      // statistic: (item, bin) values recomputed, [2]: double-buffered by API call
    int stat_parity = 0;                      // the scan adds to dRefined[stat_parity]; the merge clears the other one
    bool stat_next_clean = true;              // false after a call that failed before its merge ran
    int refine_off = 0;            // lab (BAZ_MUSIC_NO_REFINE=1): projector form everywhere
    int lab_cov_old = 0;           // lab (BAZ_MUSIC_COV_OLD=1): the round-1 covariance kernel at m = 4
    int force_nsplit = 0;          // tests / lab (BAZ_MUSIC_NSPLIT=k): bin ranges per row in the scan, 0 = by batch size
    // wide arrays (17 <= m <= BAZ_MUSIC_MAX_M): the run-time-m kernels of music_wide_kernels.hip.h
    bool wide = false;
    DevBuf<double2> dGw;           // noise eigenvectors, [items][m - n][m]
    DevBuf<double> dWS;            // fp64 strengths, [items][res] (the top-n's input)
    DevBuf<double2> dSw;           // signal eigenvectors, [items][n][m] (the scan's short form where 2n <= m)
    int wide_literal_only = 0;     // lab (BAZ_MUSIC_WIDE_LITERAL=1): no short form in scan_wide_kernel
    uint32_t wide_cov_blocks = 512;
    int wide_cov_mfma = 0;         // 17 <= m <= 32: cov_wide_mfma_kernel, 33 <= m <= 64: cov_wide_pairs_kernel (BAZ_MUSIC_WIDE_COV_MFMA=0: lab)
    int wide_mfma = 0;             // 17 <= m <= 64, n <= 8: the scan on the fp64 matrix core (scan_wide_mfma_kernel; BAZ_MUSIC_WIDE_MFMA=0: lab)
    uint32_t wide_cap = 0;         // items the three buffers above (and dR) hold
    DevBuf<double> dSs;            // short_form_applies(): coefficient vectors of the scan's short form, [2n * 2m][q_stride]
    int sig_scan = 1;              // lab / tests: BAZ_MUSIC_SIG_SCAN=0 keeps the projector GEMM
    DevBuf<uint8_t> dRedo;         // [cap] items evd_sub_kernel hands back to the Jacobi
    int sub_evd = 1;               // signal subspace by orthogonal iteration where n <= 4 (run-time-m kernels: n <= 8) (lab: BAZ_MUSIC_SUB_EVD=0)
    int fused_covevd = 0;          // m = 4, K % 256 == 0: covariance + EVD in one kernel (BAZ_MUSIC_FUSE=0: lab, two kernels)
    uint32_t covevd_blocks = 512u; // grid of cov4_evd_kernel: the workgroups resident at once (2 per CU)
    uint32_t covevd_park = 0;      // tasks a wave of cov4_evd_kernel holds in registers before it rotates: 0 = one rotation phase per task (shipped); lab (BAZ_MUSIC_COVEVD_DEFER=1): COVEVD_PARK
    int covevd_task_items = 0;     // lab (BAZ_MUSIC_COVEVD_TASK_ITEMS = 64 / 32 / 16): items per wave task of cov4_evd_kernel, 0 = by batch size
    uint32_t cov4_resident_blocks = 256u;        // grid of cov4_x4_kernel (persistent waves): one workgroup per CU
    // coarse-gated scan (scan_coarse_kernels.hip.h): m <= 8, spectrum port not wired
    uint32_t cs_tiles = 0;         // tiles in the image (a multiple of 8)
    int coarse = 1;                // BAZ_MUSIC_COARSE=0: the full fp64 scan also without the spectrum port (A/B, tests)
    int coarse_rg = 4;             // BAZ_MUSIC_COARSE_RG: row groups (x 16 items) per wave, 2 or 4 (lab)
    int coarse_lab = 0;            // BAZ_MUSIC_COARSE_LAB=1: never run an exact tile (cost of the coarse passes alone; wrong results)
    int coarse_stats = 0;          // BAZ_MUSIC_COARSE_STATS=1: count exact tile evaluations (baz_music_debug_coarse_fired)
    DevBuf<unsigned long long> dMargin;      // baz_music_debug_coarse_margin: worst error / allowance (float bits << 32 | where)
#ifdef BAZ_MUSIC_LAB
    // Sorting the items of a batch by their nulls in front of the gated scan (sort_kernels.hip.h), while that scan reports many fired tiles
    DevBuf<uint16_t> dKeys;
    DevBuf<uint32_t> dHist;        // items per key (KEY_BUCKETS)
    DevBuf<uint32_t> dCursor;      // items per range of keys (KEY_BLOCKS)
    DevBuf<uint32_t> dPerm;
    uint32_t sort_cap = 0;         // items dKeys / dPerm hold
    DevBuf<unsigned long long> dFire;           // [2] exact evaluations / (row group, tile) pairs walked by the gated scan of the call in flight
    PinBuf<unsigned long long> hFire;           // page-locked [4]: the same of a FINISHED call, [2] = its tag (call number << 1 | sorted), written by its merge
    unsigned long long* hFireDev = nullptr;     // ... its device address
    unsigned long long fire_calls = 0, fire_seen = 0;
    int sort_mode = 0;             // 0 never (the product), 1 always, -1 adaptive -- LAB builds only (BAZ_MUSIC_SORT).  Measured and not shipped:
                                   // the order cuts the exact evaluations of an incoherent batch from 22 % to 4.6 % of the tile pairs, but key + sort cost
                                   // 0.17 ms (0.08 with a library radix sort) of the 0.22 ms the scan gains (profiles/r05_sort_negative.txt)
    bool sort_on = false;
    uint32_t sort_streak = 0;
    uint64_t sort_clock = 0, sort_retry_at = 0;
    double rate_unsorted = 0.0;
    uint64_t sorted_calls = 0, unsorted_calls = 0;     // (tap: baz_music_debug_sort_state)
#endif
    uint32_t scan_lds_pad = 0;     // lab (BAZ_MUSIC_SCAN_LDS_PAD bytes): dynamic LDS the fp64 scan asks for and never touches -- caps its workgroups per CU
                                   // (tests/lab/two_ctx_split.py: does a low-register covariance of ANOTHER context fit beside three of them?)
    int seq_walk = 0;              // lab (BAZ_MUSIC_SEQ_WALK=1): scan_mfma_kernel walks its steps left to right (round 4's order; A/B of the strided walk)
#ifdef BAZ_MUSIC_LAB
    int i8p_on = 0;                // LAB builds only (BAZ_MUSIC_I8P=1): the level-packed int8 scan at m <= 4.  Measured and not shipped
                                   // (profiles/r05_i8p_negative.txt): its arithmetic is 0.31 ms against the fp64 scan's 0.56, but the spectrum
                                   // stores alone take what the fp64 scan takes (0.59 - 0.73 ms by box), and incoherent batches run 2.4 x slower
#endif
    // int8-matrix-core scan (scan_i8_kernels.hip.h): 6 <= m <= 16, n <= 4
    int i8_on = 1;                 // BAZ_MUSIC_EXACT=1: every value on the fp64 matrix core (A/B; the round-3 scan)
    int i8_abl = 0;                // lab (BAZ_MUSIC_I8_ABL): ablation mask of scan_i8_kernel (timing only)
    int refine_nocount = 0;        // lab (BAZ_MUSIC_NO_REFINE_COUNT): the scans do not count the values they recompute
    uint32_t num_cus = 256;        // compute units of the device (launch geometry of scan_i8_kernel)
    int i8_wgs_per_cu[2][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};   // [NMAX > 2][SPEC][VEC4]: resident workgroups per CU (occupancy API, on first use)
    DevBuf<unsigned long long> dI8Stat;      // [0] wave tiles that ran the refined form, [1] wave tiles walked, [2] .. [4] VAL margins
    int peak_mode = 0;      // 0: the reference's n strongest bins; 1 (opt-in extension): n strongest local maxima
    DevBuf<float> dPeakSpec;      // internal spectrum when peak mode runs without the spectrum port
    uint32_t call_items = 0;        // items of the last process*() call: what the reader of a mode that was off reports on (the out_* below)
    // Opt-in per-item emitter count (baz_music_set_order_mode; NOT reference behaviour; order_kernels.hip.h).  While
    // order_mode is 0 none of the mode's kernels is launched and nothing below is allocated on the process path.
    int order_mode = 0;             // 0: the fixed n of the reference; 1 MDL, 2 AIC: n is the largest count
    uint32_t order_nsnap = 0;       // snapshots N of the criterion; 0: K (the smoothing mode hands its inner context the outer K)
    SideOut out_ord;                // one count (uint8) per item; after a call with the mode off every count is n
    bool ord_driven = false;        // an inner context of the smoothing mode: the outer context opens the call (order_begin)
    uint8_t* ord_cur = nullptr;     // where the EVD launched next writes its counts (null: a debug tap -> dOrdTap)
    DevBuf<uint8_t> dOrdTap;        // counts of the debug taps' EVD launches (never read back)
    // Opt-in sub-bin angle refinement (baz_music_set_refine_mode; NOT reference behaviour; refine_kernels.hip.h).  While
    // refine_mode is 0 its kernel is not launched and nothing below is allocated.
    int refine_mode = 0;            // 0: ang on the grid (the reference); 1: parabolic fit of the null
    DevBuf<float> dRefAl;           // ang | lvl of the chunk in flight as the pickers leave them (refine_kernel writes the caller's)
    SideOut out_ref;                // delta (double) per (item, slot); after a call with the mode off every offset is 0
    // Opt-in per-emitter Capon power (baz_music_set_power_mode; NOT reference behaviour; power_kernels.hip.h).  While
    // power_mode is 0 its kernel is not launched and nothing below is allocated.  The pickers' staging buffer is dRefAl, shared with
    // the refinement: one buffer with either mode or both on.
    int power_mode = 0;             // 0: off (the reference); 1: the estimates behind baz_music_last_powers; 2: ... and lvl carries (float)P
    SideOut out_pow;                // P (double) per (item, slot); after a call with the mode off every power is 0
    // Opt-in MVDR beamformer output per reported entry (baz_music_set_beam_mode; NOT reference behaviour; beam_kernels.hip.h, DESIGN.md
    // 8g).  While beam_mode is 0 its two kernels are not launched and nothing below is allocated.  The pickers' staging buffer is dRefAl.
    int beam_mode = 0;              // 0: off (the reference); 1: MVDR
    double beam_loading = 0.0;      // diagonal loading, in units of the mean diagonal of R
    enum { BEAM_Y = 0, BEAM_W = 1 };
    SideOut out_beam;               // [BEAM_Y] y (complex64) per (item, slot, snapshot), [BEAM_W] w (complex128) per (item, slot, antenna);
                                    // after a call with the mode off every beam and weight is 0
    // Opt-in covariance averaging across the items of the stream (baz_music_set_averaging; NOT reference behaviour; average_kernels.hip.h,
    // DESIGN.md 8e).  While avg_window is 1 none of the mode's kernels is launched and nothing below is allocated.
    uint32_t avg_window = 1;        // W: 1 = off (the reference)
    double avg_beta = 1.0;          // forgetting factor (1: boxcar)
    double avg_neff = 1.0;          // effective items of a full window: the emitter-count criterion's N is K * avg_neff
    bazavg::AvgTable avg_tab = {};  // weights and normalisations of (W, beta): handed to average_kernel by value
    uint32_t avg_hist = 0;          // plain covariances of the stream so far that the history holds: min(t, W - 1), t = items since create / reset
    int avg_parity = 0;             // dAvgHist[avg_parity] is the history the next launch reads; it writes the other one
    DevBuf<double2> dAvgHist[2];    // [W - 1][m*m] each: the last W - 1 plain covariances, oldest first
    DevBuf<double2> dRavg;          // averaged covariances of the launch in flight (what the EVD reads while the mode is on)
    // Opt-in per-antenna gain / phase calibration (baz_music_set_calibration; NOT reference behaviour; calib_kernels.hip.h).
    // While calib_on is false build_tables_device launches what it launched before the mode existed; hRaw always holds the caller's
    // table.  calib_on / calib_gamma change under `tab_mtx` (they are read by the table builders only).  The estimator's buffers are
    // allocated by its first call.
    bool calib_on = false;
    bazcalib::CalibGamma calib_gamma = {};   // gamma_r, r < m
    DevBuf<float> dCalIn;           // baz_music_calibrate: the chunk's input on the device
    DevBuf<double> dCalPart;        // the runs' partial sums, [groups][2 m^2], then R-bar, [2 m^2]
    // Opt-in noise pre-whitening (baz_music_set_noise_covariance; NOT reference behaviour; whiten_kernels.hip.h).  While it
    // is off build_tables_device and the launch sequences launch what they launched before the mode existed and nothing below is
    // allocated.  wh_on / wh_Rn / hWh change under `tab_mtx` (the table builders read them); wh_want -- the mode is on or being switched
    // on -- changes under `mtx` (what set_beam_mode / set_estimator refuse on); the stage's buffers belong to the launch sequences (`mtx`).
    bool wh_on = false;
    bool wh_want = false;
    std::vector<double> wh_Rn;      // Rn as given (m*m complex128), for get_noise_covariance
    PinBuf<double2> hWh;            // W, m x m row-major, page-locked: the builders copy it into the set they build
    DevBuf<double2> dRwh;           // R' of the launch in flight (what the EVD reads while the mode is on)
    DevBuf<double2> dWhT;           // 17 .. 64 antennas: (W R)^H between the two passes
    // Opt-in choice of estimator (baz_music_set_estimator; NOT reference behaviour; spectrum_kernels.hip.h).  While
    // estimator is 0 none of the mode's kernels is launched and nothing is allocated for it.  With it on the spectrum is written to
    // port 2 or, where that is not wired, to the private spectrum peak mode keeps (dPeakSpec).
    int estimator = 0;              // 0: MUSIC (the reference); 1: Capon; 2: Bartlett
    size_t chunk_bytes = 0;   // host-fed path: traffic per pipelined chunk (BAZ_MUSIC_CHUNK_MIB); 0 = by buffer kind
    // host-fed path: page ranges of the caller's buffers this context has page-locked (baz_music_host_register)
    struct HostPin { uintptr_t lo, hi; uint32_t asked; };   // [lo, hi): the caller's exact bytes
    std::vector<HostPin> pins;                           // the registrations we hold a share of (g_pins): disjoint, not touching
    std::vector<HostPin> refused;                        // requests the runtime refused (`asked` again so many times since)
    uint64_t pinned_bytes = 0;
    uint64_t pin_limit = 4096ull << 20;                  // BAZ_MUSIC_PIN_LIMIT_MIB
    int auto_pin = 0;                                    // baz_music_set_host_pinning
    int zero_copy = 1;                                   // small calls on page-locked memory: no copies (BAZ_MUSIC_ZERO_COPY=0: lab)
    int single_limit_mib = 64;                           // page-locked calls below this much traffic run as ONE chunk (BAZ_MUSIC_SINGLE_MIB)
    StageProf prof[BAZ_MUSIC_NUM_STAGES];
    std::string stage_name[BAZ_MUSIC_NUM_STAGES];
    char scan_names[4][64] = {{0}, {0}, {0}, {0}};   // baz_music_stage_name(SCAN) by scan_kind, written once by baz_music_create
    int scan_kind = -1;     // the scan kernel the LAST launch took (ScanKind; -1: none yet): only baz_music_stage_name reads it
    char hip_err[256] = {0};
    // Opt-in forward-backward averaging / spatial smoothing (baz_music_set_smoothing; NOT reference behaviour).  While `inner` is
    // set, every process* call re-stacks its items (smoothing_kernels.hip.h) into `dY` and runs them through `inner`, a context of
    // shape (ms, n, ms K', res) on the first ms columns of the table, launching on this context's stream.  Null: off -- none of the
    // mode's code runs and every other member keeps the reference's behaviour.  Changed under `tab_mtx` + `mtx`.
    //
    // The record is "a front-end with an inner context": the opt-in beamspace mode (baz_music_set_beamspace; beamspace_kernels.hip.h,
    // DESIGN.md 8k) is the same construction with a projection kernel where the gather is (kind == FRONT_BEAMSPACE: ms = B beams,
    // Kp = K, the inner context of shape (B, n, B K, res) on the table T^H a).  The two kinds exclude each other; what every forwarder
    // below does for `inner` serves both.
    //
    // The opt-in wideband (subband) mode (baz_music_set_subbands; subband_kernels.hip.h) is a front-end that drives S inner
    // contexts instead of one (kind == FRONT_SUBBAND): `inner` is subband 0, `sb_more` holds subbands 1 .. S-1, each of shape
    // (m, n, m K / F, res) on its own table; ms = m and Kp = S K / F, so that Kp ms is the size of a channelised item as it is for
    // the two other kinds.  The forwarders that serve `inner` serve every subband (each_inner); the pickers run on this context.
    enum { FRONT_SMOOTHING = 0, FRONT_BEAMSPACE = 1, FRONT_SUBBAND = 2 };
    struct Smoothing {
        baz_music_ctx* inner = nullptr;
        int kind = FRONT_SMOOTHING;              // which front-end feeds `inner` (meaningful while it is set)
        int bs_norm = 0;                         // beamspace: rows of the table T^H a scaled to unit norm
        std::vector<double> bs_T;                // beamspace: T as given (m x B complex128), for get_beamspace and retunes
        DevBuf<double2> dTc;                     // beamspace: conj(T), [m][B], what beamspace_kernel reads
        std::vector<baz_music_ctx*> sb_more;     // subband: the inner contexts of subbands 1 .. S-1
        uint32_t sb_F = 0, sb_S = 0;             // subband: block length, used subbands
        int sb_combine = 0;                      // subband: BAZ_MUSIC_SUBBAND_HARMONIC / _ARITHMETIC
        std::vector<uint32_t> sb_bins;           // subband: the DFT indices k_s as given
        DevBuf<double2> dW;                      // subband: the twiddles W, [S][F], what subband_kernel reads
        DevBuf<float> dPs;                       // subband: the chunk's S private spectra, [s][item][bin]
        DevBuf<float> dRow;                      // subband: the chunk's combined rows while port 2 is not wired
        uint32_t ms = 0, L = 1, Kp = 0;          // subarray size, subarrays, columns of a re-stacked item
        int fb = 0;
        bazsmooth::Perm perm = {};
        DevBuf<float2> dY;                       // re-stacked chunk (BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES)
        DevBuf<float> dX;                        // host path: the chunk's input ...
        DevBuf<float> dAl;                       // ... its ang | lvl ...
        DevBuf<float> dSpec;                     // ... and its spectrum on the device
    } sm;
};

namespace {

int hip_fail(baz_music_ctx* c, hipError_t e, const char* what)
{
    if (c) snprintf(c->hip_err, sizeof(c->hip_err), "%s: %s", what, hipGetErrorString(e));
    (void)hipGetLastError();   // the runtime's per-thread "last error" is sticky: do not let the next call find this one
    return BAZ_MUSIC_E_HIP;
}

#define HIP_TRY(ctx, call)                                         \
    do {                                                           \
        hipError_t e__ = (call);                                   \
        if (e__ != hipSuccess) return hip_fail((ctx), e__, #call); \
    } while (0)

// F[bin][i*m+j]: i==j |a_i|^2 ; i<j Re(conj(a_i) a_j) ; i>j Im(conj(a_j) a_i)  (pair (j,i), j<i).
// The fp32 table entries are widened exactly (.cc:110-112); the products are fp64.
void build_F(const float* table_ri, uint32_t m, uint32_t res, std::vector<double>& F)
{
    const size_t mm = (size_t)m * m;
    F.assign((size_t)res * mm, 0.0);
    for (uint32_t s = 0; s < res; ++s) {
        const float* a = table_ri + (size_t)s * m * 2;
        double* f = F.data() + (size_t)s * mm;
        for (uint32_t i = 0; i < m; ++i) {
            const double air = a[2 * i], aii = a[2 * i + 1];
            f[i * m + i] = air * air + aii * aii;
            for (uint32_t j = i + 1; j < m; ++j) {
                const double ajr = a[2 * j], aji = a[2 * j + 1];
                // conj(a_i) a_j = (air - i aii)(ajr + i aji)
                f[i * m + j] = air * ajr + aii * aji;
                f[j * m + i] = air * aji - aii * ajr;
            }
        }
    }
}

// MFMA B-operand image of the table (scan_mfma_kernel): FB[step][c2][lane] (double2), c2 = 2*s + (t>>1),
// component t&1, lane = (g = lane>>4, c = lane&15):
//     value = F[bin = 64*step + 4*c + t][e = 4*s + g]          (0 for the K padding e >= m*m)
// i.e. tile t of a 64-bin step carries the bins 4c + t in its columns, so that a lane's accumulator
// registers of the 4 tiles are 4 consecutive bins.  step runs from -1 to `steps` inclusive (array index step + 1):
// the scan's row classes read windows shifted by up to 60 bins.  Bins outside [0, res) get a huge
// diagonal: d = BIG * trace(Q) = BIG * (m - n), finite, never stored, never among the top n.
void build_FB(const std::vector<double>& F, uint32_t m, uint32_t res, uint32_t steps, std::vector<double>& FB)
{
    const uint32_t mm = m * m;
    const uint32_t ks = (mm + 3) / 4;
    const double BIG = 1e300;
    FB.assign((size_t)(steps + 2) * 2 * ks * 64 * 2, 0.0);
    for (uint32_t sti = 0; sti < steps + 2; ++sti)
        for (uint32_t s = 0; s < ks; ++s)
            for (uint32_t t = 0; t < 4; ++t)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t g = lane >> 4, c = lane & 15;
                    const int64_t bin = 64 * ((int64_t)sti - 1) + 4 * c + t;
                    const uint32_t e = 4 * s + g;
                    double v = 0.0;
                    if (e < mm) {
                        if (bin >= 0 && bin < (int64_t)res) v = F[(size_t)bin * mm + e];
                        else v = ((e / m) == (e % m)) ? BIG : 0.0;
                    }
                    FB[(((size_t)sti * 2 * ks + 2 * s + (t >> 1)) * 64 + lane) * 2 + (t & 1)] = v;
                }
}

// The raw table in the same B-operand order, for the literal form ||G^H a||^2 of near-null tiles (literal_tile):
// K dimension = the 2m real coordinates (re a_0, im a_0, re a_1, ...), fp32 entries widened exactly (.cc:110-112):
//     TB[step][2*s + (t>>1)][lane].{x,y}[t&1] = (e & 1 ? imag : real)(table[bin = 64*step + 4*c + t][e >> 1]),  e = 4*s + g
// zero outside [0, res) (those bins keep their projector value) and for the K padding e >= 2m.
void build_TB(const float* table_ri, uint32_t m, uint32_t res, uint32_t steps, std::vector<double>& TB)
{
    const uint32_t ks2 = (2 * m + 3) / 4;
    TB.assign((size_t)(steps + 2) * 2 * ks2 * 64 * 2, 0.0);
    for (uint32_t sti = 0; sti < steps + 2; ++sti)
        for (uint32_t s = 0; s < ks2; ++s)
            for (uint32_t t = 0; t < 4; ++t)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t g = lane >> 4, c = lane & 15;
                    const int64_t bin = 64 * ((int64_t)sti - 1) + 4 * c + t;
                    const uint32_t e = 4 * s + g;
                    double v = 0.0;
                    if (e < 2 * m && bin >= 0 && bin < (int64_t)res) v = (double)table_ri[((size_t)bin * m + (e >> 1)) * 2 + (e & 1)];
                    TB[(((size_t)sti * 2 * ks2 + 2 * s + (t >> 1)) * 64 + lane) * 2 + (t & 1)] = v;
                }
}

uint32_t round_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }

using baztab::f16_bits;
using baztab::f16_value;

// Table images of the coarse-gated scan (scan_coarse_kernel): the C array (1,024 B per 16-bin tile) followed by the X
// array (2,048 B per tile):
//   C    Fh then Fl, each 32 entries x 8 f16: entry (gb, c), j < 8 -> piece[bin = 16 tile + c][e = 8 gb + j]
//        (lane (g, c) of the K = 32 B operand [F | F] reads entry (g & 1, c))
//   X    k-step pair p, lane (g, c), component s & 1: F[bin][e = 4 s + g], s = 2 p + (s & 1)   (fp64 B operand)
// Fs = F * FS, Fh = f16(Fs), Fl = f16(Fs - Fh); bins outside the table: a huge diagonal (never selected), like build_FB.
// Returns false when the table's scale cannot be represented (the full scan is used then).
// The coarse form's scales and thresholds from max|F| (shared by the device builders and the host checker); false when the
// table's scale cannot be represented.
bool coarse_params_from(double fmax, uint32_t m, CoarseParams& cp, double& FS)
{
    if (!(fmax > 0.0) || !std::isfinite(fmax)) return false;
    int ex = 0;
    (void)std::frexp(fmax, &ex);                    // fmax = f * 2^ex, f in [0.5, 1)
    const int fs_exp = 14 - ex;                     // fmax * 2^fs_exp in [2^13, 2^14)
    if (fs_exp < -90 || fs_exp > 90) return false;  // SC must stay a comfortable float
    FS = std::ldexp(1.0, fs_exp);
    const double SC = 1024.0 * FS;
    cp.sc = SC;
    cp.fmax = fmax;
    const double nga = (double)cs_ng((int)m);             // the allowance E = nga 2^-16 (S + D)
    cp.sc_up = std::nextafter((float)(SC * (1.0 + nga * 0x1p-16) * (1.0 + 0x1p-20)), INFINITY);
    cp.es_factor = std::nextafter((float)(nga * 0x1p-16 * fmax * SC), INFINITY);
    return true;
}

bool build_coarse_image(const std::vector<double>& F, uint32_t m, uint32_t res, uint32_t tiles, std::vector<uint8_t>& img,
                        CoarseParams& cp)
{
    const uint32_t mm = m * m;
    double fmax = 0.0;
    for (double v : F) {
        if (!std::isfinite(v)) return false;
        fmax = std::max(fmax, std::fabs(v));
    }
    double FS = 0.0;
    if (!coarse_params_from(fmax, m, cp, FS)) return false;
    const uint32_t ng = (uint32_t)cs_groups((int)m);      // groups of 16 terms (fp64 operand)
    const bool wide = m > 4;                              // coarse operands in groups of 32 terms, Fh and Fl 1 KiB each
    const size_t cbytes = (size_t)cs_c_units((int)m) * 16, xbytes = (size_t)ng * CS_X_UNITS * 16;
    // [C of every tile and of one more (the kernel stages the first tile of the NEXT phase with every phase)][X of every tile]
    img.assign((size_t)(tiles + 1) * cbytes + (size_t)tiles * xbytes, 0);
    for (uint32_t t = 0; t <= tiles; ++t) {
        uint8_t* T = img.data() + (size_t)t * cbytes;
        std::vector<double> xpad(256 * ng);
        double* X = (t < tiles) ? reinterpret_cast<double*>(img.data() + (size_t)(tiles + 1) * cbytes + (size_t)t * xbytes) : xpad.data();
        for (uint32_t c = 0; c < 16; ++c) {
            const uint32_t bin = 16 * t + c;
            for (uint32_t e = 0; e < 16 * ng; ++e) {
                if (wide && e >= 32u * (uint32_t)cs_groups32((int)m)) continue;
                uint16_t* fh = reinterpret_cast<uint16_t*>(T + (wide ? (size_t)(e >> 5) * 2048 : 0));          // group: Fh then Fl
                uint16_t* fl = reinterpret_cast<uint16_t*>(T + (wide ? (size_t)(e >> 5) * 2048 + 1024 : 512));
                uint16_t hi = 0, lo = 0;
                if (e < mm) {
                    if (bin >= res) hi = ((e / m) == (e % m)) ? f16_bits(32768.0f) : 0;
                    else {
                        const float fs = (float)(F[(size_t)bin * mm + e] * FS);
                        hi = f16_bits(fs);
                        lo = f16_bits(fs - f16_value(hi));
                    }
                }
                const uint32_t gb = wide ? ((e >> 3) & 3u) : (e >> 3), j = e & 7u;       // entry (gb, c), j: k = 8 gb + j
                fh[(gb * 16 + c) * 8 + j] = hi;
                fl[(gb * 16 + c) * 8 + j] = lo;
            }
            for (uint32_t g = 0; g < 4; ++g)
                for (uint32_t sidx = 0; sidx < 4 * ng; ++sidx) {
                    const uint32_t e = 4 * sidx + g, lane = g * 16 + c;
                    double v = 0.0;
                    if (e < mm) v = (bin < res) ? F[(size_t)bin * mm + e] : (((e / m) == (e % m)) ? 1e300 : 0.0);
                    X[(sidx >> 1) * 128 + lane * 2 + (sidx & 1)] = v;
                }
        }
    }
    return true;
}


// Digit images of the table for the int8-matrix-core scan (scan_i8_kernels.hip.h): Fi = rint(F 2^54 / Fscale) cut into ND = 7
// balanced base-256 digits, most significant first (digits 1.. in [-128, 127], the first what is left: |.| <= 65), laid out as
// B operands of v_mfma_i32_16x16x64_i8 -- the five leading digits in `img` (staged through LDS by every tile), digits 5 and 6
// behind them (read from L2 by the tiles that refine):
//     img [(((st*4 + t)*NKB + kb)*5 + s)*1024 + lane*16 + j]          = digit s     of Fi[bin = 64 st + 4 c + t][e = 64 kb + 16 g + j]
//     img2[(((st*4 + t)*NKB + kb)*2 + s)*1024 + lane*16 + j]          = digit 5 + s   (img2 = img + i8_image_bytes5)
// (lane = 16 g + c; 0 for e >= m^2 and for bins outside the table, which the kernel gives a huge d).  Fills the kernel's
// parameters.  false: table not finite / all zero / scale out of range (the fp64 scan runs then).
constexpr size_t I8_IMAGE_LIMIT = (size_t)384 << 20;
size_t i8_image_bytes5(uint32_t m, uint32_t steps) { return (size_t)steps * 4 * i8_nkb((int)m) * I8_NS * 1024; }
size_t i8_image_bytes(uint32_t m, uint32_t steps) { return (size_t)steps * 4 * i8_nkb((int)m) * I8_ND * 1024; }

// The int8 forms' fixed-point scale, level weights and a-priori bounds from max|F| (shared by the device builders and the host
// checker); sf = the factor that turns F into its 2^54-scaled integer.  false: scale out of range.
bool i8_params_from(double fmax, uint32_t m, I8Params& ip, double& sf)
{
    const uint32_t mm = m * m;
    constexpr int NS = I8_NS, ND = I8_ND;
    if (!(fmax > 0.0) || !std::isfinite(fmax)) return false;
    int ex = 0;
    (void)std::frexp(fmax / I8_QMAX, &ex);          // fmax / QMAX = f 2^ex, f in [0.5, 1)  ->  fmax / 2^ex < QMAX
    // (float) wt[3] = Fscale 2^-36 must scale the bulk form's integer V in [1, 2^48) without leaving the normal float range
    if (ex < -88 || ex > 100) return false;
    const double fscale = std::ldexp(1.0, ex);
    const double sq = std::ldexp(1.0, 8 * ND - 2);
    sf = sq / fscale;
    for (int l = 0; l < ND; ++l) ip.wt[l] = std::ldexp(fscale, -12 - 8 * l);
    ip.sq = sq;
    // digits cut off + levels dropped + the low byte of the level-4 sum (scan_i8_kernels.hip.h, "Error bound")
    ip.e_bound = (double)mm * fscale * (double)NS * 1.01 * std::ldexp(1.0, 2 - 8 * NS) + fscale * std::ldexp(1.0, -12 - 8 * (NS - 2));
    ip.t_acc = ip.e_bound * (1.0 + 1.0 / I8_EPS);
    // first tier: four leading digits, levels 0 .. 3
    ip.e4_bound = (double)mm * fscale * (double)(NS - 1) * 1.01 * std::ldexp(1.0, 2 - 8 * (NS - 1));
    const double t4 = ip.e4_bound * (1.0 + 1.0 / I8_EPS);
    ip.t4_f = (float)t4;
    if ((double)ip.t4_f < t4) ip.t4_f = std::nextafterf(ip.t4_f, INFINITY);
    ip.ws_f = (float)ip.wt[NS - 2];
    ip.t_acc_f = (float)ip.t_acc;
    if ((double)ip.t_acc_f < ip.t_acc) ip.t_acc_f = std::nextafterf(ip.t_acc_f, INFINITY);
    // (VAL) the refined form against the fp64 form it is compared with: its own digits (7.07 2^-54 MM Fscale) plus the fp64
    // form's accumulation error, <= MM 2^-53 sum_e |q_e F_e| <= MM^2 2^-53 Fscale in the worst case
    ip.e_refined = (double)mm * fscale * std::ldexp(1.0, -54) * (7.07 + 2.0 * (double)mm);
    return true;
}

bool build_i8_image(const std::vector<double>& F, uint32_t m, uint32_t res, uint32_t steps, std::vector<uint8_t>& img,
                    I8Params& ip)
{
    const uint32_t mm = m * m, nkb = (uint32_t)i8_nkb((int)m);
    constexpr int NS = I8_NS, ND = I8_ND;
    double fmax = 0.0;
    for (double v : F) {
        if (!std::isfinite(v)) return false;
        fmax = std::max(fmax, std::fabs(v));
    }
    double sf = 0.0;
    if (!i8_params_from(fmax, m, ip, sf)) return false;
    img.assign(i8_image_bytes(m, steps), 0);
    uint8_t* img2 = img.data() + i8_image_bytes5(m, steps);
    for (uint32_t bin = 0; bin < res; ++bin) {
        const uint32_t st = bin >> 6, w = bin & 63u, c = w >> 2, t = w & 3u;
        for (uint32_t e = 0; e < mm; ++e) {
            const uint32_t kb = e >> 6, g = (e >> 4) & 3u, j = e & 15u;
            long long v = std::llrint(F[(size_t)bin * mm + e] * sf);          // |v| <= 2^54 (1 + 2^-10); the product is exact
            const size_t tile = (size_t)(st * 4 + t) * nkb + kb, in_lane = (size_t)(g * 16 + c) * 16 + j;
            for (int s = ND - 1; s >= 1; --s) {
                const long long h = (v + 128) >> 8;          // floor((v + 128) / 256)  (arithmetic shift)
                const uint8_t dg = (uint8_t)((v - h * 256) & 255);
                if (s >= NS) img2[(tile * (ND - NS) + (size_t)(s - NS)) * 1024 + in_lane] = dg;
                else img[(tile * NS + (size_t)s) * 1024 + in_lane] = dg;
                v = h;
            }
            img[(tile * NS) * 1024 + in_lane] = (uint8_t)(v & 255);
        }
    }
    return true;
}

#ifdef BAZ_MUSIC_LAB
// Level-packed digit operands for 2 .. 4 antennas (scan_i8p_kernels.hip.h), host checker of baztab::build_i8p_kernel:
//     B [((st + 1) * 4 + t) * 64 + 16 s + c][j]  = digit s (0 .. 3) of Fi[bin = 64 st + 4 c + t][e = j]       (16 bytes per entry)
//     B'[ ...                     16 s + c][j]  = digit 4 + s (s = 0 .. 2), slot 3 zero;  B' follows B (i8p_operand_units each)
bool build_i8p_image(const std::vector<double>& F, uint32_t m, uint32_t res, uint32_t steps, std::vector<uint8_t>& img, I8Params& ip)
{
    const uint32_t mm = m * m;
    constexpr int ND = I8_ND;
    double fmax = 0.0;
    for (double v : F) {
        if (!std::isfinite(v)) return false;
        fmax = std::max(fmax, std::fabs(v));
    }
    double sf = 0.0;
    if (!i8_params_from(fmax, m, ip, sf)) return false;
    img.assign(i8p_image_bytes(steps), 0);
    uint8_t* img2 = img.data() + i8p_operand_units(steps) * 16;
    for (uint32_t bin = 0; bin < res; ++bin) {
        const uint32_t st = bin >> 6, w = bin & 63u, c = w >> 2, t = w & 3u;
        for (uint32_t e = 0; e < mm; ++e) {
            long long v = std::llrint(F[(size_t)bin * mm + e] * sf);
            const size_t unit = ((size_t)(st + 1) * 4 + t) * 64 + c;
            int dgs[ND];
            for (int s = ND - 1; s >= 1; --s) {
                const long long h = (v + 128) >> 8;
                dgs[s] = (int)((v - h * 256) & 255);
                v = h;
            }
            dgs[0] = (int)(v & 255);
            for (int s = 0; s < ND; ++s) {
                uint8_t* base = (s < 4) ? img.data() + (unit + (size_t)s * 16) * 16 : img2 + (unit + (size_t)(s - 4) * 16) * 16;
                base[e] = (uint8_t)dgs[s];
            }
        }
    }
    return true;
}
#endif

// the scan's short form (scan_mfma_kernel, SIG) needs fewer MFMAs than the projector GEMM
bool short_form_applies(uint32_t m, uint32_t n) { return (n == 2 && m >= 9 && m <= 16) || (n == 1 && m >= 6 && m <= 16); }
// the shapes that get a digit image of the table (alloc_table_set)
bool wants_i8_image(const baz_music_ctx* c)
{
    return !c->wide && c->m >= 6 && c->n <= 4 && i8_image_bytes(c->m, c->fb_steps) <= I8_IMAGE_LIMIT;
}
// The int8-matrix-core scan applies: 6 .. 16 antennas (row classes below, run-time-m kernels above), lists of <= 4 keys.
// (launch_scan_i8 / _i8p / _coarse hold `if constexpr` bounds equal to what i8_active / i8p_active / coarse_applies admit: widen both or get E_UNSUPPORTED)
bool i8_active(const baz_music_ctx* c)
{
    return c->i8_on && c->tab.i8_ok && c->tab.dIB && c->m >= 6 && c->m <= 16 && c->n <= 4 && !c->lab_variant;
}
// ... and its level-packed form for 2 .. 4 antennas (scan_i8p_kernels.hip.h), with the spectrum port: lab builds only
#ifdef BAZ_MUSIC_LAB
bool i8p_active(const baz_music_ctx* c)
{
    return c->i8_on && c->i8p_on && c->tab.i8_ok && c->tab.dIP && c->m <= 4 && c->n <= 4 && !c->lab_variant;
}
#else
constexpr bool i8p_active(const baz_music_ctx*) { return false; }
#endif
bool short_form_in_use(const baz_music_ctx* c)
{
    // (the integer form evaluates the projector form: the EVD must write its coefficients)
    return short_form_applies(c->m, c->n) && c->sig_scan && c->dSs && c->tab.dA2p && !c->lab_variant && !i8_active(c);
}

// The buffers of one workspace grow together, to `items` items (contents are not kept; n == 0: the shape has no such buffer):
// one drain where any of them exists, all released, then all allocated.
template <typename T> struct WorkBuf { DevBuf<T>& buf; size_t n; };
template <typename T> WorkBuf<T> sized(DevBuf<T>& buf, size_t n) { return {buf, n}; }
template <typename... T>
int regrow_workspace(baz_music_ctx* c, uint32_t& cap, uint32_t items, WorkBuf<T>... bufs)
{
    bazbuf::Once once(drain(c));
    hipError_t e = hipSuccess;
    (void)(... && ((e = bufs.buf.retire(once)) == hipSuccess));
    HIP_TRY(c, e);
    cap = 0;
    (void)(... && ((e = bufs.n ? bufs.buf.allocate(bufs.n) : hipSuccess) == hipSuccess));
    HIP_TRY(c, e);
    cap = items;
    return BAZ_MUSIC_OK;
}

// 17 .. 64 antennas (the run-time-m kernels): room for a pass of `items` items
int ensure_wide_workspace(baz_music_ctx* c, uint32_t items)
{
    if (items <= c->wide_cap) return BAZ_MUSIC_OK;
    const size_t mm = (size_t)c->m * c->m;
    return regrow_workspace(c, c->wide_cap, items, sized(c->dR, items * mm), sized(c->dGw, (size_t)items * (c->m - c->n) * c->m),
                            sized(c->dWS, (size_t)items * c->res), sized(c->dSw, (size_t)items * c->n * c->m), sized(c->dRedo, items));
}

// The workspace of the context's shape, for launches of up to `batch` items
int ensure_workspace(baz_music_ctx* c, uint32_t batch)
{
    if (c->wide) return ensure_wide_workspace(c, batch);
    if (batch <= c->cap) return BAZ_MUSIC_OK;
    const uint32_t cap = round_up(batch, 64);
    const size_t mm = (size_t)c->m * c->m;
    return regrow_workspace(c, c->cap, cap, sized(c->dR, cap * mm), sized(c->dQ, cap * mm), sized(c->dG, cap * mm * 2), sized(c->dRedo, cap),
                            sized(c->dSs, short_form_applies(c->m, c->n) ? (size_t)cap * 4 * c->n * c->m : 0));
}

struct ProfScope {
    baz_music_ctx* c;
    int stage;
    hipEvent_t stop = nullptr;
    ProfScope(baz_music_ctx* ctx, int st) : c(ctx), stage(st)
    {
        if (!c->profiling || (c->profiling == 2 && stage != BAZ_MUSIC_STAGE_SCAN)) return;
        StageProf& p = c->prof[stage];
        if (p.used + 2 > p.ev.size()) {
            for (int k = 0; k < 2; ++k) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) return;
                p.ev.push_back(e);
            }
        }
        (void)hipEventRecord(p.ev[p.used], c->stream);
        stop = p.ev[p.used + 1];
        p.used += 2;
    }
    ~ProfScope()
    {
        if (stop) (void)hipEventRecord(stop, c->stream);
    }
};

void prof_collect(baz_music_ctx* c)
{
    for (int s = 0; s < BAZ_MUSIC_NUM_STAGES; ++s) {
        StageProf& p = c->prof[s];
        for (size_t k = 0; k + 1 < p.used; k += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.ev[k], p.ev[k + 1]) == hipSuccess) {
                p.total_ms += ms;
                p.launches += 1;
            }
        }
        p.used = 0;
    }
}

// Grows one buffer to `need` elements (contents are not kept): the owner's regrow, drained on the context's stream.
template <typename Buf>
int grow(baz_music_ctx* c, Buf& buf, size_t need)
{
    HIP_TRY(c, buf.regrow(need, drain(c)));
    return BAZ_MUSIC_OK;
}

// ---- the opt-in modes' per-call side outputs (SideOut) --------------------------------------------------------------------------
int grow_bytes(baz_music_ctx* c, DevBuf<uint8_t>& p, size_t need) { return grow(c, p, (need + 255) / 256 * 256); }

// the four records of a context, each with whether its mode is on now
struct SideMode { SideOut* out; bool mode_on; };
std::array<SideMode, 4> side_modes(baz_music_ctx* c)
{
    return {{{&c->out_ord, c->order_mode != 0}, {&c->out_ref, c->refine_mode != 0}, {&c->out_pow, c->power_mode != 0}, {&c->out_beam, c->beam_mode != 0}}};
}

// room for a call of `items` items
int side_grow(baz_music_ctx* c, SideOut& s, uint32_t items)
{
    for (SideOut::Buf& b : s.buf)
        if (const int r = grow_bytes(c, b.p, (size_t)items * b.item_bytes)) return r;
    return BAZ_MUSIC_OK;
}

// Opens a process*() call of `items` items for the modes' readers: the counts / offsets / powers / beams of all its chunks land in
// their buffers in call order.  With the modes off this is nine stores.
int order_begin(baz_music_ctx* c, uint32_t items)
{
    c->call_items = items;
    for (const SideMode& md : side_modes(c)) {
        md.out->count = 0;
        md.out->on = md.mode_on;
        if (const int r = md.mode_on ? side_grow(c, *md.out, items) : BAZ_MUSIC_OK) return r;
    }
    return BAZ_MUSIC_OK;
}

// A launch sequence is REFUSED (BAZ_MUSIC_E_HIP, message in baz_music_last_hip_error) when a device pointer it is about to hand to a
// kernel -- or to offset -- is null: a bug of that kind must come back as an error code, never as a GPU memory fault that takes the
// process down (BENCH_r05: "Memory access fault ... on address 0x10000").  Host-side, a dozen compares per call.
int refuse_null(baz_music_ctx* c, const void* p, const char* name)
{
    if (p) return BAZ_MUSIC_OK;
    snprintf(c->hip_err, sizeof(c->hip_err), "internal: device pointer %s is null at launch (m=%u n=%u res=%u): launch refused", name, c->m, c->n, c->res);
    return BAZ_MUSIC_E_HIP;
}
#define BAZ_REQUIRE(c, ptr) do { if (const int rn__ = refuse_null((c), (c)->ptr, #ptr)) return rn__; } while (0)
#define BAZ_REQUIRE_TAB(c, ptr) do { if (const int rn__ = refuse_null((c), (c)->tab.ptr, #ptr)) return rn__; } while (0)

// A chunk of `batch` items under a mode that is on: refused unless the call was opened with the mode on (order_begin) and the chunk
// ends inside what the call was sized for.
int side_refuse(baz_music_ctx* c, const SideMode& md, uint32_t batch)
{
    if (!md.mode_on) return BAZ_MUSIC_OK;
    bool fits = md.out->on;
    for (const SideOut::Buf& b : md.out->buf)
        fits = fits && (!b.item_bytes || (b.p && ((size_t)md.out->count + batch) * b.item_bytes <= b.p.cap()));
    return fits ? BAZ_MUSIC_OK : refuse_null(c, nullptr, md.out->what);
}

// The first `count` units of the last call's buffer k -> out, `per_item` units to an item (so a unit is item_bytes / per_item bytes);
// returns how many there were.  After a call made with the mode off: the byte `fill` for every unit of its `off_items` items.
int side_read(baz_music_ctx* c, const SideOut& s, int k, void* out, uint32_t count, uint32_t per_item, int fill, uint32_t off_items)
{
    DeviceGuard guard(c->device);
    const size_t unit = s.buf[k].item_bytes / per_item;
    const uint32_t have = (uint32_t)std::min<uint64_t>(count, (uint64_t)(s.on ? s.count : off_items) * per_item);
    if (!s.on) {
        if (have) memset(out, fill, have * unit);
        return (int)have;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (have) HIP_TRY(c, hipMemcpy(out, s.buf[k].p, have * unit, hipMemcpyDeviceToHost));
    return (int)have;
}

// the ORDER kernels' extra arguments for an EVD launch over `batch` items
int order_args(baz_music_ctx* c, uint32_t batch, OrderArgs& oa)
{
    oa.ord = c->ord_cur;
    if (!oa.ord) {
        const int r = grow_bytes(c, c->dOrdTap, batch);
        if (r) return r;
        oa.ord = c->dOrdTap;
    }
    oa.crit = c->order_mode;
    oa.nsnap = (double)(c->order_nsnap ? c->order_nsnap : c->K);
    if (c->avg_window > 1) oa.nsnap *= c->avg_neff;      // averaging on: the effective snapshots of a full window
    return BAZ_MUSIC_OK;
}

// The `n` the scans hand to their literal form (rows = m - n noise eigenvectors per item).  Mode on: the uniform row count the
// ORDER epilogues pad with zero rows -- m from 5 antennas on, m - 1 below (all literal_tile carries there).
uint32_t scan_n(const baz_music_ctx* c) { return c->order_mode ? (c->m <= 4 ? 1u : 0u) : c->n; }

// ---- kernel dispatch -------------------------------------------------------------------

template <int M>
int launch_cov_t(baz_music_ctx* c, const float* d_in, uint32_t batch, double2* dR)
{
    if constexpr (M == 4) {
        if ((c->K % 256u) == 0 && !c->lab_cov_old) {   // dwordx4 stream + LDS transpose + 4x4x4 MFMA blocks
            // persistent waves, one workgroup per CU (see baz_music_create)
            const uint32_t blocks = std::min<uint32_t>((batch + 3) / 4, c->cov4_resident_blocks);
            hipLaunchKernelGGL(cov4_x4_kernel, dim3(blocks), dim3(256), 0, c->stream, d_in, dR, batch, c->K);
            HIP_TRY(c, hipGetLastError());
            return BAZ_MUSIC_OK;
        }
    }
    if constexpr (M <= 8) {    // one 16x16 Gram tile holds 16/(2m) items
        constexpr int IPT = 16 / (2 * M);
        const uint32_t ntiles = (batch + IPT - 1) / IPT;
        const uint32_t blocks = std::min<uint32_t>((ntiles + 3) / 4, 256u * 32u);
        hipLaunchKernelGGL((cov_mfma_kernel<M>), dim3(blocks), dim3(256), 0, c->stream, d_in, dR, batch, c->K);
    } else {                   // 2x2 tiles per item
        const uint32_t blocks = std::min<uint32_t>((batch + 3) / 4, 256u * 32u);
        hipLaunchKernelGGL((cov_mfma2_kernel<M>), dim3(blocks), dim3(256), 0, c->stream, d_in, dR, batch, c->K);
    }
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

#ifdef BAZ_MUSIC_QUICK      // lab: a library that only knows m = 4, 8, 16 (a sixth of the compile time; tests/lab iterations)
#define BAZ_M_CASES(CALL) case 4: return CALL(4); case 8: return CALL(8); case 16: return CALL(16);
#else
#define BAZ_M_CASES(CALL)                                                                          \
    case 2: return CALL(2); case 3: return CALL(3); case 4: return CALL(4); case 5: return CALL(5); \
    case 6: return CALL(6); case 7: return CALL(7); case 8: return CALL(8); case 9: return CALL(9); \
    case 10: return CALL(10); case 11: return CALL(11); case 12: return CALL(12); case 13: return CALL(13); \
    case 14: return CALL(14); case 15: return CALL(15); case 16: return CALL(16);
#endif

// 17 .. 64 antennas: the run-time-m covariance kernels of music_wide_kernels.hip.h
int launch_cov_wide(baz_music_ctx* c, const float* d_in, uint32_t nb, double2* dR)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_COV);
    if (c->wide_cov_mfma && c->m > 32) {   // 33 <= m <= 64: one wave per (item, pair of 16-antenna blocks)
        const uint32_t nblk = (c->m + 15u) / 16u, npairs = nblk * (nblk + 1u) / 2u;
        const uint64_t tasks = (uint64_t)nb * npairs;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((tasks + 3) / 4, 8u * (uint64_t)c->wide_cov_blocks);
        hipLaunchKernelGGL(bazwide::cov_wide_pairs_kernel, dim3(blocks), dim3(256), 0, c->stream,
                           reinterpret_cast<const float2*>(d_in), dR, nb, c->m, c->K, npairs);
    } else if (c->wide_cov_mfma) {  // 17 <= m <= 32: one wave per item on the fp64 matrix core, 2 workgroups per CU at most
        const uint32_t blocks = std::min<uint32_t>((nb + 3) / 4, c->wide_cov_blocks);
        hipLaunchKernelGGL(bazwide::cov_wide_mfma_kernel, dim3(blocks), dim3(256), 0, c->stream,
                           reinterpret_cast<const float2*>(d_in), dR, nb, c->m, c->K);
    } else {
        hipLaunchKernelGGL(bazwide::cov_wide_kernel, dim3(nb), dim3(bazwide::WB), (size_t)bazwide::COV_TC * c->m * sizeof(float2),
                           c->stream, reinterpret_cast<const float2*>(d_in), dR, c->m, c->K);
    }
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// The plain covariances of `batch` items -> dR, by the kernel of the context's shape
int launch_cov(baz_music_ctx* c, const float* d_in, uint32_t batch, double2* dR)
{
    if (c->wide) return launch_cov_wide(c, d_in, batch, dR);
    ProfScope ps(c, BAZ_MUSIC_STAGE_COV);
#define BAZ_CALL(MV) launch_cov_t<MV>(c, d_in, batch, dR)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

template <int M>
int launch_evd_t(baz_music_ctx* c, const double2* dR, uint32_t batch, double* dQ, uint32_t qstride, double* dG)
{
    if (c->order_mode) {      // opt-in emitter count: the ORDER twins; every item takes the Jacobi (evd_sub_kernel has no noise eigenvalues)
        OrderArgs oa;
        const int ro = order_args(c, batch, oa);
        if (ro) return ro;
        if constexpr (M <= 4) {
            hipLaunchKernelGGL((evd_proj_order_kernel<M>), dim3((batch + 63) / 64), dim3(64), 0, c->stream, dR, dQ, batch, c->n, qstride, dG, oa);
        } else {
            constexpr uint32_t IPW = 64 / M;
            double* ss = (dQ == c->dQ && batch <= c->cap) ? c->dSs : nullptr;
            double* const dQw = (ss && short_form_in_use(c)) ? nullptr : dQ;
            hipLaunchKernelGGL((evd_proj_lds_order_kernel<M>), dim3((batch + IPW - 1) / IPW), dim3(64), 0, c->stream, dR, dQw, batch, c->n,
                               qstride, dG, ss, oa);
        }
        HIP_TRY(c, hipGetLastError());
        return BAZ_MUSIC_OK;
    }
    if constexpr (M <= 4) {   // one item per lane, register resident
        const uint32_t blocks = (batch + 63) / 64;
        hipLaunchKernelGGL((evd_proj_kernel<M>), dim3(blocks), dim3(64), 0, c->stream, dR, dQ, batch, c->n, qstride, dG);
    } else {                  // M lanes per item, matrices in LDS
        constexpr uint32_t IPW = 64 / M;
        const uint32_t blocks = (batch + IPW - 1) / IPW;
        // few emitters: the signal subspace by orthogonal iteration (evd_sub_kernel), then the Jacobi only for the items
        // it hands back (gap too small, zero / non-finite R)
        // (the scan's short form wants the signal vectors of the product's own workspace only: dQ == c->dQ)
        double* ss = (dQ == c->dQ && batch <= c->cap) ? c->dSs : nullptr;
        // ... and when that scan runs, nothing reads the projector coefficients: they are not written either
        double* const dQw = (ss && short_form_in_use(c)) ? nullptr : dQ;
        const uint8_t* only = nullptr;
        if (c->sub_evd && c->n <= 4 && 2 * c->n <= (uint32_t)M && c->dRedo && batch <= c->cap) {
            constexpr uint32_t GS = M <= 8 ? 8 : 16, IPS = 64 / GS;
            const uint32_t sblocks = (batch + IPS - 1) / IPS;
            if (c->n == 1) hipLaunchKernelGGL((evd_sub_kernel<M, 1>), dim3(sblocks), dim3(64), 0, c->stream, dR, dQw, batch, qstride, dG, c->dRedo, ss);
            else if (c->n == 2) hipLaunchKernelGGL((evd_sub_kernel<M, 2>), dim3(sblocks), dim3(64), 0, c->stream, dR, dQw, batch, qstride, dG, c->dRedo, ss);
            else if (c->n == 3) { if constexpr (M >= 6) hipLaunchKernelGGL((evd_sub_kernel<M, 3>), dim3(sblocks), dim3(64), 0, c->stream, dR, dQw, batch, qstride, dG, c->dRedo); }
            else { if constexpr (M >= 8) hipLaunchKernelGGL((evd_sub_kernel<M, 4>), dim3(sblocks), dim3(64), 0, c->stream, dR, dQw, batch, qstride, dG, c->dRedo); }
            HIP_TRY(c, hipGetLastError());
            only = c->dRedo;
        }
        hipLaunchKernelGGL((evd_proj_lds_kernel<M>), dim3(blocks), dim3(64), 0, c->stream, dR, dQw, batch, c->n, qstride, dG, only, ss);
    }
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// m = 4, K % 256 == 0: covariance and EVD in one kernel (cov4_evd_kernel); d_R_dbg optionally receives R (test tap)
int launch_covevd(baz_music_ctx* c, const float* d_in, uint32_t batch, double* dQ, uint32_t qstride, double* dG,
                  double2* d_R_dbg = nullptr)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_COV);
    // items per wave task: 64 where that still makes >= 256 tasks (one per CU), else 32 / 16 -- a small batch needs more waves reading than
    // lanes rotating (a host-fed 1,024-item call read its input over PCIe at 40 GB/s with 16 waves; cov4_evd_kernel)
    const uint32_t ti = c->covevd_task_items ? (uint32_t)c->covevd_task_items : (batch >= 16384u ? 64u : (batch >= 8192u ? 32u : 16u));
    const uint32_t ntasks = (batch + ti - 1) / ti;
    const uint32_t blocks = std::min<uint32_t>((ntasks + 3) / 4, c->covevd_blocks);
    if (c->order_mode) {
        OrderArgs oa;
        const int ro = order_args(c, batch, oa);
        if (ro) return ro;
        hipLaunchKernelGGL(cov4_evd_order_kernel, dim3(blocks), dim3(256), 0, c->stream, d_in, dQ, dG, d_R_dbg, batch, c->K, c->n,
                           qstride, ti, c->covevd_park, oa);
        HIP_TRY(c, hipGetLastError());
        return BAZ_MUSIC_OK;
    }
    hipLaunchKernelGGL(cov4_evd_kernel, dim3(blocks), dim3(256), 0, c->stream, d_in, dQ, dG, d_R_dbg, batch, c->K, c->n,
                       qstride, ti, c->covevd_park);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

int launch_evd(baz_music_ctx* c, const double2* dR, uint32_t batch, double* dQ, uint32_t qstride, double* dG)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_EVD);
#define BAZ_CALL(MV) launch_evd_t<MV>(c, dR, batch, dQ, qstride, dG)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// ---- opt-in covariance averaging across the items of the stream (average_kernels.hip.h) ------------------------------------------
// The mode's buffers: both history buffers for a window of W items (zero-filled on the launch stream when they are allocated, so
// slots in front of the stream's start hold defined values; they are never taps) and, for `items` > 0, the averaged covariances.
// Growing a history buffer loses its contents: only a change of W does that, and it resets the history anyway.
int ensure_average(baz_music_ctx* c, uint32_t W, uint32_t items)
{
    const size_t E = (size_t)c->m * c->m, need = (size_t)(W - 1) * E;
    for (int k = 0; k < 2; ++k) {
        if (need <= c->dAvgHist[k].cap()) continue;
        const int r = grow(c, c->dAvgHist[k], need);
        if (r) return r;
        HIP_TRY(c, hipMemsetAsync(c->dAvgHist[k], 0, need * sizeof(double2), c->stream));
    }
    return items ? grow(c, c->dRavg, (size_t)round_up(items, 64) * E) : BAZ_MUSIC_OK;
}

// The averaging stage of one launch sequence: dRout[i] = R-bar of item i of `batch` plain covariances dRin, then the history of the
// next launch (the other buffer), then the host's stream position.  The stream orders the two kernels behind the covariance
// kernel and in front of the EVD; the next launch's kernels read the new history behind this one's writes.
int launch_average(baz_music_ctx* c, const double2* dRin, uint32_t batch, double2* dRout)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_COV);
    const uint32_t E = c->m * c->m, W = c->avg_window;
    const double2* const Ho = c->dAvgHist[c->avg_parity];
    double2* const Hn = c->dAvgHist[c->avg_parity ^ 1];
    if (!Ho || !Hn || !dRin || !dRout || c->dAvgHist[0].cap() < (size_t)(W - 1) * E || c->dAvgHist[1].cap() < (size_t)(W - 1) * E)
        return refuse_null(c, nullptr, "dAvgHist / dRavg (ensure_average)");
    // items per lane: 8 up to a window of 8 (R is read at most 15/8 times), 16 beyond (79/16 times at W = 64)
    const uint32_t T = W <= 8 ? 8u : 16u;
    const uint64_t threads = (uint64_t)((batch + T - 1) / T) * E;
    const dim3 grid((unsigned)((threads + bazavg::AVG_THREADS - 1) / bazavg::AVG_THREADS));
    if (T == 8) hipLaunchKernelGGL((bazavg::average_kernel<8>), grid, dim3(bazavg::AVG_THREADS), 0, c->stream, dRin, Ho, dRout, c->avg_tab, batch, E, W, c->avg_hist);
    else hipLaunchKernelGGL((bazavg::average_kernel<16>), grid, dim3(bazavg::AVG_THREADS), 0, c->stream, dRin, Ho, dRout, c->avg_tab, batch, E, W, c->avg_hist);
    HIP_TRY(c, hipGetLastError());
    const uint32_t hthreads = (W - 1) * E;
    hipLaunchKernelGGL(bazavg::average_history_kernel, dim3((hthreads + bazavg::AVG_THREADS - 1) / bazavg::AVG_THREADS), dim3(bazavg::AVG_THREADS), 0,
                       c->stream, dRin, Ho, Hn, batch, E, W);
    HIP_TRY(c, hipGetLastError());
    c->avg_parity ^= 1;
    c->avg_hist = (uint32_t)std::min<uint64_t>((uint64_t)c->avg_hist + batch, W - 1);
    return BAZ_MUSIC_OK;
}

// ---- opt-in noise pre-whitening (whiten_kernels.hip.h) ------------------------------------------------------------------------------
// The covariance in force: what this launch sequence's EVD decomposes and what refinement's vectors, the power / beam kernels and the
// estimators' scan follow from -- R' where whitening is on, else the averaged covariances where averaging is on, else the plain ones.
double2* cov_in_force(const baz_music_ctx* c)
{
    if (c->tab.wh_on) return c->dRwh;
    return c->avg_window > 1 ? c->dRavg : c->dR;
}

// The stage's buffers for a launch of `items` items: R' and, on the 17 .. 64 antenna path, the pass between the two products.
int ensure_whiten(baz_music_ctx* c, uint32_t items, bool want_out)
{
    const size_t need = (size_t)round_up(items, 64) * c->m * c->m;
    int r = want_out ? grow(c, c->dRwh, need) : BAZ_MUSIC_OK;
    if (r == BAZ_MUSIC_OK && c->wide) r = grow(c, c->dWhT, need);
    return r;
}

template <int M>
int launch_whiten_t(baz_music_ctx* c, const double2* dRin, uint32_t batch, double2* dRout)
{
    constexpr uint32_t IPB = bazwhiten::WhitenGeom<M>::IPB;
    hipLaunchKernelGGL((bazwhiten::whiten_kernel<M>), dim3((batch + IPB - 1) / IPB), dim3(bazwhiten::WhitenGeom<M>::THREADS), 0, c->stream,
                       dRin, dRout, c->tab.dWh, batch);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// The whitening stage of one launch sequence: dRout[i] = W dRin[i] W^H with the W of the table set in force, between the covariance
// (or the averaging stage) and the EVD.  ensure_whiten() came first.
int launch_whiten(baz_music_ctx* c, const double2* dRin, uint32_t batch, double2* dRout)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_COV);
    if (const int rn = refuse_null(c, c->tab.dWh, "dWh")) return rn;
    if (!dRin || !dRout) return refuse_null(c, nullptr, "dRwh (ensure_whiten)");
    if (c->wide) {
        if (c->dWhT.cap() < (size_t)batch * c->m * c->m) return refuse_null(c, nullptr, "dWhT (ensure_whiten)");
        const size_t lds = (size_t)c->m * (c->m + 1) / 2 * sizeof(double2);
        hipLaunchKernelGGL((bazwhiten::whiten_wide_kernel<true>), dim3(batch), dim3(bazwhiten::WHITEN_THREADS), lds, c->stream, dRin, c->dWhT,
                           c->tab.dWh, c->m);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL((bazwhiten::whiten_wide_kernel<false>), dim3(batch), dim3(bazwhiten::WHITEN_THREADS), lds, c->stream, c->dWhT, dRout,
                           c->tab.dWh, c->m);
        HIP_TRY(c, hipGetLastError());
        return BAZ_MUSIC_OK;
    }
#define BAZ_CALL(MV) launch_whiten_t<MV>(c, dRin, batch, dRout)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// The buffers of the two opt-in stages between covariance and EVD, for launches of up to `items` items
int ensure_cov_stages(baz_music_ctx* c, uint32_t items)
{
    const int r = c->avg_window > 1 ? ensure_average(c, c->avg_window, items) : BAZ_MUSIC_OK;
    return (r == BAZ_MUSIC_OK && c->tab.wh_on) ? ensure_whiten(c, items, true) : r;
}

// The covariance chain of every launch sequence: the plain covariances of `batch` items into c->dR, their averages where averaging is on
// (the history runs from launch to launch), either whitened where whitening is on.  The result lies where cov_in_force() points.
// ensure_cov_stages() came first.
int launch_cov_stages(baz_music_ctx* c, const float* in, uint32_t batch)
{
    const double2* R = c->dR;
    int r = launch_cov(c, in, batch, c->dR);
    if (r == BAZ_MUSIC_OK && c->avg_window > 1) {
        r = launch_average(c, R, batch, c->dRavg);
        R = c->dRavg;
    }
    if (r == BAZ_MUSIC_OK && c->tab.wh_on) r = launch_whiten(c, R, batch, c->dRwh);
    return r;
}

// Covariance + EVD of `batch` items: the projector coefficients into `dQ` (the workspace's c->dQ, or a debug tap's own buffer), the
// noise eigenvectors into c->dG.  The fused kernel where it applies, else two kernels through c->dR.  ensure_workspace() came first.
int launch_frontend(baz_music_ctx* c, const void* d_in, uint32_t batch, double* dQ, uint32_t qstride)
{
    const float* in = static_cast<const float*>(d_in);
    if (c->avg_window > 1 || c->tab.wh_on) {   // opt-in averaging / whitening: always two kernels through c->dR, the stages between them
        // (ensure_average() came first; R' is sized here as well: a debug tap comes without a sequence in front)
        int ra = c->tab.wh_on ? ensure_whiten(c, batch, true) : BAZ_MUSIC_OK;
        if (ra == BAZ_MUSIC_OK) ra = launch_cov_stages(c, in, batch);
        return ra ? ra : launch_evd(c, cov_in_force(c), batch, dQ, qstride, c->dG);
    }
    // (power / beam mode on: the fused kernel also stores its R, the tap baz_music_debug_cov uses -- same kernel, same Q and G bits)
    if (c->fused_covevd) return launch_covevd(c, in, batch, dQ, qstride, c->dG, (c->power_mode || c->beam_mode) ? c->dR : nullptr);
    const int r = launch_cov(c, in, batch, c->dR);
    return r ? r : launch_evd(c, c->dR, batch, dQ, qstride, c->dG);
}

// ---- launch geometry of the scan kernels, and beside each the candidate keys it can ask for -----------------------------------------
// Every bin range of every item yields topn_list_len(n) candidate keys for topn_merge_kernel.  nb * nsplit(nb) is not monotonic in nb
// (nsplit = ceil(wanted / groups) while that stays under the kernel's cap), so a reservation for `batch` items is sized for the worst
// launch of ANY nb <= batch (*_cand_ranges): a smaller batch or the short tail chunk of baz_music_process never re-allocates mid-pipeline.
uint32_t topn_list_len(uint32_t n) { return n <= 2 ? 2u : (n <= 4 ? 4u : (n <= 8 ? 8u : 16u)); }
// tests / lab (BAZ_MUSIC_NSPLIT=k > 0): k bin ranges per item, as far as the kernel has that many
uint32_t forced_nsplit(int force_nsplit, uint32_t most) { return std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)force_nsplit, most)); }

// The fp64 scan (and the level-packed int8 scan of lab builds): rows are taken class by class (class k = items nclass*j + k, see the
// kernel's ROW CLASSES note), every class padded to a multiple of 64 rows (one block = 4 waves x 16 rows of ONE class), times
// `nsplit` ranges of 64-bin steps, chosen so that a launch has >= ~8 waves/SIMD worth of wave tasks even for small
// batches / long tables (config 3: 4,096 items x 36,000 bins).
struct ScanGeom { uint32_t groups, nsplit, blocks, rows_per_class; };
// Wave tasks wanted = 2 x the waves the chip holds at once (256 CUs x 4 SIMDs x 4): enough to balance the tail,
// and no more -- every extra range restarts the top-n lists (the gate fires until they fill), writes another
// candidate list per item and multiplies the row streams written at once: 262,144 cfg2 items ran the scan in 0.716 /
// 0.758 / 0.826 ms at 1 / 2 / 4 ranges (round 1 asked for 8 waves/SIMD worth = 32,768 tasks, i.e. 2 ranges there).
// From 9 antennas on the kernel holds 2 waves per SIMD (256 registers) and a task costs more to set up (the short form's
// 32 coefficient registers): ONE round of the 2,048 wave slots is best there -- 16 antennas, 3,600 bins: 16,384 items ran
// the scan in 0.358 / 0.278 / 0.294 / 0.321 ms at 1 / 2 / 4 / 8 ranges, 4,096 items in 0.093 / 0.088 / 0.095 / 0.107 ms at
// 4 / 8 / 16 / 32 (profiles/r03_bin_ranges_by_shape.txt; 5..8 antennas do not care between 2 and 8).
constexpr uint32_t SCAN_WANT_TASKS = 256u * 4u * 4u * 2u;      // up to 8 antennas; a quarter of it from 9 on
constexpr uint32_t SCAN_MAX_NSPLIT = 64;
ScanGeom scan_geometry(uint32_t batch, uint32_t nsteps, uint32_t nclass, int force_nsplit, uint32_t m)
{
    ScanGeom G;
    G.rows_per_class = round_up((batch + nclass - 1) / nclass, 64);
    G.groups = nclass * (G.rows_per_class / 16);
    const uint32_t live_groups = (batch + 15) / 16;
    const uint32_t want_tasks = (m >= 9) ? SCAN_WANT_TASKS / 4u : SCAN_WANT_TASKS;
    const uint32_t ns = (want_tasks + live_groups - 1) / live_groups;
    G.nsplit = std::max<uint32_t>(1u, std::min<uint32_t>(ns, std::min<uint32_t>(nsteps, SCAN_MAX_NSPLIT)));
    if (force_nsplit > 0) G.nsplit = forced_nsplit(force_nsplit, std::min<uint32_t>(nsteps, SCAN_MAX_NSPLIT));
    G.blocks = (G.groups / 4) * G.nsplit;
    return G;
}
// nb * nsplit(nb) < nb * (want_tasks / ceil(nb/16) + 1) <= 16 * want_tasks + nb, and <= nb * min(64, nsteps)
size_t scan_cand_ranges(const baz_music_ctx* c, uint32_t batch)
{
    const size_t cap_split = std::min<size_t>(SCAN_MAX_NSPLIT, std::max<uint32_t>(1u, c->fb_steps));
    const size_t exact = (size_t)batch * scan_geometry(batch, c->fb_steps, c->nclass, c->force_nsplit, c->m).nsplit;
    const size_t worst = std::min<size_t>((size_t)batch * cap_split, (size_t)16u * SCAN_WANT_TASKS + (size_t)batch);
    const size_t forced = c->force_nsplit > 0 ? (size_t)batch * forced_nsplit(c->force_nsplit, (uint32_t)cap_split) : 0;
    return std::max(std::max(exact, worst), std::max(forced, (size_t)batch));
}

// Bin ranges per item of scan_i8_kernel: its workgroups (4 waves x 16 items, one range of 64-bin steps) should fill the
// slots the chip holds at once -- `slots` = CUs x resident workgroups per CU -- a whole number of times: 16,384 config-3 items
// are 256 groups; 8 ranges made 2,048 workgroups for 768 slots, 2.67 rounds of which the last ran a third empty, where 3 ranges
// fill every slot exactly once (and restart the top-n lists 3 times instead of 8).  Up to 8 rounds are tried; the fewest
// rounds within 3 % of the best filling win.  Ranges of fewer than 4 steps are not made.
constexpr uint32_t I8_MAX_NSPLIT = 16, I8_MAX_ROUNDS = 8;
uint32_t i8_nsplit(uint32_t batch, uint32_t nsteps, uint32_t slots, int force_nsplit)
{
    const uint32_t groups = std::max<uint32_t>(1u, (batch + 63) / 64);
    const uint32_t cap = std::max<uint32_t>(1u, std::min<uint32_t>(I8_MAX_NSPLIT, nsteps / 4));
    if (force_nsplit > 0) return forced_nsplit(force_nsplit, std::min<uint32_t>(nsteps, SCAN_MAX_NSPLIT));
    uint32_t best = 1;
    double best_fill = 0.0;
    for (uint32_t r = 1; r <= I8_MAX_ROUNDS; ++r) {
        const uint32_t ns = std::max<uint32_t>(1u, std::min<uint32_t>(cap, (uint32_t)(((uint64_t)r * slots) / groups)));
        const uint64_t blocks = (uint64_t)groups * ns;
        const uint64_t rounds = (blocks + slots - 1) / slots;
        const double fill = (double)blocks / (double)(rounds * slots);
        if (fill > best_fill * 1.03) { best_fill = fill; best = ns; }
        if (ns == cap) break;
    }
    return best;
}
// nsplit <= r slots / ceil(nb / 64) with r <= I8_MAX_ROUNDS rounds of <= 4 x 256-CU slots, and <= I8_MAX_NSPLIT
size_t i8_cand_ranges(const baz_music_ctx* c, uint32_t batch)
{
    if (!c->tab.dIB) return 0;
    const size_t exact = (size_t)batch * (c->force_nsplit > 0 ? forced_nsplit(c->force_nsplit, SCAN_MAX_NSPLIT) : I8_MAX_NSPLIT);
    return std::max(exact, std::min<size_t>((size_t)batch * I8_MAX_NSPLIT, (size_t)64u * I8_MAX_ROUNDS * 4u * c->num_cus + (size_t)batch));
}

int ensure_candidates(baz_music_ctx* c, size_t entries) { return grow(c, c->dCand, entries); }

// The coarse-gated scan applies: spectrum port not wired, m <= 8, n <= 4, the table's scale representable.
bool coarse_applies(const baz_music_ctx* c)
{
    // (one emitter from 6 antennas on: the full scan is the SHORT form, a quarter of the projector GEMM's work, and the
    // gated scan's exact tiles are the projector form -- not the same bits; that case keeps the full scan)
    return c->coarse && c->tab.cs_ok && c->tab.dCS && c->m <= 8 && c->n <= 4 && !c->lab_variant && !short_form_applies(c->m, c->n);
}

constexpr int coarse_rg_wide(int m, int nmax) { return (cs_groups(m) == 4 && nmax > 2) ? 1 : 2; }   // (what the register file holds without spilling)
// its launch geometry: a workgroup = 4 waves x RG x 16 items; ranges of table phases so that small batches still fill the chip
constexpr uint32_t COARSE_WANT_BLOCKS = 1024, COARSE_MAX_NSPLIT = 16;
struct CoarseGeom { uint32_t groups, nsplit, nphases, tpp; };
CoarseGeom coarse_geometry(const baz_music_ctx* c, uint32_t batch)
{
    CoarseGeom G;
    // four row groups per wave where the lists fit the register file beside them (n <= 2), else two
    // (m >= 5: 2 .. 4 operand groups per tile -- two row groups while the register file holds them, else one)
    const uint32_t rg = (c->m > 4) ? (uint32_t)coarse_rg_wide((int)c->m, c->n <= 2 ? 2 : 4)
                                   : ((c->coarse_rg == 2 || c->n > 2) ? 2u : 4u);
    G.tpp = (rg <= 2) ? 4u : 8u;
    G.nphases = c->cs_tiles / G.tpp;
    G.groups = (batch + 64 * rg - 1) / (64 * rg);
    const uint32_t ns = (COARSE_WANT_BLOCKS + G.groups - 1) / G.groups;
    G.nsplit = std::max(1u, std::min(ns, std::min(G.nphases, COARSE_MAX_NSPLIT)));
    if (c->force_nsplit > 0) G.nsplit = forced_nsplit(c->force_nsplit, std::min(G.nphases, COARSE_MAX_NSPLIT));
    return G;
}
// nsplit = ceil(COARSE_WANT_BLOCKS / ceil(nb / (64 rg))) <= 16, rg <= 4 row groups per wave  ->  nb * nsplit <= 256 * WANT + nb
size_t coarse_cand_ranges(const baz_music_ctx* c, uint32_t batch)
{
    if (c->m > 8) return 0;
    const size_t exact = c->tab.dCS ? (size_t)batch * coarse_geometry(c, batch).nsplit : 0;
    return std::max(exact, std::min<size_t>((size_t)batch * COARSE_MAX_NSPLIT, (size_t)256u * COARSE_WANT_BLOCKS + (size_t)batch));
}

// the candidate buffer for launches of up to `batch` items: the largest of the kernels this context can take with either port wiring
int reserve_candidates(baz_music_ctx* c, uint32_t batch)
{
    const size_t ranges = std::max(scan_cand_ranges(c, batch), std::max(coarse_cand_ranges(c, batch), i8_cand_ranges(c, batch)));
    return ensure_candidates(c, ranges * topn_list_len(c->n));
}

// ---- sorting in front of the gated scan (sort_kernels.hip.h): LAB builds only --------------------------------------------------------
#ifdef BAZ_MUSIC_LAB
constexpr uint32_t SORT_MIN_BATCH = 4096;      // below this a launch is a handful of workgroups either way
constexpr double SORT_ON_RATE = 0.06;          // share of (row group, tile) pairs an UNSORTED call evaluated exactly above which sorting pays
constexpr uint32_t SORT_PROBE_EVERY = 64;      // while sorting: every so many calls one call unsorted, whose statistic decides anew

int ensure_sort_workspace(baz_music_ctx* c, uint32_t batch)
{
    if (c->sort_mode == 0) return BAZ_MUSIC_OK;                   // (nothing of the sorting exists unless it was asked for)
    if (!c->dFire) {
        HIP_TRY(c, c->dFire.allocate(2));
        HIP_TRY(c, hipMemsetAsync(c->dFire, 0, 2 * sizeof(unsigned long long), c->stream));
        HIP_TRY(c, c->hFire.allocate(4));
        std::memset(c->hFire, 0, 4 * sizeof(unsigned long long));
        HIP_TRY(c, hipHostGetDevicePointer((void**)&c->hFireDev, c->hFire, 0));
    }
    if (!c->tab.dKT) return BAZ_MUSIC_OK;
    if (!c->dHist) {
        HIP_TRY(c, c->dHist.allocate(bazsort::KEY_BUCKETS));
        HIP_TRY(c, c->dCursor.allocate(bazsort::KEY_BUCKETS));
        HIP_TRY(c, hipMemsetAsync(c->dHist, 0, bazsort::KEY_BUCKETS * sizeof(uint32_t), c->stream));
    }
    if (batch > c->sort_cap) {
        const uint32_t cap = round_up(batch, 4096);
        if (const int r = regrow_workspace(c, c->sort_cap, cap, sized(c->dKeys, cap), sized(c->dPerm, cap))) return r;
    }
    return BAZ_MUSIC_OK;
}

// Sort this call's items?  The gated scan's merge leaves, in page-locked memory, how many of its (row group, tile) pairs were evaluated exactly and
// whether that call was sorted; the answer of some EARLIER call is there when this one is launched (nothing waits for it).
//   * an unsorted call with a high share starts a trial (sorting on);
//   * a sorted call must bring the share clearly below the unsorted one (x 0.6), else sorting goes off again and is not tried for a while
//     (a small coherent batch cut into many bin ranges has a high share that no order improves);
//   * while sorting, every SORT_PROBE_EVERY-th call runs unsorted: a low share there (the stream turned coherent) switches it off.
// Up to 4 antennas (the rows' coefficients sit in registers; from 5 on the exact tiles fetch them from L2, where an index list costs gathers).
bool sort_decide(baz_music_ctx* c, uint32_t batch)
{
    if (batch < SORT_MIN_BATCH || !c->tab.dKT || !c->hFire || c->m > 4 || c->n > 2 || c->coarse_rg == 2 || c->coarse_lab) return false;
    if (c->sort_mode >= 0) return c->sort_mode != 0;
    ++c->sort_clock;
    const unsigned long long tag = static_cast<volatile unsigned long long*>(c->hFire)[2];
    if (tag != c->fire_seen) {
        c->fire_seen = tag;
        const unsigned long long fired = static_cast<volatile unsigned long long*>(c->hFire)[0];
        const unsigned long long walked = static_cast<volatile unsigned long long*>(c->hFire)[1];
        const double rate = walked ? (double)fired / (double)walked : 0.0;
        if (tag & 1ull) {                              // a sorted call
            if (c->sort_on && rate > 0.6 * c->rate_unsorted) {
                c->sort_on = false;
                c->sort_retry_at = c->sort_clock + 512;
            }
        } else {
            c->rate_unsorted = rate;
            if (rate <= SORT_ON_RATE) c->sort_on = false;
            else if (!c->sort_on && c->sort_clock >= c->sort_retry_at) c->sort_on = true;
        }
    }
    if (c->sort_on && ++c->sort_streak >= SORT_PROBE_EVERY) {
        c->sort_streak = 0;
        return false;                                  // the probe
    }
    return c->sort_on;
}

template <int M>
int launch_sort_t(baz_music_ctx* c, const double* dQ, uint32_t qstride, uint32_t batch)
{
    if constexpr (M <= 8) {
        const uint32_t ns = bazsort::key_samples(c->res);
        const uint32_t padded = round_up(batch, 256);          // whole workgroups of the key kernel = whole 8-key loads of the sweeps
        hipLaunchKernelGGL((bazsort::coarse_key_kernel<M>), dim3(padded / 256), dim3(256), 0, c->stream, dQ, c->tab.dKT, ns, batch, qstride, c->dKeys);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL((bazsort::key_sweep_kernel<false>), dim3(bazsort::KEY_BLOCKS), dim3(256), 0, c->stream, c->dKeys, padded / 8, c->dHist,
                           c->dCursor, c->dPerm);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL((bazsort::key_sweep_kernel<true>), dim3(bazsort::KEY_BLOCKS), dim3(256), 0, c->stream, c->dKeys, padded / 8, c->dHist,
                           c->dCursor, c->dPerm);
        HIP_TRY(c, hipGetLastError());
    }
    return BAZ_MUSIC_OK;
}
#endif   // BAZ_MUSIC_LAB

// The refinement arguments of a product scan launch (literal_tile()): the noise eigenvectors of the workspace, the raw-table image in
// force and its threshold, the statistic counter of the call in flight; `a2`: with ||a||^2 per bin, which the fp64 scan's short form reads.
ScanRefine scan_refine(const baz_music_ctx* c, bool a2)
{
    ScanRefine rf;
    rf.Gs = c->refine_off ? nullptr : c->dG;
    rf.TB = c->tab.dTB + c->tb_step_elems;
    rf.below = c->tab.refine_below;
    rf.count = c->refine_nocount ? nullptr : c->dRefined + c->stat_parity;
    rf.A2 = (a2 && c->tab.dA2p) ? c->tab.dA2p + 64 : nullptr;
    return rf;
}
// ... and of the debug taps' validation launches: nothing refined, nothing counted
ScanRefine scan_refine_validation(const baz_music_ctx* c) { return {nullptr, c->tab.dTB + c->tb_step_elems, 0.0, nullptr, nullptr}; }

// ---- the scan: which kernel a launch takes (scan_form), one launcher per kernel ------------------------------------------------------
enum ScanKind { SCAN_FP64 = 0, SCAN_I8 = 1, SCAN_COARSE = 2, SCAN_I8P = 3 };   // the order of baz_music_ctx::scan_names
struct ScanForm { ScanKind kind; bool short_form; };   // short_form (SCAN_FP64): ||a||^2 - sum_c |s_c^H a|^2 on c->dSs, not the projector form on c->dQ

// The scan kernel of a launch, from the context and the port wiring alone (`spec`: the launch writes a spectrum -- the caller's, or the
// private one of peak mode).  In priority order (DESIGN.md 5.0 has the table):
//   1. no spectrum: the coarse-gated scan where it applies.  (Not in emitter-count mode: the gate reads n both as list length and as the
//      literal form's row count, and its list-length bound is what prunes tiles; the full scans' n is the row count alone.)
//   2. lab builds, 2 .. 4 antennas with a spectrum: the level-packed int8 scan.
//   3. 6 .. 16 antennas: the int8 scan -- except a shape of the gated scan without a spectrum whose gate does not apply (BAZ_MUSIC_COARSE=0,
//      emitter-count mode, an unrepresentable table scale): COARSE=0 is the gate's A/B and must stay bit-identical to it, so the fp64 scan.
//   4. the fp64 scan: its short form where that needs fewer MFMAs (n = 2 from 9 antennas, n = 1 from 6), else the projector form.
ScanForm scan_form(const baz_music_ctx* c, bool spec)
{
    if (!spec && coarse_applies(c) && !c->order_mode) return {SCAN_COARSE, false};
    if (spec && i8p_active(c)) return {SCAN_I8P, false};
    const bool gated_shape = c->m <= 8 && !short_form_applies(c->m, c->n);
    if (i8_active(c) && (spec || !gated_shape)) return {SCAN_I8, false};
    return {SCAN_FP64, short_form_in_use(c)};
}

// One scan launch over the workspace: c->dQ (c->dSs: the short form) -> candidates in c->dCand; spec: where a spectrum is written (vec4: 16-byte stores)
struct ScanCall { uint32_t batch, qstride; float* spec; bool vec4; };
ScanCall scan_call(const baz_music_ctx* c, uint32_t batch, uint32_t qstride, float* spec)
{
    return {batch, qstride, spec, spec && (c->res % 4u) == 0 && (reinterpret_cast<uintptr_t>(spec) % 16u) == 0};
}

// What a scan launch did, for the merge that folds its candidate lists (nsplit: bin ranges per item)
struct ScanDone {
    int rc;
    ScanKind kind;
    uint32_t nsplit;
    bool last_pass = true;  // the merge behind it clears the NEXT call's statistic counter (17 .. 64 antennas: the last pass's merge only)
#ifdef BAZ_MUSIC_LAB
    bool sorted = false;    // (BAZ_MUSIC_SORT) the gated scan walked the items through its index list
#endif
};
// a launcher's last word: the outcome, and for baz_music_stage_name the kernel this context last LAUNCHED (a refused launch leaves it)
ScanDone scan_result(baz_music_ctx* c, ScanDone done, int rc) { done.rc = rc; if (rc == BAZ_MUSIC_OK) c->scan_kind = done.kind; return done; }
int launch_rc(baz_music_ctx* c) { HIP_TRY(c, hipGetLastError()); return BAZ_MUSIC_OK; }
ScanDone scan_no_kernel(ScanKind kind) { return {BAZ_MUSIC_E_UNSUPPORTED, kind, 1}; }   // (a launcher outside its kernel's bounds: scan_form sends no shape there)
// The argument lists, each written once: the product launches below and the validation taps (baz_music_debug_coarse_margin,
// baz_music_debug_i8_margin) differ in the instantiation, the grid and what the structs here hold.
struct CoarseLaunch {
    uint32_t blocks, nphases, nsplit;
    ScanRefine rf;
    unsigned long long* stats;                 // lab: exact tile evaluations, summed over launches; VAL: the margin
    float* val_dump = nullptr;
    const uint32_t* perm = nullptr;            // the product walks the items in their own order and keeps no fire statistic
    unsigned long long* fstat = nullptr;
};
template <int M, typename Kernel>
void coarse_launch(baz_music_ctx* c, Kernel kernel, const CoarseLaunch& L, uint32_t batch, uint32_t qstride)
{
    hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(256), 0, c->stream, c->dQ, c->tab.dCS, c->tab.dCS + (size_t)(c->cs_tiles + 1) * cs_c_units(M),
                       c->dCand, batch, c->res, qstride, L.nphases, L.nsplit, c->keep_mask, c->n, L.rf, c->tab.cs, L.stats, L.val_dump, L.perm, L.fstat);
}

struct I8Launch {                              // scan_i8_kernel and, in lab builds, scan_i8p_kernel
    uint32_t blocks, nsplit, n;
    float* spec;
    ScanRefine rf;
    unsigned long long *stat, *margin;         // margin: VAL
};
template <typename Kernel>
void i8_launch(baz_music_ctx* c, Kernel kernel, const I8Launch& L, uint32_t batch, uint32_t qstride)
{
    hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(256), 0, c->stream, c->dQ, c->tab.dIB, c->tab.dIB + i8_image_bytes5(c->m, c->fb_steps) / 16,
                       c->tab.dFB + c->fb_step_elems, L.spec, c->dCand, batch, c->res, qstride, L.nsplit, c->keep_mask, L.n, L.rf, c->tab.i8, L.stat, L.margin);
}

template <int M, int NMAX>
ScanDone launch_scan_coarse(baz_music_ctx* c, const ScanCall& s)
{
    if constexpr (M <= 8 && NMAX <= 4) {
        const CoarseGeom CG = coarse_geometry(c, s.batch);
        ScanDone done{BAZ_MUSIC_OK, SCAN_COARSE, CG.nsplit};
        if ((size_t)s.batch * CG.nsplit * NMAX > c->dCand.cap()) return scan_result(c, done, BAZ_MUSIC_E_INVALID);   // reserve_candidates() sized it
        CoarseLaunch L{CG.groups * CG.nsplit, CG.nphases, CG.nsplit, scan_refine(c, false), c->coarse_stats ? c->dMargin : nullptr};
        auto* kernel = &scan_coarse_kernel<M, NMAX, (M > 4 ? coarse_rg_wide(M, NMAX) : 4), (M > 4 ? 4 : 8)>;
        if constexpr (M <= 4) if (CG.tpp == 4) kernel = &scan_coarse_kernel<M, NMAX, 2, 4>;
#ifdef BAZ_MUSIC_LAB
        // lab (BAZ_MUSIC_SORT): the items in an order in which neighbours share their nulls, while the scan's own statistic says that pays
        int sr = ensure_sort_workspace(c, s.batch);
        done.sorted = !sr && sort_decide(c, s.batch);
        if (done.sorted) sr = launch_sort_t<M>(c, c->dQ, s.qstride, s.batch);
        if (sr) return scan_result(c, done, sr);
        if (done.sorted) ++c->sorted_calls;
        else ++c->unsorted_calls;
        L.perm = done.sorted ? c->dPerm : nullptr;
        L.fstat = c->dFire;
        if constexpr (M <= 4) {
            if (CG.tpp != 4) {                 // (two row groups per wave have the product's kernel alone)
                if (c->sort_mode != 0 && !c->coarse_lab) kernel = &scan_coarse_kernel<M, NMAX, 4, 8, false, 0, true>;   // the index list and the fire statistic
                else if (c->coarse_lab == 1) kernel = &scan_coarse_kernel<M, NMAX, 4, 8, false, 1>;
                else if (c->coarse_lab == 2) kernel = &scan_coarse_kernel<M, NMAX, 4, 8, false, 2>;
            }
        }
#endif
        coarse_launch<M>(c, kernel, L, s.batch, s.qstride);
        return scan_result(c, done, launch_rc(c));
    }
    return scan_no_kernel(SCAN_COARSE);
}

// The bulk of the values on the int8 matrix core, exactly accumulated; steps with a value under the accuracy threshold in this
// kernel's own fp64 form (scan_i8_kernels.hip.h).  Its own bin ranges: whole rounds of the resident workgroup slots (i8_nsplit).
template <int M, int NMAX>
ScanDone launch_scan_i8(baz_music_ctx* c, const ScanCall& s)
{
    if constexpr (M >= 6 && NMAX <= 4) {
        auto* kernel = &scan_i8_kernel<M, NMAX, false, false>;
        if (s.vec4) kernel = &scan_i8_kernel<M, NMAX, true, true>;
        else if (s.spec) kernel = &scan_i8_kernel<M, NMAX, true, false>;
        int& per_cu = c->i8_wgs_per_cu[NMAX > 2 ? 1 : 0][s.spec ? 1 : 0][s.vec4 ? 1 : 0];
        if (per_cu == 0) {
            int occ = 0;
            const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 256, 0);
            per_cu = (oe == hipSuccess && occ > 0) ? occ : 2;
            (void)hipGetLastError();
        }
        const uint32_t nsplit = i8_nsplit(s.batch, c->fb_steps, c->num_cus * (uint32_t)per_cu, c->force_nsplit);
        ScanDone done{BAZ_MUSIC_OK, SCAN_I8, nsplit};
        if ((size_t)s.batch * nsplit * NMAX > c->dCand.cap()) return scan_result(c, done, BAZ_MUSIC_E_INVALID);
        const ScanGeom G = scan_geometry(s.batch, c->fb_steps, c->nclass, c->force_nsplit, c->m);     // (its groups: nclass = 1 from m = 6 on)
        I8Launch L{(G.groups / 4) * nsplit, nsplit, scan_n(c), s.spec, scan_refine(c, false), c->dI8Stat, nullptr};
#ifdef BAZ_MUSIC_LAB
        if constexpr ((M == 8 || M == 16) && NMAX == 2) {        // lab (BAZ_MUSIC_I8_ABL): ablations of the bulk loop (timing only, wrong results)
            if (s.vec4 && c->i8_abl) {
                L.n = c->n;
                switch (c->i8_abl) {
                    case 1: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 1>; break;      // no spectrum stores
                    case 4: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 4>; break;      // no MFMAs
                    case 5: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 5>; break;
                    case 33: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 33>; break;    // staging and barriers alone
                    case 256: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 256>; break;  // the steps left to right (round 4's walk): A/B of the strided walk
                    case 257: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 257>; break;  // ... without the stores
                    case 9: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 9>; break;      // first phase staged only, no stores: the tiles' arithmetic alone
                    default: kernel = &scan_i8_kernel<M, NMAX, true, true, false, 32>; break;    // staging, barriers and stores alone
                }
            }
        }
#endif
        i8_launch(c, kernel, L, s.batch, s.qstride);
        return scan_result(c, done, launch_rc(c));
    }
    return scan_no_kernel(SCAN_I8);
}

#ifdef BAZ_MUSIC_LAB
// LAB (BAZ_MUSIC_I8P=1): 2 .. 4 antennas with the spectrum port: the int8 matrix core with level-packed operands
// (scan_i8p_kernels.hip.h); the geometry (row classes, bin ranges) and candidate lists of the fp64 scan.
template <typename Kernel>
void i8p_launch(baz_music_ctx* c, Kernel kernel, const I8Launch& L, uint32_t rows_per_class, uint32_t batch, uint32_t qstride)
{
    const uint4* p1 = c->tab.dIP + I8P_STEP_UNITS;                            // step 0 (a padded step lies in front)
    const uint4* p2 = p1 + i8p_operand_units(c->fb_steps);
    hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(256), 0, c->stream, c->dQ, p1, p2, c->tab.dFB + c->fb_step_elems, L.spec, c->dCand, batch, c->res,
                       qstride, L.nsplit, c->nclass, rows_per_class, c->keep_mask, L.n, L.rf, c->tab.i8, L.stat, L.margin);
}

template <int M, int NMAX>
ScanDone launch_scan_i8p(baz_music_ctx* c, const ScanCall& s)
{
    if constexpr (M <= 4 && NMAX <= 4) {
        const ScanGeom G = scan_geometry(s.batch, c->fb_steps, c->nclass, c->force_nsplit, c->m);
        ScanDone done{BAZ_MUSIC_OK, SCAN_I8P, G.nsplit};
        if ((size_t)s.batch * G.nsplit * NMAX > c->dCand.cap()) return scan_result(c, done, BAZ_MUSIC_E_INVALID);
        const I8Launch L{G.blocks, G.nsplit, c->n, s.spec, scan_refine(c, false), c->dI8Stat, nullptr};
        auto* kernel = s.vec4 ? &scan_i8p_kernel<M, NMAX, true, true> : &scan_i8p_kernel<M, NMAX, true, false>;
        if constexpr (M == 4 && NMAX == 2) {       // lab (BAZ_MUSIC_I8_ABL): timing ablations (wrong results)
            if (s.vec4 && c->i8_abl) {
                switch (c->i8_abl) {
                    case 1: kernel = &scan_i8p_kernel<M, NMAX, true, true, false, 1>; break;
                    case 2: kernel = &scan_i8p_kernel<M, NMAX, true, true, false, 2>; break;
                    case 4: kernel = &scan_i8p_kernel<M, NMAX, true, true, false, 4>; break;
                    case 5: kernel = &scan_i8p_kernel<M, NMAX, true, true, false, 5>; break;
                    default: kernel = &scan_i8p_kernel<M, NMAX, true, true, false, 3>; break;
                }
            }
        }
        i8p_launch(c, kernel, L, G.rows_per_class, s.batch, s.qstride);
        return scan_result(c, done, launch_rc(c));
    }
    return scan_no_kernel(SCAN_I8P);
}
#else
template <int M, int NMAX>
ScanDone launch_scan_i8p(baz_music_ctx*, const ScanCall&) { return scan_no_kernel(SCAN_I8P); }
#endif

// scan_mfma_kernel<M, NMAX, SPEC, VEC4, ABL, AUX, SIG> by what the launch writes
template <int M, int NMAX, int SIG>
auto* scan_fp64_kernel(const ScanCall& s)
{
    if (s.vec4) return &scan_mfma_kernel<M, NMAX, true, true, 0, (1 | 2 | 16), SIG>;
    if (s.spec) return &scan_mfma_kernel<M, NMAX, true, false, 0, (1 | 2 | 16), SIG>;
    return &scan_mfma_kernel<M, NMAX, false, false, 0, (1 | 2 | 16), SIG>;
}

// The fp64 matrix core throughout.  One or two emitters: the short form ||a||^2 - sum_c |s_c^H a|^2 (SIG) where it needs fewer
// MFMAs than the projector GEMM: n = 2 from 9 antennas, n = 1 from 6.
template <int M, int NMAX>
ScanDone launch_scan_fp64(baz_music_ctx* c, const ScanCall& s, bool short_form)
{
    const ScanGeom G = scan_geometry(s.batch, c->fb_steps, c->nclass, c->force_nsplit, c->m);
    ScanDone done{BAZ_MUSIC_OK, SCAN_FP64, G.nsplit};
    if ((size_t)s.batch * G.nsplit * NMAX > c->dCand.cap()) return scan_result(c, done, BAZ_MUSIC_E_INVALID);   // reserve_candidates() sized it
    auto* kernel = scan_fp64_kernel<M, NMAX, 0>(s);
    if constexpr (M >= 6 && NMAX == 2) {
        if (short_form && c->n == 1) kernel = scan_fp64_kernel<M, NMAX, 1>(s);
        if constexpr (M >= 9) if (short_form && c->n == 2) kernel = scan_fp64_kernel<M, NMAX, 2>(s);
    }
#ifdef BAZ_MUSIC_LAB
    if constexpr (M == 4 && NMAX == 2) {   // lab switches for the A/Bs in profiles/HISTORY_r01_r02.md 5.3 (BAZ_MUSIC_SCAN_VARIANT)
        if (s.vec4 && c->lab_variant) {
            switch (c->lab_variant) {
                case 2: kernel = &scan_mfma_kernel<M, NMAX, true, true, 64, (1 | 2 | 16)>; break;   // ungated top-n network (round 1)
                case 3: kernel = &scan_mfma_kernel<M, NMAX, true, true, 0, 0>; break;               // plain cached spectrum stores
                case 4: kernel = &scan_mfma_kernel<M, NMAX, true, true, 0, 2>; break;               // nt
                case 5: kernel = &scan_mfma_kernel<M, NMAX, true, true, 0, (1 | 16)>; break;        // sc0 sc1
                // (6-8: timing only, wrong results -- tests/lab/scan_ablate.py, profiles/r03_scan_ablation_real_inputs.txt)
                case 6: kernel = &scan_mfma_kernel<M, NMAX, true, true, 1, (1 | 2 | 16)>; break;              // everything but the spectrum stores
                case 7: kernel = &scan_mfma_kernel<M, NMAX, true, true, (8 | 2 | 4), (1 | 2 | 16)>; break;    // stores + staging + barriers only
                case 8: kernel = &scan_mfma_kernel<M, NMAX, true, true, (1 | 2), (1 | 2 | 16)>; break;        // MFMA + conversions, no top-n, no stores
                // (9 - 11, round 5: A/B of the rotating LDS-DMA loader; results are right)
                case 9: kernel = &scan_mfma_kernel<M, NMAX, true, true, 1024, (1 | 2 | 16)>; break;           // rotating loader (negative: profiles/r05_loader_ab.txt)
                case 10: kernel = &scan_mfma_kernel<M, NMAX, true, true, (1024 | 2048), (1 | 2 | 16)>; break;  // rotating loader at 3 waves per SIMD (168 registers: no spills)
                case 11: kernel = &scan_mfma_kernel<M, NMAX, true, true, 2048, (1 | 2 | 16)>; break;          // register staging (the product's) at 3 waves per SIMD
                case 12: kernel = &scan_mfma_kernel<M, NMAX, true, true, 4096, (1 | 2 | 16)>; break;          // blocks in the compact order (negative: profiles/r05_write_order.txt)
                case 13: kernel = &scan_mfma_kernel<M, NMAX, true, true, (8 | 2 | 4 | 4096), (1 | 2 | 16)>; break;   // stores + staging + barriers only, compact order
                case 14: kernel = &scan_mfma_kernel<M, NMAX, true, true, 8192, (1 | 2 | 16)>; break;          // (round 6) s_setprio 3 around the MFMAs of a step
                case 15: kernel = &scan_mfma_kernel<M, NMAX, true, true, 16384, (1 | 2 | 16)>; break;         // ... s_setprio 3 around epilogue, staging and stores instead
                default: break;
            }
        }
    }
#endif
    // short form: coefficient vectors x raw table image; projector form: projector x product image, and the lab's LDS padding (step 0 of either image)
    const double* coeff = short_form ? c->dSs : c->dQ;
    const double2* image = short_form ? c->tab.dTB + c->tb_step_elems : c->tab.dFB + c->fb_step_elems;
    hipLaunchKernelGGL(kernel, dim3(G.blocks), dim3(256), short_form ? 0 : (size_t)c->scan_lds_pad, c->stream, coeff, image, s.spec, c->dCand, s.batch,
                       c->res, s.qstride, G.nsplit, c->nclass, G.rows_per_class, c->keep_mask, scan_n(c), scan_refine(c, true), (uint32_t)c->seq_walk);
    return scan_result(c, done, launch_rc(c));
}

template <int M, int NMAX>
ScanDone launch_scan_t(baz_music_ctx* c, ScanForm form, const ScanCall& s)
{
    switch (form.kind) {
        case SCAN_COARSE: return launch_scan_coarse<M, NMAX>(c, s);
        case SCAN_I8P: return launch_scan_i8p<M, NMAX>(c, s);
        case SCAN_I8: return launch_scan_i8<M, NMAX>(c, s);
        default: return launch_scan_fp64<M, NMAX>(c, s, form.short_form);
    }
}

template <int M>
ScanDone launch_scan_m(baz_music_ctx* c, ScanForm form, const ScanCall& s)
{
    if (c->n <= 2) return launch_scan_t<M, 2>(c, form, s);
    if (c->n <= 4) return launch_scan_t<M, 4>(c, form, s);
    if constexpr (M > 5) {
        if (c->n <= 8) return launch_scan_t<M, 8>(c, form, s);
    }
    if constexpr (M > 9) return launch_scan_t<M, 16>(c, form, s);
    return scan_no_kernel(form.kind);   // unreachable: n < m
}

// The scan of `batch` items of the workspace
ScanDone launch_scan(baz_music_ctx* c, uint32_t qstride, uint32_t batch, float* d_spec)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_SCAN);
    const ScanForm form = scan_form(c, d_spec != nullptr);
    const ScanCall s = scan_call(c, batch, qstride, d_spec);
#define BAZ_CALL(MV) launch_scan_m<MV>(c, form, s)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return scan_no_kernel(form.kind);
    }
#undef BAZ_CALL
}

// topn_merge_kernel folds the scan's candidate lists of every item into its n entries
int launch_merge(baz_music_ctx* c, const ScanDone& scan, uint32_t batch, float* d_ang, float* d_lvl, float* d_spec)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    auto* kernel = &topn_merge_kernel<16>;
    switch (topn_list_len(c->n)) {
        case 2: kernel = &topn_merge_kernel<2>; break;
        case 4: kernel = &topn_merge_kernel<4>; break;
        case 8: kernel = &topn_merge_kernel<8>; break;
        default: break;
    }
    unsigned long long *fire_dev = nullptr, *fire_host = nullptr, fire_tag = 0ull;
#ifdef BAZ_MUSIC_LAB
    // lab (BAZ_MUSIC_SORT): the gated scan just ran with its fire statistic on -- it travels to page-locked memory with this merge
    if (scan.kind == SCAN_COARSE && c->sort_mode != 0 && c->dFire && c->hFireDev) {
        fire_dev = c->dFire;
        fire_host = c->hFireDev;
        fire_tag = ((++c->fire_calls) << 1) | (scan.sorted ? 1ull : 0ull);
    }
#endif
    hipLaunchKernelGGL(kernel, dim3((batch + 255) / 256), dim3(256), 0, c->stream, c->dCand, d_spec, d_ang, d_lvl, batch, c->res, c->n,
                       scan.nsplit, c->keep_mask, scan.last_pass ? c->dRefined + (c->stat_parity ^ 1) : nullptr, fire_dev, fire_host, fire_tag);
    return launch_rc(c);
}

int launch_peaks(baz_music_ctx* c, uint32_t batch, float* d_ang, float* d_lvl, const float* d_spec)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    auto* kernel = &peak_pick_kernel<16>;
    switch (topn_list_len(c->n)) {
        case 2: kernel = &peak_pick_kernel<2>; break;
        case 4: kernel = &peak_pick_kernel<4>; break;
        case 8: kernel = &peak_pick_kernel<8>; break;
        default: break;
    }
    hipLaunchKernelGGL(kernel, dim3((batch + 3) / 4), dim3(256), 0, c->stream, d_spec, d_ang, d_lvl, batch, c->res, c->n);
    return launch_rc(c);
}

// ---------------------------------------------------------------------------------------------------------------
// Wide arrays (m > BAZ_MUSIC_FAST_M): the run-time-m kernels of music_wide_kernels.hip.h, one workgroup per item.
// ---------------------------------------------------------------------------------------------------------------
size_t wide_evd_lds(uint32_t m)
{
    const size_t ld = m + 1, np = (m + (m & 1u)) / 2;
    return 2 * (size_t)m * ld * sizeof(double2) + np * 6 * sizeof(double) + bazwide::WB * sizeof(double) + 2 * np * sizeof(int) +
           m * sizeof(int);
}

// items per pass: bounds the fp64 strength scratch (res doubles per item) to ~256 MiB
uint32_t wide_pass_items(const baz_music_ctx* c)
{
    const size_t per_item = (size_t)c->res * sizeof(double);
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(8192, ((size_t)256 << 20) / per_item));
}

// launch geometry of scan_wide_mfma_kernel for a pass of nb items (one place: process_wide_locked launches with it, baz_music_reserve sizes for it)
struct WideScanGeom { uint32_t ipw, nk, groups, nsplit; };
WideScanGeom wide_scan_geometry(const baz_music_ctx* c, uint32_t nb)
{
    WideScanGeom W;
    W.ipw = (c->n <= 2) ? 4u : (c->n <= 4 ? 2u : 1u);                          // items per wave (tile = ipw items x 16 / ipw outputs)
    W.nk = 8u / W.ipw;                                                         // list length
    W.groups = (nb + 4u * W.ipw - 1) / (4u * W.ipw);                           // workgroups of 4 waves
    W.nsplit = std::max(1u, std::min((1024u + W.groups - 1) / W.groups, std::min(c->fb_steps, 16u)));
    return W;
}
// candidate keys of ANY pass of up to `pass` items: nb * nsplit(nb) is not monotonic in nb (see scan_cand_ranges)
size_t wide_cand_entries(const baz_music_ctx* c, uint32_t pass)
{
    const WideScanGeom W = wide_scan_geometry(c, pass);
    const size_t cap_split = std::min<uint32_t>(c->fb_steps, 16u);
    // nsplit <= 1024 / groups + 1 and groups >= nb / (4 ipw): nb * nsplit <= 4096 ipw + nb; and <= nb * cap_split
    const size_t worst = std::min<size_t>((size_t)pass * cap_split, (size_t)4096u * W.ipw + (size_t)pass);
    return std::max<size_t>(worst, (size_t)pass * W.nsplit) * W.nk;
}

// the items of the largest launch of a call of `batch` items: the call itself, or a pass of it at 17 .. 64 antennas
uint32_t largest_launch_items(const baz_music_ctx* c, uint32_t batch) { return c->wide ? std::min(batch, wide_pass_items(c)) : batch; }

// Which scan a launch of this sequence takes.  One place: process_wide_locked launches by it, baz_music_reserve sizes the candidate
// lists by it, check_launch_pointers demands the table images by it.  MFMA (n <= 8): the short form on the fp64 matrix core
// (scan_wide_mfma_kernel), candidates for bazmusic's merge; SHORT, LITERAL: scan_wide_kernel, with ||a||^2 - ||S^H a||^2 away from the
// nulls where the emitters are few (2n <= m), or the literal form throughout.
enum WideScanForm { WIDE_SCAN_MFMA, WIDE_SCAN_SHORT, WIDE_SCAN_LITERAL };
WideScanForm wide_scan_form(const baz_music_ctx* c)
{
    if (c->wide_literal_only) return WIDE_SCAN_LITERAL;
    if (c->wide_mfma) return WIDE_SCAN_MFMA;
    return 2 * c->n <= c->m ? WIDE_SCAN_SHORT : WIDE_SCAN_LITERAL;
}

// The device pointers a launch sequence of this context's shape hands to its kernels (refuse_null)
int check_launch_pointers(baz_music_ctx* c)
{
    BAZ_REQUIRE(c, dRefined);
    BAZ_REQUIRE(c, dR);
    BAZ_REQUIRE(c, dRedo);
    if (c->avg_window > 1) { BAZ_REQUIRE(c, dRavg); BAZ_REQUIRE(c, dAvgHist[0]); BAZ_REQUIRE(c, dAvgHist[1]); }
    if (c->tab.wh_on) { BAZ_REQUIRE(c, dRwh); BAZ_REQUIRE_TAB(c, dWh); }
    if (c->wide) {
        BAZ_REQUIRE(c, dGw); BAZ_REQUIRE(c, dWS); BAZ_REQUIRE(c, dSw); BAZ_REQUIRE_TAB(c, dTA); BAZ_REQUIRE_TAB(c, dA2);
        if (wide_scan_form(c) == WIDE_SCAN_MFMA) { BAZ_REQUIRE_TAB(c, dTB); BAZ_REQUIRE_TAB(c, dA2p); }
        return BAZ_MUSIC_OK;
    }
    BAZ_REQUIRE(c, dQ); BAZ_REQUIRE(c, dG); BAZ_REQUIRE(c, dCand); BAZ_REQUIRE_TAB(c, dFB); BAZ_REQUIRE_TAB(c, dTB);
    if (short_form_applies(c->m, c->n)) { BAZ_REQUIRE(c, dSs); BAZ_REQUIRE_TAB(c, dA2p); }
    if (c->tab.cs_ok) BAZ_REQUIRE_TAB(c, dCS);
    if (c->tab.i8_ok && wants_i8_image(c)) BAZ_REQUIRE_TAB(c, dIB);
    return BAZ_MUSIC_OK;
}

template <bool TRI>
auto* sub_wide_kernel_n(uint32_t n)      // (n >= 1: baz_music_create)
{
    using namespace bazwide;
    decltype(&sub_wide_kernel<1, TRI>) const kernels[8] = {&sub_wide_kernel<1, TRI>, &sub_wide_kernel<2, TRI>, &sub_wide_kernel<3, TRI>, &sub_wide_kernel<4, TRI>,
                                                           &sub_wide_kernel<5, TRI>, &sub_wide_kernel<6, TRI>, &sub_wide_kernel<7, TRI>, &sub_wide_kernel<8, TRI>};
    return kernels[std::min(n, 8u) - 1];
}

// The EVD of a pass of nb items: noise eigenvectors into c->dGw, signal eigenvectors into c->dSw
int launch_evd_wide(baz_music_ctx* c, const double2* R, uint32_t nb)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_EVD);
    const uint8_t* only = nullptr;
    if (c->sub_evd && c->n <= 8) {     // few emitters: signal subspace by orthogonal iteration, Jacobi for what it hands back
        // from 50 antennas on the lower triangle of R only (sub_wide_kernel, TRI): four workgroups per CU instead of two or three
        const bool tri = c->m >= 50;
        const size_t lds = ((tri ? (size_t)c->m * (c->m + 1) / 2 : (size_t)c->m * (c->m + 1)) + (size_t)c->n * 64) * sizeof(double2);
        auto* kernel = tri ? sub_wide_kernel_n<true>(c->n) : sub_wide_kernel_n<false>(c->n);
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(64), lds, c->stream, R, c->dGw, c->dSw, c->dRedo, c->m);
        HIP_TRY(c, hipGetLastError());
        only = c->dRedo;
    }
    hipLaunchKernelGGL(bazwide::evd_wide_kernel, dim3(nb), dim3(bazwide::WB), wide_evd_lds(c->m), c->stream, R, c->dGw, c->dSw, c->m, c->n, only);
    return launch_rc(c);
}

// PMAX: staged phases per step (2 to 32 antennas, 4 to 64); NOUT: outputs per item (4: n <= 2, 8: n = 3, 4)
template <int PMAX, int NOUT>
auto* scan_wide_mfma_kernel_for(const ScanCall& s)
{
    if (s.vec4) return &bazwide::scan_wide_mfma_kernel<true, true, PMAX, NOUT>;
    if (s.spec) return &bazwide::scan_wide_mfma_kernel<true, false, PMAX, NOUT>;
    return &bazwide::scan_wide_mfma_kernel<false, false, PMAX, NOUT>;
}
template <int PMAX>
auto* scan_wide_mfma_kernel_n(uint32_t n, const ScanCall& s)
{
    if (n <= 2) return scan_wide_mfma_kernel_for<PMAX, 4>(s);
    if (n <= 4) return scan_wide_mfma_kernel_for<PMAX, 8>(s);
    return scan_wide_mfma_kernel_for<PMAX, 16>(s);
}

// WIDE_SCAN_MFMA over a pass of s.batch items: c->dSw, c->dGw -> candidates per bin range in c->dCand, for launch_merge
ScanDone launch_scan_wide_mfma(baz_music_ctx* c, const ScanCall& s)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_SCAN);
    const WideScanGeom W = wide_scan_geometry(c, s.batch);
    auto* kernel = c->m <= 32 ? scan_wide_mfma_kernel_n<2>(c->n, s) : scan_wide_mfma_kernel_n<4>(c->n, s);
    hipLaunchKernelGGL(kernel, dim3(W.groups * W.nsplit), dim3(256), 0, c->stream, c->dSw, c->dGw, c->tab.dTB + c->tb_step_elems, c->tab.dA2p + 64,
                       c->tab.dTA, s.spec, c->dCand, s.batch, c->m, c->n, c->res, W.nsplit, c->keep_mask, c->tab.refine_below,
                       c->dRefined + c->stat_parity);
    return {launch_rc(c), SCAN_FP64, W.nsplit};   // (the kind: what launch_merge knows as a scan without a fire statistic)
}

// WIDE_SCAN_SHORT / _LITERAL over a pass of nb items: the fp64 strengths of every bin into c->dWS, for launch_topn_wide
int launch_scan_wide_plain(baz_music_ctx* c, uint32_t nb, float* spec, bool short_form)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_SCAN);
    // enough workgroups for a small batch: split the bins of an item over several
    const uint32_t max_y = (c->res + bazwide::WB - 1) / bazwide::WB;
    const uint32_t ny = std::max(1u, std::min(max_y, (2048u + nb - 1) / nb));
    const uint32_t bpb = round_up((c->res + ny - 1) / ny, bazwide::WB);
    const uint32_t rows = c->m - c->n + (short_form ? c->n : 0u);      // the noise basis and, for the short form, the signal basis
    hipLaunchKernelGGL(bazwide::scan_wide_kernel, dim3(nb, (c->res + bpb - 1) / bpb), dim3(bazwide::WB), (size_t)rows * c->m * sizeof(double2),
                       c->stream, c->dGw, short_form ? c->dSw : nullptr, c->tab.dTA, c->tab.dA2, c->tab.refine_below, c->dWS, spec, c->m, c->n,
                       c->res, bpb);
    return launch_rc(c);
}

int launch_topn_wide(baz_music_ctx* c, uint32_t nb, float* d_ang, float* d_lvl)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    hipLaunchKernelGGL(bazwide::topn_wide_kernel, dim3(nb), dim3(bazwide::WB), 0, c->stream, c->dWS, d_ang, d_lvl, c->res, c->n);
    return launch_rc(c);
}

// One call of `batch` items at 17 .. 64 antennas, in passes of at most wide_pass_items(): each pass is the whole sequence over its
// slice of in / ang / lvl / spec.  The averaging history runs from pass to pass; the passes' scan statistics add up.
int process_wide_locked(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl, void* d_spec)
{
    const uint32_t pass = largest_launch_items(c, batch);
    int r = ensure_workspace(c, pass);
    if (r == BAZ_MUSIC_OK) r = ensure_cov_stages(c, pass);
    if (r == BAZ_MUSIC_OK) r = check_launch_pointers(c);
    if (r) return r;
    const float* in = static_cast<const float*>(d_in);
    float* ang = static_cast<float*>(d_ang);
    float* lvl = static_cast<float*>(d_lvl);
    float* spec = static_cast<float*>(d_spec);
    const WideScanForm form = wide_scan_form(c);
    for (uint32_t off = 0; off < batch; off += pass) {
        const uint32_t nb = std::min(pass, batch - off);
        float* const p_ang = ang + (size_t)off * c->n;
        float* const p_lvl = lvl ? lvl + (size_t)off * c->n : nullptr;
        float* const p_spec = spec ? spec + (size_t)off * c->res : nullptr;
        r = launch_cov_stages(c, in + (size_t)off * c->nsamples * 2, nb);
        if (r == BAZ_MUSIC_OK) r = launch_evd_wide(c, cov_in_force(c), nb);
        if (r) return r;
        if (form != WIDE_SCAN_MFMA) {
            r = launch_scan_wide_plain(c, nb, p_spec, form == WIDE_SCAN_SHORT);
            if (r == BAZ_MUSIC_OK) r = launch_topn_wide(c, nb, p_ang, p_lvl);
            if (r) return r;
            continue;
        }
        const WideScanGeom W = wide_scan_geometry(c, nb);
        r = ensure_candidates(c, std::max(wide_cand_entries(c, pass), (size_t)nb * W.nsplit * W.nk));
        if (r == BAZ_MUSIC_OK) r = refuse_null(c, c->dCand, "dCand");
        if (r) return r;
        ScanDone scan = launch_scan_wide_mfma(c, scan_call(c, nb, 0, p_spec));
        if (scan.rc) return scan.rc;
        scan.last_pass = off + nb >= batch;      // the statistic counter of the NEXT call is cleared by the last pass's merge only
        r = launch_merge(c, scan, nb, p_ang, p_lvl, p_spec);
        if (r) return r;
    }
    c->stat_next_clean = true;     // (the last pass's merge cleared the next call's statistic counter; the plain scan counts nothing)
    return BAZ_MUSIC_OK;
}

// ---- the table's device images: allocation, device-side construction, exchange -----------------------------------
using TableSet = baz_music_ctx::TableSet;

size_t coarse_image_bytes(const baz_music_ctx* c)
{
    return ((size_t)(c->cs_tiles + 1) * cs_c_units((int)c->m) + (size_t)c->cs_tiles * CS_X_UNITS * cs_groups((int)c->m)) * 16;
}

// One set of buffers for the configuration of `c`.  A failed allocation leaves what it did allocate: the set's owners free it.
int alloc_table_set(baz_music_ctx* c, TableSet& T)
{
    const size_t pad_steps = (size_t)c->fb_steps + 2;
    bool ok = true;
    const auto want = [&ok](auto& buf, size_t n) { ok = ok && buf.allocate(n) == hipSuccess; };
    if (c->wide) {
        want(T.dTA, (size_t)c->m * c->res);
        want(T.dA2, c->res);
        if (c->wide_mfma) {
            want(T.dTB, pad_steps * c->tb_step_elems);
            want(T.dA2p, pad_steps * 64);
        }
        return ok ? BAZ_MUSIC_OK : BAZ_MUSIC_E_NOMEM;
    }
    want(T.dFB, pad_steps * c->fb_step_elems);
    want(T.dTB, pad_steps * c->tb_step_elems);
    want(T.dRW, (size_t)c->res * c->m);
    if (c->m <= 8) want(T.dCS, coarse_image_bytes(c) / sizeof(uint4));
#ifdef BAZ_MUSIC_LAB
    if (c->m <= 8 && c->sort_mode != 0) want(T.dKT, (size_t)bazsort::key_samples(c->res) * c->m * c->m);   // (lab: the sort key's table)
    if (c->i8p_on && c->m <= 4 && c->n <= 4) want(T.dIP, i8p_image_bytes(c->fb_steps) / sizeof(uint4));
#endif
    if (wants_i8_image(c)) want(T.dIB, i8_image_bytes(c->m, c->fb_steps) / sizeof(uint4));
    if (short_form_applies(c->m, c->n)) want(T.dA2p, pad_steps * 64);
    return ok ? BAZ_MUSIC_OK : BAZ_MUSIC_E_NOMEM;
}

inline dim3 grid_for(size_t threads) { return dim3((unsigned)((threads + 255) / 256)); }

// Waits for a short piece of work on `s` by polling: a blocking hipStreamSynchronize sleeps on an interrupt after a brief spin, and on this stack
// such a sleep now and then lasts 5 - 11 ms when another thread of the process is waiting for its own stream at the same time (1 retune in ~100
// at config 3).  The table builders take 0.1 - 0.3 ms: poll for up to 3 ms, then fall back to the blocking wait.
hipError_t wait_stream_polling(hipStream_t s)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(3)) {
            (void)hipGetLastError();
            return hipStreamSynchronize(s);
        }
        std::this_thread::yield();
    }
}

// Builds every image of the table in c->hRaw into `T` on c->s_tab and WAITS for them (the caller holds c->tab_mtx, not c->mtx):
// raw table H2D, the three scalars (table_stats_kernel, one small D2H), the parameters on the host, the image kernels.
int build_tables_device(baz_music_ctx* c, TableSet& T)
{
    hipStream_t s = c->s_tab;
    const uint32_t m = c->m, res = c->res, steps = c->fb_steps;
    const size_t raw_bytes = (size_t)res * m * 2 * sizeof(float);
    // (no copy engines on this path: copy_words_kernel reads the page-locked staging copy over the link, see table_kernels.hip.h)
    void *zRaw = nullptr, *zStats = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer(&zRaw, c->hRaw, 0));
    HIP_TRY(c, hipHostGetDevicePointer(&zStats, c->hTabStats, 0));
    T.wh_on = c->wh_on;
    if (c->wh_on) {    // opt-in whitening: this set's W first (the stage reads it), then the same read over the link, times gamma where on, times W
        if (!T.dWh && T.dWh.allocate((size_t)m * m) != hipSuccess) return BAZ_MUSIC_E_NOMEM;
        void* zW = nullptr;
        HIP_TRY(c, hipHostGetDevicePointer(&zW, c->hWh, 0));
        hipLaunchKernelGGL(baztab::copy_words_kernel, dim3((m * m * 2 + 255) / 256), dim3(256), 0, s, static_cast<const unsigned long long*>(zW),
                           reinterpret_cast<unsigned long long*>(T.dWh.get()), (size_t)m * m * 2);
        HIP_TRY(c, hipGetLastError());
        const uint32_t bps = bazwhiten::WHITEN_THREADS / m;
        hipLaunchKernelGGL(bazwhiten::table_whiten_kernel, dim3(std::min<uint32_t>(512, (res + bps - 1) / bps)), dim3(bazwhiten::WHITEN_THREADS),
                           (size_t)m * (m + 1) / 2 * sizeof(double2), s, static_cast<const float2*>(zRaw), reinterpret_cast<float2*>(c->dRaw.get()), res, m,
                           T.dWh, c->calib_on ? 1 : 0, c->calib_gamma);
    } else if (c->calib_on)   // opt-in calibration: the same read over the link, times gamma (calib_kernels.hip.h); every image below follows from dRaw
        hipLaunchKernelGGL(bazcalib::table_calib_kernel, dim3((unsigned)std::min<size_t>(512, (raw_bytes / 8 + 255) / 256)), dim3(bazcalib::CALIB_THREADS), 0, s,
                           static_cast<const float2*>(zRaw), reinterpret_cast<float2*>(c->dRaw.get()), raw_bytes / 8, m, c->calib_gamma);
    else
        hipLaunchKernelGGL(baztab::copy_words_kernel, dim3((unsigned)std::min<size_t>(512, (raw_bytes / 8 + 255) / 256)), dim3(256), 0, s,
                           static_cast<const unsigned long long*>(zRaw), reinterpret_cast<unsigned long long*>(c->dRaw.get()), raw_bytes / 8);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemsetAsync(c->dTabStats, 0, sizeof(baztab::TableStats), s));
    hipLaunchKernelGGL(baztab::table_stats_kernel, grid_for(res), dim3(256), 0, s, c->dRaw, m, res, c->wide ? 0 : 1,
                       c->dTabStats);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(baztab::copy_words_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(c->dTabStats.get()),
                       static_cast<unsigned long long*>(zStats), sizeof(baztab::TableStats) / 8);
    HIP_TRY(c, hipGetLastError());
    // (meanwhile: the images that need no scalar)
    const size_t pad_steps = (size_t)steps + 2;
    if (T.dFB) {
        hipLaunchKernelGGL(baztab::build_fb_kernel, grid_for(pad_steps * c->fb_step_elems), dim3(256), 0, s, c->dRaw, m, res, steps, T.dFB);
        HIP_TRY(c, hipGetLastError());
    }
    if (T.dTB) {
        hipLaunchKernelGGL(baztab::build_tb_kernel, grid_for(pad_steps * c->tb_step_elems), dim3(256), 0, s, c->dRaw, m, res, steps, T.dTB);
        HIP_TRY(c, hipGetLastError());
    }
    if (T.dA2p) {   // ||a||^2 per bin, huge outside the table like FB's diagonal there
        hipLaunchKernelGGL(baztab::build_a2_kernel, grid_for(pad_steps * 64), dim3(256), 0, s, c->dRaw, m, res, (uint32_t)(pad_steps * 64), 64u, T.dA2p);
        HIP_TRY(c, hipGetLastError());
    }
    if (T.dA2) {
        hipLaunchKernelGGL(baztab::build_a2_kernel, grid_for(res), dim3(256), 0, s, c->dRaw, m, res, res, 0u, T.dA2);
        HIP_TRY(c, hipGetLastError());
    }
    if (T.dRW) {    // the set's own copy of the raw table (the refinement's steering rows)
        hipLaunchKernelGGL(baztab::copy_words_kernel, dim3((unsigned)std::min<size_t>(512, (raw_bytes / 8 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const unsigned long long*>(c->dRaw.get()), reinterpret_cast<unsigned long long*>(T.dRW.get()), raw_bytes / 8);
        HIP_TRY(c, hipGetLastError());
    }
    if (T.dTA) {
        hipLaunchKernelGGL(baztab::build_ta_kernel, grid_for((size_t)m * res), dim3(256), 0, s, reinterpret_cast<const float2*>(c->dRaw.get()), m, res, T.dTA);
        HIP_TRY(c, hipGetLastError());
    }
#ifdef BAZ_MUSIC_LAB
    if (T.dKT) {
        const uint32_t ns = bazsort::key_samples(res);
        hipLaunchKernelGGL(bazsort::build_key_table_kernel, grid_for((size_t)ns * m * m), dim3(256), 0, s, c->dRaw, m, res, ns, T.dKT);
        HIP_TRY(c, hipGetLastError());
    }
#endif
    if (T.dCS) HIP_TRY(c, hipMemsetAsync(T.dCS, 0, coarse_image_bytes(c), s));
    if (T.dIB) HIP_TRY(c, hipMemsetAsync(T.dIB, 0, i8_image_bytes(m, steps), s));
    HIP_TRY(c, wait_stream_polling(s));                  // the scalars are on the host
    const baztab::TableStats st = *c->hTabStats;
    double fmax, amax2;
    std::memcpy(&fmax, &st.fmax_bits, sizeof(double));
    std::memcpy(&amax2, &st.amax2_bits, sizeof(double));
    // projector-form accuracy: |error(d)| ~ m^2 eps ||a||^2 absolute; a d at or below m 1e-8 max||a||^2 (relative
    // error there <~ 1e-7) is recomputed in the reference's literal form (literal_tile() in the scan)
    T.refine_below = amax2 * (double)m * 1e-8;
    T.cs_ok = false;
    T.i8_ok = false;
    const bool finite = st.nonfinite == 0;
    if (T.dCS && finite) {    // coarse-gated scan: f16 pieces of the scaled table + the fp64 operand, per 16-bin tile
        double FS = 0.0;
        if (coarse_params_from(fmax, m, T.cs, FS)) {
            T.cs.lazy = 1;
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COARSE_LAZY")) T.cs.lazy = atoi(v);            // lab
            uint8_t* img = reinterpret_cast<uint8_t*>(T.dCS.get());
            hipLaunchKernelGGL(baztab::build_coarse_c_kernel, grid_for((size_t)(c->cs_tiles + 1) * 16 * m * m), dim3(256), 0, s,
                               c->dRaw, m, res, c->cs_tiles, FS, img);
            HIP_TRY(c, hipGetLastError());
            double* X0 = reinterpret_cast<double*>(img + (size_t)(c->cs_tiles + 1) * cs_c_units((int)m) * 16);
            hipLaunchKernelGGL(baztab::build_coarse_x_kernel, grid_for((size_t)c->cs_tiles * 256 * cs_groups((int)m)), dim3(256), 0, s,
                               c->dRaw, m, res, c->cs_tiles, X0);
            HIP_TRY(c, hipGetLastError());
            T.cs_ok = true;
        }
    }
#ifdef BAZ_MUSIC_LAB
    if (T.dIP) HIP_TRY(c, hipMemsetAsync(T.dIP, 0, i8p_image_bytes(steps), s));
    if (T.dIP && finite) {    // 2 .. 4 antennas: level-packed digit operands
        double sf = 0.0;
        if (i8_params_from(fmax, m, T.i8, sf)) {
            hipLaunchKernelGGL(baztab::build_i8p_kernel, grid_for(res), dim3(256), 0, s, c->dRaw, m, res, steps, sf, T.dIP);
            HIP_TRY(c, hipGetLastError());
            T.i8_ok = true;
        }
    }
#endif
    if (T.dIB && finite) {    // int8-matrix-core scan: the table's digit image
        double sf = 0.0;
        if (i8_params_from(fmax, m, T.i8, sf)) {
            uint8_t* img = reinterpret_cast<uint8_t*>(T.dIB.get());
            hipLaunchKernelGGL(baztab::build_i8_kernel, grid_for((size_t)res * i8_nkb((int)m) * 4), dim3(256), 0, s, c->dRaw, m, res,
                               steps, sf, img, img + i8_image_bytes5(m, steps));
            HIP_TRY(c, hipGetLastError());
            T.i8_ok = true;
        }
    }
    HIP_TRY(c, wait_stream_polling(s));
    return BAZ_MUSIC_OK;
}

// Replaces set_array_response's body (.cc:60-70).  The caller holds c->tab_mtx.  `first`: called from baz_music_create (no
// batch can be in flight, the images go straight into the active set).  table_ri == nullptr: the table c->hRaw already holds
// (baz_music_set_calibration: the same table under another gamma).
int retune(baz_music_ctx* c, const float* table_ri, bool first)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (table_ri) std::memcpy(c->hRaw, table_ri, (size_t)c->res * c->m * 2 * sizeof(float));
    if (first) return build_tables_device(c, c->tab);
    // the shadow set was the active one until the previous swap: batches launched before that swap may still read it
    if (c->swap_recorded) HIP_TRY(c, hipStreamWaitEvent(c->s_tab, c->ev_swap, 0));
    const int r = build_tables_device(c, c->shadow);
    if (r != BAZ_MUSIC_OK) return r;                      // the old table stays in force
    const auto t1 = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lk(c->mtx);           // .cc:67 -- for the exchange of a few pointers only
        std::swap(c->tab, c->shadow);
        c->swap_recorded = hipEventRecord(c->ev_swap, c->stream) == hipSuccess;
        if (!c->swap_recorded) {                          // cannot order the next retune behind the batches in flight: drain them now
            (void)hipGetLastError();
            (void)hipStreamSynchronize(c->stream);
        }
    }
    const auto t2 = std::chrono::steady_clock::now();
    c->last_retune_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
    c->last_swap_wait_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return BAZ_MUSIC_OK;
}

// the slots' events go and the slots start over (their buffers go with their owners); the caller has drained the stream
void free_slots(baz_music_ctx* c)
{
    for (auto& sl : c->slot) {
        if (sl.h2d) (void)hipEventDestroy(sl.h2d);
        if (sl.comp) (void)hipEventDestroy(sl.comp);
        if (sl.d2h) (void)hipEventDestroy(sl.d2h);
        sl = baz_music_ctx::Slot();
    }
    c->s_cap = 0;
    c->s_has_spec = false;
}

int ensure_slots(baz_music_ctx* c, uint32_t chunk, bool want_spec)
{
    if (chunk <= c->s_cap && (!want_spec || c->s_has_spec)) return BAZ_MUSIC_OK;
    bazbuf::Once once(drain(c));
    for (auto& sl : c->slot) {
        HIP_TRY(c, sl.in.retire(once));
        HIP_TRY(c, sl.al.retire(once));
        HIP_TRY(c, sl.h_al.retire(once));
        HIP_TRY(c, sl.spec.retire(once));
    }
    const bool spec = want_spec || c->s_has_spec;
    const uint32_t cap = std::max(chunk, c->s_cap);
    free_slots(c);
    if (!c->s_h2d) HIP_TRY(c, hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking));
    if (!c->s_d2h) HIP_TRY(c, hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking));
    for (auto& sl : c->slot) {
        HIP_TRY(c, sl.in.allocate((size_t)cap * c->nsamples * 2));
        HIP_TRY(c, sl.al.allocate((size_t)cap * c->n * 2));
        HIP_TRY(c, sl.h_al.allocate((size_t)cap * c->n * 2));
        if (spec) HIP_TRY(c, sl.spec.allocate((size_t)cap * c->res));
        HIP_TRY(c, hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&sl.comp, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&sl.d2h, hipEventDisableTiming));
    }
    c->s_cap = cap;
    c->s_has_spec = spec;
    return BAZ_MUSIC_OK;
}

// Is this caller pointer page-locked (hipHostMalloc / hipHostRegister / torch pinned memory)?
bool is_pinned_host(const void* p)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();     // plain pageable memory: not an error for us
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// Is the WHOLE range [p, p + bytes) page-locked and addressable from the device as one piece?  Both ends must be
// page-locked host memory and their device addresses must be `bytes - 1` apart (one mapping, or mappings that continue
// each other): a range of which only the head lies inside a registration -- two blocks fanned out from one upstream
// buffer, one of them owning the registration -- would otherwise hand the zero-copy kernels a device pointer that runs
// into unmapped host memory (a GPU fault, not an error code).  Such a range takes the pageable path.
bool range_is_pinned(const void* p, size_t bytes)
{
    if (!p || !bytes) return false;
    const char* last = static_cast<const char*>(p) + bytes - 1;
    if (!is_pinned_host(p) || !is_pinned_host(last)) return false;
    void *d0 = nullptr, *d1 = nullptr;
    if (hipHostGetDevicePointer(&d0, const_cast<void*>(p), 0) != hipSuccess ||
        hipHostGetDevicePointer(&d1, const_cast<char*>(last), 0) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return static_cast<char*>(d1) - static_cast<char*>(d0) == (ptrdiff_t)(bytes - 1);
}

// hipMemcpyAsync between a device buffer and a caller range that may be only PARTLY inside someone's page-lock
// registration (measured: the runtime answers such a copy with "invalid argument", also when the range straddles two
// registrations).  The whole range is tried first -- the only call the ordinary cases ever make --; a refused range
// is halved at a page boundary of the host address until the pieces are homogeneous, and a piece of at most one page
// that is still refused (a registration boundary inside it: registrations are byte-exact) crosses through a bounce
// buffer with a synchronize.  Only the refused (rare) case costs anything.
hipError_t copy_host_range(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream);
    if (e != hipErrorInvalidValue || bytes == 0) return e;
    (void)hipGetLastError();
    const bool h2d = kind == hipMemcpyHostToDevice;
    const uintptr_t host = (uintptr_t)(h2d ? src : dst);
    if (bytes > 4096) {
        uintptr_t mid = (host + bytes / 2) & ~(uintptr_t)4095;
        if (mid <= host || mid >= host + bytes) mid = host + bytes / 2;
        const size_t first = mid - host;
        e = copy_host_range(dst, src, first, kind, stream);
        if (e != hipSuccess) return e;
        return copy_host_range((char*)dst + first, (const char*)src + first, bytes - first, kind, stream);
    }
    char bounce[4096];
    if (h2d) {
        memcpy(bounce, src, bytes);
        e = hipMemcpyAsync(dst, bounce, bytes, kind, stream);
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(stream);      // the bounce buffer dies with this frame
    }
    e = hipMemcpyAsync(bounce, src, bytes, kind, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e == hipSuccess) memcpy(dst, bounce, bytes);
    return e;
}

// Page-lock [p, p + bytes) for this context: see include/baz_music_hip.h.  Caller holds c->mtx.
// The runtime rejects a copy whose host range is only PARTLY inside a registration (hipMemcpyAsync: invalid argument --
// measured, also when the range straddles two registrations).  So (i) registrations are the caller's exact byte
// ranges, never rounded out to pages (a neighbouring heap object must not end up half inside one); (ii) a request that
// overlaps or touches earlier registrations replaces them by ONE registration of the union (a circular stream buffer
// is covered after its first few calls); (iii) a request that cannot be locked as a whole (limit, refusal) leaves
// nothing of itself locked: the registrations it touches are dropped.
//
// Registrations are PROCESS-wide objects with a count of the contexts that use them (g_pins): two blocks reading the
// same stream buffer (a fan-out) share one registration, and it is released when the LAST of them lets go -- a context
// that stops must not unmap memory another context's copies or kernels are still addressing.
struct SharedPin { uintptr_t lo, hi; int refs; };
std::mutex g_pin_mtx;
std::vector<SharedPin> g_pins;
constexpr uint32_t REFUSED_RETRY_AFTER = 1024;    // a refused range is tried again after this many requests for it

void shared_pin_release(uintptr_t lo, uintptr_t hi)         // caller holds g_pin_mtx
{
    for (size_t i = 0; i < g_pins.size(); ++i)
        if (g_pins[i].lo == lo && g_pins[i].hi == hi) {
            if (--g_pins[i].refs <= 0) {
                if (hipHostUnregister((void*)lo) != hipSuccess) (void)hipGetLastError();   // already unmapped
                g_pins.erase(g_pins.begin() + i);
            }
            return;
        }
}

int host_register_locked(baz_music_ctx* c, const void* p, size_t bytes)
{
    if (!p || !bytes) return BAZ_MUSIC_OK;
    uintptr_t lo = (uintptr_t)p, hi = (uintptr_t)p + bytes;
    for (const auto& pin : c->pins)
        if (pin.lo <= lo && hi <= pin.hi) return BAZ_MUSIC_OK;                       // known (the per-call case)
    for (size_t i = 0; i < c->refused.size(); ++i) {
        auto& r = c->refused[i];
        if (r.lo < hi && lo < r.hi) {
            if (++r.asked < REFUSED_RETRY_AFTER) return BAZ_MUSIC_E_HIP;             // refused not long ago
            c->refused.erase(c->refused.begin() + i);                                // (a transient refusal must not last until stop())
            break;
        }
    }
    std::lock_guard<std::mutex> g(g_pin_mtx);
    for (auto& sp : g_pins)
        if (sp.lo <= lo && hi <= sp.hi) {                                            // another context's registration: share it
            if (c->pinned_bytes + (sp.hi - sp.lo) > c->pin_limit) return BAZ_MUSIC_E_UNSUPPORTED;
            ++sp.refs;
            c->pins.push_back({sp.lo, sp.hi, 0});
            c->pinned_bytes += sp.hi - sp.lo;
            return BAZ_MUSIC_OK;
        }
    std::vector<size_t> touch;
    uint64_t held = 0;
    for (size_t i = 0; i < c->pins.size(); ++i)
        if (c->pins[i].hi >= lo && c->pins[i].lo <= hi) {
            touch.push_back(i);
            held += c->pins[i].hi - c->pins[i].lo;
        }
    if (touch.empty() && range_is_pinned(p, bytes))
        return BAZ_MUSIC_OK;                   // its owner's page-locked memory (hipHostMalloc, torch): not ours to manage
    for (size_t i : touch) {
        lo = std::min(lo, c->pins[i].lo);
        hi = std::max(hi, c->pins[i].hi);
    }
    // the union replaces what it touches -- possible only where nobody else holds those registrations, and where no
    // registration of another context lies inside the union (the runtime would refuse the overlap)
    for (const auto& sp : g_pins) {
        if (!(sp.lo < hi && lo < sp.hi)) continue;
        bool ours = false;
        for (size_t i : touch) ours = ours || (c->pins[i].lo == sp.lo && c->pins[i].hi == sp.hi);
        if (!ours || sp.refs > 1) return BAZ_MUSIC_E_UNSUPPORTED;                    // (the copy path splits at the boundaries)
    }
    const bool fits = c->pinned_bytes - held + (hi - lo) <= c->pin_limit;
    for (size_t k = touch.size(); k-- > 0;) {                                         // back to front: indices stay valid
        shared_pin_release(c->pins[touch[k]].lo, c->pins[touch[k]].hi);
        c->pins.erase(c->pins.begin() + touch[k]);
    }
    c->pinned_bytes -= held;
    if (!fits) return BAZ_MUSIC_E_UNSUPPORTED;
    const hipError_t e = hipHostRegister((void*)lo, hi - lo, hipHostRegisterDefault);
    if (e == hipSuccess) {
        g_pins.push_back({lo, hi, 1});
        c->pins.push_back({lo, hi, 0});
        c->pinned_bytes += hi - lo;
        return BAZ_MUSIC_OK;
    }
    c->refused.push_back({lo, hi, 0});
    return hip_fail(c, e, "hipHostRegister");
}

void host_unregister_all_locked(baz_music_ctx* c)
{
    {
        std::lock_guard<std::mutex> g(g_pin_mtx);
        for (const auto& pin : c->pins) shared_pin_release(pin.lo, pin.hi);
    }
    c->pins.clear();
    c->refused.clear();
    c->pinned_bytes = 0;
}

// One pass of the hot path over `batch` device-resident items: covariance, EVD, scan (with the literal-form
// refinement of near-null tiles inside) and the tiny top-n merge, back to back on the context's stream.  (Cutting the batch into sub-batches and overlapping covariance/EVD of
// sub-batch i+1 with the scan of sub-batch i on two extra streams was measured and is SLOWER -- 0.53 ms ->
// 0.60 / 0.70 / 1.05 ms at 2 / 4 / 8 sub-batches, profiles/r01_two_stream_pipeline_negative.txt: the
// cross-stream event dependencies cost more than the overlap buys.)
// Start the statistic of one API call: flip to the counter the previous call's merge kernel cleared (a memset only
// after a call that failed before its merge).
int begin_statistic(baz_music_ctx* c)
{
    c->stat_parity ^= 1;
    if (!c->stat_next_clean)
        HIP_TRY(c, hipMemsetAsync(c->dRefined + c->stat_parity, 0, sizeof(unsigned long long), c->stream));
    c->stat_next_clean = false;
    return BAZ_MUSIC_OK;
}

// Opt-in sub-bin refinement of the chunk's entries (refine_kernels.hip.h): reads the staged ang | lvl, the item's projector / noise
// vectors of this launch sequence and the raw image of the table in force; writes the caller's ang / lvl and this chunk's offsets.
template <int M>
int launch_refine_t(baz_music_ctx* c, const bazrefine::RefineArgs& A)
{
    const uint64_t entries = (uint64_t)A.batch * A.n;
    hipLaunchKernelGGL((bazrefine::refine_kernel<M>), dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

int launch_refine(baz_music_ctx* c, uint32_t batch, uint32_t qstride, float* d_ang, float* d_lvl)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    BAZ_REQUIRE(c, dRefAl); BAZ_REQUIRE_TAB(c, dRW);
    bazrefine::RefineArgs A;
    const size_t entries = (size_t)batch * c->n;
    A.ang_in = c->dRefAl;
    A.lvl_in = c->dRefAl + entries;
    A.ang_out = d_ang;
    A.lvl_out = d_lvl;
    A.off_out = c->out_ref.chunk<double>();
    // (where the scan runs its short form the EVD writes no projector coefficients, launch_evd_t: the literal form throughout)
    A.Qs = short_form_in_use(c) ? nullptr : c->dQ;
    A.Gs = c->dG;
    A.raw = c->tab.dRW;
    A.below = c->refine_off ? -1.0 : c->tab.refine_below;
    A.batch = batch; A.n = c->n; A.res = c->res; A.qstride = qstride;
    A.rows = c->m - scan_n(c);      // the rows the scans' literal form runs over (emitter-count mode: zero-padded to a uniform count)
#define BAZ_CALL(MV) launch_refine_t<MV>(c, A)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// What PowerArgs and BeamWeightsArgs share (capon_kernel of capon_solve.hip.h): the staged ang | lvl, the caller's ang / lvl where this
// kernel is the one to write them (d_ang / d_lvl null: nothing), the covariances this sequence's EVD read, the raw table in force.
template <class Args>
int capon_args(baz_music_ctx* c, uint32_t batch, float* d_ang, float* d_lvl, Args& A)
{
    BAZ_REQUIRE(c, dRefAl); BAZ_REQUIRE_TAB(c, dRW);
    A.R = cov_in_force(c);                           // what launch_frontend handed to the EVD
    if (const int rn = refuse_null(c, A.R, "the covariance in force")) return rn;
    A.ang_in = c->dRefAl;
    A.lvl_in = c->dRefAl + (size_t)batch * c->n;
    A.ang_out = d_ang;
    A.lvl_out = d_lvl;
    A.raw = c->tab.dRW;
    A.rel_floor = BAZ_MUSIC_POWER_PIVOT_FLOOR;
    A.batch = batch; A.n = c->n; A.res = c->res;
    return BAZ_MUSIC_OK;
}

// Opt-in Capon power of the chunk's entries (power_kernels.hip.h), the last launch of a sequence: reads the staged ang | lvl (ang on the
// grid, refinement or not), the covariances this sequence's EVD read and the raw image of the table in force; writes this chunk's
// powers and whatever of the caller's ang / lvl refine_kernel has not written (d_ang / d_lvl null: nothing).
template <int M>
int launch_power_t(baz_music_ctx* c, const bazpower::PowerArgs& A)
{
    constexpr uint32_t IPB = bazpower::PowerGeom<M>::IPB;
    hipLaunchKernelGGL((bazpower::power_kernel<M>), dim3((A.batch + IPB - 1) / IPB), dim3(256), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

int launch_power(baz_music_ctx* c, uint32_t batch, float* d_ang, float* d_lvl)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    bazpower::PowerArgs A;
    if (const int r = capon_args(c, batch, d_ang, d_lvl, A)) return r;
    A.pow_out = c->out_pow.chunk<double>();
    A.lvl_is_power = c->power_mode == 2;
#define BAZ_CALL(MV) launch_power_t<MV>(c, A)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// Opt-in MVDR weights of the chunk's entries (beam_kernels.hip.h), behind refine_kernel / power_kernel: reads what launch_power reads
// (on R plus the loading), writes this chunk's weights and whatever of the caller's ang / lvl no earlier kernel has written.
template <int M>
int launch_beam_weights_t(baz_music_ctx* c, const bazbeam::BeamWeightsArgs& A)
{
    constexpr uint32_t IPB = bazbeam::BeamGeom<M>::IPB;
    hipLaunchKernelGGL((bazbeam::beam_weights_kernel<M>), dim3((A.batch + IPB - 1) / IPB), dim3(bazbeam::BeamGeom<M>::THREADS), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

int launch_beam_weights(baz_music_ctx* c, uint32_t batch, float* d_ang, float* d_lvl)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    bazbeam::BeamWeightsArgs A;
    if (const int r = capon_args(c, batch, d_ang, d_lvl, A)) return r;
    A.w_out = c->out_beam.chunk<double2>(baz_music_ctx::BEAM_W);
    A.loading = c->beam_loading;
#define BAZ_CALL(MV) launch_beam_weights_t<MV>(c, A)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// y = w^H X of the chunk (beam_kernels.hip.h), the last launch of a sequence: reads the chunk's input a second time (d_in: device
// memory, or the caller's mapped input on the zero-copy path) and the weights launch_beam_weights just wrote.
template <int M>
int launch_beam_apply_t(baz_music_ctx* c, const bazbeam::BeamApplyArgs& A)
{
    const uint64_t units = (uint64_t)A.batch * A.nseg;
    const dim3 grid((unsigned)((units + bazbeam::APPLY_WAVES - 1) / bazbeam::APPLY_WAVES));
    const size_t lds = (size_t)bazbeam::APPLY_WAVES * A.n * (M * sizeof(double2) + sizeof(uint32_t));   // the waves' weights, then their flags
    if constexpr (M % 2 == 0) {
        if (((uintptr_t)A.x & 15u) == 0) {
            hipLaunchKernelGGL((bazbeam::beam_apply_kernel<M, true>), grid, dim3(bazbeam::APPLY_THREADS), lds, c->stream, A);
            HIP_TRY(c, hipGetLastError());
            return BAZ_MUSIC_OK;
        }
    }
    hipLaunchKernelGGL((bazbeam::beam_apply_kernel<M, false>), grid, dim3(bazbeam::APPLY_THREADS), lds, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

int launch_beam_apply(baz_music_ctx* c, const void* d_in, uint32_t batch)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    bazbeam::BeamApplyArgs A;
    A.x = static_cast<const float2*>(d_in);
    A.w = c->out_beam.chunk<double2>(baz_music_ctx::BEAM_W);
    A.y = c->out_beam.chunk<float2>(baz_music_ctx::BEAM_Y);
    A.batch = batch; A.n = c->n; A.K = c->K;
    A.nseg = (c->K + bazbeam::APPLY_SEG - 1) / bazbeam::APPLY_SEG;
    if ((uint64_t)batch * A.nseg > 0x7fffffffull * bazbeam::APPLY_WAVES) return BAZ_MUSIC_E_UNSUPPORTED;   // (the grid's x extent)
#define BAZ_CALL(MV) launch_beam_apply_t<MV>(c, A)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// ---- opt-in Capon / Bartlett spectrum estimators (spectrum_kernels.hip.h) ----------------------------------------------------------
// Launch geometry of spectrum_scan_kernel: groups of IG items times ranges of whole 256-bin passes.  A workgroup factorises its
// items once per range (m^3 / 3 against m^2 / 2 per bin), so a row is cut only while the launch has fewer than ~8 workgroups per CU.
struct SpecGeom { uint32_t groups, nranges, range_bins; };
SpecGeom spectrum_geometry(const baz_music_ctx* c, uint32_t batch, uint32_t ig)
{
    SpecGeom g;
    g.groups = (batch + ig - 1) / ig;
    const uint32_t passes = (c->res + 255u) / 256u;
    const uint32_t want = std::max<uint32_t>(1u, (8u * c->num_cus + g.groups - 1) / g.groups);
    const uint32_t per = (passes + std::min(want, passes) - 1) / std::min(want, passes);     // passes per range
    g.range_bins = per * 256u;
    g.nranges = (passes + per - 1) / per;
    return g;
}

template <int M>
int launch_spectrum_t(baz_music_ctx* c, bazspectrum::SpectrumArgs& A)
{
    const SpecGeom g = spectrum_geometry(c, A.batch, (uint32_t)bazspectrum::ScanGeom<M>::IG);
    if ((uint64_t)g.groups * g.nranges > 0x7fffffffull) return BAZ_MUSIC_E_UNSUPPORTED;   // (the grid's x extent)
    A.nranges = g.nranges;
    A.range_bins = g.range_bins;
    if (c->estimator == BAZ_MUSIC_ESTIMATOR_CAPON)
        hipLaunchKernelGGL((bazspectrum::spectrum_scan_kernel<M, bazspectrum::KIND_CAPON>), dim3(g.groups * g.nranges), dim3(256), 0, c->stream, A);
    else
        hipLaunchKernelGGL((bazspectrum::spectrum_scan_kernel<M, bazspectrum::KIND_BARTLETT>), dim3(g.groups * g.nranges), dim3(256), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// The scan of `batch` items: reads the covariances this sequence's frontend left (averaged where that mode is on) and the raw image
// of the table in force, writes every word of d_spec.
int launch_spectrum(baz_music_ctx* c, uint32_t batch, float* d_spec)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_SCAN);
    BAZ_REQUIRE_TAB(c, dRW);
    if (const int rn = refuse_null(c, cov_in_force(c), "the covariance in force")) return rn;
    if (const int rn = refuse_null(c, d_spec, "d_spec (estimator)")) return rn;
    if (c->res > 0x7fffff00u) return BAZ_MUSIC_E_UNSUPPORTED;                             // (bin + 256 in 32 bits)
    bazspectrum::SpectrumArgs A;
    A.R = cov_in_force(c);
    A.raw = c->tab.dRW;
    A.spec = d_spec;
    A.rel_floor = BAZ_MUSIC_POWER_PIVOT_FLOOR;
    A.batch = batch; A.res = c->res;
    A.nranges = 1; A.range_bins = 256;
#define BAZ_CALL(MV) launch_spectrum_t<MV>(c, A)
    switch (c->m) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// the reference's top-n rule on the float32 spectrum the scan just wrote (peak mode 0 under an estimator)
int launch_topn_spec(baz_music_ctx* c, uint32_t batch, float* d_ang, float* d_lvl, const float* d_spec)
{
    ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
    auto* kernel = &bazspectrum::topn_spec_kernel<16>;
    switch (topn_list_len(c->n)) {
        case 2: kernel = &bazspectrum::topn_spec_kernel<2>; break;
        case 4: kernel = &bazspectrum::topn_spec_kernel<4>; break;
        case 8: kernel = &bazspectrum::topn_spec_kernel<8>; break;
        default: break;
    }
    hipLaunchKernelGGL(kernel, dim3((batch + 3) / 4), dim3(256), 0, c->stream, d_spec, d_ang, d_lvl, batch, c->res, c->n);
    return launch_rc(c);
}

// ---- the tail of the 2 .. 16 antenna sequences: the pickers' staging, and what runs behind the pickers --------------------------------
// Where the pickers of a chunk write ang / lvl.  Refinement / power / beam mode: into the staging buffer of this context, ang | lvl
// (lvl always: it marks the real entries), and refine_kernel / power_kernel / beam_weights_kernel write the caller's -- which may be
// host memory mapped over the link, never read back.  Otherwise: the caller's.
struct PickerOut { float *ang, *lvl; };
int stage_picker_out(baz_music_ctx* c, uint32_t batch, void* d_ang, void* d_lvl, PickerOut& out)
{
    out = {static_cast<float*>(d_ang), static_cast<float*>(d_lvl)};
    if (!c->refine_mode && !c->power_mode && !c->beam_mode) return BAZ_MUSIC_OK;
    const size_t entries = (size_t)batch * c->n;
    if (const int r = grow(c, c->dRefAl, entries * 2)) return r;
    out = {c->dRefAl, c->dRefAl + entries};
    return BAZ_MUSIC_OK;
}

// What follows the pickers where a mode staged them: refinement (MUSIC only: the setters refuse it under an estimator), power, beam
// weights and beam apply, in this order, each where its mode is on; each adds the chunk to its side output.  All read the staging
// buffer.  A caller-visible word is written exactly once, by the last kernel that has something to say about it: the angle by
// refine_kernel, the level by power_kernel in power mode 2 (lvl carries P); a word nobody has anything to say about by the first
// kernel that runs.  The caller's pointers each kernel receives (-: null; port 1 not wired: lvl is null in every column; beam mode
// on / off changes no row):
//   refine  power | refine_kernel  power_kernel  beam_weights_kernel
//   off     0     |                               ang  lvl
//   off     1, 2  |                ang  lvl        -    -
//   on      0     |  ang  lvl                      -    -
//   on      1     |  ang  lvl       -    -         -    -
//   on      2     |  ang   -        -   lvl        -    -
int launch_after_pickers(baz_music_ctx* c, const void* d_in, uint32_t batch, uint32_t qstride, void* d_ang, void* d_lvl)
{
    enum Writer { REFINE, POWER, BEAM };
    const Writer ang_by = c->refine_mode ? REFINE : (c->power_mode ? POWER : BEAM);
    const Writer lvl_by = c->power_mode == 2 ? POWER : ang_by;
    const auto ang = [&](Writer w) { return w == ang_by ? static_cast<float*>(d_ang) : nullptr; };
    const auto lvl = [&](Writer w) { return w == lvl_by ? static_cast<float*>(d_lvl) : nullptr; };
    if (c->refine_mode) {
        if (const int r = launch_refine(c, batch, qstride, ang(REFINE), lvl(REFINE))) return r;
        c->out_ref.count += batch;
    }
    if (c->power_mode) {
        if (const int r = launch_power(c, batch, ang(POWER), lvl(POWER))) return r;
        c->out_pow.count += batch;
    }
    if (c->beam_mode) {
        int r = launch_beam_weights(c, batch, ang(BEAM), lvl(BEAM));
        if (r == BAZ_MUSIC_OK) r = launch_beam_apply(c, d_in, batch);
        if (r) return r;
        c->out_beam.count += batch;
    }
    return BAZ_MUSIC_OK;
}

// The sequence of a context whose estimator is Capon or Bartlett (up to BAZ_MUSIC_FAST_M antennas; the emitter-count mode, refinement
// and smoothing are refused while it is on): the covariance kernels of the two-kernel frontend (also at the fused shape), the averaging
// stage where it is on, spectrum_scan_kernel, a picker on the float32 spectrum, then the power / beam kernels where they are on.  No
// EVD, no MUSIC scan, no merge: nothing clears the next call's statistic counter, so stat_next_clean stays false and
// begin_statistic's memset takes over; nothing adds to this call's counter (baz_music_refined_values reports 0).  Of the workspace
// only dR is touched: the projector / noise-vector / candidate buffers are neither demanded nor sized here.
int process_estimator_body(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl, void* d_spec)
{
    int r = ensure_workspace(c, batch);
    if (r == BAZ_MUSIC_OK) r = ensure_cov_stages(c, batch);    // (whitening is refused under an estimator: the averaging buffers)
    if (r) return r;
    if (c->avg_window > 1) { BAZ_REQUIRE(c, dRavg); BAZ_REQUIRE(c, dAvgHist[0]); BAZ_REQUIRE(c, dAvgHist[1]); }
    BAZ_REQUIRE(c, dRefined); BAZ_REQUIRE(c, dR); BAZ_REQUIRE_TAB(c, dRW);
    for (const SideMode& md : side_modes(c))
        if (const int rs = side_refuse(c, md, batch)) return rs;
    r = launch_cov_stages(c, static_cast<const float*>(d_in), batch);
    if (r) return r;
    float* spec = static_cast<float*>(d_spec);
    if (!spec) {                   // the pickers read the spectrum: the private one when port 2 is not wired
        r = grow(c, c->dPeakSpec, (size_t)batch * c->res);
        if (r) return r;
        spec = c->dPeakSpec;
    }
    PickerOut al;
    r = stage_picker_out(c, batch, d_ang, d_lvl, al);
    if (r == BAZ_MUSIC_OK) r = launch_spectrum(c, batch, spec);
    if (r) return r;
    r = c->peak_mode ? launch_peaks(c, batch, al.ang, al.lvl, spec) : launch_topn_spec(c, batch, al.ang, al.lvl, spec);
    return r ? r : launch_after_pickers(c, d_in, batch, baz_music_q_stride(batch), d_ang, d_lvl);
}

// The MUSIC sequence of 2 .. 16 antennas; the contexts of the two other sequences leave it at the top
int process_device_body(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl, void* d_spec)
{
    if (c->wide) return process_wide_locked(c, d_in, batch, d_ang, d_lvl, d_spec);
    if (c->estimator) return process_estimator_body(c, d_in, batch, d_ang, d_lvl, d_spec);
    int r = ensure_workspace(c, batch);
    if (r == BAZ_MUSIC_OK) r = reserve_candidates(c, batch);
    if (r == BAZ_MUSIC_OK) r = ensure_cov_stages(c, batch);
    if (r == BAZ_MUSIC_OK) r = check_launch_pointers(c);
    if (r) return r;
    const uint32_t qstride = baz_music_q_stride(batch);
    // the modes' side outputs: this chunk's go behind those of the call's earlier chunks (order_begin sized the buffers for the call)
    for (const SideMode& md : side_modes(c))
        if (const int rs = side_refuse(c, md, batch)) return rs;
    uint8_t* const ord = c->order_mode ? c->out_ord.chunk<uint8_t>() : nullptr;
    c->ord_cur = ord;
    r = launch_frontend(c, d_in, batch, c->dQ, qstride);
    c->ord_cur = nullptr;
    if (r) return r;
    float* spec = static_cast<float*>(d_spec);
    if (c->peak_mode && !spec) {   // the peak picker reads the spectrum: keep a private one when port 2 is not wired
        r = grow(c, c->dPeakSpec, (size_t)batch * c->res);
        if (r) return r;
        spec = c->dPeakSpec;
    }
    PickerOut al;
    r = stage_picker_out(c, batch, d_ang, d_lvl, al);
    if (r) return r;
    const ScanDone scan = launch_scan(c, qstride, batch, spec);
    if (scan.rc) return scan.rc;
    r = launch_merge(c, scan, batch, al.ang, al.lvl, spec);
    if (r) return r;
    c->stat_next_clean = true;     // the merge cleared the next call's statistic counter
    if (c->peak_mode) {
        r = launch_peaks(c, batch, al.ang, al.lvl, spec);
        if (r) return r;
    }
    if (ord) {                     // (0, 0) at and beyond every item's own count: the n - k weakest entries of either picker
        ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
        hipLaunchKernelGGL(bazorder::order_truncate_kernel, dim3((unsigned)(((size_t)batch * c->n + 255) / 256)), dim3(256), 0, c->stream,
                           al.ang, al.lvl, ord, batch, c->n);
        HIP_TRY(c, hipGetLastError());
        c->out_ord.count += batch;
    }
    return launch_after_pickers(c, d_in, batch, qstride, d_ang, d_lvl);
}

// One launch sequence over `batch` items.  Averaging on: a sequence that fails forgets the history (the stream position the host
// keeps no longer describes what the device holds); the next item is t = 0.
int process_device_locked(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl,
                          void* d_spec)
{
    const int r = process_device_body(c, d_in, batch, d_ang, d_lvl, d_spec);
    if (r != BAZ_MUSIC_OK) c->avg_hist = 0;
    return r;
}

int ensure_h_al_big(baz_music_ctx* c, size_t floats) { return grow(c, c->h_al_big, floats); }

// baz_music_create: a block of n counters, zero on the context's stream (see there why on that stream)
int alloc_zeroed(baz_music_ctx* c, DevBuf<unsigned long long>& buf, size_t n)
{
    if (buf.allocate(n) != hipSuccess) return BAZ_MUSIC_E_NOMEM;
    return hipMemsetAsync(buf, 0, n * sizeof(unsigned long long), c->stream) == hipSuccess ? BAZ_MUSIC_OK : BAZ_MUSIC_E_HIP;
}

// baz_music_create's last step: both table sets, the builders' side stream and staging buffers, then the first table
int create_tables(baz_music_ctx* c, const float* table_ri)
{
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = hi = 0; (void)hipGetLastError(); }
    int prio = hi;
    if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_TAB_PRIORITY")) prio = atoi(v) > 0 ? hi : (atoi(v) < 0 ? lo : 0);   // lab: 1 highest, 0 default, -1 lowest
    if (hipStreamCreateWithPriority(&c->s_tab, hipStreamNonBlocking, prio) != hipSuccess) return BAZ_MUSIC_E_HIP;
    if (hipEventCreateWithFlags(&c->ev_swap, hipEventDisableTiming) != hipSuccess) return BAZ_MUSIC_E_HIP;
    const size_t raw_floats = (size_t)c->res * c->m * 2;
    if (c->dRaw.allocate(raw_floats) != hipSuccess || c->hRaw.allocate(raw_floats) != hipSuccess) return BAZ_MUSIC_E_NOMEM;
    if (c->dTabStats.allocate(1) != hipSuccess || c->hTabStats.allocate(1) != hipSuccess) return BAZ_MUSIC_E_NOMEM;
    int r = alloc_table_set(c, c->tab);
    if (r == BAZ_MUSIC_OK) r = alloc_table_set(c, c->shadow);
    if (r != BAZ_MUSIC_OK) return r;
    std::lock_guard<std::mutex> tl(c->tab_mtx);
    r = retune(c, table_ri, true);
    if (r != BAZ_MUSIC_OK) return r;
    // first touch of the SHADOW set here, not in the first retune (fresh device allocations are mapped on first use: one retune in twenty
    // took 7 - 12 ms and held the submitting thread up by 0.9 ms, tests/test_retune.py): build the same table into it once
    r = build_tables_device(c, c->shadow);
    return r;
}

// ---- opt-in beamspace front-end (baz_music_set_beamspace; beamspace_kernels.hip.h) ------------------------------------------------
inline bool beamspace_on(const baz_music_ctx* c) { return c->sm.inner && c->sm.kind == baz_music_ctx::FRONT_BEAMSPACE; }

// conj(T) of an m x B complex128 T, row-major [antenna][beam]: the operand of every routine of beamspace_kernels.hip.h
std::vector<double2> beamspace_conj(const double* T_ri, uint32_t m, uint32_t B)
{
    std::vector<double2> tc((size_t)m * B);
    for (size_t e = 0; e < tc.size(); ++e) tc[e] = make_double2(T_ri[2 * e], -T_ri[2 * e + 1]);
    return tc;
}

// finite entries and no all-zero column
bool beamspace_T_ok(const double* T_ri, uint32_t m, uint32_t B)
{
    for (size_t i = 0; i < (size_t)2 * m * B; ++i)
        if (!(T_ri[i] - T_ri[i] == 0.0)) return false;
    for (uint32_t b = 0; b < B; ++b) {
        bool any = false;
        for (uint32_t r = 0; r < m && !any; ++r) any = T_ri[2 * ((size_t)r * B + b)] != 0.0 || T_ri[2 * ((size_t)r * B + b) + 1] != 0.0;
        if (!any) return false;
    }
    return true;
}

// `columns` rows of m complex64 -> rows of B complex64 on the host (the definition's own routine)
void beamspace_apply_host(uint32_t m, uint32_t B, const double* T_ri, int normalise, const float* in_ri, size_t columns, float* out_ri)
{
    const std::vector<double2> tc = beamspace_conj(T_ri, m, B);
    std::vector<double> s((size_t)2 * B);
    for (size_t c = 0; c < columns; ++c)
        bazbeamspace::beamspace_row(tc.data(), m, B, reinterpret_cast<const float2*>(in_ri) + c * m, normalise, s.data(),
                                    reinterpret_cast<float2*>(out_ri) + c * B);
}

// the inner context's table a' = T^H a under the T in force (tab_mtx held: sm changes under tab_mtx + mtx)
std::vector<float> beamspace_table(const baz_music_ctx* c, const float* table_ri)
{
    std::vector<float> proj((size_t)c->res * c->sm.ms * 2);
    beamspace_apply_host(c->m, c->sm.ms, c->sm.bs_T.data(), c->sm.bs_norm, table_ri, c->res, proj.data());
    return proj;
}

template <int B>
int launch_beamspace_t(baz_music_ctx* c, const float2* d_in, uint32_t columns, float2* d_out)
{
    const uint32_t tiles = (columns + bazbeamspace::BS_TILE - 1u) / bazbeamspace::BS_TILE;
    const uint32_t blocks = std::min<uint32_t>(tiles, 3u * c->num_cus);      // three workgroups fit a CU's LDS at m = 64, B = 16
    hipLaunchKernelGGL((bazbeamspace::beamspace_kernel<B>), dim3(blocks), dim3(bazbeamspace::BS_THREADS), bazbeamspace::bs_lds_bytes(c->m, B),
                       c->stream, d_in, d_out, c->sm.dTc.get(), c->m, columns);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// the projection of `columns` snapshots (c->mtx held, the mode on)
int launch_beamspace(baz_music_ctx* c, const float2* d_in, uint32_t columns, float2* d_out)
{
    if (!c->sm.dTc || c->sm.ms > c->m) return BAZ_MUSIC_E_INVALID;
#define BAZ_CALL(B) launch_beamspace_t<B>(c, d_in, columns, d_out)
    switch (c->sm.ms) {
        BAZ_M_CASES(BAZ_CALL)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_CALL
}

// ---- opt-in wideband (subband) front-end (baz_music_set_subbands; subband_kernels.hip.h) --------------------------------------------
inline bool subband_on(const baz_music_ctx* c) { return c->sm.inner && c->sm.kind == baz_music_ctx::FRONT_SUBBAND; }

// f(inner context) for every inner context of the front-end in force (one, or the S of the subband mode), until one fails
template <typename Fn>
int each_inner(baz_music_ctx* c, Fn f)
{
    if (!c->sm.inner) return BAZ_MUSIC_OK;
    if (const int r = f(c->sm.inner)) return r;
    for (baz_music_ctx* in : c->sm.sb_more)
        if (const int r = f(in)) return r;
    return BAZ_MUSIC_OK;
}

// W[s][t] = exp(-2 pi i ((k_s t) mod F) / F) / sqrt(F): the quarter points exactly, everything else evaluated in long double and rounded once
void subband_twiddles_host(uint32_t F, uint32_t S, const uint32_t* bins, double* W_out)
{
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const long double scale = 1.0L / sqrtl((long double)F);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t t = 0; t < F; ++t) {
            const uint32_t j = (uint32_t)(((uint64_t)bins[s] * t) % F);
            long double re, im;
            if ((4u * j) % F == 0) {
                static const int qr[4] = {1, 0, -1, 0}, qi[4] = {0, -1, 0, 1};
                re = (long double)qr[4u * j / F] * scale;
                im = (long double)qi[4u * j / F] * scale;
            } else {
                const long double ph = two_pi * (long double)j / (long double)F;
                re = cosl(ph) * scale;
                im = -sinl(ph) * scale;
            }
            W_out[2 * ((size_t)s * F + t)] = (double)re;
            W_out[2 * ((size_t)s * F + t) + 1] = (double)im;
        }
}

// `blocks` blocks of F x m complex64 -> out [s][block][r] on the host (the definition's own routine)
void subband_apply_host(uint32_t m, uint32_t F, uint32_t S, const double* W_ri, const float* in_ri, size_t blocks, float* out_ri)
{
    const double2* const w = reinterpret_cast<const double2*>(W_ri);
    const float2* const x = reinterpret_cast<const float2*>(in_ri);
    float2* const y = reinterpret_cast<float2*>(out_ri);
    for (uint32_t s = 0; s < S; ++s)
        for (size_t b = 0; b < blocks; ++b)
            for (uint32_t r = 0; r < m; ++r) {
                double re[1], im[1];
                bazsubband::subband_entry<1>(w + (size_t)s * F, 1u, x + b * F * m + r, m, F, re, im);
                y[((size_t)s * blocks + b) * m + r] = make_float2((float)re[0], (float)im[0]);
            }
}

template <int SQ>
int launch_subband_t(baz_music_ctx* c, const float2* d_in, uint32_t columns, float2* d_out)
{
    const auto& S = c->sm;
    const uint32_t tiles = (columns + bazsubband::SB_TILE - 1u) / bazsubband::SB_TILE;
    const uint32_t blocks = std::min<uint32_t>(tiles, 2u * c->num_cus);      // two workgroups fit a CU's LDS at the largest shape (78 KiB)
    hipLaunchKernelGGL((bazsubband::subband_kernel<SQ>), dim3(blocks), dim3(bazsubband::SB_THREADS), bazsubband::sb_lds_bytes(c->m, S.sb_F, S.sb_S),
                       c->stream, d_in, d_out, S.dW.get(), c->m, S.sb_F, S.sb_S, columns);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// the channeliser over `nb` items (c->mtx held, the mode on): d_out is [s][item][q][r]
int launch_subband(baz_music_ctx* c, const float2* d_in, uint32_t nb, float2* d_out)
{
    const auto& S = c->sm;
    if (!S.dW || !S.sb_F || S.sb_S < 1 || S.sb_S > BAZ_MUSIC_MAX_SUBBANDS || c->K % S.sb_F) return BAZ_MUSIC_E_INVALID;
    const uint64_t columns = (uint64_t)nb * (c->K / S.sb_F) * c->m;
    if (columns == 0 || columns * S.sb_F > 0xffffffffull) return BAZ_MUSIC_E_INVALID;
    switch ((S.sb_S + 3u) / 4u) {
        case 1: return launch_subband_t<1>(c, d_in, (uint32_t)columns, d_out);
        case 2: return launch_subband_t<2>(c, d_in, (uint32_t)columns, d_out);
        case 3: return launch_subband_t<3>(c, d_in, (uint32_t)columns, d_out);
        case 4: return launch_subband_t<4>(c, d_in, (uint32_t)columns, d_out);
        case 5: return launch_subband_t<5>(c, d_in, (uint32_t)columns, d_out);
        case 6: return launch_subband_t<6>(c, d_in, (uint32_t)columns, d_out);
        case 7: return launch_subband_t<7>(c, d_in, (uint32_t)columns, d_out);
        case 8: return launch_subband_t<8>(c, d_in, (uint32_t)columns, d_out);
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
}

// dynamic LDS beyond 64 KiB needs the attribute; it is per FUNCTION, so it is set for the largest shape, never for one context's
int subband_lds_attribute(baz_music_ctx* c)
{
    int most = 0;
    for (uint32_t m = 2; m <= BAZ_MUSIC_FAST_M; ++m) most = std::max(most, (int)bazsubband::sb_lds_bytes(m, 64u, BAZ_MUSIC_MAX_SUBBANDS));
    const void* fn[8] = {reinterpret_cast<const void*>(bazsubband::subband_kernel<1>), reinterpret_cast<const void*>(bazsubband::subband_kernel<2>),
                         reinterpret_cast<const void*>(bazsubband::subband_kernel<3>), reinterpret_cast<const void*>(bazsubband::subband_kernel<4>),
                         reinterpret_cast<const void*>(bazsubband::subband_kernel<5>), reinterpret_cast<const void*>(bazsubband::subband_kernel<6>),
                         reinterpret_cast<const void*>(bazsubband::subband_kernel<7>), reinterpret_cast<const void*>(bazsubband::subband_kernel<8>)};
    for (const void* f : fn) HIP_TRY(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, most));
    return BAZ_MUSIC_OK;
}

// the S spectra of a chunk ([s][item][bin]) -> one row per item
int launch_subband_combine(baz_music_ctx* c, const float* d_ps, uint32_t nb, float* d_row)
{
    const size_t total = (size_t)nb * c->res;
    const uint32_t blocks = (uint32_t)std::min<size_t>((total + bazsubband::SBC_THREADS - 1) / bazsubband::SBC_THREADS, 64u * c->num_cus);
    hipLaunchKernelGGL(bazsubband::subband_combine_kernel, dim3(blocks), dim3(bazsubband::SBC_THREADS), 0, c->stream, d_ps, d_row,
                       c->sm.sb_S, total, c->sm.sb_combine);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// ---- opt-in forward-backward averaging / spatial smoothing (baz_music_set_smoothing) ------------------------------------------
// Structure checks on the fp32 table (include/baz_music_hip.h documents them).  Every product is formed in fp64 from the fp32
// entries; a relation holds at a bin when its residual is at most SMOOTH_TOL times the bin's scale s = max_k |a_k|^2.
constexpr double SMOOTH_TOL = 1e-5;
constexpr uint32_t SMOOTH_SCREEN_BINS = 32;   // bins the FB involution is screened on before it is verified on every bin

struct Cd { double re, im; };
inline Cd tab_at(const float* t, uint32_t m, uint32_t b, uint32_t i) { return {t[2 * ((size_t)b * m + i)], t[2 * ((size_t)b * m + i) + 1]}; }
inline Cd cmul(Cd a, Cd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline Cd cmulc(Cd a, Cd b) { return {a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re}; }   // conj(a) b
inline double dist2(Cd a, Cd b) { const double x = a.re - b.re, y = a.im - b.im; return x * x + y * y; }
inline double abs2(Cd a) { return a.re * a.re + a.im * a.im; }

double bin_scale(const float* t, uint32_t m, uint32_t cols, uint32_t b)
{
    double s = 0.0;
    for (uint32_t k = 0; k < cols; ++k) s = std::max(s, abs2(tab_at(t, m, b, k)));
    return s;
}

// SS: a_{i+l} a_0 == a_i a_l for i < ms, 1 <= l < L, every bin (O(res ms L))
bool shift_invariant(const float* t, uint32_t m, uint32_t res, uint32_t ms)
{
    const uint32_t L = m - ms + 1;
    for (uint32_t b = 0; b < res; ++b) {
        const double s = bin_scale(t, m, m, b), lim = SMOOTH_TOL * SMOOTH_TOL * s * s;
        if (!(s < INFINITY)) return false;
        const Cd a0 = tab_at(t, m, b, 0);
        for (uint32_t l = 1; l < L; ++l) {
            const Cd al = tab_at(t, m, b, l);
            for (uint32_t i = 1; i < ms; ++i)
                if (!(dist2(cmul(tab_at(t, m, b, i + l), a0), cmul(tab_at(t, m, b, i), al)) <= lim)) return false;
        }
    }
    return true;
}

// FB with the candidate involution p, at bin b: conj(a_i) a_p(k) == conj(a_k) a_p(i) for every i, k the bin's largest
// element -- i.e. conj(a_i) = c a_p(i) with c = conj(a_k) / a_p(k) (i = p(k) makes |a_p(k)| = |a_k|, so c exists)
bool fb_holds_at(const float* t, uint32_t m, uint32_t ms, const uint8_t* p, uint32_t b)
{
    uint32_t k = 0;
    double s = -1.0;
    for (uint32_t i = 0; i < ms; ++i) { const double v = abs2(tab_at(t, m, b, i)); if (v > s) { s = v; k = i; } }
    if (!(s < INFINITY)) return false;
    const double lim = SMOOTH_TOL * SMOOTH_TOL * s * s;
    const Cd ak = tab_at(t, m, b, k), apk = tab_at(t, m, b, p[k]);
    for (uint32_t i = 0; i < ms; ++i)
        if (!(dist2(cmulc(tab_at(t, m, b, i), apk), cmulc(ak, tab_at(t, m, b, p[i]))) <= lim)) return false;
    return true;
}

// FB: derive the involution p of the ms subarray elements from the table.  Screen: with k0 the element whose smallest modulus over
// the screen bins is largest, every candidate p(k0) = j0 fixes p(i) as the first j with conj(a_i) a_j0 == conj(a_k0) a_j on every
// screen bin (O(ms^3) pair tests, most of them rejected at the first bin).  A candidate that is an involution is then verified on
// every bin (fb_holds_at: O(ms res)).
bool derive_involution(const float* t, uint32_t m, uint32_t res, uint32_t ms, uint8_t* perm)
{
    const uint32_t S = std::min(res, SMOOTH_SCREEN_BINS);
    std::vector<uint32_t> sb(S);
    std::vector<double> lim(S);
    for (uint32_t s = 0; s < S; ++s) {
        sb[s] = (uint32_t)(((uint64_t)s * res) / S);
        const double sc = bin_scale(t, m, ms, sb[s]);
        if (!(sc < INFINITY)) return false;
        lim[s] = SMOOTH_TOL * SMOOTH_TOL * sc * sc;
    }
    uint32_t k0 = 0;
    double best = -1.0;
    for (uint32_t k = 0; k < ms; ++k) {
        double lo = INFINITY;
        for (uint32_t s = 0; s < S; ++s) lo = std::min(lo, abs2(tab_at(t, m, sb[s], k)));
        if (lo > best) { best = lo; k0 = k; }
    }
    auto pair_ok = [&](uint32_t i, uint32_t j, uint32_t j0) {
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t b = sb[s];
            if (!(dist2(cmulc(tab_at(t, m, b, i), tab_at(t, m, b, j0)), cmulc(tab_at(t, m, b, k0), tab_at(t, m, b, j))) <= lim[s]))
                return false;
        }
        return true;
    };
    uint8_t p[64];
    for (uint32_t j0 = 0; j0 < ms; ++j0) {
        bool ok = true;
        for (uint32_t i = 0; i < ms && ok; ++i) {
            uint32_t j = 0;
            while (j < ms && !pair_ok(i, j, j0)) ++j;
            ok = j < ms;
            if (ok) p[i] = (uint8_t)j;
        }
        for (uint32_t i = 0; i < ms && ok; ++i) ok = p[p[i]] == i;
        for (uint32_t b = 0; b < res && ok; ++b) ok = fb_holds_at(t, m, ms, p, b);
        if (ok) {
            std::memcpy(perm, p, ms);
            return true;
        }
    }
    return false;
}

int smoothing_check(uint32_t m, uint32_t res, const float* table_ri, uint32_t ms, int fb, uint8_t* perm_out)
{
    if (!table_ri || m < 2 || m > BAZ_MUSIC_MAX_M || res == 0 || ms < 2 || ms > m) return BAZ_MUSIC_E_INVALID;
    uint8_t p[64];
    for (uint32_t i = 0; i < ms; ++i) p[i] = (uint8_t)i;
    if (ms < m && !shift_invariant(table_ri, m, res, ms)) return BAZ_MUSIC_E_INVALID;
    if (fb && !derive_involution(table_ri, m, res, ms, p)) return BAZ_MUSIC_E_INVALID;
    if (perm_out) std::memcpy(perm_out, p, ms);
    return BAZ_MUSIC_OK;
}

// the first ms columns of a resolution x m table
std::vector<float> sub_table(const float* table_ri, uint32_t m, uint32_t res, uint32_t ms)
{
    std::vector<float> sub((size_t)res * ms * 2);
    for (uint32_t b = 0; b < res; ++b)
        std::memcpy(&sub[(size_t)b * ms * 2], table_ri + (size_t)b * m * 2, (size_t)ms * 2 * sizeof(float));
    return sub;
}

// items per chunk: the re-stacked chunk stays within BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES (at least one item)
uint32_t smooth_chunk(const baz_music_ctx* c, uint32_t batch)
{
    size_t per_item = (size_t)c->sm.Kp * c->sm.ms * sizeof(float2);
    if (c->sm.kind == baz_music_ctx::FRONT_SUBBAND)   // (... and so do the S private spectrum rows of an item)
        per_item = std::max(per_item, (size_t)c->sm.sb_S * c->res * sizeof(float));
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(batch, (size_t)BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES / per_item));
}

int launch_restack(baz_music_ctx* c, const void* d_in, uint32_t nb)
{
    auto& S = c->sm;
    if (S.kind == baz_music_ctx::FRONT_BEAMSPACE) return launch_beamspace(c, static_cast<const float2*>(d_in), nb * c->K, S.dY);
    bazsmooth::RestackGeom g;
    g.m = c->m; g.ms = S.ms; g.K = c->K; g.L = S.L; g.per_item = S.Kp * S.ms; g.fb = (uint32_t)S.fb;
    const uint32_t total = nb * g.per_item;     // <= BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES / 8 (or one item, < 2^31: set_smoothing)
    const uint32_t pairs = (total + 1u) / 2u;
    const uint32_t blocks = (pairs + bazsmooth::RESTACK_THREADS - 1u) / bazsmooth::RESTACK_THREADS;
    bazsmooth::restack_kernel<<<blocks, bazsmooth::RESTACK_THREADS, 0, c->stream>>>(static_cast<const float2*>(d_in), S.dY, g,
                                                                                     S.perm, total);
    HIP_TRY(c, hipGetLastError());
    return BAZ_MUSIC_OK;
}

// process_device with the subband mode on (c->mtx held): per chunk, the channeliser into dY ([s][item][q][r]: subband s's items are
// one contiguous batch), inner context s on its batch with its spectrum port wired into dPs, the combine into the caller's spectrum
// (or the private row), then a picker of THIS context on the combined rows.  An inner context's own ang goes where the picker's will
// (the same stream: the picker writes last); its lvl port stays unwired.
int subband_device_locked(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl, void* d_spec)
{
    auto& S = c->sm;
    const uint32_t chunk = smooth_chunk(c, batch);
    const size_t per_sub = (size_t)(c->K / S.sb_F) * c->m;        // complex64 of one subband's item
    int r = grow(c, S.dY, (size_t)chunk * S.Kp * S.ms);
    if (r == BAZ_MUSIC_OK) r = grow(c, S.dPs, (size_t)chunk * S.sb_S * c->res);
    if (r == BAZ_MUSIC_OK && !d_spec) r = grow(c, S.dRow, (size_t)chunk * c->res);
    baz_music_ctx* failed = nullptr;
    for (uint32_t done = 0; done < batch && r == BAZ_MUSIC_OK; done += chunk) {
        const uint32_t nb = std::min(chunk, batch - done);
        float* const ang = static_cast<float*>(d_ang) + (size_t)done * c->n;
        float* const row = d_spec ? static_cast<float*>(d_spec) + (size_t)done * c->res : S.dRow.get();
        r = launch_subband(c, static_cast<const float2*>(d_in) + (size_t)done * c->nsamples, nb, S.dY);
        uint32_t s = 0;
        if (r == BAZ_MUSIC_OK)
            r = each_inner(c, [&](baz_music_ctx* in) {
                const int ri = baz_music_process_device(in, S.dY + (size_t)s * nb * per_sub, nb, ang, nullptr, S.dPs + (size_t)s * nb * c->res);
                if (ri) failed = in;
                ++s;
                return ri;
            });
        if (r == BAZ_MUSIC_OK) r = launch_subband_combine(c, S.dPs, nb, row);
        if (r == BAZ_MUSIC_OK) {
            float* const lvl = d_lvl ? static_cast<float*>(d_lvl) + (size_t)done * c->n : nullptr;
            r = c->peak_mode ? launch_peaks(c, nb, ang, lvl, row) : launch_topn_spec(c, nb, ang, lvl, row);
        }
    }
    if (r == BAZ_MUSIC_E_HIP && failed) snprintf(c->hip_err, sizeof(c->hip_err), "%s", baz_music_last_hip_error(failed));
    return r;
}

// process_device with the mode on (c->mtx held): per chunk, re-stack into dY and run the inner context on the same stream
int smooth_device_locked(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl, void* d_spec)
{
    auto& S = c->sm;
    if (S.kind == baz_music_ctx::FRONT_SUBBAND) return subband_device_locked(c, d_in, batch, d_ang, d_lvl, d_spec);
    const uint32_t chunk = smooth_chunk(c, batch);
    int r = grow(c, S.dY, (size_t)chunk * S.Kp * S.ms);
    for (uint32_t done = 0; done < batch && r == BAZ_MUSIC_OK; done += chunk) {
        const uint32_t nb = std::min(chunk, batch - done);
        r = launch_restack(c, static_cast<const float2*>(d_in) + (size_t)done * c->nsamples, nb);
        if (r == BAZ_MUSIC_OK)
            r = baz_music_process_device(S.inner, S.dY, nb, static_cast<float*>(d_ang) + (size_t)done * c->n,
                                         d_lvl ? static_cast<float*>(d_lvl) + (size_t)done * c->n : nullptr,
                                         d_spec ? static_cast<float*>(d_spec) + (size_t)done * c->res : nullptr);
    }
    if (r == BAZ_MUSIC_E_HIP && S.inner)
        snprintf(c->hip_err, sizeof(c->hip_err), "%s", baz_music_last_hip_error(S.inner));
    return r;
}

// baz_music_process with the mode on (c->mtx held): the SAME chunks as the device path, staged through device buffers, so the
// two give the same bits
int smooth_host_locked(baz_music_ctx* c, const float* in_ri, uint32_t batch, float* ang, float* lvl, float* spectrum)
{
    auto& S = c->sm;
    const uint32_t chunk = smooth_chunk(c, batch);
    int r = grow(c, S.dX, (size_t)chunk * c->nsamples * 2);
    if (r == BAZ_MUSIC_OK) r = grow(c, S.dAl, (size_t)chunk * c->n * 2);
    if (r == BAZ_MUSIC_OK && spectrum) r = grow(c, S.dSpec, (size_t)chunk * c->res);
    if (r) return r;
    for (uint32_t done = 0; done < batch && r == BAZ_MUSIC_OK; done += chunk) {
        const uint32_t nb = std::min(chunk, batch - done);
        const size_t cnt = (size_t)nb * c->n;
        hipError_t e = copy_host_range(S.dX, in_ri + (size_t)done * c->nsamples * 2, (size_t)nb * c->nsamples * 8,
                                       hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { r = hip_fail(c, e, "hipMemcpyAsync(in)"); break; }
        r = smooth_device_locked(c, S.dX, nb, S.dAl, lvl ? S.dAl + cnt : nullptr, spectrum ? S.dSpec : nullptr);
        if (r == BAZ_MUSIC_OK) e = hipMemcpyAsync(ang + (size_t)done * c->n, S.dAl, cnt * 4, hipMemcpyDeviceToHost, c->stream);
        if (r == BAZ_MUSIC_OK && e == hipSuccess && lvl)
            e = hipMemcpyAsync(lvl + (size_t)done * c->n, S.dAl + cnt, cnt * 4, hipMemcpyDeviceToHost, c->stream);
        if (r == BAZ_MUSIC_OK && e == hipSuccess && spectrum)
            e = copy_host_range(spectrum + (size_t)done * c->res, S.dSpec, (size_t)nb * c->res * 4, hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);   // (also after a failure: no copy may still target the caller)
        if (r == BAZ_MUSIC_OK && e != hipSuccess) r = hip_fail(c, e, "hipMemcpyAsync(out)");
        if (r == BAZ_MUSIC_OK && es != hipSuccess) r = hip_fail(c, es, "hipStreamSynchronize");
    }
    return r ? r : (int)batch;
}

// One device-side call (c->mtx held), the body of both device entry points: opens the call for baz_music_last_orders, then the
// smoothing mode's chunks or the statistic and one pass of the hot path.
int process_device_call_locked(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl, void* d_spec)
{
    if (!c->ord_driven) {                     // (an inner context of the smoothing mode: its outer context has opened the call)
        const int ro = order_begin(c->sm.inner ? c->sm.inner : c, batch);
        if (ro) return ro;
    }
    if (c->sm.inner) return smooth_device_locked(c, d_in, batch, d_ang, d_lvl, d_spec);
    const int r = begin_statistic(c);
    return r ? r : process_device_locked(c, d_in, batch, d_ang, d_lvl, d_spec);
}

}  // namespace

extern "C" {

int baz_music_create(baz_music_ctx** out, uint32_t m, uint32_t n, uint32_t nsamples, uint32_t resolution,
                     const float* table_ri, int device_id)
{
    if (!out) return BAZ_MUSIC_E_INVALID;
    *out = nullptr;
    // lib/baz_music_doa.cc:45-50 (asserts, compiled out in Release) made real; n == m underflows .cc:93
    if (m == 0 || n == 0 || n >= m || nsamples == 0 || (nsamples % m) != 0 || resolution == 0 || !table_ri)
        return BAZ_MUSIC_E_INVALID;
    if (m > BAZ_MUSIC_MAX_M || n > BAZ_MUSIC_MAX_N) return BAZ_MUSIC_E_UNSUPPORTED;   // see baz_music_strerror()
    const bool wide = m > BAZ_MUSIC_FAST_M;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BAZ_MUSIC_E_NODEVICE;
    int dev = device_id;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return BAZ_MUSIC_E_NODEVICE;
    }
    if (dev >= ndev) return BAZ_MUSIC_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return BAZ_MUSIC_E_NODEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BAZ_MUSIC_E_NODEVICE;   // kernels are gfx950-only

    baz_music_ctx* c = new (std::nothrow) baz_music_ctx;
    if (!c) return BAZ_MUSIC_E_NOMEM;
    c->m = m; c->n = n; c->nsamples = nsamples; c->res = resolution; c->K = nsamples / m;
    c->out_ord.buf[0].item_bytes = 1;                                   c->out_ord.what = "dOrd (order_begin)";
    c->out_ref.buf[0].item_bytes = (size_t)n * sizeof(double);          c->out_ref.what = "dRefOff (order_begin)";
    c->out_pow.buf[0].item_bytes = (size_t)n * sizeof(double);          c->out_pow.what = "dPow (order_begin)";
    c->out_beam.buf[baz_music_ctx::BEAM_Y].item_bytes = (size_t)n * c->K * sizeof(float2);
    c->out_beam.buf[baz_music_ctx::BEAM_W].item_bytes = (size_t)n * m * sizeof(double2);
    c->out_beam.what = "dBeam (order_begin)";
    c->device = dev;
    if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_SCAN_VARIANT")) c->lab_variant = atoi(v);
    if (const char* v = getenv("BAZ_MUSIC_CHUNK_MIB")) c->chunk_bytes = (size_t)std::max(1, std::min(1024, atoi(v))) << 20;
    if (const char* v = getenv("BAZ_MUSIC_PIN_LIMIT_MIB")) c->pin_limit = (uint64_t)std::max(0, atoi(v)) << 20;
    if (const char* v = getenv("BAZ_MUSIC_ZERO_COPY")) c->zero_copy = atoi(v) != 0;
    if (const char* v = getenv("BAZ_MUSIC_SINGLE_MIB")) c->single_limit_mib = std::max(1, std::min(1024, atoi(v)));
    DeviceGuard guard(dev);
    int r = BAZ_MUSIC_OK;
    do {
        if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { r = BAZ_MUSIC_E_HIP; break; }
        c->stream = c->own_stream;
        // (every fill of a device buffer below is alloc_zeroed's hipMemsetAsync ON THIS STREAM: hipMemset of device memory may return before the fill has
        // run, and the null stream orders nothing against a non-blocking stream -- round 6, found when the guard allocator's own prefill raced with a scan)
        c->wide = wide;
        if (wide) {   // run-time-m kernels: only the transposed table and the statistic counters (which stay 0)
            if (resolution > (1u << 20)) { r = BAZ_MUSIC_E_UNSUPPORTED; break; }
            {   // dynamic LDS beyond 64 KiB needs the attribute; it is per FUNCTION (shared by every context of the process),
                // so it is always set for the largest m, never for this context's
                constexpr uint32_t MX = BAZ_MUSIC_MAX_M;
                const int evd_lds = (int)wide_evd_lds(MX), scan_lds = (int)((size_t)MX * MX * sizeof(double2));
                const int sub_lds = (int)(((size_t)MX * (MX + 1) + 8u * 64u) * sizeof(double2));
                const void* fn[10] = {reinterpret_cast<const void*>(bazwide::evd_wide_kernel),
                                      reinterpret_cast<const void*>(bazwide::scan_wide_kernel),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<1, false>),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<2, false>),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<3, false>),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<4, false>),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<5, false>),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<6, false>),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<7, false>),
                                      reinterpret_cast<const void*>(bazwide::sub_wide_kernel<8, false>)};
                // (the triangular instantiations, m >= 50, stay below 64 KiB: 33 KiB + 8 KiB at 64 antennas and 8 emitters)
                const int sz[10] = {evd_lds, scan_lds, sub_lds, sub_lds, sub_lds, sub_lds, sub_lds, sub_lds, sub_lds, sub_lds};
                bool ok = true;
                for (int k = 0; k < 10; ++k)
                    ok = ok && hipFuncSetAttribute(fn[k], hipFuncAttributeMaxDynamicSharedMemorySize, sz[k]) == hipSuccess;
                if (!ok) { r = BAZ_MUSIC_E_HIP; break; }
            }
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_SUB_EVD")) c->sub_evd = atoi(v);                   // lab / tests
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_WIDE_LITERAL")) c->wide_literal_only = atoi(v);   // lab / tests
            if ((r = alloc_zeroed(c, c->dRefined, 2)) != BAZ_MUSIC_OK) break;
            c->wide_cov_mfma = 1;
            c->wide_cov_blocks = 2u * (uint32_t)std::max(1, prop.multiProcessorCount);
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_WIDE_COV_MFMA")) c->wide_cov_mfma = (c->wide_cov_mfma && atoi(v)) ? 1 : 0;   // lab / tests
            c->wide_mfma = (n <= 8) ? 1 : 0;
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_WIDE_MFMA")) c->wide_mfma = (c->wide_mfma && atoi(v)) ? 1 : 0;   // lab / tests
            if (c->wide_mfma) {
                c->fb_steps = (resolution + 63) / 64;
                c->keep_mask = (resolution <= (1u << 16)) ? 0xFFFF0000u : 0xFFF00000u;
                c->tb_step_elems = (size_t)2 * ((2 * m + 3) / 4) * 64;
            }
            r = create_tables(c, table_ri);
            break;
        }
        c->fb_steps = (resolution + 63) / 64;
        // bin field of the top-n key: 16 bits up to 65,536 bins (d truncated by <= 2^-36), else 20 bits
        if (resolution > (1u << 20)) { r = BAZ_MUSIC_E_UNSUPPORTED; break; }
        c->keep_mask = (resolution <= (1u << 16)) ? 0xFFFF0000u : 0xFFF00000u;
        c->fb_step_elems = (size_t)2 * ((m * m + 3) / 4) * 64;
        c->tb_step_elems = (size_t)2 * ((2 * m + 3) / 4) * 64;
        // row classes of the spectrum port (scan kernel, ROW CLASSES): rows whose byte offset 4*res*i agrees mod 256.
        // Only where the scan is bound by its stores (m <= 5: <= 28 fp64 FMAs per 4 stored bytes); from m = 6 on it is
        // bound by the matrix core and the shifted table windows only cost (config 5: scan 0.706 -> 0.773 ms).
        if (resolution % 4u == 0 && m <= 5) {
            uint32_t gcd = 64;
            while (resolution % gcd) gcd >>= 1;
            c->nclass = 64u / gcd;
        }
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_NO_ROWCLASS")) { if (atoi(v)) c->nclass = 1; }   // lab: round-1 row order
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_NO_REFINE")) c->refine_off = atoi(v);              // lab
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_NO_REFINE_COUNT")) c->refine_nocount = atoi(v);    // lab: no statistic atomics
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COV_OLD")) c->lab_cov_old = atoi(v);               // lab
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_SUB_EVD")) c->sub_evd = atoi(v);                   // lab / tests
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_NSPLIT")) c->force_nsplit = std::max(0, atoi(v));  // tests / lab
        {   // covariance + EVD fused (cov4_evd_kernel) wherever the dwordx4 covariance applies
            int fuse = 1;
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_FUSE")) fuse = atoi(v);                        // lab: 0 = two kernels
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_SCAN_LDS_PAD")) c->scan_lds_pad = (uint32_t)std::max(0, atoi(v));
            c->fused_covevd = (fuse > 0 && m == 4 && (c->K % 256u) == 0 && !c->lab_cov_old) ? 1 : 0;
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cov4_evd_kernel, 256, 0) == hipSuccess && per_cu > 0)
                c->covevd_blocks = (uint32_t)per_cu * (uint32_t)std::max(1, prop.multiProcessorCount);
            else (void)hipGetLastError();
            // lab: a smaller grid gives a wave several tasks at a test's batch size (else only from 131,073 items on)
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COVEVD_BLOCKS")) { if (atoi(v) > 0) c->covevd_blocks = std::min(c->covevd_blocks, (uint32_t)atoi(v)); }
            // lab: 1 = the deferred rotation (measured: no gain in a step's time that clears the run-to-run spread, profiles/r06_covevd_deferred.txt)
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COVEVD_DEFER")) c->covevd_park = atoi(v) > 0 ? (uint32_t)COVEVD_PARK : 0u;
        }
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_SIG_SCAN")) c->sig_scan = atoi(v);                  // lab / tests
        if (const char* v = getenv("BAZ_MUSIC_COARSE")) c->coarse = atoi(v);                      // A/B, tests
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COARSE_RG")) c->coarse_rg = atoi(v);                // lab
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COARSE_LAB")) c->coarse_lab = atoi(v);              // lab
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COARSE_STATS")) c->coarse_stats = atoi(v);          // lab
        if (m <= 8) {
            c->cs_tiles = round_up((resolution + 15) / 16, 8);
            if ((r = alloc_zeroed(c, c->dMargin, 1)) != BAZ_MUSIC_OK) break;
        }
        if (const char* v = getenv("BAZ_MUSIC_EXACT")) c->i8_on = atoi(v) ? 0 : 1;                // A/B: 1 = the fp64 scan everywhere
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_I8_ABL")) c->i8_abl = atoi(v);                  // lab
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_SEQ_WALK")) c->seq_walk = atoi(v) ? 1 : 0;        // lab
#ifdef BAZ_MUSIC_LAB
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_SORT")) c->sort_mode = atoi(v) < 0 ? -1 : (atoi(v) ? 1 : 0);   // lab / tests: 0 never, 1 always
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_I8P")) c->i8p_on = atoi(v) ? 1 : 0;             // lab: 1 = the level-packed int8 scan at m <= 4
#endif
        if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COVEVD_TASK_ITEMS")) { const int t = atoi(v); c->covevd_task_items = (t == 64 || t == 32 || t == 16) ? t : 0; }
        bool wants_i8_stat = wants_i8_image(c);
#ifdef BAZ_MUSIC_LAB
        wants_i8_stat = wants_i8_stat || (c->i8p_on && m <= 4 && n <= 4);
#endif
        if (wants_i8_stat) {
            if ((r = alloc_zeroed(c, c->dI8Stat, 8)) != BAZ_MUSIC_OK) break;
        }
        {
            // ONE workgroup per CU (4 persistent waves, 8 KiB in flight each = 8 MB chip-wide): measured against 2 / 3 / 4 /
            // 6 (the occupancy limit) / 8 per CU, the fewest concurrent input streams read fastest -- 0.370 vs 0.396 ms per
            // 262,144 items inside the pipeline (profiles/r02_cov_grid.txt); more waves only queue more requests.
            c->cov4_resident_blocks = (uint32_t)std::max(1, prop.multiProcessorCount);
            c->num_cus = (uint32_t)std::max(1, prop.multiProcessorCount);
            if (const char* v = BAZ_LAB_ENV("BAZ_MUSIC_COV_BLOCKS_PER_CU"))    // lab: grid of the covariance kernel
                if (atoi(v) > 0) c->cov4_resident_blocks = (uint32_t)atoi(v) * (uint32_t)std::max(1, prop.multiProcessorCount);
        }
        if ((r = alloc_zeroed(c, c->dRefined, 2)) != BAZ_MUSIC_OK) break;
        r = create_tables(c, table_ri);
    } while (0);
    if (r != BAZ_MUSIC_OK) {
        baz_music_destroy(c);
        return r;
    }
    if (wide) {
        c->stage_name[BAZ_MUSIC_STAGE_COV] = !c->wide_cov_mfma ? "bazwide::cov_wide_kernel" : (m > 32 ? "bazwide::cov_wide_pairs_kernel" : "bazwide::cov_wide_mfma_kernel");
        c->stage_name[BAZ_MUSIC_STAGE_EVD] = "bazwide::evd_wide_kernel";
        c->stage_name[BAZ_MUSIC_STAGE_SCAN] = c->wide_mfma ? "bazwide::scan_wide_mfma_kernel" : "bazwide::scan_wide_kernel";
        c->stage_name[BAZ_MUSIC_STAGE_MERGE] = c->wide_mfma ? (n <= 2 ? "bazmusic::topn_merge_kernel<2>" : (n <= 4 ? "bazmusic::topn_merge_kernel<4>" : "bazmusic::topn_merge_kernel<8>")) : "bazwide::topn_wide_kernel";
        *out = c;
        return BAZ_MUSIC_OK;
    }
    char buf[128];
    snprintf(buf, sizeof(buf), m <= 8 ? "bazmusic::cov_mfma_kernel<%u>" : "bazmusic::cov_mfma2_kernel<%u>", m);
    c->stage_name[BAZ_MUSIC_STAGE_COV] = buf;
    if (m == 4 && (c->K % 256u) == 0 && !c->lab_cov_old) c->stage_name[BAZ_MUSIC_STAGE_COV] = "bazmusic::cov4_x4_kernel";
    if (c->fused_covevd) c->stage_name[BAZ_MUSIC_STAGE_COV] = "bazmusic::cov4_evd_kernel";
    snprintf(buf, sizeof(buf), m <= 4 ? "bazmusic::evd_proj_kernel<%u>" : "bazmusic::evd_proj_lds_kernel<%u>", m);
    c->stage_name[BAZ_MUSIC_STAGE_EVD] = buf;
    snprintf(buf, sizeof(buf), "bazmusic::topn_merge_kernel<%u>", topn_list_len(n));
    c->stage_name[BAZ_MUSIC_STAGE_MERGE] = buf;
    static const char* const scan_kernels[4] = {"scan_mfma_kernel", "scan_i8_kernel", "scan_coarse_kernel", "scan_i8p_kernel"};   // by ScanKind
    for (int k = 0; k < 4; ++k) snprintf(c->scan_names[k], sizeof(c->scan_names[k]), "bazmusic::%s<%u,", scan_kernels[k], m);
    *out = c;
    return BAZ_MUSIC_OK;
}

// What has an order is here; every device and page-locked buffer goes with its owner when the context is deleted, on its device.
void baz_music_destroy(baz_music_ctx* c)
{
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->sm.inner) baz_music_destroy(c->sm.inner);   // (drains this context's stream: the inner one launches on it)
    c->sm.inner = nullptr;
    for (baz_music_ctx* in : c->sm.sb_more) baz_music_destroy(in);   // (the subband mode's other inner contexts)
    c->sm.sb_more.clear();
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->s_tab) (void)hipStreamSynchronize(c->s_tab);
    for (auto& p : c->prof)
        for (auto e : p.ev) (void)hipEventDestroy(e);
    host_unregister_all_locked(c);
    free_slots(c);
    for (hipEvent_t e : {c->ev_swap, c->ev_in, c->ev_out})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {c->s_tab, c->s_h2d, c->s_d2h, c->own_stream})
        if (s) (void)hipStreamDestroy(s);
    delete c;
}

int baz_music_set_table(baz_music_ctx* c, const float* table_ri)
{
    if (!c || !table_ri) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> tl(c->tab_mtx);   // one retune at a time; work() is held up for the pointer exchange only (retune())
    DeviceGuard guard(c->device);
    if (!c->sm.inner || c->sm.kind == baz_music_ctx::FRONT_SUBBAND) return retune(c, table_ri, false);   // (subband on: the table "off" returns to)
    if (c->sm.kind == baz_music_ctx::FRONT_BEAMSPACE) {   // beamspace on: a' of the new table under the T in force, forwarded
        const std::vector<float> proj = beamspace_table(c, table_ri);
        const int rb = retune(c, table_ri, false);
        if (rb != BAZ_MUSIC_OK) return rb;
        std::lock_guard<std::mutex> lk(c->mtx);
        return baz_music_set_table(c->sm.inner, proj.data());
    }
    // smoothing on: the new table must keep the mode's premise, else nothing changes
    bazsmooth::Perm perm = {};
    if (smoothing_check(c->m, c->res, table_ri, c->sm.ms, c->sm.fb, perm.p) != BAZ_MUSIC_OK) return BAZ_MUSIC_E_INVALID;
    int r = retune(c, table_ri, false);
    if (r != BAZ_MUSIC_OK) return r;
    const std::vector<float> sub = sub_table(table_ri, c->m, c->res, c->sm.ms);
    std::lock_guard<std::mutex> lk(c->mtx);      // the inner table and the involution change between two batches
    r = baz_music_set_table(c->sm.inner, sub.data());
    if (r == BAZ_MUSIC_OK) c->sm.perm = perm;
    return r;
}

int baz_music_last_retune_ms(baz_music_ctx* c, double* total_ms, double* swap_ms)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> tl(c->tab_mtx);
    if (total_ms) *total_ms = c->last_retune_ms;
    if (swap_ms) *swap_ms = c->last_swap_wait_ms;
    return BAZ_MUSIC_OK;
}

int baz_music_set_stream(baz_music_ctx* c, void* hip_stream)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    return each_inner(c, [&](baz_music_ctx* in) { return baz_music_set_stream(in, c->stream); });
}

int baz_music_sync(baz_music_ctx* c)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BAZ_MUSIC_OK;
}

int baz_music_reserve(baz_music_ctx* c, uint32_t max_batch)
{
    if (!c || max_batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!c->ord_driven) {   // the modes' side outputs of a whole call, kept by the context that runs the kernels (whose modes mirror this one's)
        baz_music_ctx* const oc = c->sm.inner ? c->sm.inner : c;
        for (const SideMode& md : side_modes(oc))
            if (const int ro = md.mode_on ? side_grow(oc, *md.out, max_batch) : BAZ_MUSIC_OK) return ro;
    }
    if (c->sm.inner) {   // smoothing on: the inner context's workspace for one chunk, and the re-stacked chunk
        const uint32_t chunk = smooth_chunk(c, max_batch);
        int rs = grow(c, c->sm.dY, (size_t)chunk * c->sm.Kp * c->sm.ms);
        if (rs == BAZ_MUSIC_OK && subband_on(c)) rs = grow(c, c->sm.dPs, (size_t)chunk * c->sm.sb_S * c->res);
        return rs ? rs : each_inner(c, [&](baz_music_ctx* in) { return baz_music_reserve(in, chunk); });
    }
    // averaging: both history buffers and the averaged covariances of the largest launch; whitening: its R' (and the pass between the
    // two products at 17 .. 64 antennas)
    const uint32_t items = largest_launch_items(c, max_batch);
    int r = ensure_cov_stages(c, items);
    if (r) return r;
    if (c->wide) {
        r = ensure_workspace(c, items);
        // ... and the candidate lists of the matrix-core scan's largest pass (they used to be allocated inside the first process call)
        return (r || wide_scan_form(c) != WIDE_SCAN_MFMA) ? r : ensure_candidates(c, wide_cand_entries(c, items));
    }
    r = ensure_workspace(c, max_batch);
    if (r == BAZ_MUSIC_OK && (c->refine_mode || c->power_mode || c->beam_mode)) r = grow(c, c->dRefAl, (size_t)max_batch * c->n * 2);   // (the pickers' staging)
    if (r == BAZ_MUSIC_OK && c->estimator) r = grow(c, c->dPeakSpec, (size_t)max_batch * c->res);   // (the private spectrum of calls without port 2)
#ifdef BAZ_MUSIC_LAB
    if (r == BAZ_MUSIC_OK && c->sort_mode != 0) r = ensure_sort_workspace(c, max_batch);
#endif
    return r ? r : reserve_candidates(c, max_batch);
}

uint32_t baz_music_q_stride(uint32_t batch) { return round_up(batch ? batch : 1, 64); }

int baz_music_process_device(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_ang, void* d_lvl,
                             void* d_spec)
{
    if (!c || !d_in || !d_ang) return BAZ_MUSIC_E_INVALID;
    if (batch == 0) return BAZ_MUSIC_OK;
    std::lock_guard<std::mutex> lk(c->mtx);   // .cc:101
    DeviceGuard guard(c->device);
    (void)hipGetLastError();                  // launches below are checked with hipGetLastError(): start from a clean slate
    return process_device_call_locked(c, d_in, batch, d_ang, d_lvl, d_spec);
}

int baz_music_process_device_on(baz_music_ctx* c, void* caller_stream, const void* d_in, uint32_t batch, void* d_ang,
                                void* d_lvl, void* d_spec)
{
    if (!c || !d_in || !d_ang) return BAZ_MUSIC_E_INVALID;
    if (batch == 0) return BAZ_MUSIC_OK;
    std::lock_guard<std::mutex> lk(c->mtx);   // .cc:101
    DeviceGuard guard(c->device);
    (void)hipGetLastError();                  // launches below are checked with hipGetLastError(): start from a clean slate
    hipStream_t cs = static_cast<hipStream_t>(caller_stream);
    const bool foreign = (cs != c->stream);
    if (foreign) {
        if (!c->ev_in) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
        if (!c->ev_out) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->ev_in, cs));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_in, 0));
    }
    int r = process_device_call_locked(c, d_in, batch, d_ang, d_lvl, d_spec);
    if (foreign) {   // also after a failed launch: whatever was enqueued is ordered before the caller's next work
        hipError_t e = hipEventRecord(c->ev_out, c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(cs, c->ev_out, 0);
        if (e != hipSuccess && r == BAZ_MUSIC_OK) r = hip_fail(c, e, "hipStreamWaitEvent(caller_stream)");
    }
    return r;
}

int baz_music_process(baz_music_ctx* c, const float* in_ri, uint32_t batch, float* ang, float* lvl,
                      float* spectrum)
{
    if (!c || !in_ri || !ang) return BAZ_MUSIC_E_INVALID;
    if (batch == 0) return 0;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    (void)hipGetLastError();

    if (c->auto_pin) {   // the caller's (scheduler's) buffers: lock what this call touches and is not locked yet
        // (the two DMA targets; ang / lvl travel through the slots' own page-locked image)
        (void)host_register_locked(c, in_ri, (size_t)batch * c->nsamples * 8);
        if (spectrum) (void)host_register_locked(c, spectrum, (size_t)batch * c->res * 4);
    }
    if (const int ro = order_begin(c->sm.inner ? c->sm.inner : c, batch)) return ro;   // (all chunks of this call: baz_music_last_orders)
    if (c->sm.inner) return smooth_host_locked(c, in_ri, batch, ang, lvl, spectrum);
    // Cutting a call into chunks (H2D of chunk i+1, the kernels of chunk i and D2H of chunk i-1 overlap on three
    // streams) only pays when a chunk carries enough bytes to hide what the extra copies, events and stream hops cost.
    // Measured under the scheduler model (profiles/r02_flowgraph_model_rates.txt): a 128-item config-2 call (2.9 MB) cut
    // in two ran at 0.41-0.53 ms, as one chunk on one stream at 0.20-0.22 ms; pageable 2,048-item calls (46 MB) in four
    // chunks were SLOWER per item than 512-item calls in one (the runtime stages pageable copies and blocks in them, so
    // little overlaps).  Hence:
    //   page-locked caller memory   below 64 MiB of traffic (BAZ_MUSIC_SINGLE_MIB; without the spectrum port: always) ONE chunk on ONE stream -- without copies
    //                               when zero-copy applies: a 1,024-item config-2 call (23 MB) ran at 2.06e6 items/s that way and
    //                               at 1.53e6 cut into three pipelined chunks (round 3, scripts/gpu/r03l.sh); above, >= 4 chunks of
    //                               >= 8 MiB and <= 32 MiB each;
    //   pageable caller memory      one chunk up to 64 MiB, 64-MiB chunks beyond (profiles/r01h_hostfed_chunk_sweep.txt);
    //   BAZ_MUSIC_CHUNK_MIB         forces the chunk size (tests, lab).
    const size_t per_item = (size_t)c->nsamples * 8 + (spectrum ? (size_t)c->res * 4 : 0) + (size_t)c->n * 8;   // what this call moves per item
    // "locked" is a statement about the WHOLE of both ranges (the first byte alone is not enough)
    const bool locked = range_is_pinned(in_ri, (size_t)batch * c->nsamples * 8) &&
                        (!spectrum || range_is_pinned(spectrum, (size_t)batch * c->res * 4));
    uint32_t chunk;
    if (c->chunk_bytes) {
        chunk = (uint32_t)std::min<size_t>(batch, std::max<size_t>(64, c->chunk_bytes / per_item));
    } else if (!locked) {
        chunk = (uint32_t)std::min<size_t>(batch, std::max<size_t>(64, (64u << 20) / per_item));
    } else if (!spectrum || (size_t)batch * per_item < (size_t)c->single_limit_mib << 20) {
        // (without the spectrum port a call moves its input only: the covariance kernel reads it over the link at the link's rate, and cutting the
        // call can only add to that -- 8,192 / 16,384-item calls ran at 6.5 / 6.6e6 items/s as one zero-copy sequence, at 5.5e6 cut into chunks:
        // profiles/r06_hostfed_chunk_sweep.txt)
        chunk = batch;
    } else {
        const size_t floor_items = std::max<size_t>(64, (8u << 20) / per_item);
        const size_t by_count = std::max<size_t>(floor_items, ((size_t)batch + 3) / 4);
        chunk = (uint32_t)std::min<size_t>(batch, std::min<size_t>(std::max<size_t>(64, (32u << 20) / per_item), by_count));
    }
    const bool single = chunk >= batch;
    const bool want_spec = spectrum != nullptr;
    int r = BAZ_MUSIC_OK;

    // Small call on page-locked caller memory: no copies at all.  The kernels address the caller's buffers over PCIe
    // (hipHostGetDevicePointer): the covariance kernel reads every input byte once, the scan stores every spectrum value
    // once, ang / lvl land in a page-locked image -- each byte crosses the link once, inside the launches, instead of
    // through two or three DMA transfers with their submission and completion latencies.  Larger calls keep the pipelined
    // copies below (there the DMA engines overlap both directions with the kernels).
    // A launch sequence uses the link in one direction at a time (a 1,024-item config-2 call: 0.21 ms in, then 0.26 ms out), and round 5
    // tried twice to overlap the two inside a call -- sub-chunks alternating between two contexts with event-staggered kernels, and the
    // input of sub-chunk i + 1 by DMA on a side stream beside the kernels of sub-chunk i.  Both LOSE at every call size: each sub-chunk
    // costs 0.1 - 0.17 ms of copy start-up and cross-stream event hops on this stack (profiles/r05_hostfed_calls.txt).  A third form without
    // events (finished groups of items counted by cov4_evd_kernel, their scans on a second stream behind a spinning one-wave gate) ran the
    // two side by side and gained nothing: kernel-issued reads and writes of host memory share most of one budget (75.8 GB/s in + out
    // against 56 / 53 alone; the covariance took twice as long beside a scan; profiles/r05_hostfed_overlap_negative.txt).  What pays is a
    // larger call (the host block's look-back) and more, shorter covariance tasks for small batches (launch_covevd).
    if (single && locked && c->zero_copy) {
        void *z_in = nullptr, *z_spec = nullptr, *z_al = nullptr;
        bool ok = ensure_h_al_big(c, (size_t)batch * c->n * 2) == BAZ_MUSIC_OK;
        ok = ok && hipHostGetDevicePointer(&z_in, (void*)in_ri, 0) == hipSuccess;
        if (ok && want_spec) ok = hipHostGetDevicePointer(&z_spec, (void*)spectrum, 0) == hipSuccess;
        if (ok) ok = hipHostGetDevicePointer(&z_al, (void*)c->h_al_big, 0) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();           // not addressable from the device after all: the copy path below
        } else {
            float* z_ang = static_cast<float*>(z_al);
            int zr = begin_statistic(c);
            if (zr == BAZ_MUSIC_OK)           // (sizes the workspace and the candidate lists for `batch` itself, before its first launch)
                zr = process_device_locked(c, z_in, batch, z_ang, z_ang + (size_t)batch * c->n, want_spec ? z_spec : nullptr);
            const hipError_t es = hipStreamSynchronize(c->stream);   // also after a failed launch
            if (zr == BAZ_MUSIC_OK && es != hipSuccess) zr = hip_fail(c, es, "hipStreamSynchronize");
            if (zr != BAZ_MUSIC_OK) return zr;
            const size_t cnt = (size_t)batch * c->n;
            memcpy(ang, c->h_al_big, cnt * 4);
            if (lvl) memcpy(lvl, c->h_al_big + cnt, cnt * 4);
            return (int)batch;
        }
    }

    r = ensure_slots(c, chunk, want_spec);
    if (r) return r;
    if (!c->wide) {
        r = ensure_workspace(c, chunk);
        if (r) return r;
        r = reserve_candidates(c, chunk);
        if (r) return r;
    }

    int rc = BAZ_MUSIC_OK;
    uint32_t idx = 0;
    rc = begin_statistic(c);                  // statistic of this call (all its chunks add to the same counter)
    // A failing HIP call must not return from inside the loop: copies already queued still target the caller's
    // buffers, so every exit goes through the drain below.
#define HIP_STEP(call)                                                     \
    if (rc == BAZ_MUSIC_OK) {                                              \
        hipError_t e__ = (call);                                           \
        if (e__ != hipSuccess) rc = hip_fail(c, e__, #call);               \
    }
    // ang / lvl of a finished chunk: from the slot's page-locked image to the caller's two streams
    auto hand_over = [&](baz_music_ctx::Slot& sl) {
        if (!sl.pend_nb) return;
        const size_t cnt = (size_t)sl.pend_nb * c->n;
        memcpy(ang + (size_t)sl.pend_done * c->n, sl.h_al, cnt * 4);
        if (lvl) memcpy(lvl + (size_t)sl.pend_done * c->n, sl.h_al + cnt, cnt * 4);
        sl.pend_nb = 0;
    };
    hipStream_t s_in = single ? c->stream : c->s_h2d, s_out = single ? c->stream : c->s_d2h;
    // Page-locked caller memory, more than one chunk (round 6): the WHOLE call is enqueued without the host waiting for anything -- four
    // slots, a slot's reuse ordered on the device (the copy into slot.in behind the kernels that last read it, the kernels that write
    // slot.spec / slot.al behind the copy that last drained them), ang / lvl of every chunk copied straight into the call's page-locked
    // image and handed to the caller after the one synchronise at the end.  The copy engines then run both directions of the link side
    // by side (96 GB/s in + out against 57 one way, profiles/r05_hostfed_overlap_negative.txt) with the kernels in their shadow; the
    // two-slot form below blocked the host in hipEventSynchronize before every third chunk and so never had more than one copy queued
    // per direction.
    const bool deep = !single && locked && ensure_h_al_big(c, (size_t)batch * c->n * 2) == BAZ_MUSIC_OK;
    const uint32_t nslot = deep ? (uint32_t)BAZ_MUSIC_NSLOT : 2u;
    for (uint32_t done = 0; done < batch && rc == BAZ_MUSIC_OK; done += chunk, ++idx) {
        baz_music_ctx::Slot& sl = c->slot[idx % nslot];
        const uint32_t nb = std::min(chunk, batch - done);
        if (sl.busy && !deep) {   // chunk idx-2 used this slot: its outputs must be on the host before we reuse it
            HIP_STEP(hipEventSynchronize(sl.d2h));
            if (rc == BAZ_MUSIC_OK) hand_over(sl);
            sl.busy = false;
        }
        if (sl.busy && deep) {    // chunk idx-4 used this slot: order the reuse on the device, the host runs ahead
            HIP_STEP(hipStreamWaitEvent(s_in, sl.comp, 0));          // its kernels have read slot.in
            HIP_STEP(hipStreamWaitEvent(c->stream, sl.d2h, 0));      // its outputs have left slot.spec / slot.al
        }
        float* d_ang = sl.al;
        float* d_lvl = sl.al + (size_t)nb * c->n;
        HIP_STEP(copy_host_range(sl.in, in_ri + (size_t)done * c->nsamples * 2, (size_t)nb * c->nsamples * 8,
                                 hipMemcpyHostToDevice, s_in));
        if (!single) {
            HIP_STEP(hipEventRecord(sl.h2d, s_in));
            HIP_STEP(hipStreamWaitEvent(c->stream, sl.h2d, 0));
        }
        if (rc == BAZ_MUSIC_OK) rc = process_device_locked(c, sl.in, nb, d_ang, d_lvl, want_spec ? sl.spec : nullptr);
        if (!single) {
            HIP_STEP(hipEventRecord(sl.comp, c->stream));
            HIP_STEP(hipStreamWaitEvent(s_out, sl.comp, 0));
        }
        // (deep: chunk `done` keeps its [ang | lvl] image at 2 n done floats of the call's image: handed over after the final synchronise)
        HIP_STEP(hipMemcpyAsync(deep ? c->h_al_big + (size_t)done * c->n * 2 : sl.h_al, sl.al, (size_t)nb * c->n * 8, hipMemcpyDeviceToHost, s_out));
        if (want_spec)
            HIP_STEP(copy_host_range(spectrum + (size_t)done * c->res, sl.spec, (size_t)nb * c->res * 4,
                                     hipMemcpyDeviceToHost, s_out));
        if (!single) HIP_STEP(hipEventRecord(sl.d2h, s_out));
        sl.busy = (rc == BAZ_MUSIC_OK);
        if (sl.busy && !deep) {
            sl.pend_done = done;
            sl.pend_nb = nb;
        }
    }
#undef HIP_STEP
    // drain (also on the error path) so that no copy still targets the caller's buffers
    if (!single) (void)hipStreamSynchronize(c->s_h2d);
    (void)hipStreamSynchronize(c->stream);
    if (!single) (void)hipStreamSynchronize(c->s_d2h);
    for (auto& sl : c->slot) {
        if (rc == BAZ_MUSIC_OK && sl.busy) hand_over(sl);
        sl.busy = false;
        sl.pend_nb = 0;
    }
    if (deep && rc == BAZ_MUSIC_OK) {           // every chunk's [ang | lvl] image is on the host now
        for (uint32_t done = 0; done < batch; done += chunk) {
            const size_t cnt = (size_t)std::min(chunk, batch - done) * c->n;
            const float* img = c->h_al_big + (size_t)done * c->n * 2;
            memcpy(ang + (size_t)done * c->n, img, cnt * 4);
            if (lvl) memcpy(lvl + (size_t)done * c->n, img + cnt, cnt * 4);
        }
    }
    if (rc != BAZ_MUSIC_OK) c->avg_hist = 0;       // (averaging: a failed call forgets the history, also when a copy failed)
    return rc ? rc : (int)batch;
}

int baz_music_host_register(baz_music_ctx* c, const void* p, size_t bytes)
{
    if (!c || (!p && bytes)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    return host_register_locked(c, p, bytes);
}

int baz_music_set_host_pinning(baz_music_ctx* c, int enable)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    c->auto_pin = enable ? 1 : 0;
    return BAZ_MUSIC_OK;
}

int baz_music_host_unregister_all(baz_music_ctx* c)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    (void)hipStreamSynchronize(c->s_h2d ? c->s_h2d : c->stream);
    host_unregister_all_locked(c);
    return BAZ_MUSIC_OK;
}

uint64_t baz_music_host_pinned_bytes(baz_music_ctx* c)
{
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mtx);
    return c->pinned_bytes;
}

int baz_music_profile(baz_music_ctx* c, int enable)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (enable) {
        for (auto& p : c->prof) { p.used = 0; p.total_ms = 0.0; p.launches = 0; }
        c->profiling = (enable == 2) ? 2 : 1;
    } else {
        prof_collect(c);
        c->profiling = 0;
    }
    return BAZ_MUSIC_OK;
}

int baz_music_stage_ms(baz_music_ctx* c, int stage, double* total_ms, uint64_t* launches)
{
    if (!c || stage < 0 || stage >= BAZ_MUSIC_NUM_STAGES) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (total_ms) *total_ms = c->prof[stage].total_ms;
    if (launches) *launches = c->prof[stage].launches;
    return BAZ_MUSIC_OK;
}

const char* baz_music_stage_name(baz_music_ctx* c, int stage)
{
    if (!c || stage < 0 || stage >= BAZ_MUSIC_NUM_STAGES) return "";
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (c->sm.inner) return "";   // smoothing on: no stage of this context runs (baz_music_set_smoothing)
        // averaging / whitening on: the fused shape runs its two-kernel form (launch_frontend)
        if (stage == BAZ_MUSIC_STAGE_COV && c->fused_covevd && (c->avg_window > 1 || c->estimator || c->tab.wh_on)) return "bazmusic::cov4_x4_kernel";
    }
    if (stage == BAZ_MUSIC_STAGE_SCAN && !c->wide) {
        {
            std::lock_guard<std::mutex> lk(c->mtx);
            if (c->estimator) return "bazspectrum::spectrum_scan_kernel";
        }
        // the kernel the LAST scan launch took (it depends on the wiring of the call and on the table in force: ADVICE r4);
        // before the first launch: what a call with the spectrum port would take
        // (the four names are formatted once, in baz_music_create: the pointer handed out stays valid for the context's life)
        std::lock_guard<std::mutex> lk(c->mtx);
        return c->scan_names[c->scan_kind >= 0 ? c->scan_kind : (int)scan_form(c, true).kind];
    }
    return c->stage_name[stage].c_str();
}

int baz_music_debug_cov(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_R)
{
    if (!c || !d_in || !d_R || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    if (c->fused_covevd) {   // the product's covariance lives inside the fused kernel: run THAT with its R tap
        int r = ensure_workspace(c, batch);
        if (r) return r;
        return launch_covevd(c, static_cast<const float*>(d_in), batch, c->dQ, baz_music_q_stride(batch), c->dG,
                             static_cast<double2*>(d_R));
    }
    return launch_cov(c, static_cast<const float*>(d_in), batch, static_cast<double2*>(d_R));
}

int baz_music_debug_q(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_Q)
{
    if (!c || !d_in || !d_Q || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->wide || c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;   // the wide path forms no projector (literal form straight from G)
    if (c->avg_window > 1) return BAZ_MUSIC_E_UNSUPPORTED;        // (averaging on: the tap would consume history)
    int r = ensure_workspace(c, batch);
    if (r) return r;
    return launch_frontend(c, d_in, batch, static_cast<double*>(d_Q), baz_music_q_stride(batch));
}

// Validation of the coarse-gated scan's error bound on this hardware (scan_coarse_kernels.hip.h, VAL): covariance + EVD of
// the batch, then EVERY (item, bin) in both forms; *worst = max |coarse / SC - exact| / (2^-16 (S + |exact|)).  The gate is
// sound while this stays below 1; the bound was derived with a factor > 2 to spare.
int baz_music_debug_coarse_margin(baz_music_ctx* c, const void* d_in, uint32_t batch, float* worst)
{
    if (!c || !d_in || !worst || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->wide || c->m > 8 || c->n > 4 || !c->tab.cs_ok || c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    if (c->avg_window > 1) return BAZ_MUSIC_E_UNSUPPORTED;        // (averaging on: the tap would consume history)
    int r = ensure_workspace(c, batch);
    if (r) return r;
    r = reserve_candidates(c, batch);
    if (r) return r;
    const uint32_t qstride = baz_music_q_stride(batch);
    r = launch_frontend(c, d_in, batch, c->dQ, qstride);
    if (r) return r;
    HIP_TRY(c, hipMemsetAsync(c->dMargin, 0, sizeof(unsigned long long), c->stream));
    const bool big = c->m > 4;                   // (m >= 5: the RG = 2, TPP = 4 instantiation, like the scan's)
    const uint32_t per_group = big ? 64u * (uint32_t)coarse_rg_wide((int)c->m, 2) : 256u;
    // one range per row: every (item, bin) in both forms
    CoarseLaunch L{(batch + per_group - 1) / per_group, c->cs_tiles / (big ? 4u : 8u), 1u, scan_refine_validation(c), c->dMargin};
    DevBuf<float> d_dump;                        // lab (BAZ_MUSIC_DEBUG_DUMP=<file>): every ratio, [item][bin] float32
    const char* dump_path = BAZ_LAB_ENV("BAZ_MUSIC_DEBUG_DUMP");
    if (dump_path) (void)d_dump.allocate((size_t)batch * c->res);
    if (d_dump) (void)hipMemsetAsync(d_dump, 0, (size_t)batch * c->res * sizeof(float), c->stream);
    L.val_dump = d_dump;
#define BAZ_VAL(MV, NV, RGV, TPV) coarse_launch<MV>(c, &scan_coarse_kernel<MV, NV, RGV, TPV, true>, L, batch, qstride)
    const bool n2 = c->n <= 2;
    switch (c->m) {
        case 2: BAZ_VAL(2, 2, 4, 8); break;
        case 3: if (n2) BAZ_VAL(3, 2, 4, 8); else BAZ_VAL(3, 4, 4, 8); break;
        case 4: if (n2) BAZ_VAL(4, 2, 4, 8); else BAZ_VAL(4, 4, 4, 8); break;
        case 5: BAZ_VAL(5, 2, coarse_rg_wide(5, 2), 4); break;         // (the lists are not used by the validation build)
        case 6: BAZ_VAL(6, 2, coarse_rg_wide(6, 2), 4); break;
        case 7: BAZ_VAL(7, 2, coarse_rg_wide(7, 2), 4); break;
        default: BAZ_VAL(8, 2, coarse_rg_wide(8, 2), 4); break;
    }
#undef BAZ_VAL
    HIP_TRY(c, hipGetLastError());
    unsigned long long packed = 0;
    HIP_TRY(c, hipMemcpyAsync(&packed, c->dMargin, sizeof(packed), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (d_dump) {
        std::vector<float> h((size_t)batch * c->res);
        if (hipMemcpy(h.data(), d_dump, h.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess)
            if (FILE* f = fopen(dump_path, "wb")) { fwrite(h.data(), sizeof(float), h.size(), f); fclose(f); }
    }
    const unsigned int bits = (unsigned int)(packed >> 32);
    std::memcpy(worst, &bits, sizeof(float));
    if (BAZ_LAB_ENV("BAZ_MUSIC_DEBUG_MARGIN"))   // lab: where the worst value sits
        fprintf(stderr, "[baz_music] coarse margin %.4g at bin %u, item %% 4096 = %u\n", *worst, (unsigned)(packed & 0xFFFFFu),
                (unsigned)((packed >> 20) & 0xFFFu));
    return BAZ_MUSIC_OK;
}

// lab statistic (BAZ_MUSIC_COARSE_STATS=1 at create): exact (16-item row group, 16-bin tile) evaluations of all coarse-gated
// scan launches since the last read; resets the counter.  -1 when the statistic is off.
int64_t baz_music_debug_coarse_fired(baz_music_ctx* c)
{
    if (!c || !c->coarse_stats || !c->dMargin) return -1;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    unsigned long long v = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&v, c->dMargin, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemsetAsync(c->dMargin, 0, sizeof(v), c->stream) != hipSuccess) return -1;
    return (int64_t)v;
}

namespace {
// the three VAL margins a validation launch of the int8 forms left in dI8Stat[2 .. 4] (float bits), read back behind a drain of the stream
int read_i8_margins(baz_music_ctx* c, float* worst)
{
    unsigned long long packed[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(packed, c->dI8Stat + 2, sizeof(packed), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) {
        const unsigned int bits = (unsigned int)packed[k];
        std::memcpy(worst + k, &bits, sizeof(float));
    }
    return BAZ_MUSIC_OK;
}
}  // namespace

// Validation of the int8 scan's a-priori bounds on this hardware (scan_i8_kernels.hip.h, VAL): covariance + EVD of the batch,
// then EVERY (item, bin) in the four-, five-, seven-digit and the fp64 form; worst[0] = max |d5 - d| / E5, worst[1] = max |d7 - d| /
// allowance, worst[2] = max |d4 - d| / E4 over the items that take the integer forms.
int baz_music_debug_i8_margin(baz_music_ctx* c, const void* d_in, uint32_t batch, float* worst)
{
    if (!c || !d_in || !worst || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    if (c->avg_window > 1) return BAZ_MUSIC_E_UNSUPPORTED;        // (averaging on: the tap would consume history)
#ifdef BAZ_MUSIC_LAB
    if (!c->wide && c->m <= 4 && c->m >= 2 && c->n <= 4 && c->tab.dIP && c->tab.i8_ok) {
        // 2 .. 4 antennas: the level-packed form (scan_i8p_kernels.hip.h), VAL instantiation, one bin range per row
        int r = ensure_workspace(c, batch);
        if (r) return r;
        r = reserve_candidates(c, batch);
        if (r) return r;
        const uint32_t qstride = baz_music_q_stride(batch);
        r = launch_frontend(c, d_in, batch, c->dQ, qstride);
        if (r) return r;
        HIP_TRY(c, hipMemsetAsync(c->dI8Stat + 2, 0, 3 * sizeof(unsigned long long), c->stream));
        const ScanGeom G = scan_geometry(batch, c->fb_steps, c->nclass, 1, c->m);
        const I8Launch L{G.blocks, 1u, c->n, nullptr, scan_refine_validation(c), nullptr, c->dI8Stat + 2};
#define BAZ_VALP(MV) case MV: i8p_launch(c, &scan_i8p_kernel<MV, 2, false, false, true>, L, G.rows_per_class, batch, qstride); break;
        switch (c->m) {
#ifndef BAZ_MUSIC_QUICK
            BAZ_VALP(2) BAZ_VALP(3)
#endif
            BAZ_VALP(4)
            default: return BAZ_MUSIC_E_UNSUPPORTED;
        }
#undef BAZ_VALP
        HIP_TRY(c, hipGetLastError());
        return read_i8_margins(c, worst);
    }
#endif
    if (c->wide || !c->tab.dIB || !c->tab.i8_ok || c->m < 6 || c->m > 16 || c->n > 4) return BAZ_MUSIC_E_UNSUPPORTED;
    int r = ensure_workspace(c, batch);
    if (r) return r;
    r = reserve_candidates(c, batch);
    if (r) return r;
    const uint32_t qstride = baz_music_q_stride(batch);
    const int on = c->i8_on;
    c->i8_on = 1;                       // (the EVD must write the projector coefficients: short_form_in_use())
    r = launch_frontend(c, d_in, batch, c->dQ, qstride);
    c->i8_on = on;
    if (r) return r;
    HIP_TRY(c, hipMemsetAsync(c->dI8Stat + 2, 0, 3 * sizeof(unsigned long long), c->stream));
    const I8Launch L{(batch + 63) / 64, 1u, c->n, nullptr, scan_refine_validation(c), nullptr, c->dI8Stat + 2};
#define BAZ_VAL8(MV) case MV: i8_launch(c, &scan_i8_kernel<MV, 2, false, false, true>, L, batch, qstride); break;
    switch (c->m) {
        BAZ_VAL8(6) BAZ_VAL8(7) BAZ_VAL8(8) BAZ_VAL8(9) BAZ_VAL8(10) BAZ_VAL8(11) BAZ_VAL8(12) BAZ_VAL8(13) BAZ_VAL8(14)
        BAZ_VAL8(15) BAZ_VAL8(16)
        default: return BAZ_MUSIC_E_UNSUPPORTED;
    }
#undef BAZ_VAL8
    HIP_TRY(c, hipGetLastError());
    return read_i8_margins(c, worst);
}

// Statistic of the int8 scan since the last read (resets): wave tiles (16 items x 16 bins) that ran the refined (seven-digit)
// form, and wave tiles walked.  BAZ_MUSIC_E_UNSUPPORTED where that scan does not exist for the configuration.
int baz_music_debug_i8_stats(baz_music_ctx* c, uint64_t* refined_tiles, uint64_t* tiles)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (!c->dI8Stat || c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    unsigned long long v[2] = {0, 0};
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(v, c->dI8Stat, sizeof(v), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemsetAsync(c->dI8Stat, 0, sizeof(v), c->stream));
    if (refined_tiles) *refined_tiles = v[0];
    if (tiles) *tiles = v[1];
    return BAZ_MUSIC_OK;
}

#ifdef BAZ_MUSIC_LAB
// lab: the s_memtime sums of scan_i8_kernel's ABL 8192 instrumentation since the last read (wait, stores, barrier, whole loop; per wave, summed)
extern "C" __attribute__((visibility("default"))) int baz_music_debug_i8_times(baz_music_ctx* c, uint64_t out[4])
{
    if (!c || !c->dI8Stat) return BAZ_MUSIC_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    unsigned long long v[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(v, c->dI8Stat + 4, sizeof(v), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemsetAsync(c->dI8Stat + 4, 0, sizeof(v), c->stream));
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return BAZ_MUSIC_OK;
}
#endif

// 1 when this context's scan runs on the int8 matrix core (6 <= m <= 16, n <= 4, a table whose digit image exists, not
// BAZ_MUSIC_EXACT=1), else 0.  With smoothing on: the answer of the inner context, whose scan runs.
int baz_music_uses_i8_scan(const baz_music_ctx* c)
{
    if (c && c->sm.inner) return baz_music_uses_i8_scan(c->sm.inner);
    return (c && !c->wide && (i8_active(c) || i8p_active(c))) ? 1 : 0;
}

// HOST-ONLY tap (no device needed): the bin ranges per item i8_nsplit() chooses for a launch of `batch` items over `nsteps`
// 64-bin steps on a device with `slots` resident workgroups (CUs x workgroups per CU).
uint32_t baz_music_debug_i8_nsplit(uint32_t batch, uint32_t nsteps, uint32_t slots)
{
    return i8_nsplit(batch, nsteps, std::max<uint32_t>(1u, slots), 0);
}

// HOST-ONLY tap (no device needed): the digit images and parameters build_i8_image() produces for a table.  Returns the
// images' size in bytes (also when `out` is NULL or too small: nothing is written then), 0 when the table has no image.
// params[0 .. 6] = level weights, [7] = 2^54, [8] = T, [9] = E5, [10] = allowance of the refined form, [11] = 5, [12] = 7,
// [13] = E4, [14] = T4 (as the float the kernel compares with).
size_t baz_music_debug_i8_image(uint32_t m, uint32_t resolution, const float* table_ri, uint8_t* out, size_t out_bytes,
                                double* params)
{
    if (!table_ri || m < 6 || m > BAZ_MUSIC_FAST_M || resolution == 0) return 0;
    std::vector<double> F;
    build_F(table_ri, m, resolution, F);
    std::vector<uint8_t> img;
    I8Params ip = {};
    if (!build_i8_image(F, m, resolution, (resolution + 63) / 64, img, ip)) return 0;
    if (params) {
        for (int l = 0; l < I8_ND; ++l) params[l] = ip.wt[l];
        params[7] = ip.sq; params[8] = ip.t_acc; params[9] = ip.e_bound; params[10] = ip.e_refined;
        params[11] = (double)I8_NS; params[12] = (double)I8_ND;
        params[13] = ip.e4_bound; params[14] = (double)ip.t4_f;
    }
    if (out && out_bytes >= img.size()) std::memcpy(out, img.data(), img.size());
    return img.size();
}

// ---- the table images: what the device builders produced (active set) against the former host builders -------------------
// which: 0 FB, 1 TB, 2 coarse (C then X), 3 int8 digits (0 .. 4 then 5, 6), 4 ||a||^2 padded, 5 transposed table (m > 16),
// 6 ||a||^2 plain (m > 16), 7 the parameters as BAZ_MUSIC_TABLE_NPARAMS doubles.  Returns the image's size in bytes (0: this
// configuration has no such image); written when out_bytes suffices.
namespace {
constexpr int TABLE_NPARAMS = 22;
void pack_table_params(const TableSet& T, bool has_cs, bool has_i8, double* p)
{
    for (int i = 0; i < TABLE_NPARAMS; ++i) p[i] = 0.0;
    p[0] = T.refine_below;
    if (has_cs && T.cs_ok) { p[1] = 1.0; p[2] = T.cs.sc_up; p[3] = T.cs.es_factor; p[4] = T.cs.sc; p[5] = T.cs.fmax; }
    if (has_i8 && T.i8_ok) {
        p[6] = 1.0;
        for (int l = 0; l < I8_ND; ++l) p[7 + l] = T.i8.wt[l];
        p[14] = T.i8.sq; p[15] = T.i8.t_acc; p[16] = T.i8.e_bound; p[17] = T.i8.e_refined; p[18] = T.i8.ws_f;
        p[19] = T.i8.t_acc_f; p[20] = T.i8.t4_f; p[21] = T.i8.e4_bound;
    }
}
}  // namespace

size_t baz_music_debug_table_image(baz_music_ctx* c, int which, void* out, size_t out_bytes)
{
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (which >= BAZ_MUSIC_TABLE_IMAGE_INNER)   // beamspace on: the images of the projected table, held by the inner context
        return beamspace_on(c) ? baz_music_debug_table_image(c->sm.inner, which - BAZ_MUSIC_TABLE_IMAGE_INNER, out, out_bytes) : 0;
    DeviceGuard guard(c->device);
    const size_t pad_steps = (size_t)c->fb_steps + 2;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case 0: src = c->tab.dFB; bytes = pad_steps * c->fb_step_elems * sizeof(double2); break;
        case 1: src = c->tab.dTB; bytes = pad_steps * c->tb_step_elems * sizeof(double2); break;
        case 2: src = c->tab.dCS; bytes = c->tab.dCS ? coarse_image_bytes(c) : 0; break;
        case 3: src = c->tab.dIB; bytes = c->tab.dIB ? i8_image_bytes(c->m, c->fb_steps) : 0; break;
        case 4: src = c->tab.dA2p; bytes = pad_steps * 64 * sizeof(double); break;
        case 5: src = c->tab.dTA; bytes = (size_t)c->m * c->res * sizeof(float2); break;
        case 6: src = c->tab.dA2; bytes = (size_t)c->res * sizeof(double); break;
#ifdef BAZ_MUSIC_LAB
        case 8: src = c->tab.dIP; bytes = c->tab.dIP ? i8p_image_bytes(c->fb_steps) : 0; break;
#endif
        case 7: {
            double p[TABLE_NPARAMS];
#ifdef BAZ_MUSIC_LAB
            const bool any_i8 = c->tab.dIB != nullptr || c->tab.dIP != nullptr;
#else
            const bool any_i8 = c->tab.dIB != nullptr;
#endif
            pack_table_params(c->tab, c->tab.dCS != nullptr, any_i8, p);
            if (out && out_bytes >= sizeof(p)) std::memcpy(out, p, sizeof(p));
            return sizeof(p);
        }
        default: return 0;
    }
    if (!src) return 0;
    // an image whose parameters could not be formed is not built (its bytes are whatever the buffer held): report it as absent
    if ((which == 2 && !c->tab.cs_ok) || ((which == 3 || which == 8) && !c->tab.i8_ok)) return 0;
    if (out && out_bytes >= bytes) {
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
    }
    return bytes;
}

// HOST-ONLY (no device needed): the same image from the round-4 host builders -- the checker of the device builders.
size_t baz_music_debug_host_table_image(uint32_t m, uint32_t n, uint32_t resolution, const float* table_ri, int which, void* out,
                                        size_t out_bytes)
{
    if (!table_ri || m == 0 || n == 0 || n >= m || m > BAZ_MUSIC_MAX_M || resolution == 0) return 0;
    const bool wide = m > BAZ_MUSIC_FAST_M;
    const uint32_t res = resolution, steps = (res + 63) / 64;
    std::vector<uint8_t> bytes;
    auto from_doubles = [&](const std::vector<double>& v) {
        bytes.resize(v.size() * sizeof(double));
        std::memcpy(bytes.data(), v.data(), bytes.size());
    };
    auto a2_of = [&](uint32_t b) { return baztab::tab_a2(table_ri + 2 * (size_t)b * m, m); };   // the device builders' own routine (contraction off)
    const bool has_cs = !wide && m <= 8;
    const bool has_i8 = !wide && m >= 6 && n <= 4 && i8_image_bytes(m, steps) <= I8_IMAGE_LIMIT;
    [[maybe_unused]] const bool has_i8p = m <= 4 && n <= 4;
    const bool has_a2p = wide ? (n <= 8) : short_form_applies(m, n);
    const bool has_tb = wide ? (n <= 8) : true;
    std::vector<double> F;
    if (!wide && (which == 0 || which == 2 || which == 3 || which == 7 || which == 8)) build_F(table_ri, m, res, F);
    switch (which) {
        case 0: {
            if (wide) return 0;
            std::vector<double> FB;
            build_FB(F, m, res, steps, FB);
            from_doubles(FB);
            break;
        }
        case 1: {
            if (!has_tb) return 0;
            std::vector<double> TB;
            build_TB(table_ri, m, res, steps, TB);
            from_doubles(TB);
            break;
        }
        case 2: {
            if (!has_cs) return 0;
            CoarseParams cp = {0.0f, 0.0f, 0.0, 0.0, 1};
            if (!build_coarse_image(F, m, res, round_up((res + 15) / 16, 8), bytes, cp)) return 0;
            break;
        }
        case 3: {
            if (!has_i8) return 0;
            I8Params ip = {};
            if (!build_i8_image(F, m, res, steps, bytes, ip)) return 0;
            break;
        }
#ifdef BAZ_MUSIC_LAB
        case 8: {
            if (!has_i8p) return 0;
            I8Params ip = {};
            if (!build_i8p_image(F, m, res, steps, bytes, ip)) return 0;
            break;
        }
#endif
        case 4: {
            if (!has_a2p) return 0;
            std::vector<double> a2((size_t)(steps + 2) * 64, 1e300);
            for (uint32_t b = 0; b < res; ++b) a2[64 + b] = a2_of(b);
            from_doubles(a2);
            break;
        }
        case 5: {
            if (!wide) return 0;
            std::vector<float> ta((size_t)m * res * 2);
            for (uint32_t b = 0; b < res; ++b)
                for (uint32_t i = 0; i < m; ++i) {
                    ta[2 * ((size_t)i * res + b)] = table_ri[2 * ((size_t)b * m + i)];
                    ta[2 * ((size_t)i * res + b) + 1] = table_ri[2 * ((size_t)b * m + i) + 1];
                }
            bytes.resize(ta.size() * sizeof(float));
            std::memcpy(bytes.data(), ta.data(), bytes.size());
            break;
        }
        case 6: {
            if (!wide) return 0;
            std::vector<double> a2(res);
            for (uint32_t b = 0; b < res; ++b) a2[b] = a2_of(b);
            from_doubles(a2);
            break;
        }
        case 7: {
            TableSet T;
            double amax2 = 0.0;
            for (uint32_t b = 0; b < res; ++b) {
                const double a2 = a2_of(b);
                if (a2 > amax2 && a2 < 1e300) amax2 = a2;
            }
            T.refine_below = amax2 * (double)m * 1e-8;
            std::vector<uint8_t> scratch;
            if (has_cs) T.cs_ok = build_coarse_image(F, m, res, round_up((res + 15) / 16, 8), scratch, T.cs);
            if (has_i8) T.i8_ok = build_i8_image(F, m, res, steps, scratch, T.i8);
            // (the packed operands of m <= 4 exist in lab contexts only -- BAZ_MUSIC_I8P=1 --: their parameters are not part of this image)
            std::vector<double> p(TABLE_NPARAMS);
            pack_table_params(T, has_cs, has_i8, p.data());
            from_doubles(p);
            break;
        }
        default: return 0;
    }
    if (out && out_bytes >= bytes.size()) std::memcpy(out, bytes.data(), bytes.size());
    return bytes.size();
}

// The gated scan's sorting policy: out[0] / out[1] = gated-scan launches that sorted / did not sort their items first, out[2] / out[3] = exact
// evaluations and (row group, tile) pairs walked of the most recent FINISHED gated launch, out[4] = 1 if that launch was sorted.  Synchronises.
int baz_music_debug_sort_state(baz_music_ctx* c, uint64_t out[5])
{
    if (!c || !out) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
#ifdef BAZ_MUSIC_LAB
    out[0] = c->sorted_calls; out[1] = c->unsorted_calls;
    out[2] = c->hFire ? c->hFire[0] : 0; out[3] = c->hFire ? c->hFire[1] : 0; out[4] = c->hFire ? (c->hFire[2] & 1ull) : 0;
#else
    for (int k = 0; k < 5; ++k) out[k] = 0;               // the release library never sorts and keeps no fire statistic
#endif
    return BAZ_MUSIC_OK;
}

int baz_music_debug_evd(baz_music_ctx* c, const void* d_R, uint32_t batch, void* d_Q)
{
    if (!c || !d_R || !d_Q || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->wide || c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    return launch_evd(c, static_cast<const double2*>(d_R), batch, static_cast<double*>(d_Q), baz_music_q_stride(batch), nullptr);
}

uint64_t baz_music_bytes_per_item(const baz_music_ctx* c, int with_spectrum)
{
    if (!c) return 0;
    return 8ull * c->nsamples + 8ull * c->n + (with_spectrum ? 4ull * c->res : 0ull);
}

// Lab build with BAZ_MUSIC_GUARD=1: checks the guard zones of every live device buffer of this library (synchronises the device) and returns
// the number of zones found damaged since the process started (at this check or at an earlier free); 0 when the guard is off / in the release build.
int baz_music_debug_guard_check(void)
{
#ifdef BAZ_MUSIC_LAB
    if (!guard_on()) return 0;
    std::lock_guard<std::mutex> lk(g_guard_mtx);
    unsigned long long now = 0;
    for (const auto& g : g_guards) now += (unsigned long long)guard_check_one(g.first, g.second);
    return (int)std::min<unsigned long long>(g_guard_damaged + now, 0x7FFFFFFFull);
#else
    return 0;
#endif
}

// 1 when this library allocates with guard zones (lab build, BAZ_MUSIC_GUARD=1), else 0
int baz_music_debug_guard_active(void)
{
#ifdef BAZ_MUSIC_LAB
    return guard_on() ? 1 : 0;
#else
    return 0;
#endif
}

// the library's live device / page-locked allocations in this process (device_buffer.hip.h counts them where they are made and released)
void baz_music_debug_live_buffers(uint64_t out[2])
{
    if (out) bazbuf::g_live.report(out);
}

const char* baz_music_strerror(int code)
{
    switch (code) {
        case BAZ_MUSIC_OK: return "ok";
        case BAZ_MUSIC_E_INVALID: return "invalid argument";
        case BAZ_MUSIC_E_NOMEM: return "out of memory";
        case BAZ_MUSIC_E_HIP: return "HIP runtime error";
        case BAZ_MUSIC_E_UNSUPPORTED:
            return "configuration not supported by the gfx950 kernels (limits: m <= 64 antennas -- specialised kernels up "
                   "to 16, run-time-m kernels from 17 to 64 --, n < m emitters, resolution <= 1048576 bins, the local-maximum "
                   "picker only up to 16 antennas; the reference itself has none, lib/baz_music_doa.cc:45-50)";
        case BAZ_MUSIC_E_NODEVICE: return "no usable gfx950 device";
        default: return "unknown error";
    }
}

const char* baz_music_last_hip_error(const baz_music_ctx* c) { return c ? c->hip_err : ""; }

const char* baz_music_version(void) { return "gr_baz_amd/baz_music_hip 0.1 (gfx950)"; }

int baz_music_device_count(void)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int usable = 0;
    for (int d = 0; d < ndev; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++usable;
        else break;   // device ids must stay dense: stop at the first foreign device
    }
    return usable;
}

int baz_music_set_peak_mode(baz_music_ctx* c, int mode)
{
    if (!c || (mode != 0 && mode != 1)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (mode && c->wide && !beamspace_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // the opt-in picker exists for the specialised kernels only (beamspace: the inner context runs them)
    if (c->sm.inner && !subband_on(c)) {   // (the inner context is never wider than this one; subband: the picker of THIS context reads the combined row)
        const int r = baz_music_set_peak_mode(c->sm.inner, mode);
        if (r != BAZ_MUSIC_OK) return r;
    }
    c->peak_mode = mode;
    return BAZ_MUSIC_OK;
}

int64_t baz_music_refined_items(baz_music_ctx* c) { return baz_music_refined_values(c); }

int64_t baz_music_refined_values(baz_music_ctx* c)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    if (!c->dRefined) return 0;
    unsigned long long n = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(&n, c->dRefined + c->stat_parity, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)n;
}

int baz_music_device(const baz_music_ctx* c) { return c ? c->device : BAZ_MUSIC_E_INVALID; }

int baz_music_smoothing_check(uint32_t m, uint32_t resolution, const float* table_ri, uint32_t subarray, int forward_backward,
                              uint8_t* perm_out)
{
    return smoothing_check(m, resolution, table_ri, subarray, forward_backward ? 1 : 0, perm_out);
}

int baz_music_set_smoothing(baz_music_ctx* c, uint32_t subarray, int forward_backward)
{
    if (!c || subarray < 2 || subarray > c->m || subarray <= c->n) return BAZ_MUSIC_E_INVALID;
    const int fb = forward_backward ? 1 : 0;
    std::lock_guard<std::mutex> tl(c->tab_mtx);   // against set_table: c->hRaw is the table in force while it is held
    DeviceGuard guard(c->device);
    baz_music_ctx* old = nullptr;
    if (c->sm.inner && c->sm.kind != baz_music_ctx::FRONT_SMOOTHING)   // (two front-ends would compete for one inner context; sm changes under tab_mtx + mtx)
        return (subarray == c->m && !fb) ? BAZ_MUSIC_OK : BAZ_MUSIC_E_UNSUPPORTED;
    if (subarray == c->m && !fb) {                // off: the reference
        {
            std::lock_guard<std::mutex> lk(c->mtx);
            old = c->sm.inner;
            c->sm.inner = nullptr;
            c->sm.ms = 0; c->sm.L = 1; c->sm.Kp = 0; c->sm.fb = 0;
            c->avg_hist = 0;                      // (averaging: the shape of R changes, the history starts over)
        }
        baz_music_destroy(old);                   // (drains the stream first: batches in flight may still use it)
        return BAZ_MUSIC_OK;
    }
    {   // (the beam mode has no m-antenna weight vector for the inner context's re-stacked items)
        std::lock_guard<std::mutex> lk(c->mtx);
        if (c->beam_mode || c->estimator) return BAZ_MUSIC_E_UNSUPPORTED;   // (nor does the estimator choice reach the inner context)
    }
    if (c->calib_on) return BAZ_MUSIC_E_UNSUPPORTED;   // (raw data under Gamma != c I is not shift invariant; calib_on changes under tab_mtx)
    if (c->wh_on) return BAZ_MUSIC_E_UNSUPPORTED;      // (nor is the whitened table W a; wh_on changes under tab_mtx)
    bazsmooth::Perm perm = {};
    if (smoothing_check(c->m, c->res, c->hRaw, subarray, fb, perm.p) != BAZ_MUSIC_OK) return BAZ_MUSIC_E_INVALID;
    const uint32_t L = c->m - subarray + 1;
    const uint64_t Kp = (uint64_t)L * c->K * (fb ? 2u : 1u);
    if (Kp * subarray > (1ull << 31)) return BAZ_MUSIC_E_UNSUPPORTED;   // the re-stacked item's length must fit its 32-bit indexing
    const std::vector<float> sub = sub_table(c->hRaw, c->m, c->res, subarray);
    baz_music_ctx* inner = nullptr;
    int r = baz_music_create(&inner, subarray, c->n, (uint32_t)(Kp * subarray), c->res, sub.data(), c->device);
    if (r != BAZ_MUSIC_OK) return r;
    {
        std::lock_guard<std::mutex> lk(c->mtx);   // a batch sees the old mode or the new one
        r = (c->beam_mode || c->estimator) ? BAZ_MUSIC_E_UNSUPPORTED : baz_music_set_stream(inner, c->stream);   // (set_beam_mode / set_estimator may have come in between)
        if (r == BAZ_MUSIC_OK) r = baz_music_set_peak_mode(inner, c->peak_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_order_mode(inner, c->order_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_refine_mode(inner, c->refine_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_power_mode(inner, c->power_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_averaging(inner, c->avg_window, c->avg_beta);   // (a new inner context: an empty history)
        if (r == BAZ_MUSIC_OK) {
            inner->order_nsnap = c->K;            // N of the criterion: this context's snapshots, not the K' re-stacked columns
            inner->ord_driven = true;
            c->out_beam.on = false;               // (calls under smoothing run with the beam mode off: last_beams reports zeros)
            c->out_beam.count = 0;
            old = c->sm.inner;
            c->sm.inner = inner;
            c->sm.kind = baz_music_ctx::FRONT_SMOOTHING;
            c->sm.ms = subarray; c->sm.L = L; c->sm.Kp = (uint32_t)Kp; c->sm.fb = fb;
            c->sm.perm = perm;
            inner = nullptr;
        }
    }
    baz_music_destroy(inner);                     // (only after a failure)
    baz_music_destroy(old);
    return r;
}

int baz_music_set_order_mode(baz_music_ctx* c, int criterion)
{
    if (!c || criterion < 0 || criterion > 2) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (criterion && c->wide && !beamspace_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // the ORDER epilogues exist for the specialised kernels only
    if (criterion && c->estimator) return BAZ_MUSIC_E_UNSUPPORTED;   // (Capon / Bartlett compute no eigenvalues)
    if (criterion && subband_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;  // (one count per subband: no rule combines them here)
    if (c->sm.inner) {   // (the inner context is never wider than this one)
        const int r = baz_music_set_order_mode(c->sm.inner, criterion);
        if (r != BAZ_MUSIC_OK) return r;
    }
    c->order_mode = criterion;
    return BAZ_MUSIC_OK;
}

int baz_music_get_order_mode(const baz_music_ctx* c, int* criterion)
{
    if (!c || !criterion) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    *criterion = c->order_mode;
    return BAZ_MUSIC_OK;
}

int baz_music_last_orders(baz_music_ctx* c, uint8_t* out, uint32_t count)
{
    if (!c || (!out && count)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (c->sm.inner) return baz_music_last_orders(c->sm.inner, out, count);
    return side_read(c, c->out_ord, 0, out, count, 1, (int)c->n, c->call_items);   // (mode off: every item used the context's n)
}

const void* baz_music_last_orders_device(baz_music_ctx* c)
{
    if (!c) return nullptr;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (c->sm.inner) return baz_music_last_orders_device(c->sm.inner);
    DeviceGuard guard(c->device);
    SideOut::Buf& b = c->out_ord.buf[0];
    if (c->out_ord.on) return c->out_ord.count ? b.p : nullptr;
    if (!c->call_items) return nullptr;
    // the call ran with the mode off: the same bytes as baz_music_last_orders, filled here (nothing on the process path)
    if (grow_bytes(c, b.p, c->call_items) != BAZ_MUSIC_OK) return nullptr;
    if (hipMemsetAsync(b.p, (int)c->n, c->call_items, c->stream) != hipSuccess) return nullptr;
    return b.p;
}

int baz_music_order_estimate(uint32_t m, uint32_t nsnap, uint32_t n_max, int criterion, const double* eigvals_ascending,
                             uint32_t count, uint8_t* out)
{
    if (m == 0 || m > BAZ_MUSIC_MAX_M || n_max >= m || nsnap == 0 || (criterion != 1 && criterion != 2) ||
        (count && (!eigvals_ascending || !out)))
        return BAZ_MUSIC_E_INVALID;
    for (uint32_t it = 0; it < count; ++it) {
        const double* l = eigvals_ascending + (size_t)it * m;
        out[it] = (uint8_t)bazorder::order_decide<0>((int)m, (int)n_max, (double)nsnap, criterion, [&](int i) { return l[i]; });
    }
    return BAZ_MUSIC_OK;
}

int baz_music_set_refine_mode(baz_music_ctx* c, int mode)
{
    if (!c || (mode != 0 && mode != 1)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (mode && c->wide && !beamspace_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // no peak picker on the run-time-m path: only first entries would move
    if (mode && c->estimator) return BAZ_MUSIC_E_UNSUPPORTED;   // (the fit is on the MUSIC denominator)
    if (mode && subband_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;  // (the combined row has no single denominator to fit)
    if (c->sm.inner) {   // (the inner context is never wider than this one)
        const int r = baz_music_set_refine_mode(c->sm.inner, mode);
        if (r != BAZ_MUSIC_OK) return r;
    }
    c->refine_mode = mode;
    return BAZ_MUSIC_OK;
}

int baz_music_get_refine_mode(const baz_music_ctx* c, int* mode)
{
    if (!c || !mode) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    *mode = c->refine_mode;
    return BAZ_MUSIC_OK;
}

int baz_music_last_refine_offsets(baz_music_ctx* c, double* out, uint32_t count)
{
    if (!c || (!out && count)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (c->sm.inner) return baz_music_last_refine_offsets(c->sm.inner, out, count);
    return side_read(c, c->out_ref, 0, out, count, c->n, 0, c->call_items);        // (mode off: nothing moved)
}

int baz_music_refine_estimate(const double* y3, uint32_t count, double* delta_out)
{
    if (count && (!y3 || !delta_out)) return BAZ_MUSIC_E_INVALID;
    for (uint32_t k = 0; k < count; ++k) delta_out[k] = bazrefine::refine_decide(y3[3 * (size_t)k], y3[3 * (size_t)k + 1], y3[3 * (size_t)k + 2]);
    return BAZ_MUSIC_OK;
}

int baz_music_set_averaging(baz_music_ctx* c, uint32_t window, double forgetting)
{
    if (!c || window == 0 || window > BAZ_MUSIC_MAX_AVG_WINDOW || !(forgetting > 0.0) || !(forgetting <= 1.0)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner) {            // smoothing on: the inner context averages (and keeps the history); this one only remembers the mode
        const int r = each_inner(c, [&](baz_music_ctx* in) { return baz_music_set_averaging(in, window, forgetting); });   // (subband: each its own stream)
        if (r != BAZ_MUSIC_OK) return r;
    } else if (window > 1) {      // the history buffers, before anything changes: after an error the previous mode and history stay in force
        const int r = ensure_average(c, window, 0);
        if (r != BAZ_MUSIC_OK) return r;
    }
    if (window == c->avg_window && forgetting == c->avg_beta) return BAZ_MUSIC_OK;    // nothing changes: the history stays
    c->avg_window = window;
    c->avg_beta = forgetting;
    c->avg_neff = bazavg::averaging_table(window, forgetting, c->avg_tab);
    c->avg_hist = 0;
    return BAZ_MUSIC_OK;
}

int baz_music_get_averaging(const baz_music_ctx* c, uint32_t* window, double* forgetting)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    if (window) *window = c->avg_window;
    if (forgetting) *forgetting = c->avg_beta;
    return BAZ_MUSIC_OK;
}

int baz_music_reset_averaging(baz_music_ctx* c)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    c->avg_hist = 0;
    return each_inner(c, [](baz_music_ctx* in) { return baz_music_reset_averaging(in); });
}

int baz_music_averaging_weights(uint32_t window, double forgetting, double* w, double* inv_norm, double* n_eff)
{
    if (window == 0 || window > BAZ_MUSIC_MAX_AVG_WINDOW || !(forgetting > 0.0) || !(forgetting <= 1.0)) return BAZ_MUSIC_E_INVALID;
    bazavg::AvgTable t;
    const double ne = bazavg::averaging_table(window, forgetting, t);
    if (w) std::memcpy(w, t.w, window * sizeof(double));
    if (inv_norm) std::memcpy(inv_norm, t.inv_norm, ((size_t)window + 1) * sizeof(double));
    if (n_eff) *n_eff = ne;
    return BAZ_MUSIC_OK;
}

int baz_music_debug_average(baz_music_ctx* c, const void* d_R_in, uint32_t batch, void* d_R_out)
{
    if (!c || !d_R_in || !d_R_out || d_R_in == d_R_out || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner || c->avg_window <= 1) return BAZ_MUSIC_E_UNSUPPORTED;
    (void)hipGetLastError();
    int r = ensure_average(c, c->avg_window, 0);
    if (r == BAZ_MUSIC_OK) r = launch_average(c, static_cast<const double2*>(d_R_in), batch, static_cast<double2*>(d_R_out));
    if (r != BAZ_MUSIC_OK) c->avg_hist = 0;
    return r;
}

int baz_music_set_power_mode(baz_music_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 2) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (mode && c->wide && !beamspace_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // (power_kernel is specialised per m, like the pickers it follows)
    if (mode && subband_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // (a power per subband: no single covariance to solve on)
    if (c->sm.inner) {   // (the inner context is never wider than this one)
        const int r = baz_music_set_power_mode(c->sm.inner, mode);
        if (r != BAZ_MUSIC_OK) return r;
    }
    c->power_mode = mode;
    return BAZ_MUSIC_OK;
}

int baz_music_get_power_mode(const baz_music_ctx* c, int* mode)
{
    if (!c || !mode) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    *mode = c->power_mode;
    return BAZ_MUSIC_OK;
}

int baz_music_last_powers(baz_music_ctx* c, double* out, uint32_t count)
{
    if (!c || (!out && count)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (c->sm.inner) return baz_music_last_powers(c->sm.inner, out, count);
    return side_read(c, c->out_pow, 0, out, count, c->n, 0, c->call_items);        // (mode off: nothing was estimated)
}

// The definition of include/baz_music_hip.h on the host (bazcapon::HostSolve); the degeneracy rule and the s -> P step are the kernel's own text.
int baz_music_power_estimate(uint32_t m, const double* R_ri, const float* a_ri, uint32_t count, double* out)
{
    if (m < 1 || m > BAZ_MUSIC_MAX_M) return BAZ_MUSIC_E_INVALID;
    if (count == 0) return BAZ_MUSIC_OK;
    if (!R_ri || !a_ri || !out) return BAZ_MUSIC_E_INVALID;
    bazcapon::HostSolve S(m, R_ri, nullptr, BAZ_MUSIC_POWER_PIVOT_FLOOR);
    for (uint32_t e = 0; e < count; ++e) out[e] = S.ok ? bazcapon::power_from_s(S.solve(a_ri + 2 * (size_t)e * m)) : 0.0;
    return BAZ_MUSIC_OK;
}

int baz_music_set_estimator(baz_music_ctx* c, int kind)
{
    if (!c || kind < BAZ_MUSIC_ESTIMATOR_MUSIC || kind > BAZ_MUSIC_ESTIMATOR_BARTLETT) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (kind && c->wide && !beamspace_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // (spectrum_scan_kernel is specialised per m, like the other modes' kernels)
    // the emitter-count mode needs eigenvalues, refinement fits the MUSIC denominator, smoothing runs an inner MUSIC context
    if (kind && (c->order_mode || c->refine_mode || (c->sm.inner && !beamspace_on(c) && !subband_on(c)))) return BAZ_MUSIC_E_UNSUPPORTED;
    if (kind && c->wh_want) return BAZ_MUSIC_E_UNSUPPORTED;   // (whitening on: Capon is invariant under the transform, nothing is gained)
    if (beamspace_on(c) || subband_on(c)) {   // beamspace: the inner context evaluates the estimator on the projected items; subband: all S do
        const int r = each_inner(c, [&](baz_music_ctx* in) { return baz_music_set_estimator(in, kind); });
        if (r != BAZ_MUSIC_OK) return r;
    }
    c->estimator = kind;
    return BAZ_MUSIC_OK;
}

int baz_music_get_estimator(const baz_music_ctx* c, int* kind)
{
    if (!c || !kind) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    *kind = c->estimator;
    return BAZ_MUSIC_OK;
}

// The definitions of include/baz_music_hip.h on the host: Capon through bazcapon::HostSolve exactly as baz_music_power_estimate (the
// same bits), Bartlett through bazspectrum::bartlett_host.
int baz_music_spectrum_estimate(int kind, uint32_t m, const double* R_ri, const float* a_ri, uint32_t count, double* out)
{
    if (kind != BAZ_MUSIC_ESTIMATOR_CAPON && kind != BAZ_MUSIC_ESTIMATOR_BARTLETT) return BAZ_MUSIC_E_INVALID;
    if (kind == BAZ_MUSIC_ESTIMATOR_CAPON) return baz_music_power_estimate(m, R_ri, a_ri, count, out);
    if (m < 1 || m > BAZ_MUSIC_MAX_M) return BAZ_MUSIC_E_INVALID;
    if (count == 0) return BAZ_MUSIC_OK;
    if (!R_ri || !a_ri || !out) return BAZ_MUSIC_E_INVALID;
    for (uint32_t e = 0; e < count; ++e) out[e] = bazspectrum::bartlett_host(m, R_ri, a_ri + 2 * (size_t)e * m);
    return BAZ_MUSIC_OK;
}

int baz_music_set_beam_mode(baz_music_ctx* c, int mode, double loading)
{
    if (!c || mode < 0 || mode > 1 || !(loading - loading == 0.0) || loading < 0.0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (mode && c->wide) return BAZ_MUSIC_E_UNSUPPORTED;   // (the kernels are specialised per m, like the pickers they follow)
    if (mode && c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;   // (smoothing: no m-antenna weight vector for the re-stacked items)
    if (mode && c->wh_want) return BAZ_MUSIC_E_UNSUPPORTED;    // (whitening on: the weights would apply to unwhitened snapshots)
    c->beam_mode = mode;
    c->beam_loading = loading;
    return BAZ_MUSIC_OK;
}

int baz_music_get_beam_mode(const baz_music_ctx* c, int* mode, double* loading)
{
    if (!c || !mode || !loading) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    *mode = c->beam_mode;
    *loading = c->beam_loading;
    return BAZ_MUSIC_OK;
}

namespace {
// The first `items` items of the last call's beams or weights (buffer k): zeros after a mode-off call.
int last_beam_copy(baz_music_ctx* c, void* out, int k, uint32_t items)
{
    // (a mode-off call under smoothing: the inner context counted the call's items)
    return side_read(c, c->out_beam, k, out, items, 1, 0, c->sm.inner ? c->sm.inner->call_items : c->call_items);
}
}  // namespace

int baz_music_last_beams(baz_music_ctx* c, float* out_ri, uint32_t items)
{
    if (!c || (!out_ri && items)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    return last_beam_copy(c, out_ri, baz_music_ctx::BEAM_Y, items);
}

int baz_music_last_beam_weights(baz_music_ctx* c, double* out_ri, uint32_t items)
{
    if (!c || (!out_ri && items)) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    return last_beam_copy(c, out_ri, baz_music_ctx::BEAM_W, items);
}

int baz_music_last_beams_device(baz_music_ctx* c, const void** d_beams, uint32_t* items)
{
    if (!c || !d_beams || !items) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    *d_beams = c->out_beam.on ? c->out_beam.buf[baz_music_ctx::BEAM_Y].p : nullptr;     // (a call made with the mode off has no buffer: 0 items)
    *items = c->out_beam.on ? c->out_beam.count : 0u;
    return BAZ_MUSIC_OK;
}

// The definition of include/baz_music_hip.h on the host (bazcapon::HostSolve on R plus the loading, then the back substitution); the
// degeneracy rule and the s -> w step are the kernels' own text.
int baz_music_beam_weights(uint32_t m, const double* R_ri, const float* a_ri, uint32_t count, double loading, double* w_ri)
{
    if (m < 1 || m > BAZ_MUSIC_MAX_M || !(loading - loading == 0.0) || loading < 0.0) return BAZ_MUSIC_E_INVALID;
    if (count == 0) return BAZ_MUSIC_OK;
    if (!R_ri || !a_ri || !w_ri) return BAZ_MUSIC_E_INVALID;
    bazcapon::HostSolve S(m, R_ri, &loading, BAZ_MUSIC_POWER_PIVOT_FLOOR);
    std::vector<double> ur(m), ui(m);
    for (uint32_t e = 0; e < count; ++e) {
        double* const w = w_ri + 2 * (size_t)e * m;
        if (!S.ok) {
            for (uint32_t i = 0; i < 2 * m; ++i) w[i] = 0.0;
            continue;
        }
        const double s = S.solve(a_ri + 2 * (size_t)e * m);
        for (uint32_t i = m; i-- > 0;) {
            double xr = S.zr[i] / S.d[i], xi = S.zi[i] / S.d[i];
            for (uint32_t k = m - 1; k > i; --k) {   // conj(L_ki) u_k
                xr -= S.Lr[(size_t)k * m + i] * ur[k] + S.Li[(size_t)k * m + i] * ui[k];
                xi -= S.Lr[(size_t)k * m + i] * ui[k] - S.Li[(size_t)k * m + i] * ur[k];
            }
            ur[i] = xr; ui[i] = xi;
        }
        for (uint32_t i = 0; i < m; ++i) bazcapon::beam_w_from_u(ur[i], ui[i], s, true, &w[2 * i], &w[2 * i + 1]);
    }
    return BAZ_MUSIC_OK;
}

namespace {
bool calib_value_ok(const float re, const float im)   // finite and nonzero
{
    return (re - re == 0.0f) && (im - im == 0.0f) && (re != 0.0f || im != 0.0f);
}
bool calib_vector_ok(uint32_t m, const float* v_ri)
{
    for (uint32_t r = 0; r < m; ++r)
        if (!calib_value_ok(v_ri[2 * r], v_ri[2 * r + 1])) return false;
    return true;
}
}  // namespace

int baz_music_set_calibration(baz_music_ctx* c, const float* gamma_ri)
{
    if (!c || (gamma_ri && !calib_vector_ok(c->m, gamma_ri))) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> tl(c->tab_mtx);   // a retune of the table c->hRaw holds; against set_table and set_smoothing
    DeviceGuard guard(c->device);
    if (gamma_ri && c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;   // (sm.inner changes under tab_mtx + mtx: reading it under one is safe)
    if (!gamma_ri && !c->calib_on) return BAZ_MUSIC_OK;            // off and staying off: the images in force are the ones to keep
    const bool old_on = c->calib_on;
    const bazcalib::CalibGamma old_gamma = c->calib_gamma;
    c->calib_on = gamma_ri != nullptr;
    for (uint32_t r = 0; r < c->m; ++r)
        c->calib_gamma.g[r] = gamma_ri ? make_float2(gamma_ri[2 * r], gamma_ri[2 * r + 1]) : make_float2(1.0f, 0.0f);
    const int r = retune(c, nullptr, false);      // (smoothing is off here: it and a calibration exclude each other)
    if (r != BAZ_MUSIC_OK) {                    // the old images stay in force (retune exchanges only after a complete build)
        c->calib_on = old_on;
        c->calib_gamma = old_gamma;
    }
    return r;
}

int baz_music_get_calibration(const baz_music_ctx* c, float* gamma_ri, int* on)
{
    if (!c || !on) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> tl(const_cast<baz_music_ctx*>(c)->tab_mtx);
    *on = c->calib_on ? 1 : 0;
    if (gamma_ri)
        for (uint32_t r = 0; r < c->m; ++r) {
            gamma_ri[2 * r] = c->calib_on ? c->calib_gamma.g[r].x : 1.0f;
            gamma_ri[2 * r + 1] = c->calib_on ? c->calib_gamma.g[r].y : 0.0f;
        }
    return BAZ_MUSIC_OK;
}

// The definition of include/baz_music_hip.h on the host: table_calib_kernel's own routine, entry by entry.
int baz_music_calibration_apply(uint32_t m, uint32_t resolution, const float* table_ri, const float* gamma_ri, float* out_ri)
{
    if (m < 1 || m > BAZ_MUSIC_MAX_M || resolution == 0 || !table_ri || !gamma_ri || !out_ri) return BAZ_MUSIC_E_INVALID;
    if (!calib_vector_ok(m, gamma_ri)) return BAZ_MUSIC_E_INVALID;
    for (size_t b = 0; b < resolution; ++b)
        for (uint32_t r = 0; r < m; ++r) {
            const size_t i = 2 * (b * m + r);
            bazcalib::calib_mul(gamma_ri[2 * r], gamma_ri[2 * r + 1], table_ri[i], table_ri[i + 1], &out_ri[i], &out_ri[i + 1]);
        }
    return BAZ_MUSIC_OK;
}

// gamma-hat and quality from R-bar (include/baz_music_hip.h): a cyclic Hermitian Jacobi in fp64 on the host.  A rotation of the pair
// (p, q) with a_pq = g e^{i phi} is J = diag(1, e^{-i phi}) [[c, s], [-s, c]] with the real Jacobi angle of [[a_pp, g], [g, a_qq]];
// A <- J^H A J, V <- V J.  Pairs at or below 2^-75 of the Frobenius norm are left alone (m^2 of them stay far below the m 2^-52 |A|
// backward error of the rotations themselves); the sweeps end when one rotates nothing.
namespace {
void hermitian_jacobi(uint32_t m, std::vector<std::complex<double>>& A, std::vector<std::complex<double>>& V);
}

int baz_music_calibration_estimate(uint32_t m, const double* Rbar_ri, const float* ref_ri, double* gamma_ri, double* quality)
{
    if (m < 1 || m > BAZ_MUSIC_MAX_M || !Rbar_ri || !ref_ri || !gamma_ri || !quality) return BAZ_MUSIC_E_INVALID;
    if (!calib_vector_ok(m, ref_ri)) return BAZ_MUSIC_E_INVALID;
    typedef std::complex<double> cd;
    auto degenerate = [&]() {
        for (uint32_t r = 0; r < m; ++r) { gamma_ri[2 * r] = 1.0; gamma_ri[2 * r + 1] = 0.0; }
        *quality = 0.0;
        return BAZ_MUSIC_OK;
    };
    double trace = 0.0;
    for (size_t i = 0; i < (size_t)2 * m * m; ++i) {
        if (!(Rbar_ri[i] - Rbar_ri[i] == 0.0)) return degenerate();
    }
    for (uint32_t i = 0; i < m; ++i) trace = trace + Rbar_ri[2 * ((size_t)i * m + i)];
    if (!(trace > 0.0) || !(trace - trace == 0.0)) return degenerate();
    // (scaled by a power of two so that squares neither overflow nor vanish: exact, and the eigenvectors do not change)
    int ex = 0;
    (void)frexp(trace, &ex);
    std::vector<cd> A((size_t)m * m), V((size_t)m * m, cd(0.0, 0.0));
    for (uint32_t p = 0; p < m; ++p) {
        V[(size_t)p * m + p] = cd(1.0, 0.0);
        A[(size_t)p * m + p] = cd(ldexp(Rbar_ri[2 * ((size_t)p * m + p)], -ex), 0.0);
        for (uint32_t q = p + 1; q < m; ++q) {
            const cd a(ldexp(Rbar_ri[2 * ((size_t)p * m + q)], -ex), ldexp(Rbar_ri[2 * ((size_t)p * m + q) + 1], -ex));
            A[(size_t)p * m + q] = a;
            A[(size_t)q * m + p] = std::conj(a);
        }
    }
    hermitian_jacobi(m, A, V);
    uint32_t top = 0;
    for (uint32_t p = 1; p < m; ++p)
        if (A[(size_t)p * m + p].real() > A[(size_t)top * m + top].real()) top = p;
    const double l1 = ldexp(A[(size_t)top * m + top].real(), ex);
    double vn = 0.0;
    for (uint32_t r = 0; r < m; ++r) vn = vn + std::norm(V[(size_t)r * m + top]);
    vn = std::sqrt(vn);
    const cd v0 = V[(size_t)0 * m + top];
    if (v0 == cd(0.0, 0.0) || !(vn > 0.0)) return degenerate();
    std::vector<cd> gh(m);
    for (uint32_t r = 0; r < m; ++r) gh[r] = (V[(size_t)r * m + top] / vn) / cd((double)ref_ri[2 * r], (double)ref_ri[2 * r + 1]);
    const double a0 = std::abs(gh[0]);
    if (!(a0 > 0.0) || !(a0 - a0 == 0.0)) return degenerate();
    const cd rot = std::conj(gh[0]) / a0;
    double s2 = 0.0;
    for (uint32_t r = 0; r < m; ++r) {
        gh[r] = r == 0 ? cd(a0, 0.0) : gh[r] * rot;
        s2 = s2 + std::norm(gh[r]);
    }
    const double scale = 1.0 / std::sqrt(s2 / (double)m);
    for (uint32_t r = 0; r < m; ++r) {
        gamma_ri[2 * r] = gh[r].real() * scale;
        gamma_ri[2 * r + 1] = r == 0 ? 0.0 : gh[r].imag() * scale;
    }
    *quality = l1 / trace;
    return BAZ_MUSIC_OK;
}

namespace {
// The cyclic Hermitian Jacobi of the comment above, on the host in fp64: A (m x m, Hermitian, row-major) becomes diagonal, V (the
// identity on entry) collects the rotations: its columns are the eigenvectors.  Shared by the calibration estimate and the beamspace design.
void hermitian_jacobi(const uint32_t m, std::vector<std::complex<double>>& A, std::vector<std::complex<double>>& V)
{
    typedef std::complex<double> cd;
    double frob2 = 0.0;
    for (const cd& a : A) frob2 += std::norm(a);
    const double small = ldexp(std::sqrt(frob2), -75);
    for (int sweep = 0; sweep < 64; ++sweep) {
        bool rotated = false;
        for (uint32_t p = 0; p + 1 < m; ++p)
            for (uint32_t q = p + 1; q < m; ++q) {
                const cd apq = A[(size_t)p * m + q];
                const double g = std::abs(apq);
                if (!(g > small)) continue;
                rotated = true;
                const cd ph = apq / g;                            // e^{i phi}
                const double app = A[(size_t)p * m + p].real(), aqq = A[(size_t)q * m + q].real();
                const double tau = (aqq - app) / (2.0 * g);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
                const cd jqp = -sn * std::conj(ph), jqq = cs * std::conj(ph);   // J = [[cs, sn], [jqp, jqq]]
                for (uint32_t k = 0; k < m; ++k) {                 // A <- A J, V <- V J (columns p, q)
                    const cd akp = A[(size_t)k * m + p], akq = A[(size_t)k * m + q];
                    A[(size_t)k * m + p] = akp * cs + akq * jqp;
                    A[(size_t)k * m + q] = akp * sn + akq * jqq;
                    const cd vkp = V[(size_t)k * m + p], vkq = V[(size_t)k * m + q];
                    V[(size_t)k * m + p] = vkp * cs + vkq * jqp;
                    V[(size_t)k * m + q] = vkp * sn + vkq * jqq;
                }
                for (uint32_t k = 0; k < m; ++k) {                 // A <- J^H A (rows p, q)
                    const cd apk = A[(size_t)p * m + k], aqk = A[(size_t)q * m + k];
                    A[(size_t)p * m + k] = cs * apk + std::conj(jqp) * aqk;
                    A[(size_t)q * m + k] = sn * apk + std::conj(jqq) * aqk;
                }
                A[(size_t)p * m + q] = cd(0.0, 0.0);
                A[(size_t)q * m + p] = cd(0.0, 0.0);
                A[(size_t)p * m + p] = cd(A[(size_t)p * m + p].real(), 0.0);
                A[(size_t)q * m + q] = cd(A[(size_t)q * m + q].real(), 0.0);
            }
        if (!rotated) break;
    }
}
}  // namespace

// ---- opt-in beamspace front-end: the host side (include/baz_music_hip.h; beamspace_kernels.hip.h) ----------------------------------
int baz_music_beamspace_apply(uint32_t m, uint32_t B, const double* T_ri, int normalise, const float* in_ri, uint32_t columns, float* out_ri)
{
    if (m < 2 || m > BAZ_MUSIC_MAX_M || B < 1 || B > m || B > BAZ_MUSIC_FAST_M || !T_ri) return BAZ_MUSIC_E_INVALID;
    if (columns == 0) return BAZ_MUSIC_OK;
    if (!in_ri || !out_ri) return BAZ_MUSIC_E_INVALID;
    beamspace_apply_host(m, B, T_ri, normalise, in_ri, columns, out_ri);
    return BAZ_MUSIC_OK;
}

// C = sum over the sector's bins of a a^H in fp64, decomposed by hermitian_jacobi (scaled by a power of two first, as the calibration
// estimate does: exact, and the eigenvectors do not change); T = the eigenvectors of the B largest eigenvalues, descending (ties: the
// lower Jacobi column first), each of unit norm with its largest-modulus component (lowest index on ties) real and positive.
int baz_music_beamspace_design(uint32_t m, uint32_t resolution, const float* table_ri, uint32_t bin_lo, uint32_t bin_count, uint32_t B,
                               double* T_out, double* captured_out)
{
    if (m < 2 || m > BAZ_MUSIC_MAX_M || resolution == 0 || !table_ri || !T_out) return BAZ_MUSIC_E_INVALID;
    if (bin_count == 0 || bin_count > resolution || B < 1 || B > m || B > BAZ_MUSIC_FAST_M) return BAZ_MUSIC_E_INVALID;
    typedef std::complex<double> cd;
    std::vector<cd> A((size_t)m * m, cd(0.0, 0.0)), V((size_t)m * m, cd(0.0, 0.0));
    for (uint32_t i = 0; i < bin_count; ++i) {
        const float* a = table_ri + 2 * (size_t)(((uint64_t)bin_lo + i) % resolution) * m;
        for (uint32_t p = 0; p < m; ++p) {
            const cd ap((double)a[2 * p], (double)a[2 * p + 1]);
            for (uint32_t q = p; q < m; ++q) A[(size_t)p * m + q] += ap * std::conj(cd((double)a[2 * q], (double)a[2 * q + 1]));
        }
    }
    double trace = 0.0;
    for (uint32_t p = 0; p < m; ++p) trace = trace + A[(size_t)p * m + p].real();
    if (!(trace > 0.0) || !(trace - trace == 0.0)) return BAZ_MUSIC_E_INVALID;      // (a non-finite or all-zero sector)
    int ex = 0;
    (void)frexp(trace, &ex);
    for (uint32_t p = 0; p < m; ++p) {
        V[(size_t)p * m + p] = cd(1.0, 0.0);
        A[(size_t)p * m + p] = cd(ldexp(A[(size_t)p * m + p].real(), -ex), 0.0);
        for (uint32_t q = p + 1; q < m; ++q) {
            const cd a(ldexp(A[(size_t)p * m + q].real(), -ex), ldexp(A[(size_t)p * m + q].imag(), -ex));
            if (!(a.real() - a.real() == 0.0) || !(a.imag() - a.imag() == 0.0)) return BAZ_MUSIC_E_INVALID;
            A[(size_t)p * m + q] = a;
            A[(size_t)q * m + p] = std::conj(a);
        }
    }
    hermitian_jacobi(m, A, V);
    std::vector<uint32_t> idx(m);
    for (uint32_t p = 0; p < m; ++p) idx[p] = p;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return A[(size_t)x * m + x].real() > A[(size_t)y * m + y].real(); });
    double top = 0.0, all = 0.0;
    for (uint32_t p = 0; p < m; ++p) {
        all = all + A[(size_t)idx[p] * m + idx[p]].real();
        if (p + 1 == B) top = all;
    }
    for (uint32_t b = 0; b < B; ++b) {
        const uint32_t col = idx[b];
        uint32_t k = 0;
        double big = -1.0, n2 = 0.0;
        for (uint32_t r = 0; r < m; ++r) {
            const double v = std::norm(V[(size_t)r * m + col]);
            n2 = n2 + v;
            if (v > big) { big = v; k = r; }
        }
        if (!(big > 0.0)) return BAZ_MUSIC_E_INVALID;
        const cd vk = V[(size_t)k * m + col];
        const cd rot = std::conj(vk) / (std::abs(vk) * std::sqrt(n2));
        for (uint32_t r = 0; r < m; ++r) {
            const cd t = V[(size_t)r * m + col] * rot;
            T_out[2 * ((size_t)r * B + b)] = t.real();
            T_out[2 * ((size_t)r * B + b) + 1] = r == k ? 0.0 : t.imag();
        }
    }
    if (captured_out) *captured_out = top / all;
    return BAZ_MUSIC_OK;
}

int baz_music_set_beamspace(baz_music_ctx* c, uint32_t B, const double* T_ri, int normalise)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    const bool off = B == 0 || !T_ri;
    std::lock_guard<std::mutex> tl(c->tab_mtx);   // against set_table: c->hRaw is the table in force while it is held
    DeviceGuard guard(c->device);
    baz_music_ctx* old = nullptr;
    DevBuf<double2> old_tc;
    if (off) {
        DevBuf<float2> old_y;                     // the front-end's workspace goes with it (released behind the drain below)
        DevBuf<float> old_x, old_al, old_spec;
        {
            std::lock_guard<std::mutex> lk(c->mtx);
            if (!beamspace_on(c)) return BAZ_MUSIC_OK;   // (off and staying off; smoothing, if on, is not this mode's to end)
            old = c->sm.inner;
            c->sm.inner = nullptr;
            c->sm.kind = baz_music_ctx::FRONT_SMOOTHING;
            c->sm.ms = 0; c->sm.L = 1; c->sm.Kp = 0; c->sm.fb = 0; c->sm.bs_norm = 0;
            c->sm.bs_T.clear();
            old_tc = std::move(c->sm.dTc);
            old_y = std::move(c->sm.dY); old_x = std::move(c->sm.dX); old_al = std::move(c->sm.dAl); old_spec = std::move(c->sm.dSpec);
            c->avg_hist = 0;                      // (averaging: the shape of R changes, the history starts over)
            if (c->wide) {                        // what the run-time-m kernels do not offer goes with the front-end that carried it
                c->peak_mode = 0; c->order_mode = 0; c->refine_mode = 0; c->power_mode = 0; c->estimator = 0;
            }
        }
        baz_music_destroy(old);                   // (drains the stream first: batches in flight may still use it and conj(T))
        return BAZ_MUSIC_OK;
    }
    if (B < 2 || B > c->m || B > BAZ_MUSIC_FAST_M || B <= c->n || !beamspace_T_ok(T_ri, c->m, B)) return BAZ_MUSIC_E_INVALID;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (c->sm.inner && !beamspace_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // (smoothing on: two front-ends, one inner context)
        if (c->beam_mode) return BAZ_MUSIC_E_UNSUPPORTED;                      // (its weights would be B-vectors)
    }
    if (c->calib_on || c->wh_on) return BAZ_MUSIC_E_UNSUPPORTED;   // (both change under tab_mtx; their composition with T^H is not defined here)
    if ((uint64_t)B * c->K > (1ull << 31)) return BAZ_MUSIC_E_UNSUPPORTED;
    std::vector<float> proj((size_t)c->res * B * 2);
    beamspace_apply_host(c->m, B, T_ri, normalise ? 1 : 0, c->hRaw, c->res, proj.data());
    baz_music_ctx* inner = nullptr;
    int r = baz_music_create(&inner, B, c->n, B * c->K, c->res, proj.data(), c->device);
    if (r != BAZ_MUSIC_OK) return r;
    DevBuf<double2> tc;
    {
        const std::vector<double2> h = beamspace_conj(T_ri, c->m, B);
        hipError_t e = tc.allocate(h.size());
        if (e == hipSuccess) e = hipMemcpy(tc.get(), h.data(), h.size() * sizeof(double2), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            baz_music_destroy(inner);
            return hip_fail(c, e, "beamspace: conj(T)");
        }
    }
    {
        std::lock_guard<std::mutex> lk(c->mtx);   // a batch sees the old setting or the new one
        r = c->beam_mode ? BAZ_MUSIC_E_UNSUPPORTED : baz_music_set_stream(inner, c->stream);   // (set_beam_mode may have come in between)
        if (r == BAZ_MUSIC_OK) r = baz_music_set_peak_mode(inner, c->peak_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_order_mode(inner, c->order_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_refine_mode(inner, c->refine_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_power_mode(inner, c->power_mode);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_estimator(inner, c->estimator);
        if (r == BAZ_MUSIC_OK) r = baz_music_set_averaging(inner, c->avg_window, c->avg_beta);   // (a new inner context: an empty history)
        if (r == BAZ_MUSIC_OK) {
            inner->ord_driven = true;             // (N of the criterion is the inner context's own K)
            c->out_beam.on = false;               // (calls under the mode run with the beam mode off: last_beams reports zeros)
            c->out_beam.count = 0;
            old = c->sm.inner;
            old_tc = std::move(c->sm.dTc);
            c->sm.inner = inner;
            c->sm.dTc = std::move(tc);
            c->sm.kind = baz_music_ctx::FRONT_BEAMSPACE;
            c->sm.ms = B; c->sm.L = 1; c->sm.Kp = c->K; c->sm.fb = 0;
            c->sm.bs_norm = normalise ? 1 : 0;
            c->sm.bs_T.assign(T_ri, T_ri + (size_t)2 * c->m * B);
            inner = nullptr;
        }
    }
    baz_music_destroy(inner);                     // (only after a failure)
    baz_music_destroy(old);                       // (drains the stream; the retired conj(T) goes after it, with old_tc)
    return r;
}

int baz_music_get_beamspace(const baz_music_ctx* c, uint32_t* B, double* T_out, int* normalise)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    const bool on = beamspace_on(c);
    if (B) *B = on ? c->sm.ms : 0;
    if (normalise) *normalise = on ? c->sm.bs_norm : 0;
    if (T_out && on) std::memcpy(T_out, c->sm.bs_T.data(), c->sm.bs_T.size() * sizeof(double));
    return BAZ_MUSIC_OK;
}

int baz_music_debug_beamspace(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_out)
{
    if (!c || !d_in || !d_out || d_in == d_out || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (!beamspace_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;
    if ((uint64_t)batch * c->K > 0xffffffffull) return BAZ_MUSIC_E_INVALID;
    (void)hipGetLastError();
    return launch_beamspace(c, static_cast<const float2*>(d_in), batch * c->K, static_cast<float2*>(d_out));
}

// ---- opt-in wideband (subband) front-end: the host side (include/baz_music_hip.h; subband_kernels.hip.h) ---------------------------
namespace {
// 2 <= F <= 64, 1 <= S <= BAZ_MUSIC_MAX_SUBBANDS, S distinct bins below F
bool subband_bins_ok(uint32_t F, uint32_t S, const uint32_t* bins)
{
    if (F < 2 || F > 64 || S < 1 || S > BAZ_MUSIC_MAX_SUBBANDS || !bins) return false;
    uint64_t seen = 0;
    for (uint32_t s = 0; s < S; ++s) {
        if (bins[s] >= F || ((seen >> bins[s]) & 1u)) return false;
        seen |= 1ull << bins[s];
    }
    return true;
}

// Builds the S inner contexts and the twiddles beside the running stream and exchanges them with the setting in force under c->mtx
// (c->tab_mtx held).  Both setters end here: a batch sees all S old tables or all S new ones.
int subband_install(baz_music_ctx* c, uint32_t F, uint32_t S, const uint32_t* bins, const float* tables_ri, int combine)
{
    const uint32_t Q = c->K / F;
    const size_t tab_words = (size_t)c->res * c->m * 2;
    std::vector<baz_music_ctx*> fresh;
    const auto drop = [&](int rc) {
        for (baz_music_ctx* in : fresh) baz_music_destroy(in);
        return rc;
    };
    int r = BAZ_MUSIC_OK;
    for (uint32_t s = 0; s < S && r == BAZ_MUSIC_OK; ++s) {
        baz_music_ctx* in = nullptr;
        r = baz_music_create(&in, c->m, c->n, c->m * Q, c->res, tables_ri + (size_t)s * tab_words, c->device);
        if (r == BAZ_MUSIC_OK) fresh.push_back(in);
    }
    if (r != BAZ_MUSIC_OK) return drop(r);
    DevBuf<double2> w;
    {
        std::vector<double> h((size_t)2 * S * F);
        subband_twiddles_host(F, S, bins, h.data());
        hipError_t e = w.allocate((size_t)S * F);
        if (e == hipSuccess) e = hipMemcpy(w.get(), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) return drop(hip_fail(c, e, "subbands: W"));
    }
    if ((r = subband_lds_attribute(c)) != BAZ_MUSIC_OK) return drop(r);
    std::vector<baz_music_ctx*> old;
    DevBuf<double2> old_w;
    DevBuf<float2> old_y;
    DevBuf<float> old_ps, old_row;
    {
        std::lock_guard<std::mutex> lk(c->mtx);   // a batch sees the old setting or the new one
        if (c->order_mode || c->refine_mode || c->power_mode || c->beam_mode) r = BAZ_MUSIC_E_UNSUPPORTED;   // (a setter may have come in between)
        for (baz_music_ctx* in : fresh) {
            if (r == BAZ_MUSIC_OK) r = baz_music_set_stream(in, c->stream);
            if (r == BAZ_MUSIC_OK) r = baz_music_set_estimator(in, c->estimator);
            if (r == BAZ_MUSIC_OK) r = baz_music_set_averaging(in, c->avg_window, c->avg_beta);   // (a new inner context: an empty history)
        }
        if (r == BAZ_MUSIC_OK) {
            for (baz_music_ctx* in : fresh) in->ord_driven = true;   // (this context opens the call)
            if (c->sm.inner) old.push_back(c->sm.inner);
            old.insert(old.end(), c->sm.sb_more.begin(), c->sm.sb_more.end());
            old_w = std::move(c->sm.dW);
            old_y = std::move(c->sm.dY); old_ps = std::move(c->sm.dPs); old_row = std::move(c->sm.dRow);   // (sized for the old S and F)
            c->sm.inner = fresh[0];
            c->sm.sb_more.assign(fresh.begin() + 1, fresh.end());
            c->sm.dW = std::move(w);
            c->sm.kind = baz_music_ctx::FRONT_SUBBAND;
            c->sm.ms = c->m; c->sm.L = 1; c->sm.Kp = S * Q; c->sm.fb = 0;
            c->sm.sb_F = F; c->sm.sb_S = S; c->sm.sb_combine = combine;
            c->sm.sb_bins.assign(bins, bins + S);
            c->out_beam.on = false;
            c->out_beam.count = 0;
            fresh.clear();
        }
    }
    for (baz_music_ctx* in : old) baz_music_destroy(in);   // (drains the stream; the retired W and workspace go after it)
    return drop(r);
}
}  // namespace

int baz_music_subband_twiddles(uint32_t F, uint32_t S, const uint32_t* bins, double* W_out)
{
    if (!subband_bins_ok(F, S, bins) || !W_out) return BAZ_MUSIC_E_INVALID;
    subband_twiddles_host(F, S, bins, W_out);
    return BAZ_MUSIC_OK;
}

int baz_music_subband_apply(uint32_t m, uint32_t F, uint32_t S, const double* W_ri, const float* in_ri, uint32_t blocks, float* out_ri)
{
    if (m < 2 || m > BAZ_MUSIC_FAST_M || F < 2 || F > 64 || S < 1 || S > BAZ_MUSIC_MAX_SUBBANDS || !W_ri) return BAZ_MUSIC_E_INVALID;
    if (blocks == 0) return BAZ_MUSIC_OK;
    if (!in_ri || !out_ri) return BAZ_MUSIC_E_INVALID;
    subband_apply_host(m, F, S, W_ri, in_ri, blocks, out_ri);
    return BAZ_MUSIC_OK;
}

int baz_music_set_subbands(baz_music_ctx* c, uint32_t F, uint32_t S, const uint32_t* bins, const float* tables_ri, int combine)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> tl(c->tab_mtx);   // against set_table and the other front-ends: sm changes under tab_mtx + mtx
    DeviceGuard guard(c->device);
    if (F == 0) {
        std::vector<baz_music_ctx*> old;
        DevBuf<double2> old_w;
        DevBuf<float2> old_y;                     // the front-end's workspace goes with it (released behind the drain below)
        DevBuf<float> old_x, old_al, old_spec, old_ps, old_row;
        {
            std::lock_guard<std::mutex> lk(c->mtx);
            if (!subband_on(c)) return BAZ_MUSIC_OK;   // (off and staying off; another front-end, if on, is not this mode's to end)
            old.push_back(c->sm.inner);
            old.insert(old.end(), c->sm.sb_more.begin(), c->sm.sb_more.end());
            c->sm.inner = nullptr;
            c->sm.sb_more.clear();
            c->sm.kind = baz_music_ctx::FRONT_SMOOTHING;
            c->sm.ms = 0; c->sm.L = 1; c->sm.Kp = 0; c->sm.fb = 0;
            c->sm.sb_F = 0; c->sm.sb_S = 0; c->sm.sb_combine = 0;
            c->sm.sb_bins.clear();
            old_w = std::move(c->sm.dW);
            old_y = std::move(c->sm.dY); old_x = std::move(c->sm.dX); old_al = std::move(c->sm.dAl); old_spec = std::move(c->sm.dSpec);
            old_ps = std::move(c->sm.dPs); old_row = std::move(c->sm.dRow);
            c->avg_hist = 0;                      // (averaging: the items of R change, the history starts over)
        }
        for (baz_music_ctx* in : old) baz_music_destroy(in);   // (drains the stream first: batches in flight may still use them and W)
        return BAZ_MUSIC_OK;
    }
    if (!subband_bins_ok(F, S, bins) || !tables_ri || (combine != BAZ_MUSIC_SUBBAND_HARMONIC && combine != BAZ_MUSIC_SUBBAND_ARITHMETIC))
        return BAZ_MUSIC_E_INVALID;
    if (c->K % F) return BAZ_MUSIC_E_INVALID;
    for (size_t i = 0; i < (size_t)S * c->res * c->m * 2; ++i)
        if (!(tables_ri[i] - tables_ri[i] == 0.0f)) return BAZ_MUSIC_E_INVALID;
    if (c->wide) return BAZ_MUSIC_E_UNSUPPORTED;  // (17 .. 64 antennas: the pickers on a float32 row exist for the specialised kernels only)
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (c->sm.inner && !subband_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;   // (smoothing or beamspace on: one front-end at a time)
        if (c->order_mode || c->refine_mode || c->power_mode || c->beam_mode) return BAZ_MUSIC_E_UNSUPPORTED;
    }
    if (c->calib_on || c->wh_on) return BAZ_MUSIC_E_UNSUPPORTED;   // (both change under tab_mtx; their per-subband forms are not offered)
    return subband_install(c, F, S, bins, tables_ri, combine);
}

int baz_music_set_subband_tables(baz_music_ctx* c, const float* tables_ri)
{
    if (!c || !tables_ri) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> tl(c->tab_mtx);
    DeviceGuard guard(c->device);
    uint32_t F, S;
    int combine;
    std::vector<uint32_t> bins;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        if (!subband_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;
        F = c->sm.sb_F; S = c->sm.sb_S; combine = c->sm.sb_combine; bins = c->sm.sb_bins;
    }
    for (size_t i = 0; i < (size_t)S * c->res * c->m * 2; ++i)
        if (!(tables_ri[i] - tables_ri[i] == 0.0f)) return BAZ_MUSIC_E_INVALID;
    return subband_install(c, F, S, bins.data(), tables_ri, combine);   // (sm cannot change in between: tab_mtx is held)
}

int baz_music_get_subbands(const baz_music_ctx* c, uint32_t* F, uint32_t* S, uint32_t* bins_out, int* combine)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    const bool on = subband_on(c);
    if (F) *F = on ? c->sm.sb_F : 0;
    if (S) *S = on ? c->sm.sb_S : 0;
    if (combine) *combine = on ? c->sm.sb_combine : 0;
    if (bins_out && on) std::memcpy(bins_out, c->sm.sb_bins.data(), c->sm.sb_bins.size() * sizeof(uint32_t));
    return BAZ_MUSIC_OK;
}

int baz_music_debug_subbands(baz_music_ctx* c, const void* d_in, uint32_t batch, void* d_out)
{
    if (!c || !d_in || !d_out || d_in == d_out || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (!subband_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;
    (void)hipGetLastError();
    return launch_subband(c, static_cast<const float2*>(d_in), batch, static_cast<float2*>(d_out));
}

int baz_music_debug_subband_combine(baz_music_ctx* c, const void* d_spectra, uint32_t batch, void* d_out)
{
    if (!c || !d_spectra || !d_out || d_spectra == d_out || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (!subband_on(c)) return BAZ_MUSIC_E_UNSUPPORTED;
    (void)hipGetLastError();
    return launch_subband_combine(c, static_cast<const float*>(d_spectra), batch, static_cast<float*>(d_out));
}

namespace {
// R-bar of `batch` items (device memory, or host memory staged chunk by chunk through dCalIn) into Rbar (host, 2 m^2 doubles): the
// covariance stage debug_cov runs, chunk by chunk through the context's R workspace, cov_mean_kernel over each chunk's runs, one fold.
// The caller holds c->mtx.
int calib_mean_locked(baz_music_ctx* c, const void* in, bool in_on_host, uint32_t batch, double* Rbar)
{
    const uint32_t ncomp = 2u * c->m * c->m;
    const bazcalib::MeanGeometry G = bazcalib::mean_geometry(batch, c->m);
    const uint32_t chunk = std::min(G.chunk, batch);
    int r = ensure_workspace(c, chunk);
    if (r == BAZ_MUSIC_OK) r = grow(c, c->dCalPart, (size_t)(G.groups + 1) * ncomp);
    if (r == BAZ_MUSIC_OK && in_on_host) r = grow(c, c->dCalIn, (size_t)chunk * c->nsamples * 2);
    if (r) return r;
    BAZ_REQUIRE(c, dR); BAZ_REQUIRE(c, dCalPart);
    const dim3 gx((ncomp + bazcalib::MEAN_THREADS - 1) / bazcalib::MEAN_THREADS);
    for (uint32_t off = 0; off < batch; off += G.chunk) {
        const uint32_t nb = std::min(G.chunk, batch - off);
        const float* d_in = static_cast<const float*>(in) + (size_t)off * c->nsamples * 2;
        if (in_on_host) {
            HIP_TRY(c, hipMemcpyAsync(c->dCalIn, d_in, (size_t)nb * c->nsamples * 8, hipMemcpyHostToDevice, c->stream));
            d_in = c->dCalIn;
        }
        r = launch_cov(c, d_in, nb, c->dR);
        if (r) return r;
        ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);             // (the covariance counts under COV, the two levels of the mean under MERGE)
        const uint32_t runs = (nb + G.run - 1) / G.run;
        hipLaunchKernelGGL(bazcalib::cov_mean_kernel, dim3(gx.x, runs), dim3(bazcalib::MEAN_THREADS), 0, c->stream,
                           reinterpret_cast<const double*>(c->dR.get()), c->dCalPart + (size_t)(off / G.run) * ncomp, nb, G.run, ncomp, 1.0);
        HIP_TRY(c, hipGetLastError());
    }
    double* const dMean = c->dCalPart + (size_t)G.groups * ncomp;
    {
        ProfScope ps(c, BAZ_MUSIC_STAGE_MERGE);
        hipLaunchKernelGGL(bazcalib::cov_mean_kernel, dim3(gx.x, 1), dim3(bazcalib::MEAN_THREADS), 0, c->stream, c->dCalPart, dMean, G.groups,
                           G.groups, ncomp, 1.0 / (double)batch);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(Rbar, dMean, (size_t)ncomp * sizeof(double), hipMemcpyDeviceToHost));
    return BAZ_MUSIC_OK;
}

int calibrate_any(baz_music_ctx* c, const void* in, bool in_on_host, uint32_t batch, const float* ref_ri, double* gamma_ri, double* quality,
                  double* Rbar_ri)
{
    if (!c || !in || batch == 0 || !ref_ri || !gamma_ri || !quality) return BAZ_MUSIC_E_INVALID;
    if (!calib_vector_ok(c->m, ref_ri)) return BAZ_MUSIC_E_INVALID;
    std::vector<double> mean((size_t)2 * c->m * c->m);
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        DeviceGuard guard(c->device);
        if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
        (void)hipGetLastError();
        const int r = calib_mean_locked(c, in, in_on_host, batch, mean.data());
        if (r) return r;
    }
    if (Rbar_ri) std::memcpy(Rbar_ri, mean.data(), mean.size() * sizeof(double));
    return baz_music_calibration_estimate(c->m, mean.data(), ref_ri, gamma_ri, quality);
}
}  // namespace

int baz_music_calibrate(baz_music_ctx* c, const float* in_ri, uint32_t batch, const float* ref_ri, double* gamma_ri, double* quality,
                        double* Rbar_ri)
{
    return calibrate_any(c, in_ri, true, batch, ref_ri, gamma_ri, quality, Rbar_ri);
}

int baz_music_calibrate_device(baz_music_ctx* c, const void* d_in, uint32_t batch, const float* ref_ri, double* gamma_ri, double* quality,
                               double* Rbar_ri)
{
    return calibrate_any(c, d_in, false, batch, ref_ri, gamma_ri, quality, Rbar_ri);
}

// ---- opt-in noise pre-whitening: the host side (include/baz_music_hip.h; whiten_kernels.hip.h) -------------------------------------
// W = L^-1 of the unpivoted Cholesky factor Rn = L L^H, in fp64 from the lower triangle and the real diagonal as stored.
int baz_music_whitening_factor(uint32_t m, const double* Rn_ri, double* W_ri)
{
    if (m < 1 || m > BAZ_MUSIC_MAX_M || !Rn_ri || !W_ri) return BAZ_MUSIC_E_INVALID;
    typedef std::complex<double> cd;
    for (size_t i = 0; i < (size_t)2 * m * m; ++i)
        if (!(Rn_ri[i] - Rn_ri[i] == 0.0)) return BAZ_MUSIC_E_INVALID;
    double mean = 0.0;
    for (uint32_t i = 0; i < m; ++i) mean = mean + Rn_ri[2 * ((size_t)i * m + i)];
    mean = mean / (double)m;
    const double floor_d = BAZ_MUSIC_POWER_PIVOT_FLOOR * mean;
    std::vector<cd> L((size_t)m * m, cd(0.0, 0.0)), W((size_t)m * m, cd(0.0, 0.0));
    for (uint32_t j = 0; j < m; ++j) {
        double d = Rn_ri[2 * ((size_t)j * m + j)];
        for (uint32_t k = 0; k < j; ++k) d = d - std::norm(L[(size_t)j * m + k]);
        if (!(d - d == 0.0) || !(d > floor_d)) return BAZ_MUSIC_E_INVALID;       // (a pivot: not finite, or at / below the floor)
        const double ljj = std::sqrt(d);
        L[(size_t)j * m + j] = cd(ljj, 0.0);
        for (uint32_t i = j + 1; i < m; ++i) {
            cd s(Rn_ri[2 * ((size_t)i * m + j)], Rn_ri[2 * ((size_t)i * m + j) + 1]);
            for (uint32_t k = 0; k < j; ++k) s = s - L[(size_t)i * m + k] * std::conj(L[(size_t)j * m + k]);
            L[(size_t)i * m + j] = s / ljj;
        }
    }
    // W L = I by substitution, row by row of W (w_i L = e_i, from the diagonal leftwards): the form whose rounding errors are a
    // small relative perturbation of L per row, so that |W L - I| <= gamma |W| |L| componentwise
    for (uint32_t i = 0; i < m; ++i) {
        W[(size_t)i * m + i] = cd(1.0 / L[(size_t)i * m + i].real(), 0.0);
        for (uint32_t j = i; j-- > 0;) {
            cd s(0.0, 0.0);
            for (uint32_t k = j + 1; k <= i; ++k) s = s + W[(size_t)i * m + k] * L[(size_t)k * m + j];
            W[(size_t)i * m + j] = -s / L[(size_t)j * m + j].real();
        }
    }
    for (size_t i = 0; i < (size_t)m * m; ++i) {
        if (!(W[i].real() - W[i].real() == 0.0) || !(W[i].imag() - W[i].imag() == 0.0)) return BAZ_MUSIC_E_INVALID;
        W_ri[2 * i] = W[i].real();
        W_ri[2 * i + 1] = W[i].imag();
    }
    return BAZ_MUSIC_OK;
}

// The definition of include/baz_music_hip.h on the host: table_whiten_kernel's own routine, entry by entry.
int baz_music_whiten_table(uint32_t m, uint32_t resolution, const float* table_ri, const double* W_ri, float* out_ri)
{
    if (m < 1 || m > BAZ_MUSIC_MAX_M || resolution == 0 || !table_ri || !W_ri || !out_ri) return BAZ_MUSIC_E_INVALID;
    const double2* const W = reinterpret_cast<const double2*>(W_ri);
    std::vector<float2> row(m);
    for (size_t b = 0; b < resolution; ++b) {
        for (uint32_t k = 0; k < m; ++k) row[k] = make_float2(table_ri[2 * (b * m + k)], table_ri[2 * (b * m + k) + 1]);   // (out may be table)
        for (uint32_t r = 0; r < m; ++r)
            bazwhiten::whiten_entry(W + (size_t)r * m, row.data(), r, &out_ri[2 * (b * m + r)], &out_ri[2 * (b * m + r) + 1]);
    }
    return BAZ_MUSIC_OK;
}

int baz_music_set_noise_covariance(baz_music_ctx* c, const double* Rn_ri)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    const size_t mm = (size_t)c->m * c->m;
    std::vector<double> W;
    if (Rn_ri) {
        W.resize(2 * mm);
        if (const int rf = baz_music_whitening_factor(c->m, Rn_ri, W.data())) return rf;
    }
    std::lock_guard<std::mutex> tl(c->tab_mtx);   // a retune of the table c->hRaw holds; against set_table, set_calibration and set_smoothing
    DeviceGuard guard(c->device);
    if (Rn_ri && c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;   // (the whitened table is not shift invariant)
    if (!Rn_ri && !c->wh_on) return BAZ_MUSIC_OK;               // off and staying off: the images in force are the ones to keep
    bool old_want = false;
    {
        std::lock_guard<std::mutex> lk(c->mtx);
        // (the beam mode's weights would apply to unwhitened snapshots; Capon is invariant under the transform)
        if (Rn_ri && (c->beam_mode || c->estimator)) return BAZ_MUSIC_E_UNSUPPORTED;
        old_want = c->wh_want;
        if (Rn_ri) c->wh_want = true;             // (from here set_beam_mode / set_estimator refuse)
    }
    if (Rn_ri && !c->hWh && c->hWh.allocate(mm) != hipSuccess) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(c->mtx);
        c->wh_want = old_want;
        return BAZ_MUSIC_E_NOMEM;
    }
    const bool old_on = c->wh_on;
    std::vector<double> old_W;
    if (old_on) old_W.assign(reinterpret_cast<const double*>(c->hWh.get()), reinterpret_cast<const double*>(c->hWh.get()) + 2 * mm);
    c->wh_on = Rn_ri != nullptr;
    if (Rn_ri) std::memcpy(c->hWh, W.data(), 2 * mm * sizeof(double));     // (no builder runs: they hold tab_mtx and wait for their stream)
    const int r = retune(c, nullptr, false);
    std::lock_guard<std::mutex> lk(c->mtx);
    if (r != BAZ_MUSIC_OK) {                      // the old pair (images, W) stays in force: retune exchanges only after a complete build
        c->wh_on = old_on;
        if (old_on) std::memcpy(c->hWh, old_W.data(), 2 * mm * sizeof(double));
        c->wh_want = old_want;
        return r;
    }
    if (Rn_ri) c->wh_Rn.assign(Rn_ri, Rn_ri + 2 * mm); else c->wh_Rn.clear();
    c->wh_want = c->wh_on;
    return BAZ_MUSIC_OK;
}

int baz_music_get_noise_covariance(const baz_music_ctx* c, double* Rn_ri, int* on)
{
    if (!c || !on) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> tl(const_cast<baz_music_ctx*>(c)->tab_mtx);
    *on = c->wh_on ? 1 : 0;
    if (Rn_ri)
        for (uint32_t i = 0; i < c->m; ++i)
            for (uint32_t j = 0; j < c->m; ++j) {
                const size_t e = 2 * ((size_t)i * c->m + j);
                Rn_ri[e] = c->wh_on ? c->wh_Rn[e] : (i == j ? 1.0 : 0.0);
                Rn_ri[e + 1] = c->wh_on ? c->wh_Rn[e + 1] : 0.0;
            }
    return BAZ_MUSIC_OK;
}

int baz_music_debug_whiten(baz_music_ctx* c, const void* d_R_in, uint32_t batch, void* d_R_out)
{
    if (!c || !d_R_in || !d_R_out || d_R_in == d_R_out || batch == 0) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner || !c->tab.wh_on) return BAZ_MUSIC_E_UNSUPPORTED;
    (void)hipGetLastError();
    const int r = ensure_whiten(c, batch, false);
    return r ? r : launch_whiten(c, static_cast<const double2*>(d_R_in), batch, static_cast<double2*>(d_R_out));
}

namespace {
int mean_covariance_any(baz_music_ctx* c, const void* in, bool in_on_host, uint32_t batch, double* Rbar_ri)
{
    if (!c || !in || batch == 0 || !Rbar_ri) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mtx);
    DeviceGuard guard(c->device);
    if (c->sm.inner) return BAZ_MUSIC_E_UNSUPPORTED;
    (void)hipGetLastError();
    return calib_mean_locked(c, in, in_on_host, batch, Rbar_ri);
}
}  // namespace

int baz_music_mean_covariance(baz_music_ctx* c, const float* in_ri, uint32_t batch, double* Rbar_ri)
{
    return mean_covariance_any(c, in_ri, true, batch, Rbar_ri);
}

int baz_music_mean_covariance_device(baz_music_ctx* c, const void* d_in, uint32_t batch, double* Rbar_ri)
{
    return mean_covariance_any(c, d_in, false, batch, Rbar_ri);
}

int baz_music_get_smoothing(const baz_music_ctx* c, uint32_t* subarray, int* forward_backward)
{
    if (!c) return BAZ_MUSIC_E_INVALID;
    std::lock_guard<std::mutex> lk(const_cast<baz_music_ctx*>(c)->mtx);
    const bool on = c->sm.inner && c->sm.kind == baz_music_ctx::FRONT_SMOOTHING;
    if (subarray) *subarray = on ? c->sm.ms : c->m;
    if (forward_backward) *forward_backward = on ? c->sm.fb : 0;
    return BAZ_MUSIC_OK;
}

}  // extern "C"
