// C ABI of libtmpc_hip.so (declared in include/tmpc.h).  Host side only: condenses the
// problem (tmpc_condense.cpp), keeps it resident in HBM and enqueues the solve kernels
// (tmpc_kernels.hip) on the handle's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "tmpc_condense.hpp"
#include "tmpc_device.hpp"
#include "tmpc_hazard.hpp"
#include "tmpc_west.hpp"

namespace {

thread_local std::string g_create_error;

// Grow-only device memory.  When a call needs more, the old block is freed -- after the work queued on `stream`, which may still
// use it -- and one of exactly the new size allocated.  No destructor: the LP arena is thread_local and may outlive the HIP
// runtime; tmpc_destroy releases a handle's buffers.
struct DeviceBuffer {
    char *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes, hipStream_t stream) {
        if (bytes <= cap) return hipSuccess;
        if (p && stream) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
        }
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), bytes);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Device memory of one call, carved from a grow-only buffer: the caller lists its pieces, then carve() grows the buffer to their
// sum (each rounded up to 256 B), writes every piece's device pointer to its slot and does the listed uploads and fills.  What
// the previous call carved is gone from then on.
class Arena {
  public:
    // `src` (host memory that outlives the copy) is uploaded into the piece; without one, `fill` >= 0 is written to every byte
    template <class T> void piece(T **slot, size_t bytes, const void *src = nullptr, int fill = -1) {
        pieces_.push_back({slot, [](void *s, char *p) { *static_cast<T **>(s) = reinterpret_cast<T *>(p); }, bytes, src, fill});
    }
    // `stream` gets the uploads and fills, and a reallocation waits for its work; nullptr: synchronous copies and fills
    hipError_t carve(hipStream_t stream) {
        size_t total = 0;
        for (const Piece &q : pieces_) total += rounded(q.bytes);
        hipError_t e = buf_.reserve(total, stream);
        char *p = buf_.p;
        for (size_t i = 0; i < pieces_.size() && e == hipSuccess; p += rounded(pieces_[i++].bytes)) {
            const Piece &q = pieces_[i];
            q.set(q.slot, p);
            if (q.src && q.bytes)
                e = stream ? hipMemcpyAsync(p, q.src, q.bytes, hipMemcpyHostToDevice, stream) : hipMemcpy(p, q.src, q.bytes, hipMemcpyHostToDevice);
            else if (!q.src && q.fill >= 0)
                e = stream ? hipMemsetAsync(p, q.fill, q.bytes, stream) : hipMemset(p, q.fill, q.bytes);
        }
        pieces_.clear();
        return e;
    }
    void release() { buf_.release(); }

  private:
    struct Piece {
        void *slot;
        void (*set)(void *slot, char *p);
        size_t bytes;
        const void *src;
        int fill;
    };
    static size_t rounded(size_t bytes) { return (std::max<size_t>(bytes, 1) + 255) / 256 * 256; }
    std::vector<Piece> pieces_;
    DeviceBuffer buf_;
};

// device memory of one call, freed when the call returns (the sample buffer is far too large to keep)
struct WestMem {
    std::vector<void *> blocks;
    ~WestMem() { for (void *p : blocks) (void)hipFree(p); }
    template <class T> hipError_t get(T **out, size_t bytes) {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 8));
        if (e == hipSuccess) blocks.push_back(p);
        *out = static_cast<T *>(p);
        return e;
    }
};
struct WestEvents {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~WestEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// What the last tmpc_mc_run / tmpc_reg_run left in the loop arena for the getters (nullptr / 0: nothing).  A run resets them
// before it touches the arena, whether it gets as far as replacing them or not.
struct LoopRecords {
    double *cap = nullptr;       // the recorded trajectory: [cap_T][2 nx + nu]
    int cap_T = 0;
    long long *tick_sum = nullptr, *tick_max = nullptr;     // per-trajectory solve times
    int64_t tick_B = 0;
    double *err2_phys = nullptr; // physics-rate error (nonlinear plant)
    int64_t phys_B = 0;
    int fused = 0;               // tmpc_mc_last_fused
    std::vector<int32_t> link;   // link statistics [4][link_B]: lost_up, lost_down, max_gap, overrun -- a HOST copy, fetched with the loop's
    int64_t link_B = 0;          // other outputs (tmpc_mc_get_link_stats then costs no device call); 0: no loop has finished
};

// One launch lane of a device handle: a non-blocking stream and everything a solve launch on it mutates, so that launches on
// different lanes may overlap while the launches of one lane stay ordered.  Lane 0 (the primary lane) exists from tmpc_create on
// and takes every entry point; lane 1 is created by the first tmpc_solve_batch_device call that can run beside an unfinished one.
struct Lane {
    hipStream_t stream = nullptr;
    tmpc::WorkCounter wc;        // work counters of the wave / block kernel's launches (tmpc_device.hpp)
    DeviceBuffer blk_ws;         // block-kernel workspace
    DeviceBuffer save;           // (s, lambda) of every resident wave at its hand-over to the refinement (DeviceQP::save)
    DeviceBuffer ticks;          // tmpc_set_solve_timing: one tick count per instance of the lane's last call
    // the unfinished tmpc_solve_batch_device calls of the lane, oldest first: what they touch and the event behind their last kernel
    struct InFlight {
        tmpc::CallRanges touched;
        hipEvent_t end;
    };
    std::deque<InFlight> inflight;
    // end events for the calls beyond the 4096 timing pairs of a handle (created when first needed); a call that would take the
    // event of a record still in flight waits for that record
    std::vector<hipEvent_t> spare;
    size_t spare_next = 0;
    int64_t calls = 0;           // tmpc_solve_batch_device calls enqueued here (tmpc_debug_lane_counters)
};
constexpr size_t LANE_SPARE_EVENTS = 64;

// The stepped closed loop of a handle (tmpc_mc_open .. tmpc_mc_close): the records of tmpc_mc_run, whose arrays live in the loop
// arena until the next loop carves it -- which is why the other entry points refuse to run while `open`.
struct McSession {
    bool open = false, failed = false;   // failed: a step did not go through on the device; only close is left
    int64_t B = 0;
    int T = 0, t = 0, extended = 0;      // steps allowed / taken
    tmpc::McModel m{};
    tmpc::McState st{};
    tmpc::McExternal ext{};              // (x_t / u_t: the device staging of tmpc_mc_step; a device-pointer step brings its own)
    int32_t *ws[2] = {nullptr, nullptr}; // warm start: working sets per problem
    bool warm = false;
    std::vector<double> ref;
    bool full_ref = false;               // opened with a reference table: st.ref_tab is set and the _ref steps are allowed
    double *ref_stage = nullptr;         // device staging of tmpc_mc_step_ref's ref_next (full_ref)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;     // caller's stream -> handle's stream, and back
    char *pin = nullptr;                 // pinned host block [x_t | u_t | ref_next] of tmpc_mc_step[_ref] (nullptr: copies from / to the caller's memory)
};

struct Variant {
    tmpc::Condensed c;
    tmpc::DeviceQP d{};
    tmpc::KernelShape shape;
    bool wave_ok = false;        // a compiled one-wave-per-QP shape covers this variant
    tmpc::DeviceQP db{};         // same model with Hs / Hinv padded for the block kernel
    tmpc::BlockQP bq{};
    const tmpc::BlockArgs *bargs = nullptr;   // {db, bq} in device memory: what solve_block_kernel reads (tmpc_device.hpp)
    int tiles = 0;               // block kernel: NVP / 16 (0: not available)
    std::vector<void *> dev;     // device allocations of this variant
    std::vector<size_t> dev_bytes;       // their sizes (tmpc_debug_dump_layout)
};

}  // namespace

struct tmpc_handle {
    // the handle: its problem(s), device, stream and the scratch of the solve launches
    int device = 0;
    int n_cu = 0;
    int nvariants = 0;
    int nx = 0, nu = 0, N = 0;
    Variant v[2];
    // regulator handles (tmpc_create_regulator): no reference input -- the solves read `ref` from a zero buffer (F2 = 0)
    bool regulator = false;
    int reg_tube = 0;
    std::vector<double> hA, hB, hK, hKanc, hQ, hR;   // host copies for the closed-loop entry points
    int kernel_path = TMPC_PATH_AUTO;
    Lane lane[2];
    hipStream_t stream = nullptr;        // = lane[0].stream: everything but an overlapped tmpc_solve_batch_device call runs on it
    int overlap = 1;             // tmpc_set_call_overlap
    int cur = 0;                 // lane of the latest solve call
    int64_t lane_waits = 0;      // calls that had to wait for the other lane (tmpc_debug_lane_counters)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // event pairs of the calls since the last tmpc_kernel_ms_total(reset), and the lane each ran on: per-call device time
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    std::vector<uint8_t> pool_lane;
    size_t pool_used = 0;
    int blk_blocks = 0;          // workgroups a lane's block-kernel workspace is sized for
    int want_ticks = 0;          // per-solve durations (tmpc_set_solve_timing): one tick count per instance of the last call
    int ticks_lane = 0;          // the lane that call ran on
    int64_t ticks_n = 0;
    DeviceBuffer reg_zero;       // regulator: the zero reference
    std::string err;
    // staging buffers for the host-pointer entry point: ONE device block, inputs [x | ref | variant] then outputs
    // [u | x0 | ss | status | iters | x_nom], and a pinned host mirror of it -- a call moves its inputs with one DMA and its
    // outputs with one (round 3: nine hipMemcpyAsync from / to pageable memory per call, 60 % of the time of a call at batch 1)
    DeviceBuffer stage_dev;
    char *stage_pin = nullptr;
    size_t stage_in_bytes = 0, stage_out_bytes = 0, stage_out_core = 0;      // (core = the outputs without x_nom)
    size_t off_r = 0, off_var = 0, off_x0 = 0, off_ss = 0, off_st = 0, off_it = 0, off_xn = 0;      // offsets within the input / output parts
    double *d_x = nullptr, *d_r = nullptr, *d_u = nullptr, *d_x0 = nullptr, *d_ss = nullptr, *d_xn = nullptr;
    uint8_t *d_var = nullptr;
    int32_t *d_st = nullptr, *d_it = nullptr;
    // closed-loop settings (tmpc_mc_set_*)
    int plant = TMPC_PLANT_LINEAR, plant_substeps = 10;
    double plant_par[7] = {0, 0, 0, 0, 0, 0, 0};
    int actuator = TMPC_ACTUATOR_CONSISTENT;
    long long mc_capture = -1;   // trajectory recorded by the next tmpc_mc_run (-1: none)
    int mc_warm = 0;             // closed loop: hand every solve the working set of the trajectory's previous solve of the same variant
    int mc_fused = TMPC_MC_FUSED_AUTO;   // closed loop: one fused launch for all T steps (tmpc_mc_set_fused)
    int mc_rng_on = 0;                   // tmpc_mc_set_device_rng
    uint64_t mc_rng_seed = 0;
    int64_t mc_rng_first = 0;
    std::vector<double> mc_w_bound;
    // tmpc_mc_set_reference_table: K schedules of T_tab full-state references and the schedule of each of B trajectories (K = 0: none)
    int32_t mc_ref_K = 0, mc_ref_T = 0;
    int64_t mc_ref_B = 0;
    std::vector<double> mc_ref_tab;
    std::vector<int32_t> mc_ref_id;
    // tmpc_mc_set_channel: the Gilbert-Elliott thresholds [B][2][3] as the device compares them (mc_ch_B = 0: the Bernoulli model)
    int64_t mc_ch_B = 0;
    std::vector<double> mc_ch_thr;
    // tmpc_mc_set_plant_models (regulator handles): a linear plant per trajectory, [B][nx][nx + nu] (mc_pm_B = 0: none)
    int64_t mc_pm_B = 0;
    std::vector<double> mc_pm;
    // closed-loop state: one grow-only arena (25 hipMalloc / hipFree per call cost several milliseconds), and what the last run
    // left in it
    Arena arena;
    LoopRecords rec;
    McSession ses;
};

namespace {

#define HIP_TRY(h, expr)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return TMPC_E_DEVICE;                                                          \
        }                                                                                  \
    } while (0)

template <class T>
int upload(tmpc_handle *h, Variant &v, const T *src, size_t n, const T **dst) {
    void *p = nullptr;
    if (h->device < 0) {
        // host-only handle: the layouts the kernels read are kept in host memory (tmpc_debug_layout; tests/wavesim runs
        // the kernel sources on the CPU against them)
        p = std::malloc((n ? n : 1) * sizeof(T));
        if (!p) { h->err = "out of memory"; return TMPC_E_NOMEM; }
        v.dev.push_back(p);
        v.dev_bytes.push_back(n * sizeof(T));
        if (n) std::memcpy(p, src, n * sizeof(T));
        *dst = static_cast<const T *>(p);
        return TMPC_OK;
    }
    HIP_TRY(h, hipMalloc(&p, (n ? n : 1) * sizeof(T)));
    v.dev.push_back(p);
    v.dev_bytes.push_back(n * sizeof(T));
    if (n) HIP_TRY(h, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T *>(p);
    return TMPC_OK;
}

#ifdef TMPC_STAMPS
// diagnostic builds: 16 zeroed time stamps per layout (tmpc_debug_stamps)
int upload_stamps(tmpc_handle *h, Variant &v, long long **dbg) {
    static const long long zero[16] = {};
    const long long *p = nullptr;
    const int rc = upload(h, v, zero, 16, &p);
    *dbg = const_cast<long long *>(p);
    return rc;
}
#endif

int upload_common(tmpc_handle *h, Variant &v, const tmpc_problem &p, tmpc::DeviceQP &d, int NVP) {
    const tmpc::Condensed &c = v.c;
    const int nx = c.nx;
    std::vector<double> Hs(static_cast<size_t>(NVP) * NVP, 0.0), Hinv(Hs.size(), 0.0);
    for (int i = 0; i < NVP; ++i)
        for (int j = 0; j < NVP; ++j) {
            const bool in = i < c.nv && j < c.nv;
            Hs[static_cast<size_t>(i) * NVP + j] = in ? c.Hs(i, j) : (i == j ? 1.0 : 0.0);
            Hinv[static_cast<size_t>(i) * NVP + j] = in ? c.Hinv(i, j) : (i == j ? 1.0 : 0.0);
        }
    d.nx = c.nx; d.nu = c.nu; d.N = c.N; d.nv = c.nv; d.nc = c.nc; d.npar = c.npar; d.nth = c.nth;
    d.off_theta = c.off_theta; d.off_x0 = c.off_x0; d.off_aux = c.off_aux;
    d.max_iter = p.max_iter > 0 ? p.max_iter : 60;
    d.tol = p.tol > 0 ? p.tol : 1e-7;
    d.always_infeasible = c.always_infeasible ? 1 : 0;
    d.dbg = nullptr;
    d.ticks = nullptr;
    d.save = nullptr;
    int rc;
    if ((rc = upload(h, v, Hs.data(), Hs.size(), &d.Hs))) return rc;
    if ((rc = upload(h, v, Hinv.data(), Hinv.size(), &d.Hinv))) return rc;
    if ((rc = upload(h, v, c.F1s.a.data(), c.F1s.a.size(), &d.F1s))) return rc;
    if ((rc = upload(h, v, c.F2s.a.data(), c.F2s.a.size(), &d.F2s))) return rc;
    if ((rc = upload(h, v, c.gp0.data(), c.gp0.size(), &d.gp0))) return rc;
    if ((rc = upload(h, v, c.Ep.a.data(), c.Ep.a.size(), &d.Ep))) return rc;
    if ((rc = upload(h, v, c.Dv.data(), c.Dv.size(), &d.Dv))) return rc;
    d.Tzs = d.Txf = nullptr;
    d.nvf = c.nvf;
    if (!c.Tz.a.empty()) {
        std::vector<double> Tzs(c.Tz.a.size());
        for (int i = 0; i < c.Tz.r; ++i)
            for (int j = 0; j < c.Tz.c; ++j) Tzs[static_cast<size_t>(i) * c.Tz.c + j] = c.Tz(i, j) * c.Dv[j];
        if ((rc = upload(h, v, Tzs.data(), Tzs.size(), &d.Tzs))) return rc;
        if ((rc = upload(h, v, c.Tx.a.data(), c.Tx.a.size(), &d.Txf))) return rc;
    }
    if ((rc = upload(h, v, c.Mth.a.data(), c.Mth.a.size(), &d.Mth))) return rc;
    if ((rc = upload(h, v, p.A, static_cast<size_t>(nx) * nx, &d.A))) return rc;
    if ((rc = upload(h, v, p.B, static_cast<size_t>(nx) * c.nu, &d.B))) return rc;
    return TMPC_OK;
}

// 1 / (g_r Hs^-1 g_r') for every row of the scaled problem: the multiplier of the QP with row r alone is (violation of row r at
// the unconstrained minimiser) times this -- the scale of the multipliers the interior-point phase starts from
std::vector<double> single_row_curvature_inv(const tmpc::Condensed &c) {
    std::vector<double> ci(c.nc, 0.0), t(c.nv);
    for (int r = 0; r < c.nc; ++r) {
        double q = 0.0;
        for (int i = 0; i < c.nv; ++i) {
            double v = 0.0;
            for (int j = 0; j < c.nv; ++j) v += c.Hinv(i, j) * c.Gs(r, j);
            q += v * c.Gs(r, i);
        }
        ci[r] = q > 0.0 ? 1.0 / q : 0.0;
    }
    return ci;
}

// one-wave-per-QP path (tmpc_kernels.hip): functionals (a row and, where it exists, its mirror row) in 64-wide slots of four
// kinds -- dense paired, dense single, factored paired, factored single -- and per row side the right-hand side data
int upload_wave(tmpc_handle *h, Variant &v, const tmpc_problem &p) {
    const tmpc::Condensed &c = v.c;
    const int nx = c.nx;
    auto in_fact = [&](int r) { return c.ncc > 0 && r >= c.fb0 && r < c.fb0 + c.ncc; };
    // three layouts, most structured first: pairs + factored block; single rows + factored block; single rows, all dense
    bool use_pairs = false, use_fact = false;
    std::vector<std::pair<int, int>> dpair, cpair;     // (row, mirror row)
    std::vector<int> dsing, csing;
    bool found = false;
    for (int attempt = 0; attempt < 3 && !found; ++attempt) {
        use_pairs = attempt == 0;
        use_fact = attempt <= 1 && c.ncc > 0;
        dpair.clear(); cpair.clear(); dsing.clear(); csing.clear();
        for (int r = 0; r < c.nc; ++r) {
            const bool f = use_fact && in_fact(r);
            const int q = (use_pairs && !c.mirror.empty()) ? c.mirror[r] : -1;
            if (q >= 0 && q < r) continue;                       // second member of a pair: placed with the first
            if (q >= 0) (f ? cpair : dpair).emplace_back(r, q);
            else (f ? csing : dsing).push_back(r);
        }
        found = tmpc::pick_config(c.nv, static_cast<int>(dpair.size()), static_cast<int>(dsing.size()), use_fact ? c.kc : 0,
                                  static_cast<int>(cpair.size()), static_cast<int>(csing.size()), &v.shape);
    }
    if (found) {
        // the dense functionals in use must fit the LDS next to the workspaces of the shape's waves
        const int last = dsing.empty() ? static_cast<int>(dpair.size()) : v.shape.dp * 64 + static_cast<int>(dsing.size());
        if (tmpc::lds_bytes(v.shape, 4 * ((last + 3) / 4)) > 160 * 1024) found = false;
    }
    if (!found) return TMPC_OK;                                  // wave_ok stays false: the block kernel takes the variant
    const int NVP = v.shape.nvp, DP = v.shape.dp, DS = v.shape.ds, KCP = v.shape.kcp, CP = v.shape.cp, CS = v.shape.cs;
    const int NDP = (DP + DS) * 64, NCCP = (CP + CS) * 64, RS = 2 * DP + DS + 2 * CP + CS;
    const int kc = use_fact ? c.kc : 0;
    const int LDG = 16 * ((NVP + 1 + 15) / 16) + 1;        // Shape::LDG of tmpc_kernels.hip
    std::vector<double> Gt(static_cast<size_t>(NDP) * LDG + 1, 0.0), Hct(static_cast<size_t>(KCP) * NCCP + 1, 0.0),
        Psi(static_cast<size_t>(KCP) * NVP + 1, 0.0), g0p(static_cast<size_t>(RS) * 64, 1.0), Esp(static_cast<size_t>(RS) * 64 * nx, 0.0),
        cip(static_cast<size_t>(RS) * 64, 0.0);
    const std::vector<double> ci_rows = single_row_curvature_inv(c);
    std::vector<uint32_t> vmask(64, 0u);
    std::vector<int32_t> row_of(static_cast<size_t>(RS) * 64, -1);
    auto put_side = [&](int side, int lane, int row) {
        const size_t sl = static_cast<size_t>(side) * 64 + lane;
        g0p[sl] = c.g0s[row];
        cip[sl] = ci_rows[row];
        for (int j = 0; j < nx; ++j) Esp[static_cast<size_t>(j) * RS * 64 + sl] = c.Es(row, j);
        vmask[lane] |= 1u << side;
        row_of[sl] = row;
    };
    auto put_dense = [&](int fslot, int lane, int row) {
        for (int j = 0; j < c.nv; ++j) Gt[static_cast<size_t>(fslot * 64 + lane) * LDG + j] = c.Gs(row, j);
    };
    auto put_fact = [&](int fslot, int lane, int row) {
        for (int a = 0; a < kc; ++a) Hct[static_cast<size_t>(a) * NCCP + fslot * 64 + lane] = c.Hc(row - c.fb0, a);
    };
    for (size_t f = 0; f < dpair.size(); ++f) {
        const int k = static_cast<int>(f / 64), lane = static_cast<int>(f % 64);
        put_dense(k, lane, dpair[f].first);
        put_side(2 * k, lane, dpair[f].first);
        put_side(2 * k + 1, lane, dpair[f].second);
    }
    for (size_t f = 0; f < dsing.size(); ++f) {
        const int k = static_cast<int>(f / 64), lane = static_cast<int>(f % 64);
        put_dense(DP + k, lane, dsing[f]);
        put_side(2 * DP + k, lane, dsing[f]);
    }
    const int cb = 2 * DP + DS;
    for (size_t f = 0; f < cpair.size(); ++f) {
        const int k = static_cast<int>(f / 64), lane = static_cast<int>(f % 64);
        put_fact(k, lane, cpair[f].first);
        put_side(cb + 2 * k, lane, cpair[f].first);
        put_side(cb + 2 * k + 1, lane, cpair[f].second);
    }
    for (size_t f = 0; f < csing.size(); ++f) {
        const int k = static_cast<int>(f / 64), lane = static_cast<int>(f % 64);
        put_fact(CP + k, lane, csing[f]);
        put_side(cb + 2 * CP + k, lane, csing[f]);
    }
    for (int a = 0; a < kc; ++a)
        for (int j = 0; j < c.nv; ++j) Psi[static_cast<size_t>(a) * NVP + j] = c.Psi(a, j);
    tmpc::DeviceQP &d = v.d;
    int rc;
    if ((rc = upload_common(h, v, p, d, NVP))) return rc;
    d.nd = use_fact ? c.nd : c.nc; d.ncc = use_fact ? c.ncc : 0; d.kc = kc;
    {
        // k-steps (4 functionals each) of the MFMA pass over the dense functionals: up to the last one in use
        const int last = dsing.empty() ? static_cast<int>(dpair.size()) : DP * 64 + static_cast<int>(dsing.size());
        d.nks = (last + 3) / 4;
    }
    if ((rc = upload(h, v, Gt.data(), Gt.size(), &d.Gt))) return rc;
    if ((rc = upload(h, v, Hct.data(), Hct.size(), &d.Hct))) return rc;
    if ((rc = upload(h, v, Psi.data(), Psi.size(), &d.Psi))) return rc;
    if ((rc = upload(h, v, g0p.data(), g0p.size(), &d.g0p))) return rc;
    if ((rc = upload(h, v, Esp.data(), Esp.size(), &d.Esp))) return rc;
    if ((rc = upload(h, v, cip.data(), cip.size(), &d.cip))) return rc;
    if ((rc = upload(h, v, vmask.data(), vmask.size(), &d.vmask))) return rc;
    if ((rc = upload(h, v, row_of.data(), row_of.size(), &d.row_of))) return rc;
#ifdef TMPC_STAMPS
    if ((rc = upload_stamps(h, v, &d.dbg))) return rc;
#endif
    v.wave_ok = true;
    return TMPC_OK;
}

// workgroup-per-QP path (tmpc_block.hip): every row dense, nv padded to a multiple of 16
int upload_block(tmpc_handle *h, Variant &v, const tmpc_problem &p) {
    const tmpc::Condensed &c = v.c;
    v.tiles = tmpc::block_tiles(c.nv);
    if (v.tiles == 0) return TMPC_OK;
    const int NVP = 16 * v.tiles, nx = c.nx;
    // the Z rows of a free initial state touch x_0 only: the block kernel treats them as a narrow class when there are many
    const int nz4 = (c.off_x0 >= 0 && c.nz >= 256) ? (c.nz / 4) * 4 : 0;
    // Functionals (tmpc_device.hpp, BlockQP): when every row has its mirror row (the two sides of a box-type constraint; exact
    // to 1e-13 after scaling, Condensed::mirror) a row of G serves both, and the G-sized passes read half the rows.
    // TMPC_BLOCK_PAIRS=0 (developer knob) keeps a row of G per constraint row.
    bool paired = nz4 == 0 && c.nc >= 2 && static_cast<int>(c.mirror.size()) == c.nc;
    for (int r = 0; paired && r < c.nc; ++r) paired = c.mirror[r] >= 0 && c.mirror[r] < c.nc && c.mirror[r] != r && c.mirror[c.mirror[r]] == r;
    if (const char *e = std::getenv("TMPC_BLOCK_PAIRS")) paired = paired && std::atoi(e) != 0;
    // rows of G: constraint rows, or the first member of every pair
    std::vector<int> grow;
    for (int r = 0; r < c.nc; ++r)
        if (!paired || c.mirror[r] > r) grow.push_back(r);
    // (a QP without inequality rows -- the unconstrained regulator -- keeps one chunk of 64 padding rows, g = 0 and h = 1: they
    // never bind, the kernel's row loops and its workspace stay those of any other problem)
    const int ng = static_cast<int>(grow.size()), ngp = std::max(64, (ng + 63) / 64 * 64);
    const int mir = paired ? ngp : 0, ncp = paired ? 2 * ngp : ngp;
    // Staircase of the condensed constraints: the rows of stage k act on u_0 .. u_k only, so the leading rows of G are
    // zero beyond a few 16-column tiles.  The general rows are ordered by the number of tiles they reach (stable), and the
    // kernel skips the tiles / columns a row does not touch (exact: the skipped entries are zero).
    std::vector<int> ext(ng, 1), order(ng);
    for (int k = 0; k < ng; ++k) {
        int last = 0;
        for (int j = 0; j < c.nv; ++j)
            if (c.Gs(grow[k], j) != 0.0) last = j;
        ext[k] = last / 16 + 1;
        order[k] = k;
    }
    std::stable_sort(order.begin() + nz4, order.end(), [&](int a, int b) { return ext[a] < ext[b]; });
    // (Grm: the NVP rows of the scaled Hessian, identity on the padding, follow the rows of G -- gt_products adds Hs z in its pass)
    std::vector<double> Grm(static_cast<size_t>(ngp + NVP) * NVP, 0.0), Gcm(static_cast<size_t>(ngp) * NVP, 0.0), g0(ncp, 1.0),
        Es(static_cast<size_t>(ncp) * nx, 0.0);
    for (int i = 0; i < NVP; ++i)
        for (int j = 0; j < NVP; ++j)
            Grm[static_cast<size_t>(ngp + i) * NVP + j] = (i < c.nv && j < c.nv) ? c.Hs(i, j) : (i == j ? 1.0 : 0.0);
    std::vector<double> Gw(paired ? static_cast<size_t>(ncp) * NVP : 0, 0.0), GH(static_cast<size_t>(ncp) * NVP, 0.0);
    std::vector<int32_t> ncols(ngp, c.nv);
    std::vector<double> ci(ncp, 0.0);
    const std::vector<double> ci_rows = single_row_curvature_inv(c);
    for (int t = 0; t <= 8; ++t) v.bq.row_start[t] = ng;
    for (int rr = ng - 1; rr >= nz4; --rr)
        for (int t = 0; t < ext[order[rr]] && t <= 8; ++t) v.bq.row_start[t] = rr;
    v.bq.row_start[0] = nz4;
    for (int rr = 0; rr < ng; ++rr) {
        const int r = grow[order[rr]];
        ncols[rr] = rr < nz4 ? c.nv : std::min(c.nv, 16 * ext[order[rr]]);
        for (int j = 0; j < c.nv; ++j) {
            const double g = c.Gs(r, j);
            Grm[static_cast<size_t>(rr) * NVP + j] = g;
            Gcm[static_cast<size_t>(j) * ngp + rr] = g;
            double t = 0.0;
            for (int k = 0; k < c.nv; ++k) t += c.Gs(r, k) * c.Hinv(k, j);
            GH[static_cast<size_t>(rr) * NVP + j] = t;
            if (paired) {
                // the lower side is the negated functional (not the mirror row's own entries, which agree to 1e-13): every
                // pass sees the same row
                Gw[static_cast<size_t>(rr) * NVP + j] = g;
                Gw[static_cast<size_t>(rr + mir) * NVP + j] = -g;
                GH[static_cast<size_t>(rr + mir) * NVP + j] = -t;
            }
        }
        g0[rr] = c.g0s[r];
        ci[rr] = ci_rows[r];
        for (int j = 0; j < nx; ++j) Es[static_cast<size_t>(rr) * nx + j] = c.Es(r, j);
        if (paired) {
            const int q = c.mirror[r];
            g0[rr + mir] = c.g0s[q];
            ci[rr + mir] = ci_rows[q];
            for (int j = 0; j < nx; ++j) Es[static_cast<size_t>(rr + mir) * nx + j] = c.Es(q, j);
        }
    }
    int rc;
    if ((rc = upload_common(h, v, p, v.db, NVP))) return rc;
    v.db.nd = c.nc; v.db.ncc = 0; v.db.kc = 0; v.db.nks = 0;
    v.db.Gt = v.db.Hct = v.db.Psi = v.db.g0p = v.db.Esp = v.db.cip = nullptr;
    v.db.vmask = nullptr; v.db.row_of = nullptr;
    v.bq.ncp = ncp;
    v.bq.nz4 = nz4;
    v.bq.zx0 = c.off_x0 >= 0 ? c.off_x0 : 0;
    v.bq.znx = nx;
    v.bq.mir = mir; v.bq.ng = ng; v.bq.ngp = ngp;
    if ((rc = upload(h, v, Grm.data(), Grm.size(), &v.bq.Grm))) return rc;
    if ((rc = upload(h, v, Gcm.data(), Gcm.size(), &v.bq.Gcm))) return rc;
    if (paired) { if ((rc = upload(h, v, Gw.data(), Gw.size(), &v.bq.Gw))) return rc; }
    else v.bq.Gw = v.bq.Grm;
    if ((rc = upload(h, v, GH.data(), GH.size(), &v.bq.GHrm))) return rc;
    if ((rc = upload(h, v, g0.data(), g0.size(), &v.bq.g0))) return rc;
    if ((rc = upload(h, v, Es.data(), Es.size(), &v.bq.Es))) return rc;
    if ((rc = upload(h, v, ncols.data(), ncols.size(), &v.bq.ncols))) return rc;
    if ((rc = upload(h, v, ci.data(), ci.size(), &v.bq.ci))) return rc;
#ifdef TMPC_STAMPS
    if ((rc = upload_stamps(h, v, &v.db.dbg))) return rc;
#endif
    {
        const tmpc::BlockArgs rec{v.db, v.bq};
        if ((rc = upload(h, v, &rec, 1, &v.bargs))) return rc;
    }
    return TMPC_OK;
}

int upload_variant(tmpc_handle *h, Variant &v, const tmpc_problem &p) {
    int rc;
    if ((rc = upload_wave(h, v, p))) return rc;
    if ((rc = upload_block(h, v, p))) return rc;
    if (!v.wave_ok && v.tiles == 0) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "condensed QP (nv=%d, rows=%d) is outside the compiled kernels (nv <= 128)", v.c.nv, v.c.nc);
        h->err = buf;
        return TMPC_E_UNSUPPORTED;
    }
    return TMPC_OK;
}

// Waits for everything enqueued on the handle, on either lane.
hipError_t sync_lanes(tmpc_handle *h) {
    hipError_t e = h->stream ? hipStreamSynchronize(h->stream) : hipSuccess;
    Lane &second = h->lane[1];
    if (e == hipSuccess && second.stream) e = hipStreamSynchronize(second.stream);
    if (e == hipSuccess)
        for (Lane &l : h->lane) l.inflight.clear();
    return e;
}

// Orders the primary lane behind what the secondary lane has been given, without blocking the host: the start of every entry
// point that runs on the primary lane alone.  Each of them ends with a synchronisation of that lane, which then covers both.
int join_lanes(tmpc_handle *h) {
    Lane &second = h->lane[1];
    if (second.stream && !second.inflight.empty()) HIP_TRY(h, hipStreamWaitEvent(h->stream, second.inflight.back().end, 0));
    h->cur = 0;
    return TMPC_OK;
}

// block-kernel workspace of a lane: one slice per resident workgroup, sized once for the largest variant (a slice is addressed
// with the launching variant's ncp)
int ensure_block_ws(tmpc_handle *h, Lane &lane) {
    if (lane.blk_ws.p) return TMPC_OK;
    int ncp = 0, occ_max = 1;
    for (int k = 0; k < h->nvariants; ++k)
        if (h->v[k].tiles) { ncp = std::max(ncp, h->v[k].bq.ncp); occ_max = std::max(occ_max, tmpc::block_occupancy(h->v[k].tiles)); }
    h->blk_blocks = h->n_cu * occ_max;
    HIP_TRY(h, lane.blk_ws.reserve(static_cast<size_t>(h->blk_blocks) * tmpc::block_workspace_rows() * ncp * sizeof(double), lane.stream));
    return TMPC_OK;
}

bool use_block(const tmpc_handle *h, const Variant &v) { return h->kernel_path == TMPC_PATH_BLOCK ? v.tiles != 0 : !v.wave_ok; }

// offsets and sub-buffers for a batch of B (tightly packed for THIS batch, whatever the capacity: the DMAs of a call move
// exactly its bytes); returns the total
size_t layout_staging(tmpc_handle *h, int64_t B) {
    const size_t nx = h->nx, nu = h->nu, N = h->N, b = static_cast<size_t>(B);
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    // inputs
    h->off_r = up(b * nx * sizeof(double));
    h->off_var = h->off_r + up(b * nx * sizeof(double));
    h->stage_in_bytes = h->off_var + up(b);
    // outputs (x_nom last: it is optional and by far the largest)
    h->off_x0 = up(b * N * nu * sizeof(double));
    h->off_ss = h->off_x0 + up(b * nx * sizeof(double));
    h->off_st = h->off_ss + up(b * (nx + nu) * sizeof(double));
    h->off_it = h->off_st + up(b * sizeof(int32_t));
    h->stage_out_core = h->off_it + up(b * sizeof(int32_t));
    h->off_xn = h->stage_out_core;
    h->stage_out_bytes = h->off_xn + up(b * (N + 1) * nx * sizeof(double));
    if (h->stage_dev.p != nullptr) {
        char *in = h->stage_dev.p, *out = h->stage_dev.p + h->stage_in_bytes;
        h->d_x = reinterpret_cast<double *>(in);
        h->d_r = reinterpret_cast<double *>(in + h->off_r);
        h->d_var = reinterpret_cast<uint8_t *>(in + h->off_var);
        h->d_u = reinterpret_cast<double *>(out);
        h->d_x0 = reinterpret_cast<double *>(out + h->off_x0);
        h->d_ss = reinterpret_cast<double *>(out + h->off_ss);
        h->d_st = reinterpret_cast<int32_t *>(out + h->off_st);
        h->d_it = reinterpret_cast<int32_t *>(out + h->off_it);
        h->d_xn = reinterpret_cast<double *>(out + h->off_xn);
    }
    return h->stage_in_bytes + h->stage_out_bytes;
}

int ensure_staging(tmpc_handle *h, int64_t B) {
    const size_t total = layout_staging(h, B);
    if (total <= h->stage_dev.cap) return TMPC_OK;
    const hipError_t e = h->stage_dev.reserve(total, h->stream);       // (waits for the queued work, which may use the mirror too)
    if (h->stage_pin) (void)hipHostFree(h->stage_pin);
    h->stage_pin = nullptr;
    HIP_TRY(h, e);
    // the pinned mirror is a convenience, not a requirement: without it (or beyond 64 MB) the call copies from / to the
    // caller's buffers directly
    if (total <= (64u << 20) && hipHostMalloc(reinterpret_cast<void **>(&h->stage_pin), total, hipHostMallocDefault) != hipSuccess) {
        h->stage_pin = nullptr;
        (void)hipGetLastError();
    }
    (void)layout_staging(h, B);             // (the sub-buffers in the new block)
    return TMPC_OK;
}

// Regulator handles: B x nx zeros in device memory, handed to the solve kernels as their reference (the condensed QP has F2 = 0, but
// 0 * garbage is not 0 when the garbage is a NaN)
int ensure_reg_zero(tmpc_handle *h, int64_t B) {
    const size_t bytes = static_cast<size_t>(B) * h->nx * sizeof(double);
    if (bytes <= h->reg_zero.cap) return TMPC_OK;
    HIP_TRY(h, sync_lanes(h));             // (launches on either lane read the old block)
    HIP_TRY(h, h->reg_zero.reserve(bytes, h->stream));
    HIP_TRY(h, hipMemset(h->reg_zero.p, 0, bytes));
    return TMPC_OK;
}

// The next pair of timing events of the handle's pool (tmpc_last_kernel_ms / tmpc_kernel_ms_total read them); records the first one
// on the lane's stream.  Beyond 4096 pairs the last one is reused.
int begin_timed_launch(tmpc_handle *h, Lane &lane) {
    hipEvent_t e0 = h->pool.back().first, e1 = h->pool.back().second;
    if (h->pool_used < 4096) {
        if (h->pool_used == h->pool.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            HIP_TRY(h, hipEventCreate(&a));
            HIP_TRY(h, hipEventCreate(&b));
            h->pool.emplace_back(a, b);
        }
        e0 = h->pool[h->pool_used].first;
        e1 = h->pool[h->pool_used].second;
        if (h->pool_lane.size() <= h->pool_used) h->pool_lane.resize(h->pool.size(), 0);
        h->pool_lane[h->pool_used] = static_cast<uint8_t>(&lane - h->lane);
        ++h->pool_used;
    }
    h->ev0 = e0; h->ev1 = e1;
    HIP_TRY(h, hipEventRecord(h->ev0, lane.stream));
    return TMPC_OK;
}

// Scratch of the solve launches of the first nvar variants over B instances: the per-solve tick buffer (zeroed; with
// tmpc_set_solve_timing on) and the wave kernel's hand-over save slots, one per resident wave (at most 8 per CU).  The variants
// share the slots: launches on one stream do not overlap, and a launch reads only what it wrote itself.  Both buffers are the
// lane's own, so the same holds for each lane while launches on different lanes overlap; a buffer that grows waits for its
// lane alone, the only one whose launches use it.
int prepare_wave_scratch(tmpc_handle *h, Lane &lane, int64_t B, int nvar) {
    long long *ticks = nullptr;
    if (h->want_ticks) {
        const size_t bytes = static_cast<size_t>(B) * sizeof(long long);
        HIP_TRY(h, lane.ticks.reserve(bytes, lane.stream));
        ticks = lane.ticks.as<long long>();
        h->ticks_n = B;
        h->ticks_lane = static_cast<int>(&lane - h->lane);
        HIP_TRY(h, hipMemsetAsync(ticks, 0, bytes, lane.stream));
    }
    size_t save = 0;
    for (int k = 0; k < nvar; ++k) {
        const tmpc::KernelShape &s = h->v[k].shape;
        if (!use_block(h, h->v[k]) && !tmpc::parks_in_lds(s))
            save = std::max(save, static_cast<size_t>(h->n_cu) * 8 * 2 * (2 * s.dp + s.ds + 2 * s.cp + s.cs) * 64 * sizeof(float));
    }
    HIP_TRY(h, lane.save.reserve(save, lane.stream));
    for (int k = 0; k < nvar; ++k) {
        Variant &v = h->v[k];
        v.d.ticks = v.db.ticks = ticks;          // (kernel arguments of the launches that follow: copied when they are enqueued)
        if (!use_block(h, v)) v.d.save = tmpc::parks_in_lds(v.shape) ? nullptr : lane.save.as<float>();
    }
    return TMPC_OK;
}

// All kernels of one solve call, on one lane and in one order: the variant marking, then one launch per variant.
int enqueue(tmpc_handle *h, Lane &lane, const tmpc::BatchIO &io, int32_t *const *ws = nullptr, bool variants_valid = false) {
    { const int rce = begin_timed_launch(h, lane); if (rce) return rce; }
    if (io.variant != nullptr && !variants_valid)      // (the closed loop's selector is its own gamma flags: always 0 or 1)
        HIP_TRY(h, tmpc::launch_mark_invalid_variants(io, h->nvariants, h->nx, h->nu, h->N, lane.stream));
    const int nvar = io.variant != nullptr ? h->nvariants : 1;        // (no per-instance selector: everything is variant 0)
    { const int rcs = prepare_wave_scratch(h, lane, io.B, nvar); if (rcs) return rcs; }
    for (int k = 0; k < nvar; ++k) {
        Variant &v = h->v[k];
        if (use_block(h, v)) {
            int rcw = ensure_block_ws(h, lane);
            if (rcw) return rcw;
            HIP_TRY(h, tmpc::launch_block(v.db, v.bargs, v.tiles, lane.blk_ws.as<double>(), h->blk_blocks, k, io, &lane.wc, lane.stream));
            continue;
        }
        HIP_TRY(h, tmpc::launch_solve(v.d, v.shape, k, io, ws ? ws[k] : nullptr, ws ? ws[k] : nullptr, &lane.wc, h->n_cu, lane.stream));
    }
    HIP_TRY(h, hipEventRecord(h->ev1, lane.stream));
    h->timed = true;
    return TMPC_OK;
}

// A stream and a zeroed work-counter ring for a lane of the handle's device.
int create_lane(tmpc_handle *h, Lane &lane) {
    HIP_TRY(h, hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking));
    lane.wc.size = 4096;
    HIP_TRY(h, hipMalloc(reinterpret_cast<void **>(&lane.wc.ring), lane.wc.size * sizeof(unsigned long long)));
    HIP_TRY(h, hipMemset(lane.wc.ring, 0, lane.wc.size * sizeof(unsigned long long)));
    return TMPC_OK;
}

// Drops the records of the lane's calls that have finished (they finish in order).
void prune_finished(Lane &lane) {
    while (!lane.inflight.empty()) {
        if (hipEventQuery(lane.inflight.front().end) != hipSuccess) { (void)hipGetLastError(); break; }     // (not ready is no error)
        lane.inflight.pop_front();
    }
}

bool conflicts_with_lane(const Lane &lane, const tmpc::CallRanges &call) {
    for (const Lane::InFlight &f : lane.inflight)
        if (tmpc::calls_conflict(f.touched, call)) return true;
    return false;
}

// The lane of a tmpc_solve_batch_device call.  It goes to the other lane than the call before it when it has no RAW, WAW or WAR
// overlap with the unfinished calls of that call's lane: it may then run beside them, and on its own lane it is ordered behind
// whatever that lane holds.  Otherwise it stays on the lane of the call it conflicts with, behind it; if unfinished calls
// of the other lane conflict with it as well, its lane first waits for that lane's latest end event.  The second lane is created
// by the first call that finds unfinished, independent work to run beside.
int pick_lane(tmpc_handle *h, const tmpc::CallRanges &call, Lane **out) {
    *out = &h->lane[0];
    if (!h->overlap) return TMPC_OK;
    for (Lane &l : h->lane) prune_finished(l);
    Lane &prev = h->lane[h->cur], &other = h->lane[1 - h->cur];
    if (conflicts_with_lane(prev, call)) {
        if (other.stream && conflicts_with_lane(other, call)) {
            HIP_TRY(h, hipStreamWaitEvent(prev.stream, other.inflight.back().end, 0));
            ++h->lane_waits;
        }
        *out = &prev;
        return TMPC_OK;
    }
    if (!other.stream) {
        if (prev.inflight.empty()) { *out = &prev; return TMPC_OK; }
        if (const int rc = create_lane(h, other)) return rc;
    }
    *out = &other;
    return TMPC_OK;
}

// Notes a tmpc_solve_batch_device call just enqueued on `lane` as in flight.  Its end event is the call's timing event; when that
// one is, or will be, shared with other calls (the last of the 4096 pairs), one of the lane's spare events, recorded behind it.
int note_in_flight(tmpc_handle *h, Lane &lane, const tmpc::CallRanges &call) {
    hipEvent_t end = h->ev1;
    if (h->pool_used >= 4096) {
        while (lane.inflight.size() >= LANE_SPARE_EVENTS) {
            HIP_TRY(h, hipEventSynchronize(lane.inflight.front().end));
            lane.inflight.pop_front();
        }
        if (lane.spare.size() < LANE_SPARE_EVENTS) {
            hipEvent_t e = nullptr;
            HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            lane.spare.push_back(e);
        }
        end = lane.spare[lane.spare_next++ % LANE_SPARE_EVENTS];
        HIP_TRY(h, hipEventRecord(end, lane.stream));
    }
    lane.inflight.push_back({call, end});
    ++lane.calls;
    h->cur = static_cast<int>(&lane - h->lane);
    return TMPC_OK;
}

// Uploads the condensed variant(s) of a new handle to HIP device `device` (stream, work counters, timing events, kernel layouts),
// or, for device < 0, lays out the host-only copies.  `p` carries what the layouts read beyond the condensed QP (A, B, tol,
// max_iter).
int setup_handle(tmpc_handle *h, const tmpc_problem &p, int device) {
    if (device < 0) {
        // host-only handle: the layouts are laid out for the debug dumps only.  A problem no kernel covers (nv > 128) still
        // gets its handle -- tmpc_get_condensed and the oracle-side tests use it -- and the dump calls answer UNSUPPORTED
        // (wave_ok = false, tiles = 0).
        for (int k = 0; k < h->nvariants; ++k) {
            const int rc = upload_variant(h, h->v[k], p);
            if (rc == TMPC_E_UNSUPPORTED) h->err.clear();
            else if (rc) return rc;
        }
        return TMPC_OK;
    }
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        h->err = std::string("tmpc_create: no usable HIP device: ") + hipGetErrorString(e);
        return TMPC_E_DEVICE;
    }
    h->n_cu = prop.multiProcessorCount;
    if (const int rc = create_lane(h, h->lane[0])) return rc;
    h->stream = h->lane[0].stream;
    for (int i = 0; i < 256; ++i) {       // timing events are created up front, not in the solve path
        hipEvent_t a = nullptr, b = nullptr;
        HIP_TRY(h, hipEventCreate(&a));
        HIP_TRY(h, hipEventCreate(&b));
        h->pool.emplace_back(a, b);
    }
    for (int k = 0; k < h->nvariants; ++k)
        if (const int rc = upload_variant(h, h->v[k], p)) return rc;
    return TMPC_OK;
}

// tmpc_create / tmpc_create_regulator: the dimension check, a new handle, `condense` (fills in the handle's problem and sets the
// problem the kernel layouts read; returns what is wrong with it, or "") and the device set-up.  On failure the handle is
// destroyed and the message kept for tmpc_last_error(NULL).
template <class Condense>
int create_handle(const char *who, int nx, int nu, int N, int device, tmpc_handle **out, Condense condense) {
    *out = nullptr;
    if (nx <= 0 || nu <= 0 || N <= 0 || nx > 16) {
        g_create_error = std::string(who) + ": need 0 < nx <= 16, nu > 0, N > 0";
        return TMPC_E_INVALID;
    }
    tmpc_handle *h = new (std::nothrow) tmpc_handle();
    if (!h) { g_create_error = "out of memory"; return TMPC_E_NOMEM; }
    h->device = device; h->nx = nx; h->nu = nu; h->N = N;
    int rc = TMPC_E_INVALID;
    try {
        tmpc_problem q{};
        const std::string msg = condense(h, q);
        if (msg.empty()) rc = setup_handle(h, q, device);
        else h->err = std::string(who) + ": " + msg;
    } catch (const std::exception &ex) {
        h->err = std::string(who) + ": " + ex.what();
        rc = TMPC_E_NOMEM;
    }
    if (rc != TMPC_OK) {
        g_create_error = h->err;
        tmpc_destroy(h);
        return rc;
    }
    *out = h;
    return TMPC_OK;
}

// Argument checks of tmpc_solve_batch and tmpc_solve_batch_device, in the order they are reported; `variant_range`: the ids are
// host memory and checked here.  TMPC_OK with B = 0: nothing to do.
int check_solve(tmpc_handle *h, const char *who, int64_t B, const double *x_k, const double *ref, const uint8_t *variant,
                const double *u_nom, const double *xu_ss, const int32_t *status, const int32_t *iters, bool variant_range) {
    if (!h) return TMPC_E_INVALID;
    if (h->ses.open) { h->err = std::string(who) + ": a stepped closed loop is open on this handle (tmpc_mc_close first)"; return TMPC_E_INVALID; }
    if (B < 0 || !x_k || (!ref && !h->regulator) || !u_nom || !status || !iters) { h->err = std::string(who) + ": NULL argument"; return TMPC_E_INVALID; }
    if (h->regulator && (xu_ss || variant)) {
        h->err = std::string(who) + ": a regulator handle has no steady state and one problem (xu_ss, variant must be NULL)";
        return TMPC_E_INVALID;
    }
    if (B == 0) return TMPC_OK;
    if (variant_range && variant)
        for (int64_t i = 0; i < B; ++i)
            if (variant[i] >= h->nvariants) { h->err = std::string(who) + ": variant id out of range"; return TMPC_E_INVALID; }
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    HIP_TRY(h, hipSetDevice(h->device));
    return TMPC_OK;
}

// A layout dump (tmpc_debug_dump_layout / _block_layout): the tag, the header, then every array the layout points to, in the
// order given: byte count, bytes (0: null pointer)
int write_dump(const char *path, const Variant &v, std::initializer_list<std::pair<const void *, size_t>> header,
               std::initializer_list<const void *> arrays) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return TMPC_E_INVALID;
    const int32_t tag[2] = {tmpc::DUMP_TAG, tmpc::DUMP_FORMAT};
    std::fwrite(tag, 4, 2, f);
    for (const auto &[p, n] : header) std::fwrite(p, 1, n, f);
    for (const void *q : arrays) {
        uint64_t n = 0;
        if (q)
            for (size_t i = 0; i < v.dev.size(); ++i)
                if (v.dev[i] == q) { n = v.dev_bytes[i]; break; }
        std::fwrite(&n, 8, 1, f);
        if (n) std::fwrite(q, 1, n, f);
    }
    std::fclose(f);
    return TMPC_OK;
}

// What a stepped loop holds beyond the arena: its events and its pinned block.  The caller has synchronised.
void release_session(tmpc_handle *h) {
    McSession &s = h->ses;
    if (s.ev_in) (void)hipEventDestroy(s.ev_in);
    if (s.ev_out) (void)hipEventDestroy(s.ev_out);
    if (s.pin) (void)hipHostFree(s.pin);
    s = McSession{};
}

// Common start of the closed loops: what the last run left in the arena is unreadable from here on (tmpc_mc_get_capture /
// _solve_ticks / _physics_error must not read a freed or half-written arena); the staging block's outputs take the solves'.
int begin_loop(tmpc_handle *h, int64_t B) {
    h->rec = LoopRecords{};
    HIP_TRY(h, hipSetDevice(h->device));
    if (const int rc = join_lanes(h)) return rc;
    return ensure_staging(h, B);
}

// A stepped loop runs under the handle's settings as they were at tmpc_mc_open (its arrays are carved for them): no setter changes
// one under it.  True, with the message, while a session is open.
bool session_bars(tmpc_handle *h, const char *who) {
    if (!h->ses.open) return false;
    h->err = std::string(who) + ": a stepped closed loop is open on this handle (tmpc_mc_close first)";
    return true;
}

// The cart-pole rows {M, m, b, I, g, l, Th} of n trajectories (tmpc_estimate_w_models): empty if every row
// describes a plant, otherwise the message, which names trajectory and field.
std::string cartpole_rows_error(const char *who, const double *rows, int64_t n) {
    static const char *const field[7] = {"M", "m", "b", "I", "g", "l", "Th"};
    for (int64_t b = 0; b < n; ++b)
        for (int i = 0; i < 7; ++i) {
            const double v = rows[b * 7 + i];
            const char *why = nullptr;
            if (!std::isfinite(v)) why = "is not finite";
            else if ((i == 0 || i == 1 || i == 5 || i == 6) && !(v > 0.0)) why = "must be > 0";
            else if ((i == 2 || i == 3) && v < 0.0) why = "must be >= 0";
            if (why) return std::string(who) + ": " + field[i] + " of trajectory " + std::to_string(b) + " = " + std::to_string(v) + " " + why;
        }
    return std::string();
}

}  // namespace

extern "C" {

int tmpc_abi_version(void) { return TMPC_ABI_VERSION; }

const char *tmpc_last_error(const tmpc_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int tmpc_create(const tmpc_problem *p, int device, tmpc_handle **out) {
    if (!p || !out) { g_create_error = "tmpc_create: NULL argument"; return TMPC_E_INVALID; }
    return create_handle("tmpc_create", p->nx, p->nu, p->N, device, out, [p](tmpc_handle *h, tmpc_problem &q) {
        h->hA.assign(p->A ? p->A : nullptr, p->A ? p->A + p->nx * p->nx : nullptr);
        h->hB.assign(p->B ? p->B : nullptr, p->B ? p->B + p->nx * p->nu : nullptr);
        if (p->K) h->hK.assign(p->K, p->K + p->nu * p->nx);
        if (p->K_anc) h->hKanc.assign(p->K_anc, p->K_anc + p->nu * p->nx);
        h->nvariants = p->extended ? 2 : 1;
        q = *p;
        std::string msg;
        for (int k = 0; k < h->nvariants && msg.empty(); ++k) msg = tmpc::condense(*p, k, h->v[k].c);
        return msg;
    });
}

int tmpc_create_regulator(const tmpc_regulator_problem *p, int device, tmpc_handle **out) {
    if (!p || !out) { g_create_error = "tmpc_create_regulator: NULL argument"; return TMPC_E_INVALID; }
    return create_handle("tmpc_create_regulator", p->nx, p->nu, p->N, device, out, [p](tmpc_handle *h, tmpc_problem &q) {
        h->regulator = true;
        h->reg_tube = p->tube ? 1 : 0;
        h->nvariants = 1;
        const std::string msg = tmpc::condense_regulator(*p, h->v[0].c);
        if (!msg.empty()) return msg;
        const size_t nx = p->nx, nu = p->nu;
        h->hA.assign(p->A, p->A + nx * nx);
        h->hB.assign(p->B, p->B + nx * nu);
        h->hQ.assign(p->Q, p->Q + nx * nx);
        h->hR.assign(p->R, p->R + nu * nu);
        if (p->K) h->hK.assign(p->K, p->K + nu * nx);
        // what the kernel layouts read beyond the condensed QP
        q.nx = p->nx; q.nu = p->nu; q.N = p->N;
        q.max_iter = p->max_iter; q.tol = p->tol;
        q.A = p->A; q.B = p->B;
        return msg;
    });
}

void tmpc_destroy(tmpc_handle *h) {
    if (!h) return;
    if (h->device < 0) {
        for (int k = 0; k < 2; ++k)
            for (void *p : h->v[k].dev) std::free(p);
        delete h;
        return;
    }
    (void)hipSetDevice(h->device);
    for (Lane &l : h->lane)
        if (l.stream) (void)hipStreamSynchronize(l.stream);
    release_session(h);                  // (an open stepped loop ends here: its arrays go with the arena below)
    for (Lane &l : h->lane) {
        for (DeviceBuffer *b : {&l.blk_ws, &l.save, &l.ticks}) b->release();
        if (l.wc.ring) (void)hipFree(l.wc.ring);
        for (hipEvent_t e : l.spare) (void)hipEventDestroy(e);
    }
    for (DeviceBuffer *b : {&h->reg_zero, &h->stage_dev}) b->release();
    h->arena.release();
    if (h->stage_pin) (void)hipHostFree(h->stage_pin);
    for (int k = 0; k < 2; ++k)
        for (void *p : h->v[k].dev) (void)hipFree(p);
    for (auto &pr : h->pool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (Lane &l : h->lane)
        if (l.stream) (void)hipStreamDestroy(l.stream);
    delete h;
}

int tmpc_solve_batch_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant,
                            double *u_nom, double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters) {
    if (const int rc = check_solve(h, "tmpc_solve_batch_device", B, x_k, ref, variant, u_nom, xu_ss, status, iters, false); rc || B == 0) return rc;
    if (h->regulator) {
        const int rz = ensure_reg_zero(h, B);
        if (rz) return rz;
        ref = h->reg_zero.as<double>();
    }
    // (a regulator's reference is the handle's zero block, which nothing writes: not a range of the call)
    const tmpc::CallRanges call = tmpc::solve_call_ranges(B, h->nx, h->nu, h->N, x_k, h->regulator ? nullptr : ref, variant, u_nom, x_nom0, xu_ss,
                                                          x_nom, status, iters);
    Lane *lane = nullptr;
    if (const int rc = pick_lane(h, call, &lane)) return rc;
    if (const int rc = enqueue(h, *lane, {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, x_nom, status, iters})) return rc;
    return h->overlap ? note_in_flight(h, *lane, call) : (++lane->calls, TMPC_OK);
}

int tmpc_solve_batch(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant,
                     double *u_nom, double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters) {
    int rc = check_solve(h, "tmpc_solve_batch", B, x_k, ref, variant, u_nom, xu_ss, status, iters, true);
    if (rc || B == 0) return rc;
    if ((rc = join_lanes(h))) return rc;
    if ((rc = ensure_staging(h, B))) return rc;
    if (h->regulator && (rc = ensure_reg_zero(h, B))) return rc;
    const size_t nx = h->nx, nu = h->nu, N = h->N, b = static_cast<size_t>(B);
    // the caller's arrays and their offsets in the input / output part of the staging block (host NULL: not given / not wanted)
    const struct { size_t off; const void *host; size_t bytes; } in[] = {
        {0, x_k, b * nx * sizeof(double)}, {h->off_r, h->regulator ? nullptr : ref, b * nx * sizeof(double)}, {h->off_var, variant, b}};
    const struct { size_t off; void *host; size_t bytes; } out[] = {
        {0, u_nom, b * N * nu * sizeof(double)}, {h->off_x0, x_nom0, b * nx * sizeof(double)}, {h->off_ss, xu_ss, b * (nx + nu) * sizeof(double)},
        {h->off_st, status, b * sizeof(int32_t)}, {h->off_it, iters, b * sizeof(int32_t)}, {h->off_xn, x_nom, b * (N + 1) * nx * sizeof(double)}};
    char *const dev_in = h->stage_dev.p, *const dev_out = dev_in + h->stage_in_bytes;
    auto launch = [&]() {
        return enqueue(h, h->lane[0], {B, h->d_x, h->regulator ? h->reg_zero.as<double>() : h->d_r, variant ? h->d_var : nullptr, h->d_u, h->d_x0,
                           h->d_ss, x_nom ? h->d_xn : nullptr, h->d_st, h->d_it});
    };
    if (h->stage_pin != nullptr) {
        // through the pinned mirror: one DMA in, one out, each up to the last array given
        char *const pin_in = h->stage_pin, *const pin_out = h->stage_pin + h->stage_in_bytes;
        size_t in_bytes = 0, out_bytes = 0;
        for (const auto &a : in)
            if (a.host) { std::memcpy(pin_in + a.off, a.host, a.bytes); in_bytes = a.off + a.bytes; }
        for (const auto &a : out)
            if (a.host) out_bytes = a.off + a.bytes;
        HIP_TRY(h, hipMemcpyAsync(dev_in, pin_in, in_bytes, hipMemcpyHostToDevice, h->stream));
        if ((rc = launch())) return rc;
        HIP_TRY(h, hipMemcpyAsync(pin_out, dev_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, sync_lanes(h));
        for (const auto &a : out)
            if (a.host) std::memcpy(a.host, pin_out + a.off, a.bytes);
        return TMPC_OK;
    }
    for (const auto &a : in)
        if (a.host) HIP_TRY(h, hipMemcpyAsync(dev_in + a.off, a.host, a.bytes, hipMemcpyHostToDevice, h->stream));
    if ((rc = launch())) return rc;
    for (const auto &a : out)
        if (a.host) HIP_TRY(h, hipMemcpyAsync(a.host, dev_out + a.off, a.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sync_lanes(h));
    return TMPC_OK;
}

int tmpc_set_kernel_path(tmpc_handle *h, int path) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_set_kernel_path")) return TMPC_E_INVALID;
    if (path != TMPC_PATH_AUTO && path != TMPC_PATH_WAVE && path != TMPC_PATH_BLOCK) { h->err = "tmpc_set_kernel_path: unknown path"; return TMPC_E_INVALID; }
    for (int k = 0; k < h->nvariants; ++k) {
        if (path == TMPC_PATH_WAVE && !h->v[k].wave_ok && h->device >= 0) { h->err = "tmpc_set_kernel_path: no wave-per-QP shape covers this problem"; return TMPC_E_UNSUPPORTED; }
        if (path == TMPC_PATH_BLOCK && h->v[k].tiles == 0 && h->device >= 0) { h->err = "tmpc_set_kernel_path: the block kernel needs nv <= 128"; return TMPC_E_UNSUPPORTED; }
    }
    h->kernel_path = path;
    return TMPC_OK;
}

int tmpc_get_kernel_path(const tmpc_handle *h, int variant) {
    if (!h || variant < 0 || variant >= h->nvariants) return TMPC_E_INVALID;
    return use_block(h, h->v[variant]) ? TMPC_PATH_BLOCK : TMPC_PATH_WAVE;       // (host-only handles included: the choice is made at tmpc_create)
}

int tmpc_debug_dump_layout(const tmpc_handle *h, int variant, const char *path) {
    if (!h || !path || variant < 0 || variant >= h->nvariants) return TMPC_E_INVALID;
    if (h->device >= 0) return TMPC_E_UNSUPPORTED;            // the arrays of a device handle live in HBM
    const Variant &v = h->v[variant];
    if (!v.wave_ok) return TMPC_E_UNSUPPORTED;
    const int32_t shp[6] = {v.shape.nvp, v.shape.dp, v.shape.ds, v.shape.kcp, v.shape.cp, v.shape.cs};
    const uint64_t qp_bytes = sizeof(tmpc::DeviceQP);
    return write_dump(path, v, {{shp, sizeof shp}, {&qp_bytes, sizeof qp_bytes}, {&v.d, sizeof v.d}},
                      {v.d.Gt, v.d.Hct, v.d.Psi, v.d.Hs, v.d.Hinv, v.d.F1s, v.d.F2s, v.d.g0p, v.d.Esp, v.d.vmask, v.d.row_of,
                       v.d.gp0, v.d.Ep, v.d.Dv, v.d.Tzs, v.d.Txf, v.d.Mth, v.d.A, v.d.B, v.d.cip});
}

int tmpc_debug_dump_block_layout(const tmpc_handle *h, int variant, const char *path) {
    if (!h || !path || variant < 0 || variant >= h->nvariants) return TMPC_E_INVALID;
    if (h->device >= 0) return TMPC_E_UNSUPPORTED;
    const Variant &v = h->v[variant];
    if (v.tiles == 0) return TMPC_E_UNSUPPORTED;
    const int32_t hd[2] = {v.tiles, tmpc::block_workspace_rows()};
    const uint64_t sz[2] = {sizeof(tmpc::DeviceQP), sizeof(tmpc::BlockQP)};
    return write_dump(path, v, {{hd, sizeof hd}, {sz, sizeof sz}, {&v.db, sizeof v.db}, {&v.bq, sizeof v.bq}},
                      {v.db.Hs, v.db.Hinv, v.db.F1s, v.db.F2s, v.db.gp0, v.db.Ep, v.db.Dv, v.db.Tzs, v.db.Txf, v.db.Mth, v.db.A, v.db.B,
                       v.bq.Grm, v.bq.Gcm, v.bq.GHrm, v.bq.g0, v.bq.Es, v.bq.ncols, v.bq.Gw == v.bq.Grm ? nullptr : v.bq.Gw, v.bq.ci});
}

const char *tmpc_kernel_name(const tmpc_handle *h, int variant) {
    if (!h || variant < 0 || variant >= h->nvariants) return "";
    const Variant &v = h->v[variant];
    return use_block(h, v) ? tmpc::block_kernel_name(v.tiles) : tmpc::kernel_name(v.shape);
}

int tmpc_mc_set_actuator(tmpc_handle *h, int kind) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_actuator")) return TMPC_E_INVALID;
    if (kind != TMPC_ACTUATOR_CONSISTENT && kind != TMPC_ACTUATOR_SMART) { h->err = "tmpc_mc_set_actuator: unknown actuator"; return TMPC_E_INVALID; }
    h->actuator = kind;
    return TMPC_OK;
}

int tmpc_mc_set_plant(tmpc_handle *h, int kind, const double *par7, int substeps) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_plant")) return TMPC_E_INVALID;
    if (kind == TMPC_PLANT_LINEAR) { h->plant = kind; return TMPC_OK; }
    if (kind != TMPC_PLANT_CARTPOLE || !par7 || substeps < 1) { h->err = "tmpc_mc_set_plant: unknown plant or missing parameters"; return TMPC_E_INVALID; }
    if (h->nx != 4 || h->nu != 1) { h->err = "tmpc_mc_set_plant: the cart-pole plant needs nx = 4, nu = 1"; return TMPC_E_INVALID; }
    for (int i = 0; i < 7; ++i) h->plant_par[i] = par7[i];
    h->plant = kind;
    h->plant_substeps = substeps;
    return TMPC_OK;
}

int tmpc_mc_set_plant_models(tmpc_handle *h, int kind, int64_t B, const double *models, int substeps) {
    if (!h) return TMPC_E_INVALID;
    const char *who = "tmpc_mc_set_plant_models";
    (void)substeps;
    if (session_bars(h, who)) return TMPC_E_INVALID;
    if (!h->regulator) { h->err = std::string(who) + ": only regulator handles (tmpc_reg_run) take a plant per trajectory"; return TMPC_E_UNSUPPORTED; }
    if (B < 0) { h->err = std::string(who) + ": B < 0"; return TMPC_E_INVALID; }
    if (B == 0) {
        h->mc_pm_B = 0;
        h->mc_pm.clear();
        return TMPC_OK;
    }
    if (kind == TMPC_PLANT_CARTPOLE) { h->err = std::string(who) + ": a regulator handle runs linear plants only"; return TMPC_E_INVALID; }
    if (kind != TMPC_PLANT_LINEAR) { h->err = std::string(who) + ": kind is TMPC_PLANT_LINEAR"; return TMPC_E_INVALID; }
    if (!models) { h->err = std::string(who) + ": models is NULL"; return TMPC_E_INVALID; }
    const int64_t nx = h->nx, wid = h->nx + h->nu;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t i = 0; i < nx; ++i)
            for (int64_t j = 0; j < wid; ++j)
                if (!std::isfinite(models[(b * nx + i) * wid + j])) {
                    h->err = std::string(who) + ": " + (j < nx ? "A" : "B") + "[" + std::to_string(i) + ", " + std::to_string(j < nx ? j : j - nx) +
                             "] of trajectory " + std::to_string(b) + " is not finite";
                    return TMPC_E_INVALID;
                }
    h->mc_pm.assign(models, models + static_cast<size_t>(B) * static_cast<size_t>(nx * wid));
    h->mc_pm_B = B;
    return TMPC_OK;
}

int tmpc_mc_set_capture(tmpc_handle *h, int64_t index) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_capture")) return TMPC_E_INVALID;
    h->mc_capture = index < 0 ? -1 : index;
    return TMPC_OK;
}

int tmpc_mc_get_capture(tmpc_handle *h, int32_t T, double *x_traj, double *x_nom_traj, double *u_traj) {
    if (!h) return TMPC_E_INVALID;
    if (!h->rec.cap || T != h->rec.cap_T) { h->err = "tmpc_mc_get_capture: no trajectory of this length was recorded by the last tmpc_mc_run"; return TMPC_E_INVALID; }
    const size_t nx = h->nx, nu = h->nu, w = 2 * nx + nu;
    std::vector<double> buf(static_cast<size_t>(T) * w);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(buf.data(), h->rec.cap, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int t = 0; t < T; ++t) {
        for (size_t i = 0; i < nx; ++i) {
            if (x_traj) x_traj[t * nx + i] = buf[t * w + i];
            if (x_nom_traj) x_nom_traj[t * nx + i] = buf[t * w + nx + i];
        }
        for (size_t j = 0; j < nu; ++j) if (u_traj) u_traj[t * nu + j] = buf[t * w + 2 * nx + j];
    }
    return TMPC_OK;
}

int tmpc_set_solve_timing(tmpc_handle *h, int on) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_set_solve_timing")) return TMPC_E_INVALID;
    h->want_ticks = on ? 1 : 0;
    if (!on) h->ticks_n = 0;
    return TMPC_OK;
}

int tmpc_get_solve_ticks(tmpc_handle *h, int64_t B, int64_t *ticks) {
    if (!h || !ticks) return TMPC_E_INVALID;
    const DeviceBuffer &tk = h->lane[h->ticks_lane].ticks;
    if (!h->want_ticks || B != h->ticks_n || !tk.p) { h->err = "tmpc_get_solve_ticks: no solve of this batch size was timed (tmpc_set_solve_timing)"; return TMPC_E_INVALID; }
    static_assert(sizeof(long long) == sizeof(int64_t), "tick counts are 64-bit");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    HIP_TRY(h, hipMemcpy(ticks, tk.p, static_cast<size_t>(B) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_mc_get_solve_ticks(tmpc_handle *h, int64_t B, int64_t *ticks_sum, int64_t *ticks_max) {
    if (!h) return TMPC_E_INVALID;
    if (!h->rec.tick_sum || B != h->rec.tick_B) { h->err = "tmpc_mc_get_solve_ticks: the last tmpc_mc_run was not timed (tmpc_set_solve_timing) or had another batch size"; return TMPC_E_INVALID; }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    if (ticks_sum) HIP_TRY(h, hipMemcpy(ticks_sum, h->rec.tick_sum, static_cast<size_t>(B) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (ticks_max) HIP_TRY(h, hipMemcpy(ticks_max, h->rec.tick_max, static_cast<size_t>(B) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_mc_set_device_rng(tmpc_handle *h, int on, uint64_t seed, int64_t first_trajectory, const double *w_bound) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_device_rng")) return TMPC_E_INVALID;
    h->mc_rng_on = on ? 1 : 0;
    h->mc_rng_seed = seed;
    h->mc_rng_first = first_trajectory;
    h->mc_w_bound.assign(static_cast<size_t>(h->nx), 0.0);
    if (on && w_bound)
        for (int i = 0; i < h->nx; ++i) h->mc_w_bound[i] = w_bound[i];
    return TMPC_OK;
}

int tmpc_mc_get_physics_error(tmpc_handle *h, int64_t B, double *err2_phys) {
    if (!h || !err2_phys) return TMPC_E_INVALID;
    if (!h->rec.err2_phys || B != h->rec.phys_B) { h->err = "tmpc_mc_get_physics_error: the last tmpc_mc_run had the linear plant or another batch size"; return TMPC_E_INVALID; }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    HIP_TRY(h, hipMemcpy(err2_phys, h->rec.err2_phys, static_cast<size_t>(B) * sizeof(double), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_mc_set_reference_table(tmpc_handle *h, int32_t K, int32_t T_tab, const double *table, int64_t B, const int32_t *ref_id) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_reference_table")) return TMPC_E_INVALID;
    if (h->regulator) { h->err = "tmpc_mc_set_reference_table: a regulator handle has no reference"; return TMPC_E_INVALID; }
    if (K < 0) { h->err = "tmpc_mc_set_reference_table: K < 0"; return TMPC_E_INVALID; }
    if (K == 0) {
        h->mc_ref_K = h->mc_ref_T = 0;
        h->mc_ref_B = 0;
        h->mc_ref_tab.clear();
        h->mc_ref_id.clear();
        return TMPC_OK;
    }
    if (T_tab < 1 || B < 1) { h->err = "tmpc_mc_set_reference_table: need T_tab >= 1 and B >= 1"; return TMPC_E_INVALID; }
    if (!table) { h->err = "tmpc_mc_set_reference_table: table is NULL"; return TMPC_E_INVALID; }
    if (!ref_id && K != 1 && K != B) {
        h->err = "tmpc_mc_set_reference_table: ref_id may be NULL only with K == 1 or K == B (K = " + std::to_string(K) + ", B = " + std::to_string(B) + ")";
        return TMPC_E_INVALID;
    }
    std::vector<int32_t> ids(static_cast<size_t>(B));
    for (int64_t b = 0; b < B; ++b) {
        const int32_t id = ref_id ? ref_id[b] : (K == 1 ? 0 : static_cast<int32_t>(b));
        if (id < 0 || id >= K) {
            h->err = "tmpc_mc_set_reference_table: ref_id[" + std::to_string(b) + "] = " + std::to_string(id) + " is not in [0, " + std::to_string(K) + ")";
            return TMPC_E_INVALID;
        }
        ids[static_cast<size_t>(b)] = id;
    }
    h->mc_ref_tab.assign(table, table + static_cast<size_t>(K) * static_cast<size_t>(T_tab) * static_cast<size_t>(h->nx));
    h->mc_ref_id.swap(ids);
    h->mc_ref_K = K;
    h->mc_ref_T = T_tab;
    h->mc_ref_B = B;
    return TMPC_OK;
}

int tmpc_mc_set_channel(tmpc_handle *h, int64_t B, const double *p_gb, const double *p_bg, const double *e_g, const double *e_b) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_channel")) return TMPC_E_INVALID;
    if (h->regulator) { h->err = "tmpc_mc_set_channel: a regulator handle has no network"; return TMPC_E_INVALID; }
    if (B < 0) { h->err = "tmpc_mc_set_channel: B < 0"; return TMPC_E_INVALID; }
    if (B == 0) {
        h->mc_ch_B = 0;
        h->mc_ch_thr.clear();
        return TMPC_OK;
    }
    if (!p_gb || !p_bg || !e_g || !e_b) { h->err = "tmpc_mc_set_channel: NULL argument"; return TMPC_E_INVALID; }
    const struct { const char *name; const double *v; } par[4] = {{"p_gb", p_gb}, {"p_bg", p_bg}, {"e_g", e_g}, {"e_b", e_b}};
    for (const auto &q : par)
        for (int64_t b = 0; b < B; ++b)
            if (!(q.v[b] >= 0.0 && q.v[b] <= 1.0)) {      // (NaN fails both)
                h->err = std::string("tmpc_mc_set_channel: ") + q.name + "[" + std::to_string(b) + "] = " + std::to_string(q.v[b]) + " is no probability";
                return TMPC_E_INVALID;
            }
    std::vector<double> thr(static_cast<size_t>(B) * 6);
    for (int64_t b = 0; b < B; ++b)
        for (int prev = 0; prev < 2; ++prev) {
            // a = P(B | previous state); every product and sum is rounded on its own (volatile: no contraction into a fused
            // multiply-add, whatever the host compiler's setting -- montecarlo.gilbert_elliott_thresholds is the numpy twin)
            const double a = prev == 0 ? p_gb[b] : 1.0 - p_bg[b];
            volatile double lost_b = a * e_b[b];
            volatile double good = 1.0 - a;
            volatile double lost_g = good * e_g[b];
            volatile double top = a + lost_g;
            double *r = thr.data() + (static_cast<size_t>(b) * 2 + prev) * 3;
            r[0] = lost_b; r[1] = a; r[2] = top;
        }
    h->mc_ch_thr.swap(thr);
    h->mc_ch_B = B;
    return TMPC_OK;
}

int tmpc_mc_get_channel(tmpc_handle *h, int64_t B, double *thr) {
    if (!h || !thr) return TMPC_E_INVALID;
    if (h->mc_ch_B == 0 || B != h->mc_ch_B) { h->err = "tmpc_mc_get_channel: no channel of this batch size is set (tmpc_mc_set_channel)"; return TMPC_E_INVALID; }
    std::memcpy(thr, h->mc_ch_thr.data(), h->mc_ch_thr.size() * sizeof(double));
    return TMPC_OK;
}

int tmpc_mc_get_link_stats(tmpc_handle *h, int64_t B, int32_t *lost_up, int32_t *lost_down, int32_t *max_gap, int32_t *overrun) {
    if (!h) return TMPC_E_INVALID;
    if (h->rec.link_B == 0 || B != h->rec.link_B) { h->err = "tmpc_mc_get_link_stats: no closed loop of this batch size has run (tmpc_mc_run, tmpc_mc_close)"; return TMPC_E_INVALID; }
    int32_t *const out[4] = {lost_up, lost_down, max_gap, overrun};
    const size_t b = static_cast<size_t>(B);
    for (size_t k = 0; k < 4; ++k)
        if (out[k]) std::memcpy(out[k], h->rec.link.data() + k * b, b * sizeof(int32_t));
    return TMPC_OK;
}

int tmpc_mc_set_warm_start(tmpc_handle *h, int on) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_warm_start")) return TMPC_E_INVALID;
    h->mc_warm = on ? 1 : 0;
    return TMPC_OK;
}

int tmpc_mc_set_fused(tmpc_handle *h, int mode) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_mc_set_fused")) return TMPC_E_INVALID;
    if (mode != TMPC_MC_FUSED_OFF && mode != TMPC_MC_FUSED_ON && mode != TMPC_MC_FUSED_AUTO) { h->err = "tmpc_mc_set_fused: mode is TMPC_MC_FUSED_OFF / _ON / _AUTO"; return TMPC_E_INVALID; }
    h->mc_fused = mode;
    return TMPC_OK;
}

int tmpc_mc_last_fused(const tmpc_handle *h) { return h ? h->rec.fused : 0; }

}  // extern "C"

namespace {
// packets injected by the caller (tmpc_mc_replay) and the per-step record that goes back
struct McReplay {
    const double *U, *xn0;      // host: [B][T][N+1][nu], [B][T][nx] (xn0 may be NULL unless extended)
    double *trace_f;            // host: [B][T][3 nx + nu]
    int32_t *trace_i;           // host: [B][T][3]
};

// A loop of B trajectories and T steps under the handle's reference table (tmpc_mc_set_reference_table): does it fit?
int reference_table_fits(tmpc_handle *h, const char *who, int64_t B, int32_t T) {
    if (B != h->mc_ref_B) {
        h->err = std::string(who) + ": B = " + std::to_string(B) + ", but the reference table was set for B = " + std::to_string(h->mc_ref_B) + " trajectories";
        return TMPC_E_INVALID;
    }
    if (T > h->mc_ref_T) {
        h->err = std::string(who) + ": T = " + std::to_string(T) + " steps, but the reference table has T_tab = " + std::to_string(h->mc_ref_T) + " rows";
        return TMPC_E_INVALID;
    }
    return TMPC_OK;
}
// the table's pieces of a loop's arena (uploaded with the loop, as `ref` is)
void reference_table_pieces(tmpc_handle *h, Arena &a, tmpc::McState &st) {
    a.piece(&st.ref_tab, h->mc_ref_tab.size() * 8, h->mc_ref_tab.data());
    a.piece(&st.ref_id, h->mc_ref_id.size() * 4, h->mc_ref_id.data());
    st.ref_T = h->mc_ref_T;
}

// A loop of B trajectories under the handle's loss channel (tmpc_mc_set_channel): does it fit?
int channel_fits(tmpc_handle *h, const char *who, int64_t B) {
    if (B == h->mc_ch_B) return TMPC_OK;
    h->err = std::string(who) + ": B = " + std::to_string(B) + ", but the loss channel was set for B = " + std::to_string(h->mc_ch_B) + " trajectories";
    return TMPC_E_INVALID;
}
// A loop of B trajectories under the handle's plant models (tmpc_mc_set_plant_models): does it fit?
int plant_models_fit(tmpc_handle *h, const char *who, int64_t B) {
    if (h->mc_pm_B == 0 || B == h->mc_pm_B) return TMPC_OK;
    h->err = std::string(who) + ": B = " + std::to_string(B) + ", but the plant models were set for B = " + std::to_string(h->mc_pm_B) + " trajectories";
    return TMPC_E_INVALID;
}
// the loss model's and the link statistics' pieces of a loop's arena: the channel's thresholds and link states (both links start
// in G) or p_loss, and the four counters -- one block [4][B], so that one copy brings them back (link_block_carved, fetch_link_stats)
void link_pieces(tmpc_handle *h, Arena &a, tmpc::McState &st, bool channel, size_t b, const double *p_loss) {
    if (channel) {
        a.piece(&st.ch_thr, h->mc_ch_thr.size() * 8, h->mc_ch_thr.data());
        a.piece(&st.ch_state, b * 2, nullptr, 0);
    } else {
        a.piece(&st.p_loss, b * 8, p_loss);
    }
    a.piece(&st.lost_up, b * 4 * 4, nullptr, 0);
}
void link_block_carved(tmpc::McState &st, size_t b) {
    st.lost_down = st.lost_up + b; st.max_gap = st.lost_up + 2 * b; st.overrun = st.lost_up + 3 * b;
}
// enqueues the copy of the counters into the handle's record; the caller synchronises and then sets rec.link_B
hipError_t fetch_link_stats(tmpc_handle *h, const tmpc::McState &st, size_t b) {
    h->rec.link.resize(4 * b);
    return hipMemcpyAsync(h->rec.link.data(), st.lost_up, b * 4 * 4, hipMemcpyDeviceToHost, h->stream);
}

int mc_run_impl(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *p_loss, const double *ref,
                const double *th_u, const double *ga_u, const double *w, const double *x0, const double *HZ, const double *hZ,
                int32_t rZ, double *err2, int32_t *tube_viol, int32_t *not_optimal, double *x_final, double *consistent,
                int32_t *iters_sum, const McReplay *rp) {
    if (!h) return TMPC_E_INVALID;
    if (h->ses.open) { h->err = "tmpc_mc_run: a stepped closed loop is open on this handle (tmpc_mc_close first)"; return TMPC_E_INVALID; }
    const bool host_draws = rp != nullptr || !h->mc_rng_on;
    const bool full_ref = !rp && h->mc_ref_K > 0;      // (tmpc_mc_replay solves nothing: it ignores the reference table)
    const bool channel = !rp && h->mc_ch_B > 0;        // (tmpc_mc_replay is given its arrival flags: it ignores the channel)
    if (B < 0 || T < 0 || (!p_loss && !channel) || (!ref && !full_ref) || (host_draws && (!th_u || !ga_u || !w)) || (rZ > 0 && (!HZ || !hZ))) { h->err = "tmpc_mc_run: NULL argument"; return TMPC_E_INVALID; }
    if (h->regulator) { h->err = "tmpc_mc_run: a regulator handle runs its loop with tmpc_reg_run"; return TMPC_E_INVALID; }
    if (channel)         // (an argument error: reported on a host-only handle too)
        if (const int r2 = channel_fits(h, "tmpc_mc_run", B)) return r2;
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    if (extended && h->nvariants < 2) { h->err = "tmpc_mc_run: extended loop needs a problem created with extended = 1"; return TMPC_E_INVALID; }
    if (h->hK.empty() || h->hKanc.empty()) { h->err = "tmpc_mc_run: the problem description carries no gains K / K_anc"; return TMPC_E_INVALID; }
    if (h->nu > 16) { h->err = "tmpc_mc_run: nu <= 16"; return TMPC_E_UNSUPPORTED; }
    if (full_ref)
        if (const int r2 = reference_table_fits(h, "tmpc_mc_run", B, T)) return r2;
    if (B == 0 || T == 0) return TMPC_OK;
    // full-reference mode: the scalar reference of the legacy mode is not read on the device; the launches get zeros
    const std::vector<double> ref_unused(full_ref ? static_cast<size_t>(T) : 0, 0.0);
    if (full_ref) ref = ref_unused.data();
    int rc = begin_loop(h, B);
    if (rc) return rc;
    const size_t nx = h->nx, nu = h->nu, N = h->N, b = static_cast<size_t>(B), t_ = static_cast<size_t>(T);
    // ONE launch for the whole sweep where the controller has one problem and it runs on the wave kernel: a wave keeps its
    // trajectory for all T steps, solve and state machines alternating inside the kernel (tmpc_fused.hip).  The work item of
    // that launch is a trajectory, T solves long: with B a little above a multiple of the resident waves the last round
    // of trajectories would run on a nearly empty card, so TMPC_MC_FUSED_AUTO fuses when the rounds are at least 85 % full
    // (or there is a single round) and otherwise keeps the launch per time step, whose work item is one solve.
    bool fuse = !rp && !extended && h->mc_fused != TMPC_MC_FUSED_OFF && !use_block(h, h->v[0]);
    if (fuse && h->mc_fused == TMPC_MC_FUSED_AUTO) {
        const int64_t slots = tmpc::resident_waves(h->v[0].shape, h->n_cu);
        const int64_t rounds = slots > 0 ? (B + slots - 1) / slots : 0;
        fuse = rounds == 1 || (rounds > 0 && static_cast<double>(B) >= 0.85 * static_cast<double>(rounds * slots));
    }
    // the extended controller (two problems, two kernel shapes): per time step ONE launch per problem with the state machines of
    // its trajectories inside (closed_loop_step_kernel) -- two launches per step where the plain per-step loop has three
    // (TMPC_MC_FUSED_AUTO: from one round of resident waves on -- below that a step is the latency of its launches, and the state
    // machines inside BOTH of them lengthen it: 200 trajectories at N = 20 0.0345 s with three launches per step, 0.0367 s with two)
    bool step_fuse = !rp && extended && h->mc_fused != TMPC_MC_FUSED_OFF && !use_block(h, h->v[0]) && !use_block(h, h->v[1]);
    if (step_fuse && h->mc_fused == TMPC_MC_FUSED_AUTO) step_fuse = B >= tmpc::resident_waves(h->v[1].shape, h->n_cu);
    // the fused kernels' record {model, state, T, reference}: uploaded once the state is carved; lives until the final synchronise
    tmpc::McFused mf{};
    auto run = [&]() -> int {
        tmpc::McModel m{};
        tmpc::McState st{};
        m.nx = h->nx; m.nu = h->nu; m.N = h->N; m.extended = extended ? 1 : 0; m.rZ = rZ;
        m.plant = h->plant; m.substeps = h->plant_substeps; m.smart = h->actuator == TMPC_ACTUATOR_SMART ? 1 : 0;
        for (int i = 0; i < 7; ++i) m.par[i] = h->plant_par[i];
        Arena &a = h->arena;
        a.piece(&m.A, nx * nx * 8, h->hA.data());
        a.piece(&m.B, nx * nu * 8, h->hB.data());
        a.piece(&m.K, nu * nx * 8, h->hK.data());
        a.piece(&m.K_anc, nu * nx * 8, h->hKanc.data());
        a.piece(&m.HZ, static_cast<size_t>(rZ) * nx * 8, HZ);
        a.piece(&m.hZ, static_cast<size_t>(rZ) * 8, hZ);
        link_pieces(h, a, st, channel, b, p_loss);
        if (host_draws) {
            a.piece(&st.th_u, b * t_ * 8, th_u);
            a.piece(&st.ga_u, b * t_ * 8, ga_u);
            a.piece(&st.w, b * t_ * nx * 8, w);
        } else {
            st.rng_on = 1;
            st.rng_seed = h->mc_rng_seed;
            st.rng_first = h->mc_rng_first;
            a.piece(&st.w_bound, nx * 8, h->mc_w_bound.data());
        }
        // the state starts at x0 (or 0), with last_lost = -1 (0xFF bytes), gamma = 1 and every statistic 0
        for (double **x : {&st.x, &st.x_hat, &st.x_nom}) a.piece(x, b * nx * 8, x0, 0);
        a.piece(&st.Ubuf, b * (N + 1) * nu * 8, nullptr, 0);
        a.piece(&st.u_latest0, b * nu * 8, nullptr, 0);
        for (double **x : {&st.x_nom0_latest, &st.ref_k}) a.piece(x, b * nx * 8, nullptr, 0);
        for (double **x : {&st.err2, &st.consistent}) a.piece(x, b * 8, nullptr, 0);
        for (int32_t **c : {&st.q_est, &st.q_act, &st.s, &st.Theta, &st.last_lost, &st.tube_viol, &st.not_optimal, &st.iters_sum})
            a.piece(c, b * 4, nullptr, c == &st.last_lost ? 0xFF : 0);
        a.piece(&st.gamma, b, nullptr, 1);
        a.piece(&st.dead, b, nullptr, 0);
        st.cap_index = -1;
        if (h->mc_capture >= 0 && h->mc_capture < B) {
            a.piece(&st.cap, t_ * (2 * nx + nu) * 8, nullptr, 0);
            st.cap_index = h->mc_capture;
        }
        if (m.plant != TMPC_PLANT_LINEAR) a.piece(&st.err2_phys, b * 8, nullptr, 0);
        if (h->want_ticks) {
            a.piece(&st.tick_sum, b * 8, nullptr, 0);
            a.piece(&st.tick_max, b * 8, nullptr, 0);
        }
        // warm start: one working-set record per trajectory and variant (row ids are per variant), updated in place by the
        // solve kernel; m = 0 (the zero fill) means "nothing to start from"
        int32_t *ws[2] = {nullptr, nullptr};
        if (h->mc_warm)
            for (int k = 0; k < (extended ? 2 : 1); ++k) a.piece(&ws[k], b * tmpc::WS_STRIDE * 4, nullptr, 0);
        if (full_ref) reference_table_pieces(h, a, st);
        if (rp) {
            // (plain controller: the packets carry no x_nom_0; the state machines then never read it -- zeros)
            a.piece(&st.rp_U, b * t_ * (N + 1) * nu * 8, rp->U);
            a.piece(&st.rp_xn0, b * t_ * nx * 8, rp->xn0, 0);
            a.piece(&st.trace_f, b * t_ * (3 * nx + nu) * 8, nullptr, 0);
            a.piece(&st.trace_i, b * t_ * 3 * 4, nullptr, 0);
        }
        uint8_t *gam[2] = {nullptr, nullptr};           // selector read in a step / arrival flags written in it: swapped every step
        tmpc::McFused *d_mf = nullptr;                  // the record itself lives in the arena: the kernel reads it field by field
        if (fuse || step_fuse) {
            a.piece(&mf.ref_seq, t_ * 8, ref);
            if (step_fuse) a.piece(&gam[1], b, nullptr, 1);
            a.piece(&d_mf, sizeof(mf));
        }
        HIP_TRY(h, a.carve(h->stream));
        link_block_carved(st, b);
        gam[0] = st.gamma;
        if (st.cap) { h->rec.cap = st.cap; h->rec.cap_T = T; }
        if (st.err2_phys) { h->rec.err2_phys = st.err2_phys; h->rec.phys_B = B; }
        if (st.tick_sum) { h->rec.tick_sum = st.tick_sum; h->rec.tick_max = st.tick_max; h->rec.tick_B = B; }
        HIP_TRY(h, tmpc::launch_mc_pre(m, st, B, ref[0], h->stream));
        if (fuse || step_fuse) {
            if (const int r2 = prepare_wave_scratch(h, h->lane[0], B, step_fuse ? 2 : 1)) return r2;
            st.ticks = h->want_ticks ? h->lane[0].ticks.as<long long>() : nullptr;
            mf.m = m; mf.st = st; mf.T = T;
            HIP_TRY(h, hipMemcpyAsync(d_mf, &mf, sizeof(mf), hipMemcpyHostToDevice, h->stream));
        }
        if (step_fuse) {
            // (Measured and dropped: the two launches of a step on two streams, so that the second one's workgroups start on the CUs the
            // first one's tail leaves idle -- config 4 extended 0.27 -> 0.28 s: the fork / join events of every step cost more.)
            for (int t = 0; t < T; ++t) {
                if (const int r2 = begin_timed_launch(h, h->lane[0])) return r2;
                for (int k = 0; k < 2; ++k)
                    HIP_TRY(h, tmpc::launch_solve_mc_step(h->v[k].d, h->v[k].shape, k, B, gam[t & 1], h->d_u, h->d_x0, h->d_ss, h->d_st, h->d_it, ws[k],
                                                          d_mf, t, gam[(t + 1) & 1], &h->lane[0].wc, h->n_cu, h->stream));
                HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
            }
            h->timed = true;
            h->rec.fused = 2;
        } else if (fuse) {
            if (const int r2 = begin_timed_launch(h, h->lane[0])) return r2;          // (the launch counts in tmpc_kernel_ms_total like any solve launch)
            HIP_TRY(h, tmpc::launch_solve_mc(h->v[0].d, h->v[0].shape, B, h->d_u, h->d_x0, h->d_ss, h->d_st, h->d_it, ws[0], d_mf, &h->lane[0].wc, h->n_cu,
                                             h->stream));
            HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
            h->timed = true;
            h->rec.fused = 1;
        } else {
            // per time step: the solve launch(es) -- one per problem variant in use -- and ONE launch of the state machines
            // (round 3: mc_pre, the variant check, the solve, mc_post, mc_tube).  With injected packets nothing is solved.
            for (int t = 0; t < T; ++t) {
                if (!rp) {
                    const int r2 = enqueue(h, h->lane[0], {B, st.x_hat, st.ref_k, extended ? st.gamma : nullptr, h->d_u, h->d_x0, h->d_ss, nullptr, h->d_st, h->d_it},
                                           ws, true);
                    if (r2) return r2;
                    st.ticks = h->want_ticks ? h->lane[0].ticks.as<long long>() : nullptr;       // (allocated by the first enqueue)
                }
                HIP_TRY(h, tmpc::launch_mc_step(m, st, t, T, B, ref[t], ref[t + 1 < T ? t + 1 : t], h->d_u, h->d_x0, h->d_ss, h->d_st, h->d_it,
                                                h->stream));
            }
        }
        if (rp) {
            HIP_TRY(h, hipMemcpyAsync(rp->trace_f, st.trace_f, b * t_ * (3 * nx + nu) * 8, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(rp->trace_i, st.trace_i, b * t_ * 3 * 4, hipMemcpyDeviceToHost, h->stream));
        }
        if (err2) HIP_TRY(h, hipMemcpyAsync(err2, st.err2, b * 8, hipMemcpyDeviceToHost, h->stream));
        if (tube_viol) HIP_TRY(h, hipMemcpyAsync(tube_viol, st.tube_viol, b * 4, hipMemcpyDeviceToHost, h->stream));
        if (not_optimal) HIP_TRY(h, hipMemcpyAsync(not_optimal, st.not_optimal, b * 4, hipMemcpyDeviceToHost, h->stream));
        if (x_final) HIP_TRY(h, hipMemcpyAsync(x_final, st.x, b * nx * 8, hipMemcpyDeviceToHost, h->stream));
        if (consistent) HIP_TRY(h, hipMemcpyAsync(consistent, st.consistent, b * 8, hipMemcpyDeviceToHost, h->stream));
        if (iters_sum) HIP_TRY(h, hipMemcpyAsync(iters_sum, st.iters_sum, b * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, fetch_link_stats(h, st, b));
        HIP_TRY(h, sync_lanes(h));
        h->rec.link_B = B;
        return TMPC_OK;
    };
    rc = run();
    if (rc != TMPC_OK) (void)sync_lanes(h);
    return rc;
}
}  // namespace

extern "C" {

int tmpc_mc_run(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *p_loss, const double *ref,
                const double *th_u, const double *ga_u, const double *w, const double *x0, const double *HZ, const double *hZ,
                int32_t rZ, double *err2, int32_t *tube_viol, int32_t *not_optimal, double *x_final, double *consistent,
                int32_t *iters_sum) {
    return mc_run_impl(h, B, T, extended, p_loss, ref, th_u, ga_u, w, x0, HZ, hZ, rZ, err2, tube_viol, not_optimal, x_final, consistent,
                       iters_sum, nullptr);
}

int tmpc_mc_replay(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *U_pkt, const double *xn0_pkt,
                   const uint8_t *theta, const uint8_t *gamma, const double *w, const double *x0, double *trace_f, int32_t *trace_i) {
    if (!h) return TMPC_E_INVALID;
    if (B < 0 || T < 0 || !U_pkt || !theta || !gamma || !w || !trace_f || !trace_i || (extended && !xn0_pkt)) { h->err = "tmpc_mc_replay: NULL argument"; return TMPC_E_INVALID; }
    // arrival flags as uniforms against a loss rate of one half: lost iff t > 0 and uniform < 1/2 (the draw rule of tmpc_mc_run)
    const size_t n = static_cast<size_t>(B) * static_cast<size_t>(T);
    std::vector<double> th(n), ga(n), pl(static_cast<size_t>(B), 0.5), ref(static_cast<size_t>(T), 0.0);
    for (size_t i = 0; i < n; ++i) { th[i] = theta[i] ? 1.0 : 0.0; ga[i] = gamma[i] ? 1.0 : 0.0; }
    McReplay rp{U_pkt, xn0_pkt, trace_f, trace_i};
    return mc_run_impl(h, B, T, extended, pl.data(), ref.data(), th.data(), ga.data(), w, x0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, &rp);
}

int tmpc_reg_run(tmpc_handle *h, int64_t B, int32_t T, const double *x0, const double *w,
                 const double *HX, const double *hX, int32_t rX, const double *HU, const double *hU, int32_t rU,
                 const double *HZ, const double *hZ, int32_t rZ,
                 double *cost, int32_t *x_viol, int32_t *u_viol, int32_t *tube_viol, int32_t *not_optimal, int32_t *fail_step,
                 double *x_final, int32_t *iters_sum, int64_t capture, double *cap_x, double *cap_xn, double *cap_u) {
    if (!h) return TMPC_E_INVALID;
    if (h->ses.open) { h->err = "tmpc_reg_run: a stepped closed loop is open on this handle (tmpc_mc_close first)"; return TMPC_E_INVALID; }
    if (!h->regulator) { h->err = "tmpc_reg_run: needs a regulator handle (tmpc_create_regulator); tracking handles run tmpc_mc_run"; return TMPC_E_INVALID; }
    if (B < 0 || T < 0 || !x0 || rX < 0 || rU < 0 || rZ < 0 || (rX > 0 && (!HX || !hX)) || (rU > 0 && (!HU || !hU)) || (rZ > 0 && (!HZ || !hZ))) {
        h->err = "tmpc_reg_run: NULL argument or negative count";
        return TMPC_E_INVALID;
    }
    if (h->reg_tube && h->hK.empty()) { h->err = "tmpc_reg_run: the tube regulator needs its gain K"; return TMPC_E_INVALID; }
    if (const int r2 = plant_models_fit(h, "tmpc_reg_run", B)) return r2;
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    if (h->nu > 16) { h->err = "tmpc_reg_run: nu <= 16"; return TMPC_E_UNSUPPORTED; }
    if (B == 0 || T == 0) return TMPC_OK;
    int rc = begin_loop(h, B);
    if (rc) return rc;
    if ((rc = ensure_reg_zero(h, B))) return rc;
    const size_t nx = h->nx, nu = h->nu, b = static_cast<size_t>(B), t_ = static_cast<size_t>(T);
    const bool host_w = w != nullptr, want_cap = capture >= 0 && capture < B && cap_x && cap_xn && cap_u;
    auto run = [&]() -> int {
        tmpc::RegModel m{};
        tmpc::RegState st{};
        m.nx = h->nx; m.nu = h->nu; m.N = h->N; m.tube = h->reg_tube;
        m.rX = rX; m.rU = rU; m.rZ = rZ;
        Arena &a = h->arena;
        a.piece(&m.A, 8 * nx * nx, h->hA.data());
        a.piece(&m.B, 8 * nx * nu, h->hB.data());
        a.piece(&m.Q, 8 * nx * nx, h->hQ.data());
        a.piece(&m.R, 8 * nu * nu, h->hR.data());
        a.piece(&m.K, 8 * h->hK.size(), h->hK.data());
        a.piece(&m.HX, 8 * static_cast<size_t>(rX) * nx, HX);
        a.piece(&m.hX, 8 * static_cast<size_t>(rX), hX);
        a.piece(&m.HU, 8 * static_cast<size_t>(rU) * nu, HU);
        a.piece(&m.hU, 8 * static_cast<size_t>(rU), hU);
        a.piece(&m.HZ, 8 * static_cast<size_t>(rZ) * nx, HZ);
        a.piece(&m.hZ, 8 * static_cast<size_t>(rZ), hZ);
        a.piece(&st.x, 8 * b * nx, x0);
        a.piece(&st.cost, 8 * b, nullptr, 0);
        if (h->mc_pm_B > 0) a.piece(&st.plant_lin, 8 * h->mc_pm.size(), h->mc_pm.data());      // (a regulator handle's models are linear)
        int32_t **counters[] = {&st.x_viol, &st.u_viol, &st.tube_viol, &st.not_optimal, &st.fail_step, &st.iters_sum};
        for (int32_t **c : counters) a.piece(c, 4 * b, nullptr, c == &st.fail_step ? 0xFF : 0);      // (0xFF bytes: fail_step = -1)
        if (host_w) {
            a.piece(&st.w, 8 * b * t_ * nx, w);
        } else if (h->mc_rng_on) {
            st.rng_on = 1;
            st.rng_seed = h->mc_rng_seed;
            st.rng_first = h->mc_rng_first;
            a.piece(&st.w_bound, 8 * nx, h->mc_w_bound.data());
        }
        st.cap_index = -1;
        if (want_cap) {
            a.piece(&st.cap_x, 8 * (t_ + 1) * nx);
            a.piece(&st.cap_xn, 8 * t_ * nx);
            a.piece(&st.cap_u, 8 * t_ * nu);
            st.cap_index = capture;
        }
        HIP_TRY(h, a.carve(h->stream));
        if (want_cap) HIP_TRY(h, hipMemcpyAsync(st.cap_x, x0 + static_cast<size_t>(capture) * nx, 8 * nx, hipMemcpyHostToDevice, h->stream));
        // per step: the solve launch over all trajectories (x_k = the state, in place), then the step kernel
        for (int t = 0; t < T; ++t) {
            if (const int r2 = enqueue(h, h->lane[0], {B, st.x, h->reg_zero.as<double>(), nullptr, h->d_u, h->d_x0, nullptr, nullptr, h->d_st, h->d_it})) return r2;
            HIP_TRY(h, tmpc::launch_reg_step(m, st, t, T, B, h->d_u, h->d_x0, h->d_st, h->d_it, h->stream));
        }
        if (cost) HIP_TRY(h, hipMemcpyAsync(cost, st.cost, 8 * b, hipMemcpyDeviceToHost, h->stream));
        int32_t *outs[] = {x_viol, u_viol, tube_viol, not_optimal, fail_step, iters_sum};
        for (int k = 0; k < 6; ++k)
            if (outs[k]) HIP_TRY(h, hipMemcpyAsync(outs[k], *counters[k], 4 * b, hipMemcpyDeviceToHost, h->stream));
        if (x_final) HIP_TRY(h, hipMemcpyAsync(x_final, st.x, 8 * b * nx, hipMemcpyDeviceToHost, h->stream));
        if (want_cap) {
            HIP_TRY(h, hipMemcpyAsync(cap_x, st.cap_x, 8 * (t_ + 1) * nx, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(cap_xn, st.cap_xn, 8 * t_ * nx, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(cap_u, st.cap_u, 8 * t_ * nu, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(h, sync_lanes(h));
        return TMPC_OK;
    };
    rc = run();
    if (rc != TMPC_OK) (void)sync_lanes(h);
    return rc;
}

int tmpc_mc_open(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *p_loss, const double *ref, const double *th_u,
                 const double *ga_u, const double *x0, const double *HZ, const double *hZ, int32_t rZ, const double *HX,
                 const double *hX, int32_t rX, const double *HU, const double *hU, int32_t rU) {
    if (!h) return TMPC_E_INVALID;
    if (h->ses.open) { h->err = "tmpc_mc_open: a stepped closed loop is already open on this handle (one session per handle)"; return TMPC_E_INVALID; }
    if (h->regulator) { h->err = "tmpc_mc_open: a regulator handle has no stepped loop"; return TMPC_E_INVALID; }
    const bool host_draws = !h->mc_rng_on;
    if (B <= 0 || T <= 0 || rZ < 0 || rX < 0 || rU < 0) { h->err = "tmpc_mc_open: need B > 0, T > 0 and row counts >= 0"; return TMPC_E_INVALID; }
    const bool full_ref = h->mc_ref_K > 0;
    const bool channel = h->mc_ch_B > 0;
    if ((!p_loss && !channel) || (!ref && !full_ref) || (host_draws && (!th_u || !ga_u)) || (rZ > 0 && (!HZ || !hZ)) || (rX > 0 && (!HX || !hX)) || (rU > 0 && (!HU || !hU))) {
        h->err = "tmpc_mc_open: NULL argument";
        return TMPC_E_INVALID;
    }
    if (channel)
        if (const int r2 = channel_fits(h, "tmpc_mc_open", B)) return r2;
    if (extended && h->nvariants < 2) { h->err = "tmpc_mc_open: extended loop needs a problem created with extended = 1"; return TMPC_E_INVALID; }
    if (h->hK.empty() || h->hKanc.empty()) { h->err = "tmpc_mc_open: the problem description carries no gains K / K_anc"; return TMPC_E_INVALID; }
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    if (h->nu > 16) { h->err = "tmpc_mc_open: nu <= 16"; return TMPC_E_UNSUPPORTED; }
    if (full_ref)
        if (const int r2 = reference_table_fits(h, "tmpc_mc_open", B, T)) return r2;
    int rc = begin_loop(h, B);
    if (rc) return rc;
    const size_t nx = h->nx, nu = h->nu, N = h->N, b = static_cast<size_t>(B), t_ = static_cast<size_t>(T);
    McSession &s = h->ses;
    auto open = [&]() -> int {
        tmpc::McModel &m = s.m;
        tmpc::McState &st = s.st;
        tmpc::McExternal &ext = s.ext;
        m.nx = h->nx; m.nu = h->nu; m.N = h->N; m.extended = extended ? 1 : 0; m.rZ = rZ;
        m.plant = TMPC_PLANT_EXTERNAL; m.substeps = 1; m.smart = h->actuator == TMPC_ACTUATOR_SMART ? 1 : 0;
        ext.rX = rX; ext.rU = rU;
        // the pieces of mc_run_impl without a plant state's disturbance, plus the caller's sets, counters and the staging of tmpc_mc_step
        Arena &a = h->arena;
        a.piece(&m.A, nx * nx * 8, h->hA.data());
        a.piece(&m.B, nx * nu * 8, h->hB.data());
        a.piece(&m.K, nu * nx * 8, h->hK.data());
        a.piece(&m.K_anc, nu * nx * 8, h->hKanc.data());
        a.piece(&m.HZ, static_cast<size_t>(rZ) * nx * 8, HZ);
        a.piece(&m.hZ, static_cast<size_t>(rZ) * 8, hZ);
        a.piece(&ext.HX, static_cast<size_t>(rX) * nx * 8, HX);
        a.piece(&ext.hX, static_cast<size_t>(rX) * 8, hX);
        a.piece(&ext.HU, static_cast<size_t>(rU) * nu * 8, HU);
        a.piece(&ext.hU, static_cast<size_t>(rU) * 8, hU);
        link_pieces(h, a, st, channel, b, p_loss);
        if (host_draws) {
            a.piece(&st.th_u, b * t_ * 8, th_u);
            a.piece(&st.ga_u, b * t_ * 8, ga_u);
        } else {
            st.rng_on = 1;
            st.rng_seed = h->mc_rng_seed;
            st.rng_first = h->mc_rng_first;
        }
        // (st.x is carried for the record's sake: the state machines of a session never read or write it)
        for (double **x : {&st.x, &st.x_hat, &st.x_nom}) a.piece(x, b * nx * 8, x0, 0);
        a.piece(&st.Ubuf, b * (N + 1) * nu * 8, nullptr, 0);
        a.piece(&st.u_latest0, b * nu * 8, nullptr, 0);
        for (double **x : {&st.x_nom0_latest, &st.ref_k}) a.piece(x, b * nx * 8, nullptr, 0);
        for (double **x : {&st.err2, &st.consistent}) a.piece(x, b * 8, nullptr, 0);
        for (int32_t **c : {&st.q_est, &st.q_act, &st.s, &st.Theta, &st.last_lost, &st.tube_viol, &st.not_optimal, &st.iters_sum, &ext.x_viol, &ext.u_viol})
            a.piece(c, b * 4, nullptr, c == &st.last_lost ? 0xFF : 0);
        a.piece(&st.gamma, b, nullptr, 1);
        a.piece(&st.dead, b, nullptr, 0);
        st.cap_index = -1;
        if (h->mc_capture >= 0 && h->mc_capture < B) {
            a.piece(&st.cap, t_ * (2 * nx + nu) * 8, nullptr, 0);
            st.cap_index = h->mc_capture;
        }
        if (h->want_ticks) {
            a.piece(&st.tick_sum, b * 8, nullptr, 0);
            a.piece(&st.tick_max, b * 8, nullptr, 0);
        }
        s.warm = h->mc_warm != 0;
        if (s.warm)
            for (int k = 0; k < (extended ? 2 : 1); ++k) a.piece(&s.ws[k], b * tmpc::WS_STRIDE * 4, nullptr, 0);
        double *x_stage = nullptr, *u_stage = nullptr;
        a.piece(&x_stage, b * nx * 8, nullptr, 0);
        a.piece(&u_stage, b * nu * 8, nullptr, 0);
        if (full_ref) {
            reference_table_pieces(h, a, st);
            a.piece(&s.ref_stage, b * nx * 8, nullptr, 0);
        }
        HIP_TRY(h, a.carve(h->stream));
        link_block_carved(st, b);
        ext.x_t = x_stage;
        ext.u_t = u_stage;
        HIP_TRY(h, tmpc::launch_mc_pre(m, st, B, full_ref ? 0.0 : ref[0], h->stream));
        HIP_TRY(h, hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
        // (the pinned block is a convenience: without it tmpc_mc_step copies from / to the caller's memory)
        if (hipHostMalloc(reinterpret_cast<void **>(&s.pin), b * (nx + nu + (full_ref ? nx : 0)) * 8, hipHostMallocDefault) != hipSuccess) {
            s.pin = nullptr;
            (void)hipGetLastError();
        }
        HIP_TRY(h, sync_lanes(h));       // the uploads read the caller's arrays, which are theirs again from here on
        return TMPC_OK;
    };
    rc = open();
    if (rc != TMPC_OK) {
        (void)sync_lanes(h);
        release_session(h);
        return rc;
    }
    if (full_ref) s.ref.assign(t_, 0.0);       // (not read on the device in full-reference mode)
    else s.ref.assign(ref, ref + T);
    s.full_ref = full_ref;
    s.B = B; s.T = T; s.t = 0; s.extended = extended ? 1 : 0;
    s.open = true;
    return TMPC_OK;
}

namespace {
// One step of the open session on the handle's stream: the solve launch(es) on x_hat_t, then -- behind `caller` (a stream, or
// nullptr) -- the state machines around the given x_t / u_t.
// ref_next (device, or nullptr: the schedule's row) is read by the same launch as x_t.
int session_step(tmpc_handle *h, const char *who, const double *x_t, double *u_t, hipStream_t caller, const double *ref_next = nullptr) {
    McSession &s = h->ses;
    if (!s.open) { h->err = std::string(who) + ": no stepped closed loop is open on this handle (tmpc_mc_open)"; return TMPC_E_INVALID; }
    if (s.failed) { h->err = std::string(who) + ": an earlier step of the session failed on the device; only tmpc_mc_close is left"; return TMPC_E_INVALID; }
    if (!x_t || !u_t) { h->err = std::string(who) + ": NULL argument"; return TMPC_E_INVALID; }
    if (s.t >= s.T) { h->err = std::string(who) + ": the session was opened for T steps and has taken them"; return TMPC_E_INVALID; }
    auto step = [&]() -> int {
        HIP_TRY(h, hipSetDevice(h->device));
        tmpc::McState &st = s.st;
        if (const int rc = enqueue(h, h->lane[0], {s.B, st.x_hat, st.ref_k, s.extended ? st.gamma : nullptr, h->d_u, h->d_x0, h->d_ss, nullptr, h->d_st, h->d_it},
                                   s.warm ? s.ws : nullptr, true))
            return rc;
        st.ticks = st.tick_sum ? h->lane[0].ticks.as<long long>() : nullptr;       // (timed at open; allocated by the first enqueue)
        // the solve did not need x_t; the state machines do
        if (caller) {
            HIP_TRY(h, hipEventRecord(s.ev_in, caller));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, s.ev_in, 0));
        }
        tmpc::McExternal ext = s.ext;
        ext.x_t = x_t;
        ext.u_t = u_t;
        ext.ref_next = ref_next;
        const int t = s.t;
        HIP_TRY(h, tmpc::launch_mc_step_external(s.m, st, ext, t, s.T, s.B, s.ref[t], s.ref[t + 1 < s.T ? t + 1 : t], h->d_u, h->d_x0, h->d_ss,
                                                 h->d_st, h->d_it, h->stream));
        if (caller) {
            HIP_TRY(h, hipEventRecord(s.ev_out, h->stream));
            HIP_TRY(h, hipStreamWaitEvent(caller, s.ev_out, 0));
        }
        return TMPC_OK;
    };
    const int rc = step();
    if (rc != TMPC_OK) s.failed = true;
    else ++s.t;
    return rc;
}
}  // namespace

int tmpc_mc_step_device(tmpc_handle *h, const double *x_t, double *u_t, void *caller_stream) {
    if (!h) return TMPC_E_INVALID;
    return session_step(h, "tmpc_mc_step_device", x_t, u_t, static_cast<hipStream_t>(caller_stream));
}

namespace {
// the _ref steps need a session opened in full-reference mode; refusing one leaves the session as it is
bool ref_step_barred(tmpc_handle *h, const char *who) {
    if (!h->ses.open || h->ses.full_ref) return false;      // (no session: session_step's message)
    h->err = std::string(who) + ": the session was opened without a reference table (tmpc_mc_set_reference_table before tmpc_mc_open)";
    return true;
}
int host_step(tmpc_handle *h, const char *who, const double *x_t, double *u_t, const double *ref_next);
}  // namespace

int tmpc_mc_step_device_ref(tmpc_handle *h, const double *x_t, double *u_t, const double *ref_next, void *caller_stream) {
    if (!h) return TMPC_E_INVALID;
    if (ref_step_barred(h, "tmpc_mc_step_device_ref")) return TMPC_E_INVALID;
    return session_step(h, "tmpc_mc_step_device_ref", x_t, u_t, static_cast<hipStream_t>(caller_stream), ref_next);
}

int tmpc_mc_step(tmpc_handle *h, const double *x_t, double *u_t) {
    if (!h) return TMPC_E_INVALID;
    return host_step(h, "tmpc_mc_step", x_t, u_t, nullptr);
}

int tmpc_mc_step_ref(tmpc_handle *h, const double *x_t, double *u_t, const double *ref_next) {
    if (!h) return TMPC_E_INVALID;
    if (ref_step_barred(h, "tmpc_mc_step_ref")) return TMPC_E_INVALID;
    return host_step(h, "tmpc_mc_step_ref", x_t, u_t, ref_next);
}

namespace {
// tmpc_mc_step[_ref]: HOST pointers, one DMA each way through the session's pinned block
int host_step(tmpc_handle *h, const char *who, const double *x_t, double *u_t, const double *ref_next) {
    McSession &s = h->ses;
    if (!s.open || s.failed || !x_t || !u_t || s.t >= s.T) return session_step(h, who, x_t, u_t, nullptr);     // (its message and code)
    const size_t xb = static_cast<size_t>(s.B) * h->nx * 8, ub = static_cast<size_t>(s.B) * h->nu * 8;
    double *const d_x = const_cast<double *>(s.ext.x_t), *const d_u = s.ext.u_t;
    auto copies = [&](bool in) -> int {
        HIP_TRY(h, hipSetDevice(h->device));
        if (in) {
            if (s.pin) std::memcpy(s.pin, x_t, xb);
            HIP_TRY(h, hipMemcpyAsync(d_x, s.pin ? static_cast<const void *>(s.pin) : x_t, xb, hipMemcpyHostToDevice, h->stream));
            if (ref_next) {
                if (s.pin) std::memcpy(s.pin + xb + ub, ref_next, xb);
                HIP_TRY(h, hipMemcpyAsync(s.ref_stage, s.pin ? static_cast<const void *>(s.pin + xb + ub) : ref_next, xb, hipMemcpyHostToDevice, h->stream));
            }
        } else {
            HIP_TRY(h, hipMemcpyAsync(s.pin ? static_cast<void *>(s.pin + xb) : u_t, d_u, ub, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, sync_lanes(h));
            if (s.pin) std::memcpy(u_t, s.pin + xb, ub);
        }
        return TMPC_OK;
    };
    int rc = copies(true);
    if (rc == TMPC_OK) rc = session_step(h, who, d_x, d_u, nullptr, ref_next ? s.ref_stage : nullptr);
    if (rc == TMPC_OK) rc = copies(false);
    if (rc != TMPC_OK) { s.failed = true; (void)sync_lanes(h); }
    return rc;
}
}  // namespace

int tmpc_mc_close(tmpc_handle *h, double *err2, int32_t *tube_viol, int32_t *x_viol, int32_t *u_viol, int32_t *not_optimal,
                  double *consistent, int32_t *iters_sum, int32_t *steps_done) {
    if (!h) return TMPC_E_INVALID;
    McSession &s = h->ses;
    if (!s.open) { h->err = "tmpc_mc_close: no stepped closed loop is open on this handle (tmpc_mc_open)"; return TMPC_E_INVALID; }
    const size_t b = static_cast<size_t>(s.B);
    auto close = [&]() -> int {
        HIP_TRY(h, hipSetDevice(h->device));
        const tmpc::McState &st = s.st;
        if (err2) HIP_TRY(h, hipMemcpyAsync(err2, st.err2, b * 8, hipMemcpyDeviceToHost, h->stream));
        if (consistent) HIP_TRY(h, hipMemcpyAsync(consistent, st.consistent, b * 8, hipMemcpyDeviceToHost, h->stream));
        const struct { int32_t *host; const int32_t *dev; } counters[] = {
            {tube_viol, st.tube_viol}, {x_viol, s.ext.x_viol}, {u_viol, s.ext.u_viol}, {not_optimal, st.not_optimal}, {iters_sum, st.iters_sum}};
        for (const auto &c : counters)
            if (c.host) HIP_TRY(h, hipMemcpyAsync(c.host, c.dev, b * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, fetch_link_stats(h, st, b));
        HIP_TRY(h, sync_lanes(h));
        return TMPC_OK;
    };
    const int rc = close();
    if (rc != TMPC_OK) (void)sync_lanes(h);
    if (steps_done) *steps_done = s.t;
    // what the getters read, as after a run (the arena stays as it is until the next loop)
    if (rc == TMPC_OK && s.st.cap) { h->rec.cap = s.st.cap; h->rec.cap_T = s.T; }
    if (rc == TMPC_OK && s.st.tick_sum) { h->rec.tick_sum = s.st.tick_sum; h->rec.tick_max = s.st.tick_max; h->rec.tick_B = s.B; }
    if (rc == TMPC_OK) h->rec.link_B = s.B;
    release_session(h);
    return rc;
}

int tmpc_synchronize(tmpc_handle *h) {
    if (!h) return TMPC_E_INVALID;
    if (h->device < 0) return TMPC_OK;
    HIP_TRY(h, sync_lanes(h));
    return TMPC_OK;
}

int tmpc_set_call_overlap(tmpc_handle *h, int on) {
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, "tmpc_set_call_overlap")) return TMPC_E_INVALID;
    if (h->device >= 0 && (on != 0) != (h->overlap != 0)) {
        // off: the primary lane, which takes every call from here on, goes behind what the secondary lane holds; on: no call enqueued
        // while it was off has a record, so the lanes start empty
        HIP_TRY(h, hipSetDevice(h->device));
        if (on) HIP_TRY(h, sync_lanes(h));
        else if (const int rc = join_lanes(h)) return rc;
    }
    h->overlap = on ? 1 : 0;
    return TMPC_OK;
}

int tmpc_debug_lane_counters(tmpc_handle *h, int64_t *calls_per_lane, int64_t *cross_lane_waits, int reset) {
    if (!h) return TMPC_E_INVALID;
    if (calls_per_lane)
        for (int k = 0; k < 2; ++k) calls_per_lane[k] = h->lane[k].calls;
    if (cross_lane_waits) *cross_lane_waits = h->lane_waits;
    if (reset) { h->lane[0].calls = h->lane[1].calls = 0; h->lane_waits = 0; }
    return TMPC_OK;
}

int tmpc_debug_calls_conflict(int32_t nx, int32_t nu, int32_t N, int64_t B_a, const void *const *a, int64_t B_b, const void *const *b) {
    if (!a || !b || nx <= 0 || nu <= 0 || N <= 0) return TMPC_E_INVALID;
    const tmpc::CallRanges ra = tmpc::solve_call_ranges(B_a, nx, nu, N, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
    const tmpc::CallRanges rb = tmpc::solve_call_ranges(B_b, nx, nu, N, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8]);
    return tmpc::calls_conflict(ra, rb) ? 1 : 0;
}

int tmpc_last_kernel_ms(tmpc_handle *h, float *ms) {
    if (!h || !ms) return TMPC_E_INVALID;
    if (!h->timed) { h->err = "tmpc_last_kernel_ms: no solve has been enqueued yet"; return TMPC_E_INVALID; }
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return TMPC_OK;
}

int tmpc_kernel_ms_total(tmpc_handle *h, float *total_ms, int32_t *launches, int reset) {
    if (!h) return TMPC_E_INVALID;
    if (h->device < 0) { h->err = "host-only handle"; return TMPC_E_DEVICE; }
    HIP_TRY(h, sync_lanes(h));
    // A call adds the time by which it extended the handle's busy period: from the later of its own start and the end of the
    // busy period so far (`busy`: the call that ended last) to its own end.  Calls of one lane follow each other, so only a
    // call on the other lane than `busy` can have started before that end.
    float sum = 0.f;
    size_t busy = 0;
    for (size_t i = 0; i < h->pool_used; ++i) {
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->pool[i].first, h->pool[i].second));
        if (i > 0 && h->pool_lane[i] != h->pool_lane[busy]) {
            float past = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&past, h->pool[busy].second, h->pool[i].second));
            if (past <= 0.f) continue;          // ended inside the busy period: extends nothing
            ms = std::min(ms, past);
        }
        busy = i;
        sum += ms;
    }
    if (total_ms) *total_ms = sum;
    if (launches) *launches = static_cast<int32_t>(h->pool_used);
    if (reset) h->pool_used = 0;
    return TMPC_OK;
}

#ifdef TMPC_STAMPS
int tmpc_debug_stamps(tmpc_handle *h, int variant, long long *out12 /* [16] */) {
    if (!h || !out12) return TMPC_E_INVALID;
    HIP_TRY(h, sync_lanes(h));
    const long long *src = use_block(h, h->v[variant]) ? h->v[variant].db.dbg : h->v[variant].d.dbg;
    HIP_TRY(h, hipMemcpy(out12, src, 16 * sizeof(long long), hipMemcpyDeviceToHost));
    return TMPC_OK;
}
#endif

int tmpc_get_dims(const tmpc_handle *h, int variant, int32_t *nv, int32_t *nc, int32_t *npar) {
    if (!h || variant < 0 || variant >= h->nvariants) return TMPC_E_INVALID;
    const tmpc::Condensed &c = h->v[variant].c;
    if (nv) *nv = c.nv;
    if (nc) *nc = c.nc;
    if (npar) *npar = c.npar;
    return TMPC_OK;
}

int tmpc_get_factoring(const tmpc_handle *h, int variant, int32_t *nd, int32_t *ncc, int32_t *kc) {
    if (!h || variant < 0 || variant >= h->nvariants) return TMPC_E_INVALID;
    const tmpc::Condensed &c = h->v[variant].c;
    if (nd) *nd = c.nd;
    if (ncc) *ncc = c.ncc;
    if (kc) *kc = c.kc;
    return TMPC_OK;
}

int tmpc_get_condensed(const tmpc_handle *h, int variant, double *H, double *F1, double *F2, double *G, double *g0, double *E) {
    if (!h || variant < 0 || variant >= h->nvariants) return TMPC_E_INVALID;
    const tmpc::Condensed &c = h->v[variant].c;
    if (H) std::memcpy(H, c.H.a.data(), c.H.a.size() * sizeof(double));
    if (F1) std::memcpy(F1, c.F1.a.data(), c.F1.a.size() * sizeof(double));
    if (F2) std::memcpy(F2, c.F2.a.data(), c.F2.a.size() * sizeof(double));
    if (G) std::memcpy(G, c.G.a.data(), c.G.a.size() * sizeof(double));
    if (g0) std::memcpy(g0, c.g0.data(), c.g0.size() * sizeof(double));
    if (E) std::memcpy(E, c.E.a.data(), c.E.a.size() * sizeof(double));
    return TMPC_OK;
}

// ---- offline stage: batched support-function LPs (tmpc_lp.hip)

#define LP_TRY(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            g_create_error = std::string("tmpc_lp_batch: " #expr ": ") + hipGetErrorString(e_); \
            return TMPC_E_DEVICE;                                                          \
        }                                                                                  \
    } while (0)

namespace {
// the polytope in kernel units: rows to unit norm, h to max |h| = 1 (one scalar: x scales with it, the directions do not)
struct LpHost {
    int DP = 0, nrp = 0;
    double hm = 1.0;
    bool empty_set = false, no_normal = false;
    std::vector<double> Ht, hs, rs;
};

int lp_prepare(int32_t d, int32_t nr, const double *H, const double *hv, LpHost &o) {
    o.DP = tmpc::lp_padded_dim(d);
    if (d < 1 || o.DP < 0 || nr < 1) {
        g_create_error = "tmpc_lp_batch: need 1 <= d <= 32 and nr >= 1";
        return d > 32 ? TMPC_E_UNSUPPORTED : TMPC_E_INVALID;
    }
    const int nrp = o.nrp = (nr + 63) / 64 * 64;
    o.Ht.assign(static_cast<size_t>(o.DP) * nrp, 0.0);
    o.hs.assign(nrp, 1.0);
    o.rs.assign(nrp, 0.0);
    double hm = 0.0, nmax = 0.0;
    std::vector<double> nrm(nr, 0.0);
    for (int r = 0; r < nr; ++r) {
        double n2 = 0.0;
        for (int j = 0; j < d; ++j) {
            const double v = H[static_cast<size_t>(r) * d + j];
            if (!(v == v) || std::isinf(v)) { g_create_error = "tmpc_lp_batch: H is not finite"; return TMPC_E_INVALID; }
            n2 += v * v;
        }
        if (!(hv[r] == hv[r]) || std::isinf(hv[r])) { g_create_error = "tmpc_lp_batch: h is not finite"; return TMPC_E_INVALID; }
        nrm[r] = std::sqrt(n2);
        nmax = std::max(nmax, nrm[r]);
    }
    // A row whose normal vanishes against the others (round-off left by a product of matrices) says 0 <= h_r: it
    // constrains nothing, or everything.  Scaling it to unit norm would turn the round-off into a constraint.
    for (int r = 0; r < nr; ++r) {
        if (nrm[r] <= 1e-12 * nmax) {
            if (hv[r] < -1e-9 * (1.0 + std::fabs(hv[r]))) o.empty_set = true;
            continue;                                    // stays as the padding row 0 . x <= 1
        }
        o.rs[r] = 1.0 / nrm[r];
        for (int j = 0; j < d; ++j) o.Ht[static_cast<size_t>(j) * nrp + r] = H[static_cast<size_t>(r) * d + j] / nrm[r];
        o.hs[r] = hv[r] / nrm[r];
        hm = std::max(hm, std::fabs(o.hs[r]));
    }
    o.no_normal = !(nmax > 0.0);
    if (!(hm > 0.0)) hm = 1.0;
    o.hm = hm;
    for (int r = 0; r < nr; ++r) {
        if (o.rs[r] == 0.0) continue;                    // vanishing normal: keeps h = 1 in kernel units
        o.hs[r] /= hm; o.rs[r] /= hm;
    }
    return TMPC_OK;
}

// device memory of tmpc_lp_batch: one arena per host thread (the Gilbert-Tan recursion makes hundreds of small calls; ten
// hipMalloc / hipFree pairs each cost more than the kernel), reallocated when the thread's device changes.  Lives until the
// process ends.
thread_local Arena g_lp_arena;
thread_local int g_lp_device = -1;

constexpr int LP_MAX_ITER = 80;
constexpr double LP_TOL = 1e-8;
}  // namespace

int tmpc_lp_batch(int device, int32_t d, int32_t nr, const double *H, const double *hv, int64_t B, const double *C,
                  const int32_t *relax, double relax_by, double *val, double *x, int32_t *status, int32_t *iters) {
    if (!H || !hv || (B > 0 && (!C || !val || !status || !iters)) || B < 0) {
        g_create_error = "tmpc_lp_batch: NULL argument";
        return TMPC_E_INVALID;
    }
    if (d < 1 || tmpc::lp_padded_dim(d) < 0 || nr < 1) {
        g_create_error = "tmpc_lp_batch: need 1 <= d <= 32 and nr >= 1";
        return d > 32 ? TMPC_E_UNSUPPORTED : TMPC_E_INVALID;
    }
    if (relax)
        for (int64_t b = 0; b < B; ++b)
            if (relax[b] < -1 || relax[b] >= nr) { g_create_error = "tmpc_lp_batch: relax index out of range"; return TMPC_E_INVALID; }
    if (B == 0) return TMPC_OK;
    LpHost lh;
    if (const int rc = lp_prepare(d, nr, H, hv, lh); rc != TMPC_OK) return rc;
    const int nrp = lh.nrp;
    const std::vector<double> &Ht = lh.Ht, &hs = lh.hs, &rs = lh.rs;
    const double hm = lh.hm;
    if (lh.empty_set || lh.no_normal) {
        // 0 <= h_r < 0 for some r: no point satisfies the rows; no normal at all: every direction is unbounded
        for (int64_t b = 0; b < B; ++b) {
            val[b] = lh.empty_set ? std::nan("") : INFINITY;
            status[b] = lh.empty_set ? TMPC_STATUS_INFEASIBLE : TMPC_STATUS_UNBOUNDED;
            iters[b] = 0;
            if (x) for (int j = 0; j < d; ++j) x[b * d + j] = std::nan("");
        }
        return TMPC_OK;
    }

    LP_TRY(hipSetDevice(device));
    static int cu_count[64] = {};                       // hipGetDeviceProperties costs about a millisecond: once per device
    int n_cu = (device >= 0 && device < 64) ? cu_count[device] : 0;
    if (n_cu == 0) {
        LP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        if (device >= 0 && device < 64) cu_count[device] = n_cu;
    }
    const int wpb = tmpc::lp_waves_per_block();
    const int64_t want = (B + wpb - 1) / wpb;
    const int nblocks = static_cast<int>(std::min<int64_t>(want, 2 * static_cast<int64_t>(n_cu)));
    const size_t b = static_cast<size_t>(B), dd = static_cast<size_t>(d);
    const size_t nws = static_cast<size_t>(nblocks) * wpb * tmpc::lp_workspace_arrays() * nrp;
    if (device != g_lp_device) { g_lp_arena.release(); g_lp_device = device; }
    double *dHt, *dh, *drs, *dC, *dws, *dval, *dx = nullptr;
    int32_t *dst, *dit, *drel = nullptr;
    unsigned long long *dnext;
    Arena &ar = g_lp_arena;
    ar.piece(&dHt, Ht.size() * sizeof(double), Ht.data());
    ar.piece(&dh, hs.size() * sizeof(double), hs.data());
    ar.piece(&drs, rs.size() * sizeof(double), rs.data());
    ar.piece(&dC, b * dd * sizeof(double), C);
    ar.piece(&dws, nws * sizeof(double));
    ar.piece(&dval, b * sizeof(double));
    if (x) ar.piece(&dx, b * dd * sizeof(double));
    ar.piece(&dst, b * sizeof(int32_t));
    ar.piece(&dit, b * sizeof(int32_t));
    if (relax) ar.piece(&drel, b * sizeof(int32_t), relax);
    ar.piece(&dnext, sizeof(unsigned long long), nullptr, 0);
    LP_TRY(ar.carve(nullptr));
    tmpc::LpDevice lp{};
    lp.d = d; lp.nr = nr; lp.nrp = nrp; lp.max_iter = LP_MAX_ITER;
    lp.tol = LP_TOL; lp.relax_by = relax_by; lp.hm = hm;
    lp.Ht = dHt; lp.h = dh; lp.rscale = drs;
    lp.next_item = dnext;
    LP_TRY(tmpc::launch_lp(lp, B, nblocks, dC, drel, dws, dval, dx, dst, dit, nullptr));
    LP_TRY(hipDeviceSynchronize());
    LP_TRY(hipMemcpy(val, dval, b * sizeof(double), hipMemcpyDeviceToHost));
    LP_TRY(hipMemcpy(status, dst, b * sizeof(int32_t), hipMemcpyDeviceToHost));
    LP_TRY(hipMemcpy(iters, dit, b * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (x) LP_TRY(hipMemcpy(x, dx, b * dd * sizeof(double), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

// Test support (tests/wavesim): the LP kernel's input in kernel units -- what tmpc_lp_batch uploads -- written to a file.
// No device is touched.  Format: int32 d, nr, nrp, DP, max_iter; double tol, relax_by, hm; Ht [DP][nrp], h [nrp], rscale [nrp].
int tmpc_debug_dump_lp_layout(int32_t d, int32_t nr, const double *H, const double *hv, double relax_by, const char *path) {
    if (!H || !hv || !path) { g_create_error = "tmpc_debug_dump_lp_layout: NULL argument"; return TMPC_E_INVALID; }
    LpHost lh;
    if (const int rc = lp_prepare(d, nr, H, hv, lh); rc != TMPC_OK) return rc;
    if (lh.empty_set || lh.no_normal) { g_create_error = "tmpc_debug_dump_lp_layout: the batch is decided on the host, no kernel input"; return TMPC_E_INVALID; }
    FILE *f = std::fopen(path, "wb");
    if (!f) { g_create_error = "tmpc_debug_dump_lp_layout: cannot open the file"; return TMPC_E_INVALID; }
    const int32_t hd[5] = {d, nr, lh.nrp, lh.DP, LP_MAX_ITER};
    const double sc[3] = {LP_TOL, relax_by, lh.hm};
    bool ok = std::fwrite(hd, 4, 5, f) == 5 && std::fwrite(sc, 8, 3, f) == 3;
    ok = ok && std::fwrite(lh.Ht.data(), 8, lh.Ht.size(), f) == lh.Ht.size();
    ok = ok && std::fwrite(lh.hs.data(), 8, lh.hs.size(), f) == lh.hs.size();
    ok = ok && std::fwrite(lh.rs.data(), 8, lh.rs.size(), f) == lh.rs.size();
    std::fclose(f);
    if (!ok) { g_create_error = "tmpc_debug_dump_lp_layout: short write"; return TMPC_E_INVALID; }
    return TMPC_OK;
}

// ---- the disturbance set of the linear model, estimated on the plant it was derived from (tmpc_west.hip)

#define WEST_TRY(expr)                                                                     \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            g_create_error = std::string(who) + ": " #expr ": " + hipGetErrorString(e_);   \
            return TMPC_E_DEVICE;                                                          \
        }                                                                                  \
    } while (0)

namespace {
// selection on columns that are on the device already; the answers come back to host memory
int west_select_to_host(const char *who, WestMem &mem, const double *d_data, int64_t n, int64_t col_stride, int ncol, int32_t n_rank,
                        const int64_t *ranks, double *out, int64_t *n_nonfinite, hipEvent_t before = nullptr, hipEvent_t after = nullptr) {
    unsigned long long *d_ranks = nullptr, *d_ws = nullptr, *d_nf = nullptr;
    double *d_out = nullptr;
    const size_t nr = static_cast<size_t>(n_rank), nc = static_cast<size_t>(ncol);
    WEST_TRY(mem.get(&d_ranks, nr * 8));
    WEST_TRY(mem.get(&d_ws, tmpc::west_select_ws_words(ncol) * 8));
    WEST_TRY(mem.get(&d_nf, nc * 8));
    WEST_TRY(mem.get(&d_out, nc * nr * 8));
    if (n_rank > 0) WEST_TRY(hipMemcpy(d_ranks, ranks, nr * 8, hipMemcpyHostToDevice));
    if (before) WEST_TRY(hipEventRecord(before, nullptr));
    WEST_TRY(tmpc::launch_west_select(d_data, n, col_stride, ncol, n_rank > 0 && out ? n_rank : 0, d_ranks, d_ws, d_out, d_nf, nullptr));
    if (after) WEST_TRY(hipEventRecord(after, nullptr));
    WEST_TRY(hipDeviceSynchronize());
    if (out && n_rank > 0) WEST_TRY(hipMemcpy(out, d_out, nc * nr * 8, hipMemcpyDeviceToHost));
    if (n_nonfinite) WEST_TRY(hipMemcpy(n_nonfinite, d_nf, nc * 8, hipMemcpyDeviceToHost));
    return TMPC_OK;
}
}  // namespace

int tmpc_order_statistics(int device, int64_t n, int32_t ncol, const double *data, int32_t n_rank, const int64_t *ranks, double *out,
                          int64_t *n_nonfinite) {
    const char *who = "tmpc_order_statistics";
    if (n < 1 || ncol < 1 || n_rank < 0 || !data || (n_rank > 0 && (!ranks || !out))) {
        g_create_error = "tmpc_order_statistics: need n >= 1, ncol >= 1, data, and ranks / out for n_rank > 0";
        return TMPC_E_INVALID;
    }
    for (int32_t r = 0; r < n_rank; ++r)
        if (ranks[r] < 0 || ranks[r] >= n) { g_create_error = "tmpc_order_statistics: rank out of range [0, n)"; return TMPC_E_INVALID; }
    WEST_TRY(hipSetDevice(device));
    WestMem mem;
    double *d_data = nullptr;
    const size_t bytes = static_cast<size_t>(n) * static_cast<size_t>(ncol) * 8;
    if (mem.get(&d_data, bytes) != hipSuccess) {
        (void)hipGetLastError();
        g_create_error = "tmpc_order_statistics: out of device memory";
        return TMPC_E_NOMEM;
    }
    WEST_TRY(hipMemcpy(d_data, data, bytes, hipMemcpyHostToDevice));
    return west_select_to_host(who, mem, d_data, n, n, ncol, n_rank, ranks, out, n_nonfinite);
}

int tmpc_estimate_w(int device, int32_t nx, int32_t nu, const double *A, const double *B, const double *K, int plant, const double *par7,
                    int32_t substeps, int64_t n_traj, int32_t T, const double *x0, const double *x0_lo, const double *x0_hi, uint64_t seed,
                    int64_t first_trajectory, int32_t n_rank, const int64_t *ranks, double settle_tol, double *order_stats, double *w_min,
                    double *w_max, int64_t *n_samples, int64_t *n_nonfinite, int64_t *not_settled, double *x_final_norm_max,
                    double *x0_used, double *samples, float *kernel_ms) {
    if (!par7) { g_create_error = "tmpc_estimate_w: NULL argument"; return TMPC_E_INVALID; }
    return tmpc_estimate_w_models(device, nx, nu, A, B, K, plant, par7, nullptr, substeps, n_traj, T, x0, x0_lo, x0_hi, seed, first_trajectory, n_rank,
                                  ranks, settle_tol, order_stats, w_min, w_max, n_samples, n_nonfinite, not_settled, x_final_norm_max, x0_used,
                                  samples, kernel_ms);
}

int tmpc_estimate_w_models(int device, int32_t nx, int32_t nu, const double *A, const double *B, const double *K, int plant, const double *par7,
                           const double *par_traj, int32_t substeps, int64_t n_traj, int32_t T, const double *x0, const double *x0_lo,
                           const double *x0_hi, uint64_t seed, int64_t first_trajectory, int32_t n_rank, const int64_t *ranks, double settle_tol,
                           double *order_stats, double *w_min, double *w_max, int64_t *n_samples, int64_t *n_nonfinite, int64_t *not_settled,
                           double *x_final_norm_max, double *x0_used, double *samples, float *kernel_ms) {
    const char *who = "tmpc_estimate_w";
    if (plant != TMPC_PLANT_CARTPOLE || nx != tmpc::WEST_NX || nu != 1) {
        g_create_error = "tmpc_estimate_w: only TMPC_PLANT_CARTPOLE (nx = 4, nu = 1) is supported";
        return TMPC_E_UNSUPPORTED;
    }
    if (!A || !B || !K || (!par7 && !par_traj) || (!x0 && (!x0_lo || !x0_hi)) || (n_rank > 0 && !ranks)) { g_create_error = "tmpc_estimate_w: NULL argument"; return TMPC_E_INVALID; }
    if (n_traj < 1 || T < 2 || substeps < 1 || n_rank < 0 || first_trajectory < 0) {
        g_create_error = "tmpc_estimate_w: need n_traj >= 1, T >= 2, substeps >= 1, n_rank >= 0, first_trajectory >= 0";
        return TMPC_E_INVALID;
    }
    const int64_t n = n_traj * static_cast<int64_t>(T - 1);
    for (int32_t r = 0; r < n_rank; ++r)
        if (ranks[r] < 0 || ranks[r] >= n) { g_create_error = "tmpc_estimate_w: rank out of range [0, n_traj (T - 1))"; return TMPC_E_INVALID; }
    if (par_traj) {
        const std::string bad = cartpole_rows_error("tmpc_estimate_w_models", par_traj, n_traj);
        if (!bad.empty()) { g_create_error = bad; return TMPC_E_INVALID; }
    }
    constexpr int NX = tmpc::WEST_NX;
    tmpc::WestRollout a{};
    {
#pragma clang fp contract(off)
        for (int i = 0; i < NX; ++i)
            for (int j = 0; j < NX; ++j) {
                const double bk = B[i] * K[j];           // A - B K in double, a product and a difference per entry (numpy's A - B @ K)
                a.Acl[i * NX + j] = A[i * NX + j] - bk;
            }
    }
    for (int i = 0; i < NX; ++i) { a.K[i] = K[i]; a.lo[i] = x0 ? 0.0 : x0_lo[i]; a.hi[i] = x0 ? 0.0 : x0_hi[i]; }
    for (int i = 0; i < 7; ++i) a.par[i] = par7 ? par7[i] : par_traj[i];
    a.substeps = substeps; a.T = T; a.draw = x0 ? 0 : 1;
    a.n_traj = n_traj; a.first = first_trajectory; a.seed = seed;

    WEST_TRY(hipSetDevice(device));
    WestMem mem;
    const size_t nt = static_cast<size_t>(n_traj);
    double *d_samples = nullptr, *d_x0 = nullptr, *d_x0u = nullptr, *d_norm = nullptr, *d_par = nullptr;
    unsigned long long *d_mm = nullptr;
    if (mem.get(&d_samples, static_cast<size_t>(n) * NX * 8) != hipSuccess) {
        (void)hipGetLastError();
        g_create_error = "tmpc_estimate_w: out of device memory for the samples (8 nx (T - 1) n_traj bytes)";
        return TMPC_E_NOMEM;
    }
    WEST_TRY(mem.get(&d_x0u, nt * NX * 8));
    WEST_TRY(mem.get(&d_norm, nt * 8));
    WEST_TRY(mem.get(&d_mm, 2 * NX * 8));
    if (x0) {
        WEST_TRY(mem.get(&d_x0, nt * NX * 8));
        WEST_TRY(hipMemcpy(d_x0, x0, nt * NX * 8, hipMemcpyHostToDevice));
    }
    if (par_traj) {
        WEST_TRY(mem.get(&d_par, nt * 7 * 8));
        WEST_TRY(hipMemcpy(d_par, par_traj, nt * 7 * 8, hipMemcpyHostToDevice));
    }
    WEST_TRY(hipMemset(d_mm, 0xff, NX * 8));
    WEST_TRY(hipMemset(d_mm + NX, 0, NX * 8));
    a.x0 = d_x0; a.x0_used = d_x0u; a.samples = d_samples; a.xnorm = d_norm; a.minmax = d_mm; a.par_traj = d_par;
    WestEvents ev;
    for (hipEvent_t &e : ev.ev) WEST_TRY(hipEventCreate(&e));
    WEST_TRY(hipEventRecord(ev.ev[0], nullptr));
    WEST_TRY(tmpc::launch_west_rollout(a, nullptr));
    WEST_TRY(hipEventRecord(ev.ev[1], nullptr));
    const bool want_sel = (order_stats && n_rank > 0) || n_nonfinite;
    if (want_sel)
        if (const int rc = west_select_to_host(who, mem, d_samples, n, n, NX, n_rank, ranks, order_stats, n_nonfinite, ev.ev[2], ev.ev[3]); rc != TMPC_OK) return rc;
    WEST_TRY(hipDeviceSynchronize());
    if (kernel_ms) {
        WEST_TRY(hipEventElapsedTime(&kernel_ms[0], ev.ev[0], ev.ev[1]));
        kernel_ms[1] = 0.0f;
        if (want_sel) WEST_TRY(hipEventElapsedTime(&kernel_ms[1], ev.ev[2], ev.ev[3]));
    }
    if (w_min || w_max) {
        unsigned long long mm[2 * NX];
        WEST_TRY(hipMemcpy(mm, d_mm, sizeof mm, hipMemcpyDeviceToHost));
        for (int c = 0; c < NX; ++c) {
            double lo, hi;
            const unsigned long long ul = tmpc::west_unkey(mm[c]), uh = tmpc::west_unkey(mm[NX + c]);
            std::memcpy(&lo, &ul, 8);
            std::memcpy(&hi, &uh, 8);
            const bool none = !(lo <= hi);               // no finite sample: the start values, +inf / -inf
            if (w_min) w_min[c] = none ? std::nan("") : lo;
            if (w_max) w_max[c] = none ? std::nan("") : hi;
        }
    }
    if (n_samples) *n_samples = n;
    if (not_settled || x_final_norm_max) {
        std::vector<double> nrm(nt);
        WEST_TRY(hipMemcpy(nrm.data(), d_norm, nt * 8, hipMemcpyDeviceToHost));
        int64_t bad = 0;
        double worst = 0.0;
        bool any_nan = false;
        for (double v : nrm) {
            if (!(v <= settle_tol)) ++bad;               // (a NaN has not settled either)
            if (v != v) any_nan = true;
            else if (v > worst) worst = v;
        }
        if (not_settled) *not_settled = bad;
        if (x_final_norm_max) *x_final_norm_max = any_nan ? std::nan("") : worst;
    }
    if (x0_used) WEST_TRY(hipMemcpy(x0_used, d_x0u, nt * NX * 8, hipMemcpyDeviceToHost));
    if (samples) WEST_TRY(hipMemcpy(samples, d_samples, static_cast<size_t>(n) * NX * 8, hipMemcpyDeviceToHost));
    return TMPC_OK;
}

}  // extern "C"
