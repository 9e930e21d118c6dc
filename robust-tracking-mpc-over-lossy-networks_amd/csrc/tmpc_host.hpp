// Host side of libtmpc_hip.so, internal: the handle and what it owns, shared by tmpc_api.cpp (handle, upload, lanes, batch solve),
// tmpc_loops.cpp (closed loops) and tmpc_offline.cpp (LP batches, W estimate).  Nothing here is exported.
#pragma once
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
#include "tmpc_law.hpp"

namespace tmpc_host __attribute__((visibility("hidden"))) {

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
    double *ser_e = nullptr;     // the per-step record (tmpc_mc_set_series): [ser_T][ser_B] each, where the loop left them in the arena
    uint32_t *ser_w = nullptr;
    int64_t ser_B = 0;
    int ser_T = 0;
    tmpc::LawLoop law{};         // tmpc_mc_set_law: the per-trajectory counters and the miss log, where the loop left them in the arena
    int64_t law_B = 0;           // 0: the last loop did not go through the law
};

// What a new handle starts with where the environment says nothing (TMPC_CALL_LANES): DESIGN.md 5.1 "Between launches" has the
// measurements behind the choice
constexpr int DEFAULT_CALL_LANES = 3;

// One launch lane of a device handle: a non-blocking stream and everything a solve launch on it mutates, so that launches on
// different lanes may overlap while the launches of one lane stay ordered.  Lane 0 (the primary lane) exists from tmpc_create on
// and takes every entry point; the others (tmpc::MAX_LANES in all) get their streams at tmpc_create too and are taken into use by the first
// tmpc_solve_batch_device call that finds every lane in use holding unfinished work it can run beside.
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
    bool active = false;         // taken into use by the lane choice (the stream of a lane exists from tmpc_create on, see setup_handle)
};

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
    bool law = false;                    // opened with the law on (tmpc_mc_set_law): ll is what every step's law launch is given
    tmpc::LawLoop ll{};
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

// The closed-loop settings of a handle (tmpc_mc_set_*): what the setters write, and the loops' checks and set-up read.
struct LoopSettings {
    int plant = TMPC_PLANT_LINEAR, plant_substeps = 10;
    double plant_par[7] = {0, 0, 0, 0, 0, 0, 0};
    int actuator = TMPC_ACTUATOR_CONSISTENT;
    long long capture = -1;      // trajectory recorded by the next tmpc_mc_run (-1: none)
    int warm = 0;                // hand every solve the working set of the trajectory's previous solve of the same variant
    int fused = TMPC_MC_FUSED_AUTO;      // one fused launch for all T steps (tmpc_mc_set_fused)
    int rng_on = 0;              // tmpc_mc_set_device_rng
    uint64_t rng_seed = 0;
    int64_t rng_first = 0;
    std::vector<double> w_bound;
    // tmpc_mc_set_reference_table: K schedules of T_tab full-state references and the schedule of each of B trajectories (K = 0: none)
    int32_t ref_K = 0, ref_T = 0;
    int64_t ref_B = 0;
    std::vector<double> ref_tab;
    std::vector<int32_t> ref_id;
    // tmpc_mc_set_channel: the Gilbert-Elliott thresholds [B][2][3] as the device compares them (ch_B = 0: the Bernoulli model)
    int64_t ch_B = 0;
    std::vector<double> ch_thr;
    // tmpc_mc_set_plant_models (regulator handles): a linear plant per trajectory, [B][nx][nx + nu] (pm_B = 0: none)
    int64_t pm_B = 0;
    std::vector<double> pm;
    int series = 0;              // tmpc_mc_set_series: the tracking loops keep their per-step record
    int law = 0, law_max_tries = 0;      // tmpc_mc_set_law: the tracking loops look into the explicit law's table before each solve
    int64_t law_miss_cap = 0;
};
struct LawState;                 // the explicit law's tables (tmpc_law.cpp), created by the first tmpc_law_* call
struct SensState;                // what the sensitivity entry points keep on the device (tmpc_sens.cpp), created by the first such call
}  // namespace tmpc_host

struct tmpc_handle {
    // the handle: its problem(s), device, stream and the scratch of the solve launches
    int device = 0;
    int n_cu = 0;
    int nvariants = 0;
    int nx = 0, nu = 0, N = 0;
    tmpc_host::Variant v[2];
    // regulator handles (tmpc_create_regulator): no reference input -- the solves read `ref` from a zero buffer (F2 = 0)
    bool regulator = false;
    int reg_tube = 0;
    std::vector<double> hA, hB, hK, hKanc, hQ, hR;   // host copies for the closed-loop entry points
    int kernel_path = TMPC_PATH_AUTO;
    tmpc_host::Lane lane[tmpc::MAX_LANES];
    hipStream_t stream = nullptr;        // = lane[0].stream: everything but an overlapped tmpc_solve_batch_device call runs on it
    int overlap = 1;             // tmpc_set_call_overlap
    int lanes = 2;               // lanes the calls rotate over with the overlap on (tmpc_set_call_lanes, TMPC_CALL_LANES)
    int cur = 0;                 // lane of the latest solve call
    int par = 0;                 // parity of the lane changes since the lanes were last joined; with two lanes, = cur
    int64_t par_calls[2] = {0, 0};       // calls by that parity (tmpc_debug_lane_counters)
    int64_t lane_waits = 0;      // calls that had to wait for another lane (tmpc_debug_lane_counters)
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
    tmpc_host::DeviceBuffer reg_zero;       // regulator: the zero reference
    std::string err;
    // staging buffers for the host-pointer entry point: ONE device block, inputs [x | ref | variant] then outputs
    // [u | x0 | ss | status | iters | x_nom], and a pinned host mirror of it -- a call moves its inputs with one DMA and its
    // outputs with one (round 3: nine hipMemcpyAsync from / to pageable memory per call, 60 % of the time of a call at batch 1)
    tmpc_host::DeviceBuffer stage_dev;
    char *stage_pin = nullptr;
    size_t stage_in_bytes = 0, stage_out_bytes = 0, stage_out_core = 0;      // (core = the outputs without x_nom)
    size_t off_r = 0, off_var = 0, off_x0 = 0, off_ss = 0, off_st = 0, off_it = 0, off_xn = 0;      // offsets within the input / output parts
    double *d_x = nullptr, *d_r = nullptr, *d_u = nullptr, *d_x0 = nullptr, *d_ss = nullptr, *d_xn = nullptr;
    uint8_t *d_var = nullptr;
    int32_t *d_st = nullptr, *d_it = nullptr;
    tmpc_host::LoopSettings loop;           // closed-loop settings (tmpc_mc_set_*)
    // closed-loop state: one grow-only arena (25 hipMalloc / hipFree per call cost several milliseconds), and what the last run
    // left in it
    tmpc_host::Arena arena;
    tmpc_host::LoopRecords rec;
    tmpc_host::McSession ses;
    tmpc_host::LawState *law = nullptr;     // tmpc_law_*: nullptr until the first call
    tmpc_host::SensState *sens = nullptr;   // tmpc_sens_*: nullptr until the first call (a handle that never asks allocates nothing)
};

namespace tmpc_host __attribute__((visibility("hidden"))) {

#define HIP_TRY(h, expr)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return TMPC_E_DEVICE;                                                          \
        }                                                                                  \
    } while (0)

extern thread_local std::string g_create_error;       // tmpc_last_error(NULL): the message of a call that has no handle

// What the closed loops use of the handle's solve path (tmpc_api.cpp)
hipError_t sync_lanes(tmpc_handle *h);
bool use_block(const tmpc_handle *h, const Variant &v);
int ensure_reg_zero(tmpc_handle *h, int64_t B);
int begin_timed_launch(tmpc_handle *h, Lane &lane);
int prepare_wave_scratch(tmpc_handle *h, Lane &lane, int64_t B, int nvar);
int enqueue(tmpc_handle *h, Lane &lane, const tmpc::BatchIO &io, int32_t *const *ws = nullptr, bool variants_valid = false);
void release_session(tmpc_handle *h);
int begin_loop(tmpc_handle *h, int64_t B);
// orders the primary lane behind what the other lanes hold, without blocking the host (every entry point that runs on the primary lane alone starts so)
int join_lanes(tmpc_handle *h);
// lanes a handle may use: tmpc::MAX_LANES where every variant runs on the wave kernel, two where one has the block kernel's workspace per lane
int max_lanes(const tmpc_handle *h);
bool session_bars(tmpc_handle *h, const char *who);
int pick_call_lane(tmpc_handle *h, const tmpc::CallRanges &call, Lane **out);
int note_call(tmpc_handle *h, Lane &lane, const tmpc::CallRanges &call);
// (tmpc_sens.cpp) frees what the sensitivity calls allocated; the caller has synchronised
void release_sens(tmpc_handle *h);
// (tmpc_sens.cpp) what the sensitivity entries and the explicit law (tmpc_law.cpp) both build on: the Cholesky factor of a symmetric
// matrix in place (false: not positive definite) and a solve with it, H^-1, and the model of a handle's variant beyond its condensed
// form -- F = [F1 F2], Ebar = [E 0], y = Y z + Yp p, z = Rec [y | p]
bool chol(std::vector<double> &a, int n);
void chol_solve(const std::vector<double> &L, int n, double *x);
std::string spd_inverse(const double *H, int n, std::vector<double> &Hinv);
struct HostModel {
    tmpc::Mat F, Eb, Y, Yp, Rec;
};
std::string host_model(const tmpc_handle *h, int k, HostModel &hm, int &rc);
int sens_signatures(tmpc_handle *h, const char *who, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                    const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, int32_t *flag, int32_t *n_active, uint32_t *active);
// (tmpc_law.cpp) frees what the explicit-law entries allocated; the caller has synchronised
void release_law(tmpc_handle *h);
// the solve launches of one call without its timing events: one per variant, `io.variant` the selector (tmpc_law.cpp runs them behind its own kernel)
int enqueue_solves(tmpc_handle *h, Lane &lane, const tmpc::BatchIO &io, int32_t *const *ws);
// (tmpc_law.cpp) the closed loops through the law.  law_loop_begin: the refusals of a run with the law on (nvar problems in use), the
// models and the tables' descriptions brought up to date; fills ll.t.  enqueue_law_loop: one step -- the law's launch over
// [x_hat | ref_k] (variant: the problem selector or nullptr; skip: the trajectories that have stopped) with hint = region = ll.region,
// then the solve launches of the misses with the warm-start records ws, between the timing events of an ordinary solve call.
int law_loop_begin(tmpc_handle *h, const char *who, int nvar, tmpc::LawLoop &ll);
int enqueue_law_loop(tmpc_handle *h, Lane &lane, const char *who, int64_t B, const double *x_hat, const double *ref_k, const uint8_t *variant,
                     const uint8_t *skip, const tmpc::LawLoop &ll, int32_t *const *ws);
// (tmpc_offline.cpp) cart-pole rows {M, m, b, I, g, l, Th} of n trajectories: empty, or the message naming trajectory and field
std::string cartpole_rows_error(const char *who, const double *rows, int64_t n);
}  // namespace tmpc_host
