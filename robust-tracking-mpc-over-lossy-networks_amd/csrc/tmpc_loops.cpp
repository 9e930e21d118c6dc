// The closed loops of libtmpc_hip.so (include/tmpc.h: tmpc_mc_*, tmpc_reg_run): settings, the resident loops and the stepped one.
#include "tmpc_host.hpp"
#include "tmpc_plant.hpp"
#include "tmpc_series.hpp"

using namespace tmpc_host;

namespace {
// packets injected by the caller (tmpc_mc_replay) and the per-step record that goes back
struct McReplay {
    const double *U, *xn0;      // host: [B][T][N+1][nu], [B][T][nx] (xn0 may be NULL unless extended)
    double *trace_f;            // host: [B][T][3 nx + nu]
    int32_t *trace_i;           // host: [B][T][3]
};

// A loop of B trajectories and T steps under the handle's reference table (tmpc_mc_set_reference_table): does it fit?
int reference_table_fits(tmpc_handle *h, const char *who, int64_t B, int32_t T) {
    if (B != h->loop.ref_B) {
        h->err = std::string(who) + ": B = " + std::to_string(B) + ", but the reference table was set for B = " + std::to_string(h->loop.ref_B) + " trajectories";
        return TMPC_E_INVALID;
    }
    if (T > h->loop.ref_T) {
        h->err = std::string(who) + ": T = " + std::to_string(T) + " steps, but the reference table has T_tab = " + std::to_string(h->loop.ref_T) + " rows";
        return TMPC_E_INVALID;
    }
    return TMPC_OK;
}

// A loop of B trajectories under the handle's loss channel (tmpc_mc_set_channel): does it fit?
int channel_fits(tmpc_handle *h, const char *who, int64_t B) {
    if (B == h->loop.ch_B) return TMPC_OK;
    h->err = std::string(who) + ": B = " + std::to_string(B) + ", but the loss channel was set for B = " + std::to_string(h->loop.ch_B) + " trajectories";
    return TMPC_E_INVALID;
}
// A loop of B trajectories under the handle's plant models (tmpc_mc_set_plant_models): does it fit?
int plant_models_fit(tmpc_handle *h, const char *who, int64_t B) {
    if (h->loop.pm_B == 0 || B == h->loop.pm_B) return TMPC_OK;
    h->err = std::string(who) + ": B = " + std::to_string(B) + ", but the plant models were set for B = " + std::to_string(h->loop.pm_B) + " trajectories";
    return TMPC_E_INVALID;
}
// the loss model's and the link statistics' pieces of a loop's arena: the channel's thresholds and link states (both links start
// in G) or p_loss, and the four counters -- one block [4][B], so that one copy brings them back (link_block_carved, fetch_tracking_results)
void link_pieces(tmpc_handle *h, Arena &a, tmpc::McState &st, bool channel, size_t b, const double *p_loss) {
    if (channel) {
        a.piece(&st.ch_thr, h->loop.ch_thr.size() * 8, h->loop.ch_thr.data());
        a.piece(&st.ch_state, b * 2, nullptr, 0);
    } else {
        a.piece(&st.p_loss, b * 8, p_loss);
    }
    a.piece(&st.lost_up, b * 4 * 4, nullptr, 0);
}
void link_block_carved(tmpc::McState &st, size_t b) {
    st.lost_down = st.lost_up + b; st.max_gap = st.lost_up + 2 * b; st.overrun = st.lost_up + 3 * b;
}

// A check set as the entry points take it: `rows` rows of H x <= h (0: no set), and its two pieces of a loop's arena
struct SetRows {
    const double *H, *h;
    int32_t rows;
    bool missing() const { return rows > 0 && (!H || !h); }
};
void set_pieces(Arena &a, const double **H, const double **h, const SetRows &s, size_t dim) {
    a.piece(H, static_cast<size_t>(s.rows) * dim * 8, s.H);
    a.piece(h, static_cast<size_t>(s.rows) * 8, s.h);
}
// the device generator of a loop's state (tmpc_mc_set_device_rng); w_bound: the slot of the disturbance box, nullptr where no w is drawn
void rng_fields(tmpc_handle *h, int &on, unsigned long long &seed, long long &first, const double **w_bound) {
    on = 1; seed = h->loop.rng_seed; first = h->loop.rng_first;
    if (w_bound) h->arena.piece(w_bound, static_cast<size_t>(h->nx) * 8, h->loop.w_bound.data());
}
// the end of every loop: a failure waits for what was enqueued, which may still use the caller's arrays
int finish_loop(tmpc_handle *h, int rc) {
    if (rc != TMPC_OK) (void)sync_lanes(h);
    return rc;
}

// The arguments of a tracking loop -- tmpc_mc_run, tmpc_mc_replay (rp) or tmpc_mc_open (session: the caller's plant, so no w, and the check
// sets X, U) -- and, filled in by check_tracking_loop, what the handle's settings make of them.
struct TrackingLoop {
    const char *who;
    bool session;
    int64_t B;
    int32_t T;
    int extended;
    const double *p_loss, *ref, *th_u, *ga_u, *w, *x0;
    SetRows Z, X, U;
    const McReplay *rp;         // (tmpc_mc_replay solves nothing and is given its arrival flags: it ignores the reference table and the channel)
    bool host_draws, full_ref, channel, series;       // (series: tmpc_mc_set_series -- ignored by tmpc_mc_replay like the other two)
    bool law;                   // tmpc_mc_set_law (ignored by tmpc_mc_replay)
};

// The argument checks of the tracking loops, in the order each entry point has always reported them (it differs between the resident
// loops and the session, and a host-only handle makes it visible); TMPC_OK: the loop may be set up.
int check_tracking_loop(tmpc_handle *h, TrackingLoop &q) {
    const std::string who = std::string(q.who) + ": ";
    auto refuse = [&](const char *msg, int code = TMPC_E_INVALID) { h->err = who + msg; return code; };
    auto host_only = [&]() { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; };
    if (h->ses.open) return refuse(q.session ? "a stepped closed loop is already open on this handle (one session per handle)" : "a stepped closed loop is open on this handle (tmpc_mc_close first)");
    q.host_draws = q.rp != nullptr || !h->loop.rng_on;
    q.full_ref = !q.rp && h->loop.ref_K > 0;
    q.channel = !q.rp && h->loop.ch_B > 0;
    q.series = !q.rp && h->loop.series != 0;
    q.law = !q.rp && h->loop.law != 0;
    if (q.session && h->regulator) return refuse("a regulator handle has no stepped loop");
    if (q.session && (q.B <= 0 || q.T <= 0 || q.Z.rows < 0 || q.X.rows < 0 || q.U.rows < 0)) return refuse("need B > 0, T > 0 and row counts >= 0");
    if (q.B < 0 || q.T < 0 || (!q.p_loss && !q.channel) || (!q.ref && !q.full_ref) || (q.host_draws && (!q.th_u || !q.ga_u || (!q.session && !q.w))) ||
        q.Z.missing() || q.X.missing() || q.U.missing())
        return refuse("NULL argument");
    if (h->regulator) return refuse("a regulator handle runs its loop with tmpc_reg_run");
    if (q.channel)       // (an argument error: reported on a host-only handle too)
        if (const int rc = channel_fits(h, q.who, q.B)) return rc;
    if (!q.session && h->device < 0) return host_only();
    if (q.extended && h->nvariants < 2) return refuse("extended loop needs a problem created with extended = 1");
    if (h->hK.empty() || h->hKanc.empty()) return refuse("the problem description carries no gains K / K_anc");
    if (h->device < 0) return host_only();
    if (h->nu > 16) return refuse("nu <= 16", TMPC_E_UNSUPPORTED);
    return q.full_ref ? reference_table_fits(h, q.who, q.B, q.T) : TMPC_OK;
}

// Lists the McModel / McState pieces of a tracking loop in the handle's arena and fills the scalar fields; m and st come zero-initialised, so
// that nothing of an earlier loop reaches this one.  ws: the warm-start sets; s: the session, whose extra pieces (the caller's sets and
// counters, the staging of tmpc_mc_step[_ref]) go in between -- nullptr for a run, whose arena is the list below without them.  The caller
// adds what is its own, carves and calls link_block_carved.  THE place where a new loop option gets its device memory.
void tracking_pieces(tmpc_handle *h, const TrackingLoop &q, tmpc::McModel &m, tmpc::McState &st, int32_t **ws, McSession *s, tmpc::LawLoop *ll) {
    const LoopSettings &L = h->loop;
    const size_t nx = h->nx, nu = h->nu, N = h->N, b = static_cast<size_t>(q.B), t_ = static_cast<size_t>(q.T);
    m.nx = h->nx; m.nu = h->nu; m.N = h->N; m.extended = q.extended ? 1 : 0; m.rZ = q.Z.rows;
    m.plant = s ? TMPC_PLANT_EXTERNAL : L.plant; m.substeps = s ? 1 : L.plant_substeps; m.smart = L.actuator == TMPC_ACTUATOR_SMART ? 1 : 0;
    for (int i = 0; i < 7 && !s; ++i) m.par[i] = L.plant_par[i];
    Arena &a = h->arena;
    a.piece(&m.A, nx * nx * 8, h->hA.data());
    a.piece(&m.B, nx * nu * 8, h->hB.data());
    a.piece(&m.K, nu * nx * 8, h->hK.data());
    a.piece(&m.K_anc, nu * nx * 8, h->hKanc.data());
    set_pieces(a, &m.HZ, &m.hZ, q.Z, nx);
    if (s) {
        s->ext.rX = q.X.rows; s->ext.rU = q.U.rows;
        set_pieces(a, &s->ext.HX, &s->ext.hX, q.X, nx);
        set_pieces(a, &s->ext.HU, &s->ext.hU, q.U, nu);
    }
    link_pieces(h, a, st, q.channel, b, q.p_loss);
    if (q.host_draws) {
        a.piece(&st.th_u, b * t_ * 8, q.th_u);
        a.piece(&st.ga_u, b * t_ * 8, q.ga_u);
        if (!s) a.piece(&st.w, b * t_ * nx * 8, q.w);
    } else {
        rng_fields(h, st.rng_on, st.rng_seed, st.rng_first, s ? nullptr : &st.w_bound);
    }
    // the state starts at x0 (or 0), with last_lost = -1 (0xFF bytes), gamma = 1 and every statistic 0
    // (a session carries st.x for the record's sake: its state machines never read or write it)
    for (double **x : {&st.x, &st.x_hat, &st.x_nom}) a.piece(x, b * nx * 8, q.x0, 0);
    a.piece(&st.Ubuf, b * (N + 1) * nu * 8, nullptr, 0);
    a.piece(&st.u_latest0, b * nu * 8, nullptr, 0);
    for (double **x : {&st.x_nom0_latest, &st.ref_k}) a.piece(x, b * nx * 8, nullptr, 0);
    for (double **x : {&st.err2, &st.consistent}) a.piece(x, b * 8, nullptr, 0);
    for (int32_t **c : {&st.q_est, &st.q_act, &st.s, &st.Theta, &st.last_lost, &st.tube_viol, &st.not_optimal, &st.iters_sum})
        a.piece(c, b * 4, nullptr, c == &st.last_lost ? 0xFF : 0);
    if (s)
        for (int32_t **c : {&s->ext.x_viol, &s->ext.u_viol}) a.piece(c, b * 4, nullptr, 0);
    a.piece(&st.gamma, b, nullptr, 1);
    a.piece(&st.dead, b, nullptr, 0);
    st.cap_index = -1;
    if (L.capture >= 0 && L.capture < q.B) {
        a.piece(&st.cap, t_ * (2 * nx + nu) * 8, nullptr, 0);
        st.cap_index = L.capture;
    }
    if (!s && m.plant != TMPC_PLANT_LINEAR) a.piece(&st.err2_phys, b * 8, nullptr, 0);
    if (h->want_ticks) {
        a.piece(&st.tick_sum, b * 8, nullptr, 0);
        a.piece(&st.tick_max, b * 8, nullptr, 0);
    }
    // warm start: one working-set record per trajectory and variant (row ids are per variant), updated in place by the
    // solve kernel; m = 0 (the zero fill) means "nothing to start from"
    if (L.warm)
        for (int k = 0; k < (q.extended ? 2 : 1); ++k) a.piece(&ws[k], b * tmpc::WS_STRIDE * 4, nullptr, 0);
    if (s) {
        a.piece(&s->ext.x_t, b * nx * 8, nullptr, 0);
        a.piece(&s->ext.u_t, b * nu * 8, nullptr, 0);
    }
    if (q.full_ref) {       // (the table is uploaded with the loop, as `ref` is)
        a.piece(&st.ref_tab, L.ref_tab.size() * 8, L.ref_tab.data());
        a.piece(&st.ref_id, L.ref_id.size() * 4, L.ref_id.data());
        st.ref_T = L.ref_T;
        if (s) a.piece(&s->ref_stage, b * nx * 8, nullptr, 0);
    }
    if (q.series) {         // the per-step record, time-major; zeros: "took no step here"
        a.piece(&st.ser_e, t_ * b * 8, nullptr, 0);
        a.piece(&st.ser_w, t_ * b * 4, nullptr, 0);
        st.ser_B = q.B;
    }
    if (q.law) {            // the law's bookkeeping: hint / region (-1: 0xFF bytes), the two accumulators, the miss log and its counter
        const size_t cap = static_cast<size_t>(L.law_miss_cap);
        ll->max_tries = L.law_max_tries;
        ll->miss_cap = L.law_miss_cap;
        a.piece(&ll->region, b * 4, nullptr, 0xFF);
        a.piece(&ll->hits, b * 4, nullptr, 0);
        a.piece(&ll->tries, b * 8, nullptr, 0);
        a.piece(&ll->miss_n, 8, nullptr, 0);
        a.piece(&ll->miss_p, cap * 2 * nx * 8);
        a.piece(&ll->miss_var, cap);
    }
    if (q.rp) {
        // (plain controller: the packets carry no x_nom_0; the state machines then never read it -- zeros)
        a.piece(&st.rp_U, b * t_ * (N + 1) * nu * 8, q.rp->U);
        a.piece(&st.rp_xn0, b * t_ * nx * 8, q.rp->xn0, 0);
        a.piece(&st.trace_f, b * t_ * (3 * nx + nu) * 8, nullptr, 0);
        a.piece(&st.trace_i, b * t_ * 3 * 4, nullptr, 0);
    }
}

// The end of a tracking loop: enqueues the copy-back of its statistics (a NULL destination: not wanted) and of the link counters, waits,
// and leaves what the getters read (LoopRecords; the arena stays as it is until the next loop).  T: the rows of a recorded trajectory.
using McCounter = std::pair<int32_t *, const int32_t *>;      // (host destination, device counter)
int fetch_tracking_results(tmpc_handle *h, const tmpc::McState &st, const tmpc::LawLoop *ll, int64_t B, int T, double *err2, double *consistent,
                           std::initializer_list<McCounter> counters) {
    const size_t b = static_cast<size_t>(B);
    if (err2) HIP_TRY(h, hipMemcpyAsync(err2, st.err2, b * 8, hipMemcpyDeviceToHost, h->stream));
    if (consistent) HIP_TRY(h, hipMemcpyAsync(consistent, st.consistent, b * 8, hipMemcpyDeviceToHost, h->stream));
    for (const McCounter &c : counters)
        if (c.first) HIP_TRY(h, hipMemcpyAsync(c.first, c.second, b * 4, hipMemcpyDeviceToHost, h->stream));
    h->rec.link.resize(4 * b);           // (a HOST copy: tmpc_mc_get_link_stats then costs no device call)
    HIP_TRY(h, hipMemcpyAsync(h->rec.link.data(), st.lost_up, b * 4 * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sync_lanes(h));
    if (st.cap) { h->rec.cap = st.cap; h->rec.cap_T = T; }
    if (st.err2_phys) { h->rec.err2_phys = st.err2_phys; h->rec.phys_B = B; }
    if (st.tick_sum) { h->rec.tick_sum = st.tick_sum; h->rec.tick_max = st.tick_max; h->rec.tick_B = B; }
    h->rec.link_B = B;
    if (st.ser_w) { h->rec.ser_e = st.ser_e; h->rec.ser_w = st.ser_w; h->rec.ser_B = B; h->rec.ser_T = T; }
    if (ll) { h->rec.law = *ll; h->rec.law_B = B; }
    return TMPC_OK;
}

int mc_run_impl(tmpc_handle *h, TrackingLoop q, double *err2, int32_t *tube_viol, int32_t *not_optimal, double *x_final, double *consistent,
                int32_t *iters_sum) {
    if (!h) return TMPC_E_INVALID;
    if (const int rc = check_tracking_loop(h, q)) return rc;
    const int64_t B = q.B;
    const int32_t T = q.T, extended = q.extended;
    const McReplay *const rp = q.rp;
    if (B == 0 || T == 0) return TMPC_OK;
    // full-reference mode: the scalar reference of the legacy mode is not read on the device; the launches get zeros
    const std::vector<double> ref_unused(q.full_ref ? static_cast<size_t>(T) : 0, 0.0);
    const double *const ref = q.full_ref ? ref_unused.data() : q.ref;
    if (const int rc = begin_loop(h, B)) return rc;
    // through the explicit law (tmpc_mc_set_law): the table as it stands now
    tmpc::LawLoop ll{};
    if (q.law)
        if (const int rc = law_loop_begin(h, q.who, extended ? 2 : 1, ll)) return rc;
    const size_t nx = h->nx, nu = h->nu, b = static_cast<size_t>(B), t_ = static_cast<size_t>(T);
    // ONE launch for the whole sweep where the controller has one problem and it runs on the wave kernel: a wave keeps its
    // trajectory for all T steps, solve and state machines alternating inside the kernel (tmpc_fused.hip).  The work item of
    // that launch is a trajectory, T solves long: with B a little above a multiple of the resident waves the last round
    // of trajectories would run on a nearly empty card, so TMPC_MC_FUSED_AUTO fuses when the rounds are at least 85 % full
    // (or there is a single round) and otherwise keeps the launch per time step, whose work item is one solve.
    // (a loop that keeps its per-step record runs per time step: the fused kernels are compiled without the recording)
    // (through the law: closed_loop_law, where the shape has one -- DESIGN.md 7n; the other shapes look the law up per time step)
    bool fuse = !rp && !extended && !q.series && h->loop.fused != TMPC_MC_FUSED_OFF && !use_block(h, h->v[0]) &&
                (!q.law || tmpc::law_fused_compiled(h->v[0].shape));
    if (fuse && h->loop.fused == TMPC_MC_FUSED_AUTO) {
        const int64_t slots = tmpc::resident_waves(h->v[0].shape, h->n_cu);
        const int64_t rounds = slots > 0 ? (B + slots - 1) / slots : 0;
        fuse = rounds == 1 || (rounds > 0 && static_cast<double>(B) >= 0.85 * static_cast<double>(rounds * slots));
    }
    // the extended controller (two problems, two kernel shapes): per time step ONE launch per problem with the state machines of
    // its trajectories inside (closed_loop_step_kernel) -- two launches per step where the plain per-step loop has three
    // (TMPC_MC_FUSED_AUTO: from one round of resident waves on -- below that a step is the latency of its launches, and the state
    // machines inside BOTH of them lengthen it: 200 trajectories at N = 20 0.0345 s with three launches per step, 0.0367 s with two)
    // (through the law the three-launch form below: the hits need their state machines run too)
    bool step_fuse = !rp && extended && !q.series && !q.law && h->loop.fused != TMPC_MC_FUSED_OFF && !use_block(h, h->v[0]) && !use_block(h, h->v[1]);
    if (step_fuse && h->loop.fused == TMPC_MC_FUSED_AUTO) step_fuse = B >= tmpc::resident_waves(h->v[1].shape, h->n_cu);
    // the fused kernels' record {model, state, T, reference}: uploaded once the state is carved; lives until the final synchronise
    tmpc::McFused mf{};
    auto run = [&]() -> int {
        tmpc::McModel m{};
        tmpc::McState st{};
        int32_t *ws[2] = {nullptr, nullptr};
        tracking_pieces(h, q, m, st, ws, nullptr, &ll);
        Arena &a = h->arena;
        uint8_t *gam[2] = {nullptr, nullptr};           // selector read in a step / arrival flags written in it: swapped every step
        tmpc::McFused *d_mf = nullptr;                  // the record itself lives in the arena: the kernel reads it field by field
        tmpc::LawLoop *d_ll = nullptr;                  // (and the law's, for closed_loop_law)
        if (fuse || step_fuse) {
            a.piece(&mf.ref_seq, t_ * 8, ref);
            if (step_fuse) a.piece(&gam[1], b, nullptr, 1);
            a.piece(&d_mf, sizeof(mf));
            if (q.law) a.piece(&d_ll, sizeof(ll));
        }
        HIP_TRY(h, a.carve(h->stream));
        link_block_carved(st, b);
        gam[0] = st.gamma;
        HIP_TRY(h, tmpc::launch_mc_pre(m, st, B, ref[0], h->stream));
        if (fuse || step_fuse) {
            if (const int r2 = prepare_wave_scratch(h, h->lane[0], B, step_fuse ? 2 : 1)) return r2;
            st.ticks = h->want_ticks ? h->lane[0].ticks.as<long long>() : nullptr;
            mf.m = m; mf.st = st; mf.T = T;
            HIP_TRY(h, hipMemcpyAsync(d_mf, &mf, sizeof(mf), hipMemcpyHostToDevice, h->stream));
            if (d_ll) HIP_TRY(h, hipMemcpyAsync(d_ll, &ll, sizeof(ll), hipMemcpyHostToDevice, h->stream));
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
            if (q.law)
                HIP_TRY(h, tmpc::launch_solve_mc_law(h->v[0].d, h->v[0].shape, B, h->d_u, h->d_x0, h->d_ss, h->d_st, h->d_it, ws[0], d_mf, d_ll,
                                                     &h->lane[0].wc, h->n_cu, h->stream));
            else
                HIP_TRY(h, tmpc::launch_solve_mc(h->v[0].d, h->v[0].shape, B, h->d_u, h->d_x0, h->d_ss, h->d_st, h->d_it, ws[0], d_mf, &h->lane[0].wc,
                                                 h->n_cu, h->stream));
            HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
            h->timed = true;
            h->rec.fused = 1;
        } else {
            // per time step: the solve launch(es) -- one per problem variant in use -- and ONE launch of the state machines
            // (round 3: mc_pre, the variant check, the solve, mc_post, mc_tube).  With injected packets nothing is solved.
            for (int t = 0; t < T; ++t) {
                if (!rp) {
                    const int r2 = q.law ? enqueue_law_loop(h, h->lane[0], q.who, B, st.x_hat, st.ref_k, extended ? st.gamma : nullptr, st.dead, ll, ws)
                                         : enqueue(h, h->lane[0], {B, st.x_hat, st.ref_k, extended ? st.gamma : nullptr, h->d_u, h->d_x0, h->d_ss, nullptr,
                                                                   h->d_st, h->d_it}, ws, true);
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
        if (x_final) HIP_TRY(h, hipMemcpyAsync(x_final, st.x, b * nx * 8, hipMemcpyDeviceToHost, h->stream));
        return fetch_tracking_results(h, st, q.law ? &ll : nullptr, B, T, err2, consistent,
                                      {{tube_viol, st.tube_viol}, {not_optimal, st.not_optimal}, {iters_sum, st.iters_sum}});
    };
    return finish_loop(h, run());
}

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
        if (const int rc = s.law ? enqueue_law_loop(h, h->lane[0], who, s.B, st.x_hat, st.ref_k, s.extended ? st.gamma : nullptr, st.dead, s.ll,
                                                    s.warm ? s.ws : nullptr)
                                 : enqueue(h, h->lane[0], {s.B, st.x_hat, st.ref_k, s.extended ? st.gamma : nullptr, h->d_u, h->d_x0, h->d_ss, nullptr,
                                                           h->d_st, h->d_it}, s.warm ? s.ws : nullptr, true))
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

// the _ref steps need a session opened in full-reference mode; refusing one leaves the session as it is
bool ref_step_barred(tmpc_handle *h, const char *who) {
    if (!h->ses.open || h->ses.full_ref) return false;      // (no session: session_step's message)
    h->err = std::string(who) + ": the session was opened without a reference table (tmpc_mc_set_reference_table before tmpc_mc_open)";
    return true;
}

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
    if (rc != TMPC_OK) s.failed = true;
    return finish_loop(h, rc);
}

// Opens the stepped loop `q` describes (checked by check_tracking_loop): carves the session's arrays -- and what `more` lists behind them,
// pieces of a caller that drives the session itself -- and waits for the uploads, which read the caller's arrays.
template <class More>
int open_session(tmpc_handle *h, const TrackingLoop &q, More more) {
    if (const int rc = begin_loop(h, q.B)) return rc;
    const size_t nx = h->nx, nu = h->nu, b = static_cast<size_t>(q.B);
    McSession &s = h->ses;
    s.law = false;
    s.ll = tmpc::LawLoop{};
    if (q.law) {
        if (const int rc = law_loop_begin(h, q.who, q.extended ? 2 : 1, s.ll)) return rc;
        s.law = true;
    }
    auto open = [&]() -> int {
        s.m = tmpc::McModel{}; s.st = tmpc::McState{}; s.ext = tmpc::McExternal{};
        s.warm = h->loop.warm != 0;
        tracking_pieces(h, q, s.m, s.st, s.ws, &s, &s.ll);
        more(h->arena, s);
        HIP_TRY(h, h->arena.carve(h->stream));
        link_block_carved(s.st, b);
        HIP_TRY(h, tmpc::launch_mc_pre(s.m, s.st, q.B, q.full_ref ? 0.0 : q.ref[0], h->stream));
        HIP_TRY(h, hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
        HIP_TRY(h, hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
        // (the pinned block is a convenience: without it tmpc_mc_step copies from / to the caller's memory)
        if (hipHostMalloc(reinterpret_cast<void **>(&s.pin), b * (nx + nu + (q.full_ref ? nx : 0)) * 8, hipHostMallocDefault) != hipSuccess) {
            s.pin = nullptr;
            (void)hipGetLastError();
        }
        HIP_TRY(h, sync_lanes(h));       // the uploads read the caller's arrays, which are theirs again from here on
        return TMPC_OK;
    };
    if (const int rc = finish_loop(h, open())) {
        release_session(h);
        return rc;
    }
    if (q.full_ref) s.ref.assign(static_cast<size_t>(q.T), 0.0);       // (not read on the device in full-reference mode)
    else s.ref.assign(q.ref, q.ref + q.T);
    s.full_ref = q.full_ref;
    s.B = q.B; s.T = q.T; s.t = 0; s.extended = q.extended ? 1 : 0;
    s.open = true;
    return TMPC_OK;
}

// The statistics of the open session over the steps taken, copied out behind what is enqueued; the session stays open.
int fetch_session_results(tmpc_handle *h, double *err2, int32_t *tube_viol, int32_t *x_viol, int32_t *u_viol, int32_t *not_optimal, double *consistent,
                          int32_t *iters_sum) {
    McSession &s = h->ses;
    HIP_TRY(h, hipSetDevice(h->device));
    return fetch_tracking_results(h, s.st, s.law ? &s.ll : nullptr, s.B, s.T, err2, consistent, {{tube_viol, s.st.tube_viol}, {x_viol, s.ext.x_viol}, {u_viol, s.ext.u_viol},
                                                                        {not_optimal, s.st.not_optimal}, {iters_sum, s.st.iters_sum}});
}

// Linear plants [B][nx][nx + nu], rows [A_b[i, :] | B_b[i, :]] (tmpc_mc_set_plant_models, tmpc_mc_run_plants): empty if every entry is finite,
// otherwise the message, which names trajectory and entry.
std::string linear_rows_error(const char *who, const double *models, int64_t B, int64_t nx, int64_t nu) {
    const int64_t wid = nx + nu;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t i = 0; i < nx; ++i)
            for (int64_t j = 0; j < wid; ++j)
                if (!std::isfinite(models[(b * nx + i) * wid + j]))
                    return std::string(who) + ": " + (j < nx ? "A" : "B") + "[" + std::to_string(i) + ", " + std::to_string(j < nx ? j : j - nx) +
                           "] of trajectory " + std::to_string(b) + " is not finite";
    return std::string();
}

// A family of plants as tmpc_mc_run_plants and tmpc_plant_step_device take it: kind and shape against (nx, nu); empty, or the message
std::string plant_family_error(const char *who, int kind, int nx, int nu, int substeps) {
    const std::string w = std::string(who) + ": ";
    if (kind != TMPC_PLANT_CARTPOLE && kind != TMPC_PLANT_LINEAR) return w + "kind is TMPC_PLANT_CARTPOLE or TMPC_PLANT_LINEAR";
    if (kind == TMPC_PLANT_CARTPOLE && (nx != 4 || nu != 1)) return w + "the cart-pole plant needs nx = 4, nu = 1";
    if (kind == TMPC_PLANT_CARTPOLE && substeps < 1) return w + "the cart-pole plant needs substeps >= 1";
    if (nx < 1 || nx > 16 || nu < 1 || nu > 16) return w + "need 1 <= nx <= 16 and 1 <= nu <= 16";
    return std::string();
}
// ---- ensemble statistics of the per-step record (tmpc_series.hip; include/tmpc.h: tmpc_mc_series_stats, tmpc_series_stats)
// the output tables in the order of the C entry points; any may be NULL
struct SeriesOut {
    int32_t *i[tmpc::SERIES_INT_TABLES];         // n_alive, n_nan, lost_up, lost_down, adopted, tube, not_optimal, overrun, age_max, iters_max
    int64_t *l[tmpc::SERIES_LONG_TABLES];        // age_sum, iters_sum
    double *d[tmpc::SERIES_REAL_TABLES];         // e_sum, e_max
    double *q;                                   // [T][G][n_q]
    float *kernel_ms;
};
// The argument errors of a reduction, found on the host before anything touches the device: empty, or the message, which names the argument
std::string series_args_error(const char *who, int64_t B, int32_t T, int32_t G, const int32_t *group, int32_t n_q, const double *q) {
    const std::string w = std::string(who) + ": ";
    if (B < 1) return w + "B < 1";
    if (T < 1) return w + "T < 1";
    if (G < 1) return w + "G < 1";
    if (B > 0x7fffffffll) return w + "B is beyond 2^31 - 1 trajectories";
    if (static_cast<int64_t>(T) * G > 0x7fffffffll) return w + "T * G is beyond 2^31 - 1 columns";
    if (n_q < 0 || n_q > TMPC_SER_MAX_Q) return w + "n_q = " + std::to_string(n_q) + " is not in [0, " + std::to_string(TMPC_SER_MAX_Q) + "]";
    if (n_q > 0 && !q) return w + "q is NULL";
    for (int32_t i = 0; i < n_q; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return w + "q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is not in [0, 1]";      // (NaN fails both)
    for (int64_t b = 0; group && b < B; ++b)
        if (group[b] < -1 || group[b] >= G) return w + "group[" + std::to_string(b) + "] = " + std::to_string(group[b]) + " is neither -1 nor in [0, " + std::to_string(G) + ")";
    return std::string();
}
// The reduction of a record that lies on the current device (arguments checked): the member list sorted by group, one launch on `stream`,
// the tables that are wanted copied out.  Its device memory is its own, one block: a handle's arena keeps the record.
int series_reduce(const char *who, std::string &err, const double *d_e, const uint32_t *d_w, int64_t B, int32_t T, int32_t G, const int32_t *group,
                  int32_t n_q, const double *q, const SeriesOut &out, hipStream_t stream) {
    const size_t b_ = static_cast<size_t>(B), g_ = static_cast<size_t>(G), ncol = static_cast<size_t>(T) * g_, nq = static_cast<size_t>(n_q);
    // counting sort of the trajectories by group (stable: ascending b inside a group); -1: in no group
    std::vector<int32_t> start(g_ + 1, 0), member(b_);
    for (size_t b = 0; b < b_; ++b) {
        const int32_t g = group ? group[b] : 0;
        if (g >= 0) ++start[static_cast<size_t>(g) + 1];
    }
    for (size_t g = 0; g < g_; ++g) start[g + 1] += start[g];
    {
        std::vector<int32_t> next(start.begin(), start.end() - 1);
        for (size_t b = 0; b < b_; ++b) {
            const int32_t g = group ? group[b] : 0;
            if (g >= 0) member[static_cast<size_t>(next[static_cast<size_t>(g)]++)] = static_cast<int32_t>(b);
        }
    }
    struct Block {
        char *p = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Block() {
            if (p) (void)hipFree(p);
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        }
    } blk;
    // 8-byte tables first: q | age_sum, iters_sum | e_sum, e_max | e_q | the ten int32 tables | members | group starts
    const size_t off_l = TMPC_SER_MAX_Q * 8, off_d = off_l + tmpc::SERIES_LONG_TABLES * ncol * 8, off_q = off_d + tmpc::SERIES_REAL_TABLES * ncol * 8,
                 off_i = off_q + ncol * nq * 8, off_m = off_i + tmpc::SERIES_INT_TABLES * ncol * 4, off_s = off_m + b_ * 4, total = off_s + (g_ + 1) * 4;
    auto fail = [&](const char *what, hipError_t e) { err = std::string(who) + ": " + what + ": " + hipGetErrorString(e); return TMPC_E_DEVICE; };
    if (hipMalloc(reinterpret_cast<void **>(&blk.p), total) != hipSuccess) {
        (void)hipGetLastError();
        blk.p = nullptr;
        err = std::string(who) + ": out of device memory";
        return TMPC_E_NOMEM;
    }
    hipError_t e = hipSuccess;
    if (n_q > 0 && (e = hipMemcpyAsync(blk.p, q, nq * 8, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail("upload", e);
    if ((e = hipMemcpyAsync(blk.p + off_m, member.data(), b_ * 4, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail("upload", e);
    if ((e = hipMemcpyAsync(blk.p + off_s, start.data(), (g_ + 1) * 4, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail("upload", e);
    tmpc::SeriesStats a{};
    a.B = B; a.T = T; a.G = G; a.n_q = n_q;
    a.e = d_e; a.word = d_w;
    a.member = reinterpret_cast<const int32_t *>(blk.p + off_m); a.start = reinterpret_cast<const int32_t *>(blk.p + off_s);
    a.q = reinterpret_cast<const double *>(blk.p);
    a.out_l = reinterpret_cast<int64_t *>(blk.p + off_l); a.out_d = reinterpret_cast<double *>(blk.p + off_d);
    a.out_q = reinterpret_cast<double *>(blk.p + off_q); a.out_i = reinterpret_cast<int32_t *>(blk.p + off_i);
    for (hipEvent_t &ev : blk.ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipEventRecord(blk.ev[0], stream)) != hipSuccess) return fail("hipEventRecord", e);
    if ((e = tmpc::launch_series_stats(a, stream)) != hipSuccess) return fail("launch", e);
    if ((e = hipEventRecord(blk.ev[1], stream)) != hipSuccess) return fail("hipEventRecord", e);
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail("hipStreamSynchronize", e);
    if (out.kernel_ms && (e = hipEventElapsedTime(out.kernel_ms, blk.ev[0], blk.ev[1])) != hipSuccess) return fail("hipEventElapsedTime", e);
    for (int k = 0; k < tmpc::SERIES_INT_TABLES; ++k)
        if (out.i[k] && (e = hipMemcpy(out.i[k], a.out_i + k * ncol, ncol * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail("copy-out", e);
    for (int k = 0; k < tmpc::SERIES_LONG_TABLES; ++k)
        if (out.l[k] && (e = hipMemcpy(out.l[k], a.out_l + k * ncol, ncol * 8, hipMemcpyDeviceToHost)) != hipSuccess) return fail("copy-out", e);
    for (int k = 0; k < tmpc::SERIES_REAL_TABLES; ++k)
        if (out.d[k] && (e = hipMemcpy(out.d[k], a.out_d + k * ncol, ncol * 8, hipMemcpyDeviceToHost)) != hipSuccess) return fail("copy-out", e);
    if (out.q && n_q > 0 && (e = hipMemcpy(out.q, a.out_q, ncol * nq * 8, hipMemcpyDeviceToHost)) != hipSuccess) return fail("copy-out", e);
    return TMPC_OK;
}
// the record the getters read: is there one of this shape?
bool series_missing(tmpc_handle *h, const char *who, int64_t B, int32_t T) {
    if (h->rec.ser_w && B == h->rec.ser_B && T == h->rec.ser_T) return false;
    h->err = std::string(who) + ": no tracking loop of this B and T has kept its per-step record (tmpc_mc_set_series before tmpc_mc_run, tmpc_mc_run_plants or tmpc_mc_open)";
    return true;
}
}  // namespace

extern "C" {

int tmpc_mc_set_actuator(tmpc_handle *h, int kind) {
    if (!h || session_bars(h, "tmpc_mc_set_actuator")) return TMPC_E_INVALID;
    if (kind != TMPC_ACTUATOR_CONSISTENT && kind != TMPC_ACTUATOR_SMART) { h->err = "tmpc_mc_set_actuator: unknown actuator"; return TMPC_E_INVALID; }
    h->loop.actuator = kind;
    return TMPC_OK;
}

int tmpc_mc_set_plant(tmpc_handle *h, int kind, const double *par7, int substeps) {
    if (!h || session_bars(h, "tmpc_mc_set_plant")) return TMPC_E_INVALID;
    if (kind == TMPC_PLANT_LINEAR) { h->loop.plant = kind; return TMPC_OK; }
    if (kind != TMPC_PLANT_CARTPOLE || !par7 || substeps < 1) { h->err = "tmpc_mc_set_plant: unknown plant or missing parameters"; return TMPC_E_INVALID; }
    if (h->nx != 4 || h->nu != 1) { h->err = "tmpc_mc_set_plant: the cart-pole plant needs nx = 4, nu = 1"; return TMPC_E_INVALID; }
    for (int i = 0; i < 7; ++i) h->loop.plant_par[i] = par7[i];
    h->loop.plant = kind;
    h->loop.plant_substeps = substeps;
    return TMPC_OK;
}

int tmpc_mc_set_plant_models(tmpc_handle *h, int kind, int64_t B, const double *models, int substeps) {
    const char *who = "tmpc_mc_set_plant_models";
    (void)substeps;
    if (!h || session_bars(h, who)) return TMPC_E_INVALID;
    if (!h->regulator) { h->err = std::string(who) + ": only regulator handles (tmpc_reg_run) take a plant per trajectory"; return TMPC_E_UNSUPPORTED; }
    if (B < 0) { h->err = std::string(who) + ": B < 0"; return TMPC_E_INVALID; }
    if (B == 0) {
        h->loop.pm_B = 0;
        h->loop.pm.clear();
        return TMPC_OK;
    }
    if (kind == TMPC_PLANT_CARTPOLE) { h->err = std::string(who) + ": a regulator handle runs linear plants only"; return TMPC_E_INVALID; }
    if (kind != TMPC_PLANT_LINEAR) { h->err = std::string(who) + ": kind is TMPC_PLANT_LINEAR"; return TMPC_E_INVALID; }
    if (!models) { h->err = std::string(who) + ": models is NULL"; return TMPC_E_INVALID; }
    if (const std::string bad = linear_rows_error(who, models, B, h->nx, h->nu); !bad.empty()) { h->err = bad; return TMPC_E_INVALID; }
    h->loop.pm.assign(models, models + static_cast<size_t>(B) * static_cast<size_t>(h->nx * (h->nx + h->nu)));
    h->loop.pm_B = B;
    return TMPC_OK;
}

int tmpc_mc_set_capture(tmpc_handle *h, int64_t index) {
    if (!h || session_bars(h, "tmpc_mc_set_capture")) return TMPC_E_INVALID;
    h->loop.capture = index < 0 ? -1 : index;
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
    if (!h || session_bars(h, "tmpc_mc_set_device_rng")) return TMPC_E_INVALID;
    h->loop.rng_on = on ? 1 : 0;
    h->loop.rng_seed = seed;
    h->loop.rng_first = first_trajectory;
    h->loop.w_bound.assign(static_cast<size_t>(h->nx), 0.0);
    if (on && w_bound)
        for (int i = 0; i < h->nx; ++i) h->loop.w_bound[i] = w_bound[i];
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
    if (!h || session_bars(h, "tmpc_mc_set_reference_table")) return TMPC_E_INVALID;
    if (h->regulator) { h->err = "tmpc_mc_set_reference_table: a regulator handle has no reference"; return TMPC_E_INVALID; }
    if (K < 0) { h->err = "tmpc_mc_set_reference_table: K < 0"; return TMPC_E_INVALID; }
    if (K == 0) {
        h->loop.ref_K = h->loop.ref_T = 0;
        h->loop.ref_B = 0;
        h->loop.ref_tab.clear();
        h->loop.ref_id.clear();
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
    h->loop.ref_tab.assign(table, table + static_cast<size_t>(K) * static_cast<size_t>(T_tab) * static_cast<size_t>(h->nx));
    h->loop.ref_id.swap(ids);
    h->loop.ref_K = K;
    h->loop.ref_T = T_tab;
    h->loop.ref_B = B;
    return TMPC_OK;
}

int tmpc_mc_set_channel(tmpc_handle *h, int64_t B, const double *p_gb, const double *p_bg, const double *e_g, const double *e_b) {
    if (!h || session_bars(h, "tmpc_mc_set_channel")) return TMPC_E_INVALID;
    if (h->regulator) { h->err = "tmpc_mc_set_channel: a regulator handle has no network"; return TMPC_E_INVALID; }
    if (B < 0) { h->err = "tmpc_mc_set_channel: B < 0"; return TMPC_E_INVALID; }
    if (B == 0) {
        h->loop.ch_B = 0;
        h->loop.ch_thr.clear();
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
    h->loop.ch_thr.swap(thr);
    h->loop.ch_B = B;
    return TMPC_OK;
}

int tmpc_mc_get_channel(tmpc_handle *h, int64_t B, double *thr) {
    if (!h || !thr) return TMPC_E_INVALID;
    if (h->loop.ch_B == 0 || B != h->loop.ch_B) { h->err = "tmpc_mc_get_channel: no channel of this batch size is set (tmpc_mc_set_channel)"; return TMPC_E_INVALID; }
    std::memcpy(thr, h->loop.ch_thr.data(), h->loop.ch_thr.size() * sizeof(double));
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

int tmpc_mc_set_series(tmpc_handle *h, int on) {
    if (!h || session_bars(h, "tmpc_mc_set_series")) return TMPC_E_INVALID;
    if (h->regulator) { h->err = "tmpc_mc_set_series: a regulator handle keeps no per-step record"; return TMPC_E_INVALID; }
    h->loop.series = on ? 1 : 0;
    return TMPC_OK;
}

int tmpc_mc_get_series(tmpc_handle *h, int64_t B, int32_t T, double *e, uint32_t *word) {
    if (!h) return TMPC_E_INVALID;
    if (series_missing(h, "tmpc_mc_get_series", B, T)) return TMPC_E_INVALID;
    const size_t n = static_cast<size_t>(B) * static_cast<size_t>(T);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    if (e) HIP_TRY(h, hipMemcpy(e, h->rec.ser_e, n * 8, hipMemcpyDeviceToHost));
    if (word) HIP_TRY(h, hipMemcpy(word, h->rec.ser_w, n * 4, hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_mc_series_stats(tmpc_handle *h, int64_t B, int32_t T, int32_t G, const int32_t *group, int32_t n_q, const double *q, int32_t *n_alive,
                         int32_t *n_nan, int32_t *lost_up, int32_t *lost_down, int32_t *adopted, int32_t *tube, int32_t *not_optimal, int32_t *overrun,
                         int32_t *age_max, int64_t *age_sum, int32_t *iters_max, int64_t *iters_sum, double *e_sum, double *e_max, double *e_q,
                         float *kernel_ms) {
    const char *who = "tmpc_mc_series_stats";
    if (!h) return TMPC_E_INVALID;
    if (const std::string bad = series_args_error(who, B, T, G, group, n_q, q); !bad.empty()) { h->err = bad; return TMPC_E_INVALID; }
    if (series_missing(h, who, B, T)) return TMPC_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    const SeriesOut out{{n_alive, n_nan, lost_up, lost_down, adopted, tube, not_optimal, overrun, age_max, iters_max}, {age_sum, iters_sum}, {e_sum, e_max}, e_q, kernel_ms};
    return series_reduce(who, h->err, h->rec.ser_e, h->rec.ser_w, B, T, G, group, n_q, q, out, h->stream);
}

int tmpc_series_stats(int device, int64_t B, int32_t T, const double *e, const uint32_t *word, int32_t G, const int32_t *group, int32_t n_q,
                      const double *q, int32_t *n_alive, int32_t *n_nan, int32_t *lost_up, int32_t *lost_down, int32_t *adopted, int32_t *tube,
                      int32_t *not_optimal, int32_t *overrun, int32_t *age_max, int64_t *age_sum, int32_t *iters_max, int64_t *iters_sum,
                      double *e_sum, double *e_max, double *e_q, float *kernel_ms) {
    const char *who = "tmpc_series_stats";
    if (std::string bad = series_args_error(who, B, T, G, group, n_q, q); !bad.empty() || !e || !word) {
        if (bad.empty()) bad = std::string(who) + (!e ? ": e is NULL" : ": word is NULL");
        g_create_error = bad;
        return TMPC_E_INVALID;
    }
    if (device < 0) { g_create_error = std::string(who) + ": device < 0: the reduction runs on the GPU"; return TMPC_E_DEVICE; }
    struct Record {
        char *p = nullptr;
        ~Record() { if (p) (void)hipFree(p); }
    } rec;
    const size_t n = static_cast<size_t>(B) * static_cast<size_t>(T);
    auto fail = [&](const char *what, hipError_t err) { g_create_error = std::string(who) + ": " + what + ": " + hipGetErrorString(err); return TMPC_E_DEVICE; };
    if (const hipError_t err = hipSetDevice(device); err != hipSuccess) return fail("hipSetDevice", err);
    if (hipMalloc(reinterpret_cast<void **>(&rec.p), n * 12) != hipSuccess) {
        (void)hipGetLastError();
        rec.p = nullptr;
        g_create_error = std::string(who) + ": out of device memory";
        return TMPC_E_NOMEM;
    }
    if (const hipError_t err = hipMemcpy(rec.p, e, n * 8, hipMemcpyHostToDevice); err != hipSuccess) return fail("upload", err);
    if (const hipError_t err = hipMemcpy(rec.p + n * 8, word, n * 4, hipMemcpyHostToDevice); err != hipSuccess) return fail("upload", err);
    const SeriesOut out{{n_alive, n_nan, lost_up, lost_down, adopted, tube, not_optimal, overrun, age_max, iters_max}, {age_sum, iters_sum}, {e_sum, e_max}, e_q, kernel_ms};
    return series_reduce(who, g_create_error, reinterpret_cast<const double *>(rec.p), reinterpret_cast<const uint32_t *>(rec.p + n * 8), B, T, G, group, n_q, q, out, nullptr);
}

int tmpc_mc_set_law(tmpc_handle *h, int on, int max_tries, int64_t miss_capacity) {
    if (!h || session_bars(h, "tmpc_mc_set_law")) return TMPC_E_INVALID;
    if (h->regulator) { h->err = "tmpc_mc_set_law: a regulator handle is not supported by the explicit law (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    if (miss_capacity < 0) { h->err = "tmpc_mc_set_law: miss_capacity < 0"; return TMPC_E_INVALID; }
    h->loop.law = on ? 1 : 0;
    h->loop.law_max_tries = max_tries;
    h->loop.law_miss_cap = miss_capacity;
    return TMPC_OK;
}

// the law's record the getters read: is there one?
static bool law_record_missing(tmpc_handle *h, const char *who, int64_t B, bool any_B) {
    if (h->rec.law_B > 0 && (any_B || B == h->rec.law_B)) return false;
    h->err = std::string(who) + ": no tracking loop of this B has run through the explicit law (tmpc_mc_set_law before tmpc_mc_run, tmpc_mc_run_plants or tmpc_mc_open)";
    return true;
}

int tmpc_mc_get_law_stats(tmpc_handle *h, int64_t B, int32_t *hits, int64_t *tries, int32_t *region_last) {
    if (!h) return TMPC_E_INVALID;
    if (h->ses.open) { h->err = "tmpc_mc_get_law_stats: a stepped closed loop is open on this handle (tmpc_mc_close first)"; return TMPC_E_INVALID; }
    if (law_record_missing(h, "tmpc_mc_get_law_stats", B, false)) return TMPC_E_INVALID;
    const size_t b = static_cast<size_t>(B);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    static_assert(sizeof(long long) == sizeof(int64_t), "the accumulators are copied as they are");
    if (hits) HIP_TRY(h, hipMemcpy(hits, h->rec.law.hits, b * 4, hipMemcpyDeviceToHost));
    if (tries) HIP_TRY(h, hipMemcpy(tries, h->rec.law.tries, b * 8, hipMemcpyDeviceToHost));
    if (region_last) HIP_TRY(h, hipMemcpy(region_last, h->rec.law.region, b * 4, hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_mc_get_law_misses(tmpc_handle *h, int64_t capacity, int64_t *n_total, double *x_k, double *ref, uint8_t *variant) {
    const char *who = "tmpc_mc_get_law_misses";
    if (!h) return TMPC_E_INVALID;
    if (capacity < 0) { h->err = std::string(who) + ": capacity < 0"; return TMPC_E_INVALID; }
    if (h->ses.open) { h->err = std::string(who) + ": a stepped closed loop is open on this handle (tmpc_mc_close first)"; return TMPC_E_INVALID; }
    if (law_record_missing(h, who, 0, true)) return TMPC_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    unsigned long long total = 0;
    HIP_TRY(h, hipMemcpy(&total, h->rec.law.miss_n, 8, hipMemcpyDeviceToHost));
    if (n_total) *n_total = static_cast<int64_t>(total);
    const size_t rows = static_cast<size_t>(std::min<int64_t>({static_cast<int64_t>(total), static_cast<int64_t>(h->rec.law.miss_cap), capacity})), nx = h->nx;
    if (rows == 0) return TMPC_OK;
    if (x_k || ref) {
        std::vector<double> p(rows * 2 * nx);
        HIP_TRY(h, hipMemcpy(p.data(), h->rec.law.miss_p, p.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rows; ++i) {
            if (x_k) std::copy(p.begin() + i * 2 * nx, p.begin() + i * 2 * nx + nx, x_k + i * nx);
            if (ref) std::copy(p.begin() + i * 2 * nx + nx, p.begin() + (i + 1) * 2 * nx, ref + i * nx);
        }
    }
    if (variant) HIP_TRY(h, hipMemcpy(variant, h->rec.law.miss_var, rows, hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_mc_set_warm_start(tmpc_handle *h, int on) {
    if (!h || session_bars(h, "tmpc_mc_set_warm_start")) return TMPC_E_INVALID;
    h->loop.warm = on ? 1 : 0;
    return TMPC_OK;
}

int tmpc_mc_set_fused(tmpc_handle *h, int mode) {
    if (!h || session_bars(h, "tmpc_mc_set_fused")) return TMPC_E_INVALID;
    if (mode != TMPC_MC_FUSED_OFF && mode != TMPC_MC_FUSED_ON && mode != TMPC_MC_FUSED_AUTO) { h->err = "tmpc_mc_set_fused: mode is TMPC_MC_FUSED_OFF / _ON / _AUTO"; return TMPC_E_INVALID; }
    h->loop.fused = mode;
    return TMPC_OK;
}

int tmpc_mc_last_fused(const tmpc_handle *h) { return h ? h->rec.fused : 0; }

int tmpc_mc_run(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *p_loss, const double *ref,
                const double *th_u, const double *ga_u, const double *w, const double *x0, const double *HZ, const double *hZ,
                int32_t rZ, double *err2, int32_t *tube_viol, int32_t *not_optimal, double *x_final, double *consistent,
                int32_t *iters_sum) {
    return mc_run_impl(h, {"tmpc_mc_run", false, B, T, extended, p_loss, ref, th_u, ga_u, w, x0, {HZ, hZ, rZ}}, err2, tube_viol, not_optimal, x_final, consistent, iters_sum);
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
    return mc_run_impl(h, {"tmpc_mc_run", false, B, T, extended, pl.data(), ref.data(), th.data(), ga.data(), w, x0, {}, {}, {}, &rp}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int tmpc_reg_run(tmpc_handle *h, int64_t B, int32_t T, const double *x0, const double *w,
                 const double *HX, const double *hX, int32_t rX, const double *HU, const double *hU, int32_t rU,
                 const double *HZ, const double *hZ, int32_t rZ,
                 double *cost, int32_t *x_viol, int32_t *u_viol, int32_t *tube_viol, int32_t *not_optimal, int32_t *fail_step,
                 double *x_final, int32_t *iters_sum, int64_t capture, double *cap_x, double *cap_xn, double *cap_u) {
    if (!h) return TMPC_E_INVALID;
    if (h->ses.open) { h->err = "tmpc_reg_run: a stepped closed loop is open on this handle (tmpc_mc_close first)"; return TMPC_E_INVALID; }
    if (!h->regulator) { h->err = "tmpc_reg_run: needs a regulator handle (tmpc_create_regulator); tracking handles run tmpc_mc_run"; return TMPC_E_INVALID; }
    const SetRows X{HX, hX, rX}, U{HU, hU, rU}, Z{HZ, hZ, rZ};
    if (B < 0 || T < 0 || !x0 || rX < 0 || rU < 0 || rZ < 0 || X.missing() || U.missing() || Z.missing()) { h->err = "tmpc_reg_run: NULL argument or negative count"; return TMPC_E_INVALID; }
    if (h->reg_tube && h->hK.empty()) { h->err = "tmpc_reg_run: the tube regulator needs its gain K"; return TMPC_E_INVALID; }
    if (const int r2 = plant_models_fit(h, "tmpc_reg_run", B)) return r2;
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    if (h->nu > 16) { h->err = "tmpc_reg_run: nu <= 16"; return TMPC_E_UNSUPPORTED; }
    if (B == 0 || T == 0) return TMPC_OK;
    if (const int rc = begin_loop(h, B)) return rc;
    if (const int rc = ensure_reg_zero(h, B)) return rc;
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
        set_pieces(a, &m.HX, &m.hX, X, nx);
        set_pieces(a, &m.HU, &m.hU, U, nu);
        set_pieces(a, &m.HZ, &m.hZ, Z, nx);
        a.piece(&st.x, 8 * b * nx, x0);
        a.piece(&st.cost, 8 * b, nullptr, 0);
        if (h->loop.pm_B > 0) a.piece(&st.plant_lin, 8 * h->loop.pm.size(), h->loop.pm.data());      // (a regulator handle's models are linear)
        int32_t **counters[] = {&st.x_viol, &st.u_viol, &st.tube_viol, &st.not_optimal, &st.fail_step, &st.iters_sum};
        for (int32_t **c : counters) a.piece(c, 4 * b, nullptr, c == &st.fail_step ? 0xFF : 0);      // (0xFF bytes: fail_step = -1)
        if (host_w) a.piece(&st.w, 8 * b * t_ * nx, w);
        else if (h->loop.rng_on) rng_fields(h, st.rng_on, st.rng_seed, st.rng_first, &st.w_bound);
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
    return finish_loop(h, run());
}

int tmpc_mc_open(tmpc_handle *h, int64_t B, int32_t T, int extended, const double *p_loss, const double *ref, const double *th_u,
                 const double *ga_u, const double *x0, const double *HZ, const double *hZ, int32_t rZ, const double *HX,
                 const double *hX, int32_t rX, const double *HU, const double *hU, int32_t rU) {
    if (!h) return TMPC_E_INVALID;
    TrackingLoop q{"tmpc_mc_open", true, B, T, extended, p_loss, ref, th_u, ga_u, nullptr, x0, {HZ, hZ, rZ}, {HX, hX, rX}, {HU, hU, rU}};
    if (const int rc = check_tracking_loop(h, q)) return rc;
    return open_session(h, q, [](Arena &, McSession &) {});
}

int tmpc_mc_step_device(tmpc_handle *h, const double *x_t, double *u_t, void *caller_stream) {
    if (!h) return TMPC_E_INVALID;
    return session_step(h, "tmpc_mc_step_device", x_t, u_t, static_cast<hipStream_t>(caller_stream));
}

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

int tmpc_mc_close(tmpc_handle *h, double *err2, int32_t *tube_viol, int32_t *x_viol, int32_t *u_viol, int32_t *not_optimal,
                  double *consistent, int32_t *iters_sum, int32_t *steps_done) {
    if (!h) return TMPC_E_INVALID;
    McSession &s = h->ses;
    if (!s.open) { h->err = "tmpc_mc_close: no stepped closed loop is open on this handle (tmpc_mc_open)"; return TMPC_E_INVALID; }
    const int rc = finish_loop(h, fetch_session_results(h, err2, tube_viol, x_viol, u_viol, not_optimal, consistent, iters_sum));
    if (steps_done) *steps_done = s.t;
    release_session(h);
    return rc;
}

int tmpc_plant_step_device(int device, int kind, int32_t nx, int32_t nu, int64_t B, const double *models, int substeps, const double *x, const double *u,
                           const double *w, double *x_plus, void *stream) {
    const char *who = "tmpc_plant_step_device";
    if (B < 1) { g_create_error = std::string(who) + ": B < 1"; return TMPC_E_INVALID; }
    if (const std::string bad = plant_family_error(who, kind, nx, nu, substeps); !bad.empty()) { g_create_error = bad; return TMPC_E_INVALID; }
    if (!models || !x || !u || !x_plus) { g_create_error = std::string(who) + ": NULL argument"; return TMPC_E_INVALID; }
    // one lane per trajectory (or per state row) reads the whole x of its trajectory and writes x_plus: in place the lanes would race
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), pa = reinterpret_cast<uintptr_t>(x_plus), bytes = static_cast<uintptr_t>(B) * nx * sizeof(double);
    if (xa < pa + bytes && pa < xa + bytes) { g_create_error = std::string(who) + ": x_plus overlaps x (the step is not in place)"; return TMPC_E_INVALID; }
    tmpc::PlantStep a{};
    a.kind = kind; a.nx = nx; a.nu = nu; a.substeps = substeps; a.B = B;
    a.models = models; a.x = x; a.u = u; a.x_plus = x_plus; a.w = w; a.w_stride = nx;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = tmpc::launch_plant_step(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) { g_create_error = std::string(who) + ": " + hipGetErrorString(e); return TMPC_E_DEVICE; }
    return TMPC_OK;
}

int tmpc_mc_run_plants(tmpc_handle *h, int64_t B, int32_t T, int extended, int kind, const double *models, int substeps, const double *p_loss,
                       const double *ref, const double *th_u, const double *ga_u, const double *w, const double *x0, const double *HZ, const double *hZ,
                       int32_t rZ, const double *HX, const double *hX, int32_t rX, const double *HU, const double *hU, int32_t rU, double *err2,
                       int32_t *tube_viol, int32_t *x_viol, int32_t *u_viol, int32_t *not_optimal, double *x_final, double *consistent, int32_t *iters_sum,
                       double *err2_phys) {
    const char *who = "tmpc_mc_run_plants";
    if (!h) return TMPC_E_INVALID;
    auto refuse = [&](const std::string &msg) { h->err = std::string(who) + ": " + msg; return TMPC_E_INVALID; };
    // the arguments of its own, then those of a session (check_tracking_loop, which also finds a host-only handle); nothing is launched
    // and no setting changes before the last of them
    if (h->ses.open) return refuse("a stepped closed loop is open on this handle (tmpc_mc_close first)");
    if (h->regulator) return refuse("a regulator handle has no tracking loop (tmpc_reg_run with tmpc_mc_set_plant_models)");
    if (B < 1 || T < 1) return refuse("need B >= 1 and T >= 1");
    if (const std::string bad = plant_family_error(who, kind, h->nx, h->nu, substeps); !bad.empty()) { h->err = bad; return TMPC_E_INVALID; }
    if (!models) return refuse("models is NULL");
    const bool rng = h->loop.rng_on != 0, cart = kind == TMPC_PLANT_CARTPOLE;
    if (!rng && !w) return refuse("NULL argument");
    if (h->loop.ref_K > 0)
        if (const int rc = reference_table_fits(h, who, B, T)) return rc;
    const int64_t nx = h->nx, wid = h->nx + h->nu;
    if (const std::string bad = cart ? cartpole_rows_error(who, models, B) : linear_rows_error(who, models, B, h->nx, h->nu); !bad.empty()) {
        h->err = bad;
        return TMPC_E_INVALID;
    }
    TrackingLoop q{who, true, B, T, extended, p_loss, ref, th_u, ga_u, nullptr, x0, {HZ, hZ, rZ}, {HX, hX, rX}, {HU, hU, rU}};
    if (const int rc = check_tracking_loop(h, q)) return rc;
    // the session's arena, and behind it the family, the two plant states (the linear step is not in place), the disturbance or its box,
    // and the physics-rate error, which lives in the session's state: a trajectory that stops gets its NaN from the state machines too
    const size_t b_ = static_cast<size_t>(B), t_ = static_cast<size_t>(T), nx_ = static_cast<size_t>(nx);
    double *d_models = nullptr, *d_x[2] = {nullptr, nullptr}, *d_w = nullptr, *d_wb = nullptr;
    const int rc_open = open_session(h, q, [&](Arena &a, McSession &s) {
        a.piece(&d_models, (cart ? b_ * 7 : b_ * nx_ * static_cast<size_t>(wid)) * 8, models);
        a.piece(&d_x[0], b_ * nx_ * 8, x0, 0);
        a.piece(&d_x[1], b_ * nx_ * 8);
        if (rng) a.piece(&d_wb, nx_ * 8, h->loop.w_bound.data());
        else a.piece(&d_w, b_ * t_ * nx_ * 8, w);
        if (cart) a.piece(&s.st.err2_phys, b_ * 8, nullptr, 0);
    });
    if (rc_open != TMPC_OK) return rc_open;
    McSession &s = h->ses;
    auto run = [&]() -> int {
        tmpc::PlantStep p{};
        p.kind = kind; p.nx = h->nx; p.nu = h->nu; p.substeps = substeps; p.B = B;
        p.models = d_models; p.u = s.ext.u_t; p.w_stride = static_cast<int64_t>(t_ * nx_);
        p.rng_on = rng ? 1 : 0; p.rng_seed = h->loop.rng_seed; p.rng_first = h->loop.rng_first; p.w_bound = d_wb;
        p.hold = s.st.dead;
        p.err2_phys = s.st.err2_phys; p.ref_tab = s.st.ref_tab; p.ref_id = s.st.ref_id; p.ref_T = s.st.ref_T;
        // per step: the solve launch(es) and the state machines around x_t (session_step), then the plants -- all on the handle's stream
        for (int t = 0; t < T; ++t) {
            if (const int rc = session_step(h, who, d_x[t & 1], s.ext.u_t, nullptr)) return rc;
            p.x = d_x[t & 1]; p.x_plus = d_x[(t + 1) & 1];
            p.w = d_w ? d_w + static_cast<size_t>(t) * nx_ : nullptr;
            p.t = t; p.ref_t = s.ref[static_cast<size_t>(t)];
            HIP_TRY(h, tmpc::launch_plant_step(p, h->stream));
        }
        if (x_final) HIP_TRY(h, hipMemcpyAsync(x_final, d_x[T & 1], b_ * nx_ * 8, hipMemcpyDeviceToHost, h->stream));
        if (err2_phys && cart) HIP_TRY(h, hipMemcpyAsync(err2_phys, s.st.err2_phys, b_ * 8, hipMemcpyDeviceToHost, h->stream));
        return fetch_session_results(h, err2, tube_viol, x_viol, u_viol, not_optimal, consistent, iters_sum);
    };
    const int rc = finish_loop(h, run());
    release_session(h);
    return rc;
}

}  // extern "C"
