// The offline tools of libtmpc_hip.so, none of which takes a handle: batched support-function LPs (tmpc_lp.hip) and the
// disturbance-set estimate (tmpc_west.hip).
#include "tmpc_host.hpp"
#include "tmpc_west.hpp"

using namespace tmpc_host;

namespace {

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

}  // namespace

namespace tmpc_host {
// The cart-pole rows {M, m, b, I, g, l, Th} of n trajectories (tmpc_estimate_w_models, tmpc_mc_run_plants): empty if every row
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
}  // namespace tmpc_host

extern "C" {

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
