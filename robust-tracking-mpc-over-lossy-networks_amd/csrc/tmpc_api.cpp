// C ABI of libtmpc_hip.so (declared in include/tmpc.h).  Host side only: condenses the
// problem (tmpc_condense.cpp), keeps it resident in HBM and enqueues the solve kernels
// (tmpc_kernels.hip) on the handle's stream.
#include "tmpc_host.hpp"

using namespace tmpc_host;

namespace {

constexpr size_t LANE_SPARE_EVENTS = 64;

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
    // rows of dense functionals staged in LDS: up to the last one in use, in whole k-steps of the MFMA pass
    auto dense_rows = [&]() {
        const int last = dsing.empty() ? static_cast<int>(dpair.size()) : v.shape.dp * 64 + static_cast<int>(dsing.size());
        return 4 * ((last + 3) / 4);
    };
    // the dense functionals in use must fit the LDS next to the workspaces of the shape's waves
    if (found && tmpc::lds_bytes(v.shape, dense_rows()) > 160 * 1024) found = false;
    if (!found) return TMPC_OK;                                  // wave_ok stays false: the block kernel takes the variant
    // Lane packing (pairs + factored block only).  The factored pairs beyond the last full slot -- 14 of the 206 of the cart-pole's terminal
    // set -- go to idle lanes of the dense paired slots where all of them fit: a factored row is a row of Gs like any other (Hc Psi), a lane of
    // a dense slot costs the same whether it holds a functional or padding, and the kernel then runs the body compiled without the last
    // factored slot (DeviceQP::ncs; only the shapes that hold one: skips_empty_slots).  Paired slots still hold complete pairs only.
    // TMPC_NO_LANE_PACKING=1 keeps the unpacked layout (tests, A/Bs).
    int ncs = v.shape.cp + v.shape.cs;
    {
        const char *e = std::getenv("TMPC_NO_LANE_PACKING");
        const int full = static_cast<int>(cpair.size()) / 64, need = static_cast<int>(cpair.size()) - 64 * full;
        const int idle = 64 * v.shape.dp - static_cast<int>(dpair.size());
        if (use_pairs && use_fact && csing.empty() && full == ncs - 1 && full > 0 && need > 0 && need <= idle && tmpc::skips_empty_slots(v.shape) &&
            !(e && std::atoi(e) != 0)) {
            dpair.insert(dpair.end(), cpair.end() - need, cpair.end());
            cpair.resize(cpair.size() - need);
            if (tmpc::lds_bytes(v.shape, dense_rows()) <= 160 * 1024) {
                ncs = full;
            } else {        // (the two-slot shapes are sized for 96 of their 128 dense rows: back to the unpacked layout)
                cpair.insert(cpair.end(), dpair.end() - need, dpair.end());
                dpair.resize(dpair.size() - need);
            }
        }
    }
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
    // what this layout keeps dense and what factored (tmpc_get_factoring): the rows, not Condensed's split
    d.ncc = 2 * static_cast<int>(cpair.size()) + static_cast<int>(csing.size());
    d.nd = c.nc - d.ncc;
    d.kc = d.ncc > 0 ? kc : 0;
    d.nks = dense_rows() / 4;          // k-steps (4 functionals each) of the MFMA pass over the dense functionals
    d.ncs = ncs;
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
    v.db.nd = c.nc; v.db.ncc = 0; v.db.kc = 0; v.db.nks = 0; v.db.ncs = 0;
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

// A stream and a zeroed work-counter ring for a lane of the handle's device.
int create_lane(tmpc_handle *h, Lane &lane) {
    HIP_TRY(h, hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking));
    lane.wc.size = 4096;
    HIP_TRY(h, hipMalloc(reinterpret_cast<void **>(&lane.wc.ring), lane.wc.size * sizeof(unsigned long long)));
    HIP_TRY(h, hipMemset(lane.wc.ring, 0, lane.wc.size * sizeof(unsigned long long)));
    return TMPC_OK;
}

// Lanes the handle's calls rotate over now
int lanes_in_use(const tmpc_handle *h) { return h->overlap ? std::min(h->lanes, max_lanes(h)) : 1; }

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

// The lane of a tmpc_solve_batch_device call (tmpc_hazard.hpp: pick_lane_policy).  With no RAW, WAW or WAR overlap with the unfinished
// calls of the handle it goes to the next lane of the rotation and may run beside what the other lanes hold; on its own lane it is
// ordered behind whatever that lane holds.  Otherwise it stays on a lane that holds a call it conflicts with, behind it, and that lane
// first waits for the latest end event of every other lane that holds one.  A lane is created by the first call that finds
// unfinished, independent work on every lane in use to run beside ("created": taken into use -- its stream exists since tmpc_create).
int pick_lane(tmpc_handle *h, const tmpc::CallRanges &call, Lane **out) {
    *out = &h->lane[0];
    const int n = lanes_in_use(h);
    if (n <= 1) return TMPC_OK;
    tmpc::LaneView view[tmpc::MAX_LANES];
    for (int l = 0; l < n; ++l) {
        Lane &lane = h->lane[l];
        if (!lane.active) continue;
        prune_finished(lane);
        view[l].exists = true;
        view[l].busy = !lane.inflight.empty();
        view[l].conflicts = conflicts_with_lane(lane, call);
    }
    const tmpc::LanePick pick = tmpc::pick_lane_policy(view, n, h->cur);
    Lane &lane = h->lane[pick.lane];
    if (pick.create) {
        if (!lane.stream)                  // (a lane beyond those of tmpc_create: tmpc_set_call_lanes raised the count)
            if (const int rc = create_lane(h, lane)) return rc;
        lane.active = true;
    }
    for (int l = 0; l < n; ++l)
        if (pick.wait_mask >> l & 1u) HIP_TRY(h, hipStreamWaitEvent(lane.stream, h->lane[l].inflight.back().end, 0));
    if (pick.wait_mask) ++h->lane_waits;
    *out = &lane;
    return TMPC_OK;
}

// Counts a device-pointer call enqueued on `lane` (tmpc_debug_lane_counters[_n]) and makes that lane the current one.  The two-entry
// counter goes by the parity of the lane changes since the lanes were last joined: with two lanes that is the lane itself, and calls in
// rotation alternate between its entries for every number of lanes.
void count_call(tmpc_handle *h, Lane &lane) {
    const int idx = static_cast<int>(&lane - h->lane);
    if (idx != h->cur) h->par ^= 1;
    ++h->par_calls[h->par];
    ++lane.calls;
    h->cur = idx;
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
    count_call(h, lane);
    return TMPC_OK;
}

// The environment's default of a new handle: TMPC_CALL_LANES (1 ... 4).  Read once, here.
void read_lane_settings(tmpc_handle *h) {
    h->lanes = DEFAULT_CALL_LANES;
    if (const char *e = std::getenv("TMPC_CALL_LANES")) h->lanes = std::min(std::max(std::atoi(e), 1), tmpc::MAX_LANES);
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
        read_lane_settings(h);
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
    h->lane[0].active = true;
    h->stream = h->lane[0].stream;
    for (int i = 0; i < 256; ++i) {       // timing events are created up front, not in the solve path
        hipEvent_t a = nullptr, b = nullptr;
        HIP_TRY(h, hipEventCreate(&a));
        HIP_TRY(h, hipEventCreate(&b));
        h->pool.emplace_back(a, b);
    }
    for (int k = 0; k < h->nvariants; ++k)
        if (const int rc = upload_variant(h, h->v[k], p)) return rc;
    read_lane_settings(h);
    // The streams of the other lanes are created here, one after the other, and not by the first call that needs one: the runtime binds a
    // stream to one of the process's few hardware queues (four by default) when it is created, to the one with the fewest streams, and two
    // lanes of a handle on one queue run one after the other -- the launches of one lane then wait behind WHOLE launches of the other.
    // Created together, the lanes of a handle land on different queues; created whenever a burst first needed them, between the streams of
    // other handles, they did not (the headline of `bench.py --full` at 0.93 of the two-lane handle's, measured).  A lane is still taken
    // into use (Lane::active) only by the first call that finds work to run beside.
    for (int l = 1; l < std::min(h->lanes, max_lanes(h)); ++l)
        if (const int rc = create_lane(h, h->lane[l])) return rc;
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

}  // namespace

namespace tmpc_host {

thread_local std::string g_create_error;

// Waits for everything enqueued on the handle, on every lane.
hipError_t sync_lanes(tmpc_handle *h) {
    hipError_t e = hipSuccess;
    for (Lane &l : h->lane)
        if (e == hipSuccess && l.stream) e = hipStreamSynchronize(l.stream);
    if (e == hipSuccess)
        for (Lane &l : h->lane) l.inflight.clear();
    return e;
}

// Orders the primary lane behind what the other lanes have been given, without blocking the host: the start of every entry
// point that runs on the primary lane alone.  Each of them ends with a synchronisation of that lane, which then covers all.
int join_lanes(tmpc_handle *h) {
    for (int l = 1; l < tmpc::MAX_LANES; ++l) {
        Lane &other = h->lane[l];
        if (other.stream && !other.inflight.empty()) HIP_TRY(h, hipStreamWaitEvent(h->stream, other.inflight.back().end, 0));
    }
    h->cur = h->par = 0;
    return TMPC_OK;
}

int max_lanes(const tmpc_handle *h) {
    for (int k = 0; k < h->nvariants; ++k)
        if (use_block(h, h->v[k])) return 2;
    return tmpc::MAX_LANES;
}

// The lane choice and the in-flight record of tmpc_solve_batch_device, for the other entry points that follow its ordering contract
// (tmpc_sens.cpp)
int pick_call_lane(tmpc_handle *h, const tmpc::CallRanges &call, Lane **out) { return pick_lane(h, call, out); }
int note_call(tmpc_handle *h, Lane &lane, const tmpc::CallRanges &call) { return lanes_in_use(h) > 1 ? note_in_flight(h, lane, call) : (count_call(h, lane), TMPC_OK); }

bool use_block(const tmpc_handle *h, const Variant &v) { return h->kernel_path == TMPC_PATH_BLOCK ? v.tiles != 0 : !v.wave_ok; }

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
int enqueue(tmpc_handle *h, Lane &lane, const tmpc::BatchIO &io, int32_t *const *ws, bool variants_valid) {
    { const int rce = begin_timed_launch(h, lane); if (rce) return rce; }
    if (io.variant != nullptr && !variants_valid)      // (the closed loop's selector is its own gamma flags: always 0 or 1)
        HIP_TRY(h, tmpc::launch_mark_invalid_variants(io, h->nvariants, h->nx, h->nu, h->N, lane.stream));
    if (const int rc = enqueue_solves(h, lane, io, ws)) return rc;
    HIP_TRY(h, hipEventRecord(h->ev1, lane.stream));
    h->timed = true;
    return TMPC_OK;
}

int enqueue_solves(tmpc_handle *h, Lane &lane, const tmpc::BatchIO &io, int32_t *const *ws) {
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

}  // namespace tmpc_host

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
    release_sens(h);
    release_law(h);
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
    return lanes_in_use(h) > 1 ? note_in_flight(h, *lane, call) : (count_call(h, *lane), TMPC_OK);
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
    if (!h || session_bars(h, "tmpc_set_kernel_path")) return TMPC_E_INVALID;
    if (path != TMPC_PATH_AUTO && path != TMPC_PATH_WAVE && path != TMPC_PATH_BLOCK) { h->err = "tmpc_set_kernel_path: unknown path"; return TMPC_E_INVALID; }
    for (int k = 0; k < h->nvariants; ++k) {
        if (path == TMPC_PATH_WAVE && !h->v[k].wave_ok && h->device >= 0) { h->err = "tmpc_set_kernel_path: no wave-per-QP shape covers this problem"; return TMPC_E_UNSUPPORTED; }
        if (path == TMPC_PATH_BLOCK && h->v[k].tiles == 0 && h->device >= 0) { h->err = "tmpc_set_kernel_path: the block kernel needs nv <= 128"; return TMPC_E_UNSUPPORTED; }
    }
    if (h->device >= 0 && path != h->kernel_path) {
        // (a handle with a variant on the block kernel rotates over two lanes: the records of the others must not be left behind)
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, sync_lanes(h));
        h->cur = h->par = 0;
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

int tmpc_set_solve_timing(tmpc_handle *h, int on) {
    if (!h || session_bars(h, "tmpc_set_solve_timing")) return TMPC_E_INVALID;
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

int tmpc_synchronize(tmpc_handle *h) {
    if (!h) return TMPC_E_INVALID;
    if (h->device < 0) return TMPC_OK;
    HIP_TRY(h, sync_lanes(h));
    return TMPC_OK;
}

int tmpc_set_call_overlap(tmpc_handle *h, int on) {
    if (!h || session_bars(h, "tmpc_set_call_overlap")) return TMPC_E_INVALID;
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
    // (count_call: by the parity of the lane changes -- the two lanes of a two-lane handle; calls in rotation alternate for any lane count)
    if (calls_per_lane)
        for (int k = 0; k < 2; ++k) calls_per_lane[k] = h->par_calls[k];
    if (cross_lane_waits) *cross_lane_waits = h->lane_waits;
    if (reset) {
        for (tmpc_host::Lane &l : h->lane) l.calls = 0;
        h->par_calls[0] = h->par_calls[1] = 0;
        h->lane_waits = 0;
    }
    return TMPC_OK;
}

int tmpc_debug_lane_counters_n(tmpc_handle *h, int64_t *calls_per_lane, int64_t *cross_lane_waits, int reset) {
    if (!h) return TMPC_E_INVALID;
    if (calls_per_lane)
        for (int l = 0; l < tmpc::MAX_LANES; ++l) calls_per_lane[l] = h->lane[l].calls;
    return tmpc_debug_lane_counters(h, nullptr, cross_lane_waits, reset);
}

int tmpc_set_call_lanes(tmpc_handle *h, int n) {
    if (!h || session_bars(h, "tmpc_set_call_lanes")) return TMPC_E_INVALID;
    if (n < 1 || n > tmpc::MAX_LANES) { h->err = "tmpc_set_call_lanes: 1 ... TMPC_MAX_LANES lanes"; return TMPC_E_INVALID; }
    if (h->device >= 0 && n != h->lanes) {
        // the records of the lanes that leave the rotation would no longer be looked at: the lanes start empty
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, sync_lanes(h));
        h->cur = h->par = 0;
    }
    h->lanes = n;
    return TMPC_OK;
}

int tmpc_get_call_lanes(const tmpc_handle *h) { return h ? (h->overlap ? std::min(h->lanes, max_lanes(h)) : 1) : TMPC_E_INVALID; }

int tmpc_debug_elastic_grid(const tmpc_handle *h, int32_t n_cu, int32_t lanes, int32_t wpb, int64_t B, int32_t *core, int32_t *eligible) {
    if (!h || n_cu <= 0 || lanes < 1 || lanes > tmpc::MAX_LANES || wpb <= 0) return TMPC_E_INVALID;
    const bool block_variant = max_lanes(h) < tmpc::MAX_LANES;
    const int l = std::min<int>(lanes, max_lanes(h));
    if (core) *core = tmpc::elastic_core(n_cu, l);
    if (eligible) *eligible = tmpc::elastic_eligible(B, n_cu, wpb, block_variant) && tmpc::elastic_core(n_cu, l) < n_cu ? 1 : 0;
    return TMPC_OK;
}

int tmpc_debug_surplus_yields(uint32_t followers, int32_t lanes) { return tmpc::surplus_yields(followers, lanes) ? 1 : 0; }

int tmpc_debug_plan_lanes(int32_t nx, int32_t nu, int32_t N, int32_t lanes, int32_t n_calls, const int64_t *B, const void *const *ptrs,
                          int32_t *lane_out, int32_t *waited_out, int32_t *followers_out) {
    if (!B || !ptrs || !lane_out || nx <= 0 || nu <= 0 || N <= 0 || n_calls < 0 || lanes < 1 || lanes > tmpc::MAX_LANES) return TMPC_E_INVALID;
    // no call of the script finishes: every lane keeps all it was given
    std::vector<tmpc::CallRanges> calls;
    std::vector<int> held[tmpc::MAX_LANES];
    std::vector<int32_t> fol(static_cast<size_t>(n_calls), 0);
    bool exists[tmpc::MAX_LANES] = {true, false, false, false};
    int cur = 0;
    for (int i = 0; i < n_calls; ++i) {
        const void *const *a = ptrs + static_cast<size_t>(i) * 9;
        calls.push_back(tmpc::solve_call_ranges(B[i], nx, nu, N, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]));
        tmpc::LaneView view[tmpc::MAX_LANES];
        for (int l = 0; l < lanes; ++l) {
            view[l].exists = exists[l];
            view[l].busy = !held[l].empty();
            for (int j : held[l]) view[l].conflicts = view[l].conflicts || tmpc::calls_conflict(calls[j], calls[i]);
        }
        const tmpc::LanePick pick = tmpc::pick_lane_policy(view, lanes, cur);
        exists[pick.lane] = true;
        const unsigned beside = tmpc::follower_lanes(pick, view, lanes);
        for (int l = 0; l < lanes; ++l)
            if (beside >> l & 1u)
                for (int j : held[l]) ++fol[j];
        held[pick.lane].push_back(i);
        cur = pick.lane;
        lane_out[i] = pick.lane;
        if (waited_out) waited_out[i] = static_cast<int32_t>(pick.wait_mask);
    }
    if (followers_out) std::copy(fol.begin(), fol.end(), followers_out);
    return TMPC_OK;
}

double tmpc_debug_busy_union(int32_t n, const int32_t *lane, const double *start, const double *end) {
    if (n < 0 || !lane || !start || !end) return -1.0;
    return tmpc::busy_union(static_cast<size_t>(n), [&](size_t i, double *ms) { *ms = end[i] - start[i]; return true; },
                            [&](size_t j, size_t i, double *ms) { *ms = end[i] - end[j]; return true; }, [&](size_t i) { return lane[i]; });
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
    // (tmpc_hazard.hpp: busy_union -- any number of lanes)
    hipError_t bad = hipSuccess;
    bool ok = true;
    const float sum = static_cast<float>(tmpc::busy_union(
        h->pool_used,
        [&](size_t i, double *ms) { float t = 0.f; bad = hipEventElapsedTime(&t, h->pool[i].first, h->pool[i].second); *ms = t; return bad == hipSuccess; },
        [&](size_t j, size_t i, double *ms) { float t = 0.f; bad = hipEventElapsedTime(&t, h->pool[j].second, h->pool[i].second); *ms = t; return bad == hipSuccess; },
        [&](size_t i) { return h->pool_lane[i]; }, &ok));
    if (!ok) HIP_TRY(h, bad);
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
    // the layout the variant's kernel reads: the wave kernel's slots (lane packing moves rows of the low-rank block to the dense class), or
    // the block kernel's, all dense; a host-only handle that no kernel covers has neither and reports the condensed QP's split
    const Variant &v = h->v[variant];
    const bool none = !v.wave_ok && v.tiles == 0;
    const tmpc::DeviceQP &d = use_block(h, v) ? v.db : v.d;
    if (nd) *nd = none ? v.c.nd : d.nd;
    if (ncc) *ncc = none ? v.c.ncc : d.ncc;
    if (kc) *kc = none ? v.c.kc : d.kc;
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

}  // extern "C"
