// Host side of the explicit control law (include/tmpc.h: tmpc_law_*, tmpc_qp_law_eval): the table of critical regions per problem
// variant -- built here in double from working sets, the Cholesky factor of M = G_A H^-1 G_A' of each taken from a QR factorisation -- its
// device copy, and
// the entry points that evaluate it (tmpc_law.hip) alone or in front of the handle's ordinary solve launches.
#include <map>

#include "tmpc_host.hpp"
#include "tmpc_law.hpp"

using namespace tmpc_host;

namespace tmpc_host {

// What a region is built from: the condensed QP in the notation of include/tmpc.h, row-major host arrays
struct LawModel {
    int nv = 0, nc = 0, np = 0, ny = 0, npar = 0;
    std::vector<double> L, Ft, G, F, Eb, g0, Y, Yp, Ep, gp0;       // Ep [npar][np] (zero beyond x_k); H = L L', Ft = L^-1 [F | 0] ([nv][np + 1])
    int nrow() const { return nc + npar; }
    int nrowp() const { return (nrow() + 63) / 64 * 64; }
    int nwords() const { return (nc + 31) / 32; }
};

// One region as uploaded: S [np + 1][nrowp] and K [np + 1][ny], the constants in the last row
struct LawRegion {
    std::vector<uint32_t> words;
    std::vector<double> S, K;
};

// The hops' view of a table (include/tmpc.h): the key of each region's working set and the open-addressed table of ids over the keys
struct LawKeys {
    std::vector<unsigned long long> key;         // [R]; tmpc::LAW_NO_KEY: a region without a working set
    std::vector<int32_t> slot;                   // [n_slot], -1: empty
    static size_t slots_for(size_t R) {          // the power of two >= max(64, 2 R)
        size_t n = 64;
        while (n < 2 * R) n *= 2;
        return n;
    }
    // ids in increasing order at key & (n_slot - 1), linear probing; a key already present keeps the earlier id
    void rebuild() {
        const size_t n = slots_for(key.size());
        slot.assign(n, -1);
        for (size_t id = 0; id < key.size(); ++id) {
            if (key[id] == tmpc::LAW_NO_KEY) continue;
            size_t j = key[id] & (n - 1);
            while (slot[j] >= 0 && key[slot[j]] != key[id]) j = (j + 1) & (n - 1);
            if (slot[j] < 0) slot[j] = static_cast<int32_t>(id);
        }
    }
    int32_t find(unsigned long long k) const {
        if (slot.empty()) return -1;
        const size_t n = slot.size();
        for (size_t j = k & (n - 1), c = 0; c < n; ++c, j = (j + 1) & (n - 1)) {
            if (slot[j] < 0) return -1;
            if (key[slot[j]] == k) return slot[j];
        }
        return -1;
    }
};

unsigned long long key_of_words(const uint32_t *words, int nw) {
    unsigned long long k = 0;
    for (int w = 0; w < nw; ++w)
        for (int bit = 0; bit < 32; ++bit)
            if (words[w] >> bit & 1u) k ^= tmpc::law_key_bit(w * 32 + bit);
    return k;
}

struct LawVariant {
    bool ready = false;
    LawModel m;
    std::vector<LawRegion> regions;
    std::map<std::vector<uint32_t>, int32_t> index;
    std::vector<int32_t> order;
    LawKeys keys;                // rebuilt wherever `regions` changes; tmpc_law_reorder leaves it alone
    // the device copy: room for `cap` regions
    int cap = 0;
    double *dS = nullptr, *dK = nullptr;
    int32_t *dorder = nullptr;
    unsigned long long *dhits = nullptr;
    unsigned long long *dkey = nullptr;          // [cap]
    int32_t *dslot = nullptr;                    // [LawKeys::slots_for(cap)]
    void rebuild_keys() {
        keys.key.resize(regions.size());
        for (size_t r = 0; r < regions.size(); ++r) keys.key[r] = key_of_words(regions[r].words.data(), static_cast<int>(regions[r].words.size()));
        keys.rebuild();
    }
    void release_device() {
        for (void *p : {static_cast<void *>(dS), static_cast<void *>(dK), static_cast<void *>(dorder), static_cast<void *>(dhits), static_cast<void *>(dkey),
                        static_cast<void *>(dslot)})
            if (p) (void)hipFree(p);
        dS = dK = nullptr; dorder = nullptr; dhits = nullptr; dkey = nullptr; dslot = nullptr; cap = 0;
    }
};

struct LawState {
    LawVariant v[2];
    double *dAB = nullptr;       // A [nx][nx] | B [nx][nu] for the nominal trajectory
    tmpc::LawTable *dtab = nullptr;          // the two tables' descriptions as the kernel reads them, rewritten whenever a table changes
    int max_hops = 0;            // tmpc_law_set_hops
    unsigned long long *dstats = nullptr;    // [2][LAW_HOP_STATS] the hops' counters per variant, allocated with dtab
    DeviceBuffer todo[tmpc::MAX_LANES];   // the selector bytes of a tmpc_law_solve call, one buffer per launch lane
    DeviceBuffer stage;          // the host-pointer entries' device copies
};

void release_law(tmpc_handle *h) {
    LawState *s = h->law;
    if (!s) return;
    if (h->device >= 0) {
        for (LawVariant &v : s->v) v.release_device();
        if (s->dAB) (void)hipFree(s->dAB);
        if (s->dtab) (void)hipFree(s->dtab);
        if (s->dstats) (void)hipFree(s->dstats);
        for (DeviceBuffer &b : s->todo) b.release();
        s->stage.release();
    }
    delete s;
    h->law = nullptr;
}

}  // namespace tmpc_host

namespace {

using tmpc::Mat;

// x := L^-1 x (forward) or L^-T x (backward) for the lower-triangular factor L [n][n]
void lower_solve(const std::vector<double> &L, int n, double *x, bool transposed) {
    if (!transposed) {
        for (int i = 0; i < n; ++i) {
            double s = x[i];
            for (int t = 0; t < i; ++t) s -= L[static_cast<size_t>(i) * n + t] * x[t];
            x[i] = s / L[static_cast<size_t>(i) * n + i];
        }
    } else {
        for (int i = n - 1; i >= 0; --i) {
            double s = x[i];
            for (int t = i + 1; t < n; ++t) s -= L[static_cast<size_t>(t) * n + i] * x[t];
            x[i] = s / L[static_cast<size_t>(i) * n + i];
        }
    }
}

// The derived parts of a model whose G, F, Eb, g0, Y, Yp, Ep, gp0 and sizes are set; "" or what is wrong with H
std::string finish_model(LawModel &m, const double *H) {
    const size_t nv = m.nv, np = m.np, np1 = np + 1;
    for (size_t i = 0; i < nv * nv; ++i)
        if (!std::isfinite(H[i])) return "H has a non-finite entry";
    m.L.assign(H, H + nv * nv);
    for (size_t i = 0; i < nv; ++i)
        for (size_t j = 0; j < i; ++j) m.L[i * nv + j] = m.L[j * nv + i] = 0.5 * (H[i * nv + j] + H[j * nv + i]);
    if (!chol(m.L, m.nv)) return "H is not positive definite";
    m.Ft.assign(nv * np1, 0.0);
    std::vector<double> col(nv);
    for (size_t q = 0; q < np; ++q) {
        for (size_t i = 0; i < nv; ++i) col[i] = m.F[i * np + q];
        lower_solve(m.L, m.nv, col.data(), false);
        for (size_t i = 0; i < nv; ++i) m.Ft[i * np1 + q] = col[i];
    }
    return std::string();
}

// The law of the working set `words` (bit i: row i): false when the rows of the set are dependent or a bit lies beyond nc.
// With H = L L' and V = L^-1 G_A' the matrix M = G_A H^-1 G_A' is V'V, and its Cholesky factor is the R of V = Q R: it is taken from a
// Householder factorisation of V and M is never formed -- cond(M) reaches 5e11 on the working sets of the cart-pole, and the multipliers
// from a factorisation of M itself leave 1e-8 in u_nom, where this order leaves 1e-12.  In w = L'z the conditions read
// w = -(Ft p + V lambda), V'w = Ebar_A p + g0_A, so  R lambda = -(Q'Ft p + R^-T (Ebar_A p + g0_A)).
bool build_region(const LawModel &m, const uint32_t *words, LawRegion &out) {
    const int nv = m.nv, nc = m.nc, np = m.np, ny = m.ny, np1 = np + 1, nrowp = m.nrowp();
    std::vector<int> A;
    for (int w = 0; w < m.nwords(); ++w)
        for (int bit = 0; bit < 32; ++bit)
            if (words[w] >> bit & 1u) {
                if (w * 32 + bit >= nc) return false;
                A.push_back(w * 32 + bit);
            }
    const int k = static_cast<int>(A.size());
    if (k > nv) return false;
    // V [nv][k], a column per row of the set; V0 keeps it, V becomes R (upper triangle) under the reflectors; T = Q'Ft
    std::vector<double> V(static_cast<size_t>(nv) * k), col(static_cast<size_t>(nv));
    for (int j = 0; j < k; ++j) {
        for (int c = 0; c < nv; ++c) col[c] = m.G[static_cast<size_t>(A[j]) * nv + c];
        lower_solve(m.L, nv, col.data(), false);
        for (int c = 0; c < nv; ++c) V[static_cast<size_t>(c) * k + j] = col[c];
    }
    const std::vector<double> V0 = V;
    std::vector<double> T = m.Ft, hv(static_cast<size_t>(nv));
    double rmax = 0.0;
    for (int j = 0; j < k; ++j) {
        double norm = 0.0;
        for (int c = j; c < nv; ++c) norm = std::hypot(norm, V[static_cast<size_t>(c) * k + j]);
        const double x0 = V[static_cast<size_t>(j) * k + j], alpha = x0 > 0.0 ? -norm : norm;
        rmax = std::max(rmax, norm);
        if (!(norm > 0.0) || !std::isfinite(norm)) return false;
        // v = x - alpha e_j; the reflector I - 2 v v' / v'v
        double vv = 0.0;
        for (int c = j; c < nv; ++c) { hv[c] = V[static_cast<size_t>(c) * k + j]; if (c == j) hv[c] -= alpha; vv += hv[c] * hv[c]; }
        if (vv > 0.0) {
            for (int q = j; q < k; ++q) {
                double s = 0.0;
                for (int c = j; c < nv; ++c) s += hv[c] * V[static_cast<size_t>(c) * k + q];
                s *= 2.0 / vv;
                for (int c = j; c < nv; ++c) V[static_cast<size_t>(c) * k + q] -= s * hv[c];
            }
            for (int q = 0; q < np1; ++q) {
                double s = 0.0;
                for (int c = j; c < nv; ++c) s += hv[c] * T[static_cast<size_t>(c) * np1 + q];
                s *= 2.0 / vv;
                for (int c = j; c < nv; ++c) T[static_cast<size_t>(c) * np1 + q] -= s * hv[c];
            }
        }
        V[static_cast<size_t>(j) * k + j] = alpha;
    }
    for (int j = 0; j < k; ++j)
        if (!(std::fabs(V[static_cast<size_t>(j) * k + j]) > tmpc::LAW_RANK_TOL * rmax)) return false;
    // Kl | kl = -R^-1 (T_1..k + R^-T [Ebar_A | g0_A]), a column at a time
    std::vector<double> Kl(static_cast<size_t>(k) * np1), x(static_cast<size_t>(k));
    for (int q = 0; q < np1; ++q) {
        for (int i = 0; i < k; ++i) {           // R' y = c, forward
            double s = q < np ? m.Eb[static_cast<size_t>(A[i]) * np + q] : m.g0[A[i]];
            for (int t = 0; t < i; ++t) s -= V[static_cast<size_t>(t) * k + i] * x[t];
            x[i] = s / V[static_cast<size_t>(i) * k + i];
        }
        for (int i = 0; i < k; ++i) x[i] = -(x[i] + T[static_cast<size_t>(i) * np1 + q]);
        for (int i = k - 1; i >= 0; --i) {      // R lambda = rhs, backward
            double s = x[i];
            for (int t = i + 1; t < k; ++t) s -= V[static_cast<size_t>(i) * k + t] * x[t];
            x[i] = s / V[static_cast<size_t>(i) * k + i];
        }
        for (int i = 0; i < k; ++i) Kl[static_cast<size_t>(i) * np1 + q] = x[i];
    }
    // Kz | kz = L^-T w, w = -(Ft + V0 [Kl | kl])
    std::vector<double> Kz(static_cast<size_t>(nv) * np1);
    for (int q = 0; q < np1; ++q) {
        for (int c = 0; c < nv; ++c) {
            double s = m.Ft[static_cast<size_t>(c) * np1 + q];
            for (int i = 0; i < k; ++i) s += V0[static_cast<size_t>(c) * k + i] * Kl[static_cast<size_t>(i) * np1 + q];
            col[c] = -s;
        }
        lower_solve(m.L, nv, col.data(), true);
        for (int c = 0; c < nv; ++c) Kz[static_cast<size_t>(c) * np1 + q] = col[c];
    }
    for (double v : Kz)
        if (!std::isfinite(v)) return false;
    out.words.assign(words, words + m.nwords());
    out.K.assign(static_cast<size_t>(np1) * ny, 0.0);
    for (int y = 0; y < ny; ++y)
        for (int q = 0; q < np1; ++q) {
            double s = q < np ? m.Yp[static_cast<size_t>(y) * np + q] : 0.0;
            for (int c = 0; c < nv; ++c) s += m.Y[static_cast<size_t>(y) * nv + c] * Kz[static_cast<size_t>(c) * np1 + q];
            out.K[static_cast<size_t>(q) * ny + y] = s;
        }
    out.S.assign(static_cast<size_t>(np1) * nrowp, 0.0);
    std::vector<int> pos(nc, -1);
    for (int i = 0; i < k; ++i) pos[A[i]] = i;
    for (int i = 0; i < nc; ++i)
        for (int q = 0; q < np1; ++q) {
            double s;
            if (pos[i] >= 0) {
                s = Kl[static_cast<size_t>(pos[i]) * np1 + q] + (q == np ? tmpc::LAW_MULT_TOL : 0.0);
            } else {
                s = q < np ? m.Eb[static_cast<size_t>(i) * np + q] : m.g0[i] + tmpc::LAW_FEAS_TOL;
                for (int c = 0; c < nv; ++c) s -= m.G[static_cast<size_t>(i) * nv + c] * Kz[static_cast<size_t>(c) * np1 + q];
            }
            out.S[static_cast<size_t>(q) * nrowp + i] = s;
        }
    for (int j = 0; j < m.npar; ++j)
        for (int q = 0; q < np1; ++q)
            out.S[static_cast<size_t>(q) * nrowp + nc + j] = q < np ? m.Ep[static_cast<size_t>(j) * np + q] : m.gp0[j] + tmpc::LAW_FEAS_TOL;
    for (int i = m.nrow(); i < nrowp; ++i) out.S[static_cast<size_t>(np) * nrowp + i] = 1.0;
    return true;
}

// The model of variant k of a handle
std::string handle_law_model(const tmpc_handle *h, int k, LawModel &m, int &rc) {
    HostModel hm;
    if (const std::string msg = host_model(h, k, hm, rc); !msg.empty()) return msg;
    const tmpc::Condensed &c = h->v[k].c;
    m.nv = c.nv; m.nc = c.nc; m.np = 2 * c.nx; m.ny = hm.Y.r; m.npar = c.npar;
    m.G = c.G.a; m.F = hm.F.a; m.Eb = hm.Eb.a; m.g0 = c.g0; m.Y = hm.Y.a; m.Yp = hm.Yp.a; m.gp0 = c.gp0;
    m.Ep.assign(static_cast<size_t>(c.npar) * m.np, 0.0);
    for (int j = 0; j < c.npar; ++j)
        for (int i = 0; i < c.nx; ++i) m.Ep[static_cast<size_t>(j) * m.np + i] = c.Ep(j, i);
    rc = TMPC_E_INVALID;
    if (const std::string msg = finish_model(m, c.H.a.data()); !msg.empty()) return msg;
    rc = TMPC_OK;
    return std::string();
}

// Refusals every handle entry shares, in the order of include/tmpc.h; `all_variants`: the call may touch every variant
int check_handle(tmpc_handle *h, const char *who, int variant, bool all_variants) {
    if (session_bars(h, who)) return TMPC_E_INVALID;
    if (h->regulator) { h->err = std::string(who) + ": a regulator handle is not supported (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    if (!all_variants && (variant < 0 || variant >= h->nvariants)) { h->err = std::string(who) + ": variant out of range"; return TMPC_E_INVALID; }
    for (int k = all_variants ? 0 : variant; k < (all_variants ? h->nvariants : variant + 1); ++k)
        if (h->v[k].c.off_aux >= 0) {
            h->err = std::string(who) + ": variant " + std::to_string(k) + " keeps the unpriced auxiliaries of the literal terminal row, which the outputs do not determine (give HTP / hTP)";
            return TMPC_E_UNSUPPORTED;
        }
    return TMPC_OK;
}

int ensure_state(tmpc_handle *h, const char *who) {
    if (!h->law) h->law = new (std::nothrow) LawState;
    if (!h->law) { h->err = std::string(who) + ": out of memory"; return TMPC_E_NOMEM; }
    return TMPC_OK;
}

int ensure_model(tmpc_handle *h, const char *who, int k) {
    if (const int rc = ensure_state(h, who)) return rc;
    LawVariant &v = h->law->v[k];
    if (v.ready) return TMPC_OK;
    int rc = TMPC_OK;
    if (const std::string msg = handle_law_model(h, k, v.m, rc); !msg.empty()) { h->err = std::string(who) + ": " + msg; return rc; }
    v.ready = true;
    return TMPC_OK;
}

int upload_tables(tmpc_handle *h, const char *who);

// A variant's table as the kernels read it
tmpc::LawTable describe(const LawVariant &v) {
    tmpc::LawTable t;
    t.nrow = v.m.nrow(); t.nrowp = v.m.nrowp(); t.R = static_cast<int>(v.regions.size()); t.n_order = static_cast<int>(v.order.size());
    t.S = v.dS; t.K = v.dK; t.order = v.dorder; t.hits = v.dhits;
    t.nc = v.m.nc; t.key = v.dkey; t.slot = v.dslot; t.n_slot = v.regions.empty() ? 0 : static_cast<int>(v.keys.slot.size());
    return t;
}

// The device copy of a variant's table brought up to its host copy.  `first_new`: the regions from there on are new; a table that
// outgrows its blocks moves to larger ones (hit counters carried over).  On TMPC_E_NOMEM nothing has changed on the device.
int sync_device(tmpc_handle *h, const char *who, LawVariant &v, int first_new) {
    const LawModel &m = v.m;
    const size_t sS = static_cast<size_t>(m.np + 1) * m.nrowp(), sK = static_cast<size_t>(m.np + 1) * m.ny, d = sizeof(double);
    const int R = static_cast<int>(v.regions.size());
    if (R > v.cap) {
        const int cap = std::max({R, 2 * v.cap, 16});
        LawVariant n;
        const bool ok = hipMalloc(reinterpret_cast<void **>(&n.dS), std::max<size_t>(cap * sS, 1) * d) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&n.dK), cap * sK * d) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&n.dorder), cap * sizeof(int32_t)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&n.dhits), cap * sizeof(unsigned long long)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&n.dkey), cap * sizeof(unsigned long long)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&n.dslot), LawKeys::slots_for(cap) * sizeof(int32_t)) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            n.release_device();
            h->err = std::string(who) + ": out of device memory";
            return TMPC_E_NOMEM;
        }
        HIP_TRY(h, hipMemset(n.dhits, 0, cap * sizeof(unsigned long long)));
        if (first_new > 0) HIP_TRY(h, hipMemcpy(n.dhits, v.dhits, first_new * sizeof(unsigned long long), hipMemcpyDeviceToDevice));
        v.release_device();
        v.dS = n.dS; v.dK = n.dK; v.dorder = n.dorder; v.dhits = n.dhits; v.dkey = n.dkey; v.dslot = n.dslot; v.cap = cap;
        first_new = 0;                    // (everything is uploaded again)
    }
    for (int r = first_new; r < R; ++r) {
        if (sS) HIP_TRY(h, hipMemcpy(v.dS + r * sS, v.regions[r].S.data(), sS * d, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(v.dK + r * sK, v.regions[r].K.data(), sK * d, hipMemcpyHostToDevice));
    }
    if (R) HIP_TRY(h, hipMemcpy(v.dorder, v.order.data(), R * sizeof(int32_t), hipMemcpyHostToDevice));
    if (R) {                              // (the keys and their hash whole: R + n_slot words)
        HIP_TRY(h, hipMemcpy(v.dkey, v.keys.key.data(), R * sizeof(unsigned long long), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(v.dslot, v.keys.slot.data(), v.keys.slot.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return upload_tables(h, who);
}

// The tables' descriptions on the device, after any change of a table (the lanes are idle)
int upload_tables(tmpc_handle *h, const char *who) {
    LawState &s = *h->law;
    if (!s.dstats) {
        if (hipMalloc(reinterpret_cast<void **>(&s.dstats), 2 * tmpc::LAW_HOP_STATS * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            s.dstats = nullptr;
            h->err = std::string(who) + ": out of device memory";
            return TMPC_E_NOMEM;
        }
        HIP_TRY(h, hipMemset(s.dstats, 0, 2 * tmpc::LAW_HOP_STATS * sizeof(unsigned long long)));
    }
    if (!s.dtab && hipMalloc(reinterpret_cast<void **>(&s.dtab), 2 * sizeof(tmpc::LawTable)) != hipSuccess) {
        (void)hipGetLastError();
        s.dtab = nullptr;
        h->err = std::string(who) + ": out of device memory";
        return TMPC_E_NOMEM;
    }
    tmpc::LawTable t[2];
    for (int k = 0; k < 2; ++k) t[k] = describe(s.v[k]);
    HIP_TRY(h, hipMemcpy(s.dtab, t, sizeof t, hipMemcpyHostToDevice));
    return TMPC_OK;
}

// Adds the working sets `words` [n][nw_in] to variant k's table (ids: the region of each, -1 refused); returns through n_new how many were new
int add_sets(tmpc_handle *h, const char *who, int k, int64_t n, const uint32_t *words, int nw_in, int32_t *ids, int64_t *n_new) {
    if (const int rc = ensure_model(h, who, k)) return rc;
    LawVariant &v = h->law->v[k];
    const int nw = v.m.nwords(), first_new = static_cast<int>(v.regions.size());
    std::vector<uint32_t> key(nw);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t *w = words + i * nw_in;
        bool beyond = h->v[k].c.always_infeasible;
        for (int j = nw; j < nw_in; ++j) beyond |= w[j] != 0u;
        if (beyond) { if (ids) ids[i] = -1; continue; }
        std::copy(w, w + std::min(nw, nw_in), key.begin());
        if (const auto it = v.index.find(key); it != v.index.end()) { if (ids) ids[i] = it->second; continue; }
        LawRegion reg;
        if (!build_region(v.m, key.data(), reg)) { if (ids) ids[i] = -1; continue; }
        const int32_t id = static_cast<int32_t>(v.regions.size());
        v.regions.push_back(std::move(reg));
        v.index.emplace(key, id);
        v.order.push_back(id);
        if (ids) ids[i] = id;
    }
    const int added = static_cast<int>(v.regions.size()) - first_new;
    if (n_new) *n_new = added;
    if (added == 0) return TMPC_OK;
    v.rebuild_keys();
    if (h->device < 0) return TMPC_OK;
    const int rc = sync_device(h, who, v, first_new);
    if (rc == TMPC_E_NOMEM) {             // the table as it was
        for (int r = first_new; r < static_cast<int>(v.regions.size()); ++r) v.index.erase(v.regions[r].words);
        v.regions.resize(first_new);
        v.rebuild_keys();
        v.order.erase(std::remove_if(v.order.begin(), v.order.end(), [first_new](int32_t id) { return id >= first_new; }), v.order.end());
        for (int64_t i = 0; ids && i < n; ++i)
            if (ids[i] >= first_new) ids[i] = -1;
        if (n_new) *n_new = 0;
    }
    return rc;
}

// Waits for both lanes: the entries that change a table do so between launches
int quiesce(tmpc_handle *h) {
    if (h->device < 0) return TMPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sync_lanes(h));
    h->cur = h->par = 0;
    return TMPC_OK;
}

// The device arrays of one evaluating call
struct LawCall {
    int64_t B;
    const double *x_k, *ref;
    const uint8_t *variant;
    const int32_t *hint;
    int max_tries;
    double *u_nom, *x_nom0, *xu_ss, *x_nom;
    int32_t *status, *iters, *region, *tries;
    bool fallback;
    // a closed loop's step (enqueue_law_loop): nullptr elsewhere
    const tmpc::LawLoop *loop = nullptr;
    const uint8_t *skip = nullptr;
    int32_t *const *ws = nullptr;
};

int check_call(tmpc_handle *h, const char *who, const LawCall &c) {
    if (!h) return TMPC_E_INVALID;
    if (c.B < 0 || !c.x_k || !c.ref || !c.u_nom || !c.x_nom0 || !c.xu_ss || !c.status || !c.region || (c.fallback && !c.iters)) {
        h->err = std::string(who) + (c.B < 0 ? ": B < 0" : ": NULL argument");
        return TMPC_E_INVALID;
    }
    if (const int rc = check_handle(h, who, 0, c.variant != nullptr)) return rc;
    if (c.B == 0) return TMPC_OK;
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    return TMPC_OK;
}

int enqueue_law(tmpc_handle *h, Lane &lane, const char *who, const LawCall &c) {
    const int nvar = c.variant ? h->nvariants : 1, nx = h->nx, nu = h->nu, N = h->N;
    for (int k = 0; k < nvar; ++k)
        if (const int rc = ensure_model(h, who, k)) return rc;
    LawState &s = *h->law;
    if (c.x_nom && !s.dAB) {
        std::vector<double> ab(h->hA);
        ab.insert(ab.end(), h->hB.begin(), h->hB.end());
        if (hipMalloc(reinterpret_cast<void **>(&s.dAB), ab.size() * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            s.dAB = nullptr;
            h->err = std::string(who) + ": out of device memory";
            return TMPC_E_NOMEM;
        }
        HIP_TRY(h, hipMemcpy(s.dAB, ab.data(), ab.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!s.dtab)                         // (no table has been touched yet: everything misses)
        if (const int rc = upload_tables(h, who)) return rc;
    uint8_t *todo = nullptr;
    if (c.fallback) {
        DeviceBuffer &tb = s.todo[&lane - h->lane];
        HIP_TRY(h, tb.reserve(static_cast<size_t>(c.B), lane.stream));
        todo = tb.as<uint8_t>();
    }
    tmpc::LawArgs a{};
    a.np = 2 * nx; a.ny = N * nu + 2 * nx + nu; a.nvariants = nvar;
    a.t = s.dtab;
    a.B = c.B; a.np0 = nx; a.P0 = c.x_k; a.P1 = c.ref; a.variant = c.variant; a.hint = c.hint; a.max_tries = c.max_tries;
    a.ny0 = N * nu; a.ny1 = nx; a.Y0 = c.u_nom; a.Y1 = c.x_nom0; a.Y2 = c.xu_ss;
    a.x_nom = c.x_nom; a.A = s.dAB; a.Bm = s.dAB ? s.dAB + static_cast<size_t>(nx) * nx : nullptr; a.nx = nx; a.nu = nu; a.N = N;
    a.status = c.status; a.iters = c.iters; a.region = c.region; a.tries = c.tries; a.todo = todo; a.fallback = c.fallback ? 1 : 0;
    a.max_hops = c.loop ? c.loop->max_hops : s.max_hops; a.hop_stats = s.dstats;
    if (c.loop) {
        a.skip = c.skip; a.acc_hits = c.loop->hits; a.acc_tries = c.loop->tries;
        a.miss_n = c.loop->miss_n; a.miss_cap = c.loop->miss_cap; a.miss_p = c.loop->miss_p; a.miss_var = c.loop->miss_var;
    }
    if (const int rc = begin_timed_launch(h, lane)) return rc;       // (tmpc_last_kernel_ms reads the pair)
    HIP_TRY(h, tmpc::launch_law(a, tmpc::law_blocks(c.B, h->n_cu), lane.stream));
    if (c.fallback)                       // the handle's ordinary solve launches, the misses selected by `todo`
        if (const int rc = enqueue_solves(h, lane, {c.B, c.x_k, c.ref, todo, c.u_nom, c.x_nom0, c.xu_ss, c.x_nom, c.status, c.iters}, c.ws)) return rc;
    HIP_TRY(h, hipEventRecord(h->ev1, lane.stream));
    h->timed = true;
    return TMPC_OK;
}

tmpc::CallRanges law_call_ranges(const tmpc_handle *h, const LawCall &c) {
    const size_t b = static_cast<size_t>(c.B), nx = h->nx, nu = h->nu, N = h->N, d = sizeof(double);
    tmpc::CallRanges r;
    static_assert(tmpc::CallRanges::NR >= 4 && tmpc::CallRanges::NW >= 8, "four arrays read, eight written");
    r.reads[0] = tmpc::byte_range(c.x_k, b * nx * d);
    r.reads[1] = tmpc::byte_range(c.ref, b * nx * d);
    r.reads[2] = tmpc::byte_range(c.variant, b);
    r.reads[3] = tmpc::byte_range(c.hint, b * sizeof(int32_t));
    r.writes[0] = tmpc::byte_range(c.u_nom, b * N * nu * d);
    r.writes[1] = tmpc::byte_range(c.x_nom0, b * nx * d);
    r.writes[2] = tmpc::byte_range(c.xu_ss, b * (nx + nu) * d);
    r.writes[3] = tmpc::byte_range(c.x_nom, b * (N + 1) * nx * d);
    r.writes[4] = tmpc::byte_range(c.status, b * sizeof(int32_t));
    r.writes[5] = tmpc::byte_range(c.iters, b * sizeof(int32_t));
    r.writes[6] = tmpc::byte_range(c.region, b * sizeof(int32_t));
    r.writes[7] = tmpc::byte_range(c.tries, b * sizeof(int32_t));
    auto grow = [&r](const tmpc::ByteRange &x) {
        if (x.lo >= x.hi) return;
        if (r.hull.lo >= r.hull.hi) { r.hull = x; return; }
        r.hull.lo = std::min(r.hull.lo, x.lo);
        r.hull.hi = std::max(r.hull.hi, x.hi);
    };
    for (const tmpc::ByteRange &x : r.reads) grow(x);
    for (const tmpc::ByteRange &x : r.writes) grow(x);
    return r;
}

int call_device(tmpc_handle *h, const char *who, const LawCall &c) {
    if (const int rc = check_call(h, who, c); rc || c.B == 0) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const tmpc::CallRanges call = law_call_ranges(h, c);
    Lane *lane = nullptr;
    if (const int rc = pick_call_lane(h, call, &lane)) return rc;
    if (const int rc = enqueue_law(h, *lane, who, c)) return rc;
    return note_call(h, *lane, call);
}

int call_host(tmpc_handle *h, const char *who, const LawCall &c) {
    if (const int rc = check_call(h, who, c); rc || c.B == 0) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    // the primary lane behind what the secondary lane holds
    if (const int rc = join_lanes(h)) return rc;
    if (const int rc = ensure_state(h, who)) return rc;
    const size_t b = static_cast<size_t>(c.B), nx = h->nx, nu = h->nu, N = h->N, d = sizeof(double);
    struct Part { const void *host_in; void *host_out; size_t bytes; size_t off; };
    Part parts[] = {{c.x_k, nullptr, b * nx * d, 0}, {c.ref, nullptr, b * nx * d, 0}, {c.variant, nullptr, c.variant ? b : 0, 0}, {c.hint, nullptr, c.hint ? b * 4 : 0, 0},
                    {nullptr, c.u_nom, b * N * nu * d, 0}, {nullptr, c.x_nom0, b * nx * d, 0}, {nullptr, c.xu_ss, b * (nx + nu) * d, 0},
                    {nullptr, c.x_nom, c.x_nom ? b * (N + 1) * nx * d : 0, 0}, {nullptr, c.status, b * 4, 0}, {nullptr, c.iters, c.iters ? b * 4 : 0, 0},
                    {nullptr, c.region, b * 4, 0}, {nullptr, c.tries, c.tries ? b * 4 : 0, 0}};
    size_t total = 0;
    for (Part &p : parts) { p.off = total; total += (p.bytes + 255) / 256 * 256; }
    LawState &s = *h->law;
    HIP_TRY(h, s.stage.reserve(std::max<size_t>(total, 256), h->stream));
    char *base = s.stage.p;
    for (const Part &p : parts)
        if (p.host_in && p.bytes) HIP_TRY(h, hipMemcpyAsync(base + p.off, p.host_in, p.bytes, hipMemcpyHostToDevice, h->stream));
    auto at = [&](int i) { return parts[i].bytes ? base + parts[i].off : nullptr; };
    LawCall dc = c;
    dc.x_k = reinterpret_cast<const double *>(at(0)); dc.ref = reinterpret_cast<const double *>(at(1));
    dc.variant = reinterpret_cast<const uint8_t *>(at(2)); dc.hint = reinterpret_cast<const int32_t *>(at(3));
    dc.u_nom = reinterpret_cast<double *>(at(4)); dc.x_nom0 = reinterpret_cast<double *>(at(5)); dc.xu_ss = reinterpret_cast<double *>(at(6));
    dc.x_nom = reinterpret_cast<double *>(at(7)); dc.status = reinterpret_cast<int32_t *>(at(8)); dc.iters = reinterpret_cast<int32_t *>(at(9));
    dc.region = reinterpret_cast<int32_t *>(at(10)); dc.tries = reinterpret_cast<int32_t *>(at(11));
    if (const int rc = enqueue_law(h, h->lane[0], who, dc)) return rc;
    for (const Part &p : parts)
        if (p.host_out && p.bytes) HIP_TRY(h, hipMemcpyAsync(p.host_out, base + p.off, p.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sync_lanes(h));
    return TMPC_OK;
}

int qp_law_eval(const std::string &who, int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G,
                const double *g0, const double *Ebar, const double *Y, const double *Yp, int64_t n_sets, const uint32_t *words, int64_t n_order,
                const int32_t *order, int64_t B, const double *P, const int32_t *hint, int max_tries, double *out_y, int32_t *region, int32_t *tries,
                int max_hops, int64_t *stats);

// The start of the entries that read or change one variant's table
int table_entry(tmpc_handle *h, const char *who, int variant) {
    if (!h) return TMPC_E_INVALID;
    return check_handle(h, who, variant, false);
}

}  // namespace

namespace tmpc_host {

int law_loop_begin(tmpc_handle *h, const char *who, int nvar, tmpc::LawLoop &ll) {
    if (h->regulator) { h->err = std::string(who) + ": a regulator handle is not supported by the explicit law (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    for (int k = 0; k < nvar; ++k)
        if (h->v[k].c.off_aux >= 0) {
            h->err = std::string(who) + ": with the law on (tmpc_mc_set_law), variant " + std::to_string(k) + " keeps the unpriced auxiliaries of the literal terminal row, which the outputs do not determine (give HTP / hTP)";
            return TMPC_E_UNSUPPORTED;
        }
    for (int k = 0; k < nvar; ++k)
        if (const int rc = ensure_model(h, who, k)) return rc;
    if (const int rc = upload_tables(h, who)) return rc;
    for (int k = 0; k < 2; ++k) ll.t[k] = describe(h->law->v[k]);
    ll.max_hops = h->law->max_hops;       // (as it stands now: a session keeps it, like the table)
    ll.hop_stats = h->law->dstats;
    return TMPC_OK;
}

int enqueue_law_loop(tmpc_handle *h, Lane &lane, const char *who, int64_t B, const double *x_hat, const double *ref_k, const uint8_t *variant,
                     const uint8_t *skip, const tmpc::LawLoop &ll, int32_t *const *ws) {
    LawCall c{B, x_hat, ref_k, variant, ll.region, ll.max_tries, h->d_u, h->d_x0, h->d_ss, nullptr, h->d_st, h->d_it, ll.region, nullptr, true};
    c.loop = &ll; c.skip = skip; c.ws = ws;
    return enqueue_law(h, lane, who, c);
}

}  // namespace tmpc_host

extern "C" {

int tmpc_law_add(tmpc_handle *h, int variant, int64_t n_sets, const uint32_t *words, int32_t *ids) {
    if (const int rc = table_entry(h, "tmpc_law_add", variant)) return rc;
    if (n_sets < 0 || (n_sets > 0 && !words)) { h->err = n_sets < 0 ? "tmpc_law_add: n_sets < 0" : "tmpc_law_add: NULL argument"; return TMPC_E_INVALID; }
    if (n_sets == 0) return TMPC_OK;
    if (const int rc = quiesce(h)) return rc;
    return add_sets(h, "tmpc_law_add", variant, n_sets, words, (h->v[variant].c.nc + 31) / 32, ids, nullptr);
}

int tmpc_law_learn(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom, const double *x_nom0,
                   const double *xu_ss, const int32_t *status, double act_tol, int32_t *ids, int64_t *n_new) {
    const char *who = "tmpc_law_learn";
    if (!h) return TMPC_E_INVALID;
    if (B < 0 || !x_k || !ref || !u_nom || !x_nom0 || !xu_ss) { h->err = std::string(who) + (B < 0 ? ": B < 0" : ": NULL argument"); return TMPC_E_INVALID; }
    if (const int rc = check_handle(h, who, 0, variant != nullptr)) return rc;
    if (n_new) *n_new = 0;
    if (B == 0) return TMPC_OK;
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    int nwmax = 0;
    for (int k = 0; k < h->nvariants; ++k) nwmax = std::max(nwmax, (h->v[k].c.nc + 31) / 32);
    const size_t b = static_cast<size_t>(B);
    std::vector<int32_t> flag(b), nact(b);
    std::vector<uint32_t> active(b * std::max(nwmax, 1), 0u);
    if (const int rc = sens_signatures(h, who, B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, flag.data(), nact.data(), active.data())) return rc;
    if (const int rc = quiesce(h)) return rc;
    int64_t total_new = 0;
    for (int k = 0; k < (variant ? h->nvariants : 1); ++k) {
        std::vector<int64_t> idx;
        std::vector<uint32_t> w;
        for (size_t i = 0; i < b; ++i) {
            const bool mine = (variant ? variant[i] : 0) == k, good = !(flag[i] & (TMPC_SENS_SKIPPED | TMPC_SENS_NOT_KKT));
            if (mine && good) {
                idx.push_back(static_cast<int64_t>(i));
                w.insert(w.end(), active.begin() + i * nwmax, active.begin() + (i + 1) * nwmax);
            } else if (mine && ids) {
                ids[i] = -1;
            }
        }
        std::vector<int32_t> got(idx.size(), -1);
        int64_t added = 0;
        if (!idx.empty())
            if (const int rc = add_sets(h, who, k, static_cast<int64_t>(idx.size()), w.data(), nwmax, got.data(), &added)) return rc;
        for (size_t j = 0; ids && j < idx.size(); ++j) ids[idx[j]] = got[j];
        total_new += added;
    }
    for (size_t i = 0; ids && variant && i < b; ++i)
        if (variant[i] >= h->nvariants) ids[i] = -1;
    if (n_new) *n_new = total_new;
    return TMPC_OK;
}

int tmpc_law_eval(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries, double *u_nom,
                  double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries) {
    return call_host(h, "tmpc_law_eval", {B, x_k, ref, variant, hint, max_tries, u_nom, x_nom0, xu_ss, x_nom, status, iters, region, tries, false});
}

int tmpc_law_eval_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries,
                         double *u_nom, double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries) {
    return call_device(h, "tmpc_law_eval_device", {B, x_k, ref, variant, hint, max_tries, u_nom, x_nom0, xu_ss, x_nom, status, iters, region, tries, false});
}

int tmpc_law_solve(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries, double *u_nom,
                   double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries) {
    return call_host(h, "tmpc_law_solve", {B, x_k, ref, variant, hint, max_tries, u_nom, x_nom0, xu_ss, x_nom, status, iters, region, tries, true});
}

int tmpc_law_solve_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const int32_t *hint, int max_tries,
                          double *u_nom, double *x_nom0, double *xu_ss, double *x_nom, int32_t *status, int32_t *iters, int32_t *region, int32_t *tries) {
    return call_device(h, "tmpc_law_solve_device", {B, x_k, ref, variant, hint, max_tries, u_nom, x_nom0, xu_ss, x_nom, status, iters, region, tries, true});
}

int tmpc_law_get_stats(tmpc_handle *h, int variant, int32_t *R, int64_t *hits) {
    if (const int rc = table_entry(h, "tmpc_law_get_stats", variant)) return rc;
    const LawVariant *v = h->law ? &h->law->v[variant] : nullptr;
    const int n = v ? static_cast<int>(v->regions.size()) : 0;
    if (R) *R = n;
    if (!hits || n == 0) return TMPC_OK;
    std::fill(hits, hits + n, 0);
    if (h->device < 0) return TMPC_OK;
    if (const int rc = quiesce(h)) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are copied as they are");
    HIP_TRY(h, hipMemcpy(hits, v->dhits, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_law_reorder(tmpc_handle *h, int variant) {
    if (const int rc = table_entry(h, "tmpc_law_reorder", variant)) return rc;
    if (!h->law || h->law->v[variant].regions.empty()) return TMPC_OK;
    LawVariant &v = h->law->v[variant];
    std::vector<int64_t> hits(v.regions.size(), 0);
    if (const int rc = tmpc_law_get_stats(h, variant, nullptr, hits.data())) return rc;
    std::stable_sort(v.order.begin(), v.order.end(), [&hits](int32_t a, int32_t b) { return hits[a] != hits[b] ? hits[a] > hits[b] : a < b; });
    if (h->device >= 0) HIP_TRY(h, hipMemcpy(v.dorder, v.order.data(), v.order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return TMPC_OK;          // (the table's description is unchanged)
}

int tmpc_law_clear(tmpc_handle *h, int variant) {
    if (const int rc = table_entry(h, "tmpc_law_clear", variant)) return rc;
    if (!h->law) return TMPC_OK;
    if (const int rc = quiesce(h)) return rc;
    LawVariant &v = h->law->v[variant];
    v.regions.clear();
    v.index.clear();
    v.order.clear();
    v.rebuild_keys();
    if (h->device >= 0 && v.dhits) HIP_TRY(h, hipMemset(v.dhits, 0, v.cap * sizeof(unsigned long long)));
    if (h->device >= 0 && h->law->dstats)
        HIP_TRY(h, hipMemset(h->law->dstats + variant * tmpc::LAW_HOP_STATS, 0, tmpc::LAW_HOP_STATS * sizeof(unsigned long long)));
    return h->device >= 0 ? upload_tables(h, "tmpc_law_clear") : TMPC_OK;
}

int tmpc_law_set_hops(tmpc_handle *h, int max_hops) {
    const char *who = "tmpc_law_set_hops";
    if (!h) return TMPC_E_INVALID;
    if (session_bars(h, who)) return TMPC_E_INVALID;
    if (h->regulator) { h->err = std::string(who) + ": a regulator handle is not supported (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    if (max_hops < 0) { h->err = std::string(who) + ": max_hops < 0"; return TMPC_E_INVALID; }
    if (const int rc = ensure_state(h, who)) return rc;
    if (const int rc = quiesce(h)) return rc;
    h->law->max_hops = max_hops;
    return TMPC_OK;
}

int tmpc_law_get_hops(tmpc_handle *h, int *max_hops) {
    const char *who = "tmpc_law_get_hops";
    if (!h) return TMPC_E_INVALID;
    if (h->regulator) { h->err = std::string(who) + ": a regulator handle is not supported (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    if (!max_hops) { h->err = std::string(who) + ": NULL argument"; return TMPC_E_INVALID; }
    *max_hops = h->law ? h->law->max_hops : 0;
    return TMPC_OK;
}

int tmpc_law_get_hop_stats(tmpc_handle *h, int variant, int64_t *stats) {
    if (const int rc = table_entry(h, "tmpc_law_get_hop_stats", variant)) return rc;
    if (!stats) { h->err = "tmpc_law_get_hop_stats: NULL argument"; return TMPC_E_INVALID; }
    std::fill(stats, stats + tmpc::LAW_HOP_STATS, 0);
    if (h->device < 0 || !h->law || !h->law->dstats) return TMPC_OK;
    if (const int rc = quiesce(h)) return rc;
    HIP_TRY(h, hipMemcpy(stats, h->law->dstats + variant * tmpc::LAW_HOP_STATS, tmpc::LAW_HOP_STATS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_law_clear_hop_stats(tmpc_handle *h, int variant) {
    if (const int rc = table_entry(h, "tmpc_law_clear_hop_stats", variant)) return rc;
    if (h->device < 0 || !h->law || !h->law->dstats) return TMPC_OK;
    if (const int rc = quiesce(h)) return rc;
    HIP_TRY(h, hipMemset(h->law->dstats + variant * tmpc::LAW_HOP_STATS, 0, tmpc::LAW_HOP_STATS * sizeof(unsigned long long)));
    return TMPC_OK;
}

int tmpc_law_find_key(tmpc_handle *h, int variant, uint64_t key, int32_t *id) {
    if (const int rc = table_entry(h, "tmpc_law_find_key", variant)) return rc;
    if (!id) { h->err = "tmpc_law_find_key: NULL argument"; return TMPC_E_INVALID; }
    *id = h->law ? h->law->v[variant].keys.find(key) : -1;
    return TMPC_OK;
}

int tmpc_law_get_region(tmpc_handle *h, int variant, int32_t id, uint32_t *words, double *Ky, double *ky, double *S, double *s) {
    if (const int rc = table_entry(h, "tmpc_law_get_region", variant)) return rc;
    const LawVariant *v = h->law ? &h->law->v[variant] : nullptr;
    if (!v || id < 0 || id >= static_cast<int32_t>(v->regions.size())) { h->err = "tmpc_law_get_region: no such region"; return TMPC_E_INVALID; }
    const LawRegion &r = v->regions[id];
    const int np = v->m.np, ny = v->m.ny, nrow = v->m.nrow(), nrowp = v->m.nrowp();
    if (words) std::copy(r.words.begin(), r.words.end(), words);
    for (int y = 0; y < ny; ++y) {
        for (int q = 0; Ky && q < np; ++q) Ky[static_cast<size_t>(y) * np + q] = r.K[static_cast<size_t>(q) * ny + y];
        if (ky) ky[y] = r.K[static_cast<size_t>(np) * ny + y];
    }
    for (int i = 0; i < nrow; ++i) {
        for (int q = 0; S && q < np; ++q) S[static_cast<size_t>(i) * np + q] = r.S[static_cast<size_t>(q) * nrowp + i];
        if (s) s[i] = r.S[static_cast<size_t>(np) * nrowp + i];
    }
    return TMPC_OK;
}

int tmpc_get_param_rows(tmpc_handle *h, int variant, double *gp0, double *Ep) {
    if (!h) return TMPC_E_INVALID;
    if (variant < 0 || variant >= h->nvariants) { h->err = "tmpc_get_param_rows: variant out of range"; return TMPC_E_INVALID; }
    const tmpc::Condensed &c = h->v[variant].c;
    if (gp0 && c.npar) std::memcpy(gp0, c.gp0.data(), c.npar * sizeof(double));
    if (Ep && c.npar) std::memcpy(Ep, c.Ep.a.data(), static_cast<size_t>(c.npar) * c.nx * sizeof(double));
    return TMPC_OK;
}

int tmpc_qp_law_eval(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G, const double *g0,
                     const double *Ebar, const double *Y, const double *Yp, int64_t n_sets, const uint32_t *words, int64_t n_order, const int32_t *order,
                     int64_t B, const double *P, const int32_t *hint, int max_tries, double *out_y, int32_t *region, int32_t *tries) {
    return qp_law_eval("tmpc_qp_law_eval: ", device, nv, nc, np, ny, H, F, G, g0, Ebar, Y, Yp, n_sets, words, n_order, order, B, P, hint, max_tries, out_y, region,
                       tries, 0, nullptr);
}

int tmpc_qp_law_eval_hops(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G, const double *g0,
                          const double *Ebar, const double *Y, const double *Yp, int64_t n_sets, const uint32_t *words, int64_t n_order, const int32_t *order,
                          int64_t B, const double *P, const int32_t *hint, int max_tries, double *out_y, int32_t *region, int32_t *tries, int max_hops,
                          int64_t *stats) {
    return qp_law_eval("tmpc_qp_law_eval_hops: ", device, nv, nc, np, ny, H, F, G, g0, Ebar, Y, Yp, n_sets, words, n_order, order, B, P, hint, max_tries, out_y,
                       region, tries, max_hops, stats);
}

}  // extern "C"

namespace {

int qp_law_eval(const std::string &who, int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G,
                const double *g0, const double *Ebar, const double *Y, const double *Yp, int64_t n_sets, const uint32_t *words, int64_t n_order,
                const int32_t *order, int64_t B, const double *P, const int32_t *hint, int max_tries, double *out_y, int32_t *region, int32_t *tries,
                int max_hops, int64_t *stats) {
    auto refuse = [&](int rc, const std::string &msg) { g_create_error = who + msg; return rc; };
    if (nv < 1 || nv > tmpc::LAW_MAX_NV) return refuse(TMPC_E_INVALID, "nv = " + std::to_string(nv) + " is not in [1, " + std::to_string(tmpc::LAW_MAX_NV) + "]");
    if (nc < 0 || nc > tmpc::LAW_MAX_NC) return refuse(TMPC_E_INVALID, "nc = " + std::to_string(nc) + " is not in [0, 2^20]");
    if (np < 1 || np > tmpc::LAW_MAX_NP) return refuse(TMPC_E_INVALID, "np = " + std::to_string(np) + " is not in [1, " + std::to_string(tmpc::LAW_MAX_NP) + "]");
    if (ny < 1 || ny > tmpc::LAW_MAX_NY) return refuse(TMPC_E_INVALID, "ny = " + std::to_string(ny) + " is not in [1, " + std::to_string(tmpc::LAW_MAX_NY) + "]");
    if (B < 0) return refuse(TMPC_E_INVALID, "B < 0");
    if (max_hops < 0) return refuse(TMPC_E_INVALID, "max_hops < 0");
    if (n_sets < 0 || n_sets > (1 << 20) || n_order < 0 || n_order > (1 << 20)) return refuse(TMPC_E_INVALID, "n_sets and n_order are in [0, 2^20]");
    if (!H || !F || (nc > 0 && (!G || !g0 || !Ebar)) || !Y || !Yp || (n_sets > 0 && nc > 0 && !words) || (n_order > 0 && !order) || !P || !out_y || !region)
        return refuse(TMPC_E_INVALID, "NULL argument");
    for (int64_t i = 0; i < n_order; ++i)
        if (order[i] < 0 || order[i] >= n_sets) return refuse(TMPC_E_INVALID, "order[" + std::to_string(i) + "] is not a set");
    if (stats) std::fill(stats, stats + tmpc::LAW_HOP_STATS, 0);
    if (B == 0) return TMPC_OK;
    if (device < 0) return refuse(TMPC_E_DEVICE, "device < 0: the kernel runs on the GPU");
    LawModel m;
    m.nv = nv; m.nc = nc; m.np = np; m.ny = ny; m.npar = 0;
    const size_t snv = nv, snc = nc, snp = np, sny = ny;
    m.G.assign(G, G + (nc ? snc * snv : 0)); m.F.assign(F, F + snv * snp); m.Eb.assign(Ebar, Ebar + (nc ? snc * snp : 0)); m.g0.assign(g0, g0 + (nc ? snc : 0));
    m.Y.assign(Y, Y + sny * snv); m.Yp.assign(Yp, Yp + sny * snp);
    if (const std::string msg = finish_model(m, H); !msg.empty()) return refuse(TMPC_E_INVALID, msg);
    // the regions; a set that is refused keeps its id with a polyhedron that holds no p
    const size_t sS = (snp + 1) * m.nrowp(), sK = (snp + 1) * sny, R = static_cast<size_t>(n_sets), nw = m.nwords();
    std::vector<double> S(std::max<size_t>(R * sS, 1)), K(std::max<size_t>(R * sK, 1), 0.0);
    const uint32_t none = 0u;
    LawKeys keys;
    keys.key.assign(R, tmpc::LAW_NO_KEY);
    for (size_t r = 0; r < R; ++r) {
        LawRegion reg;
        if (build_region(m, nw ? words + r * nw : &none, reg)) {
            keys.key[r] = key_of_words(nw ? words + r * nw : &none, static_cast<int>(nw));
            std::copy(reg.S.begin(), reg.S.end(), S.begin() + r * sS);
            std::copy(reg.K.begin(), reg.K.end(), K.begin() + r * sK);
        } else {
            if (sS == 0) return refuse(TMPC_E_INVALID, "set " + std::to_string(r) + " is not a working set of a problem without rows");
            std::fill(S.begin() + r * sS, S.begin() + (r + 1) * sS, 0.0);
            std::fill(S.begin() + r * sS + snp * m.nrowp(), S.begin() + (r + 1) * sS, -1.0);
        }
    }
    keys.rebuild();
    const unsigned long long zeros[tmpc::LAW_HOP_STATS] = {0, 0, 0, 0, 0, 0};
    auto fail = [&](const char *what, hipError_t e) { return refuse(TMPC_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); };
    if (const hipError_t e = hipSetDevice(device); e != hipSuccess) return fail("hipSetDevice", e);
    int n_cu = 0;
    if (const hipError_t e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device); e != hipSuccess) return fail("hipDeviceGetAttribute", e);
    struct Owner {
        char *p = nullptr;
        ~Owner() { if (p) (void)hipFree(p); }
    } own;
    const size_t b = static_cast<size_t>(B), d = sizeof(double);
    struct Part { const void *host_in; void *host_out; size_t bytes; size_t off; };
    Part parts[] = {{S.data(), nullptr, R * sS * d, 0}, {K.data(), nullptr, R * sK * d, 0}, {order, nullptr, static_cast<size_t>(n_order) * 4, 0},
                    {P, nullptr, b * snp * d, 0}, {hint, nullptr, hint ? b * 4 : 0, 0}, {nullptr, out_y, b * sny * d, 0}, {nullptr, region, b * 4, 0},
                    {nullptr, tries, tries ? b * 4 : 0, 0}, {nullptr, nullptr, sizeof(tmpc::LawTable), 0},
                    {keys.key.data(), nullptr, R * sizeof(unsigned long long), 0}, {keys.slot.data(), nullptr, keys.slot.size() * sizeof(int32_t), 0},
                    {zeros, stats, sizeof zeros, 0}};
    size_t total = 0;
    for (Part &p : parts) { p.off = total; total += (p.bytes + 255) / 256 * 256; }
    if (hipMalloc(reinterpret_cast<void **>(&own.p), std::max<size_t>(total, 256)) != hipSuccess) {
        (void)hipGetLastError();
        own.p = nullptr;
        return refuse(TMPC_E_NOMEM, "out of device memory");
    }
    for (const Part &p : parts)
        if (p.host_in && p.bytes)
            if (const hipError_t e = hipMemcpy(own.p + p.off, p.host_in, p.bytes, hipMemcpyHostToDevice); e != hipSuccess) return fail("upload", e);
    auto at = [&](int i) { return parts[i].bytes ? own.p + parts[i].off : nullptr; };
    tmpc::LawArgs a{};
    a.np = np; a.ny = ny; a.nvariants = 1;
    tmpc::LawTable t;
    t.nrow = m.nrow(); t.nrowp = m.nrowp(); t.R = static_cast<int>(R); t.n_order = static_cast<int>(n_order);
    t.S = reinterpret_cast<const double *>(at(0)); t.K = reinterpret_cast<const double *>(at(1)); t.order = reinterpret_cast<const int32_t *>(at(2));
    t.nc = nc; t.key = reinterpret_cast<const unsigned long long *>(at(9)); t.slot = reinterpret_cast<const int32_t *>(at(10));
    t.n_slot = R ? static_cast<int>(keys.slot.size()) : 0;
    if (const hipError_t e = hipMemcpy(at(8), &t, sizeof t, hipMemcpyHostToDevice); e != hipSuccess) return fail("upload", e);
    a.t = reinterpret_cast<const tmpc::LawTable *>(at(8));
    a.B = B; a.np0 = np; a.P0 = reinterpret_cast<const double *>(at(3)); a.hint = reinterpret_cast<const int32_t *>(at(4)); a.max_tries = max_tries;
    a.max_hops = max_hops; a.hop_stats = reinterpret_cast<unsigned long long *>(at(11));
    a.ny0 = ny; a.ny1 = 0; a.Y0 = reinterpret_cast<double *>(at(5));
    a.region = reinterpret_cast<int32_t *>(at(6)); a.tries = reinterpret_cast<int32_t *>(at(7));
    if (const hipError_t e = tmpc::launch_law(a, tmpc::law_blocks(B, n_cu), nullptr); e != hipSuccess) return fail("launch", e);
    if (const hipError_t e = hipDeviceSynchronize(); e != hipSuccess) return fail("hipDeviceSynchronize", e);
    for (const Part &p : parts)
        if (p.host_out && p.bytes)
            if (const hipError_t e = hipMemcpy(p.host_out, own.p + p.off, p.bytes, hipMemcpyDeviceToHost); e != hipSuccess) return fail("copy-out", e);
    return TMPC_OK;
}

}  // namespace
