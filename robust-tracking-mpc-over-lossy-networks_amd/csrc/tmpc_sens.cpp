// Host side of the sensitivity entry points (include/tmpc.h: tmpc_sens_jacobian, tmpc_sens_vjp, their _device forms and the handle-free
// tmpc_qp_sensitivity): what does not depend on the instance -- H^-1, W = G H^-1, H^-1 F, the output map (Y, Yp) and, for a handle,
// the map that rebuilds z from the solve's outputs -- is computed here once and kept in one device block; the kernel is tmpc_sens.hip.
#include "tmpc_host.hpp"
#include "tmpc_sens.hpp"

using namespace tmpc_host;

namespace tmpc_host {

// The model part of one variant on the device: one block, the pointers of `a` into it.
struct SensModel {
    bool ready = false;
    char *block = nullptr;
    tmpc::SensArgs a{};
};

// What a handle owns for its sensitivity calls (created by the first one)
struct SensState {
    SensModel m[2];
    DeviceBuffer ws[tmpc::MAX_LANES];     // the kernel's right-hand-side blocks, one slice per workgroup; one buffer per launch lane
    DeviceBuffer stage;          // the host-pointer entries' device copies
    DeviceBuffer wg[tmpc::MAX_LANES];     // tmpc_sens_vjp_weights*: adj | zrec | the partial tiles | Hbar, Fbar per variant; one buffer per launch lane
};

void release_sens(tmpc_handle *h) {
    SensState *s = h->sens;
    if (!s) return;
    for (SensModel &m : s->m)
        if (m.block) (void)hipFree(m.block);
    for (DeviceBuffer &b : s->ws) b.release();
    for (DeviceBuffer &b : s->wg) b.release();
    s->stage.release();
    delete s;
    h->sens = nullptr;
}

// What the explicit law (tmpc_law.cpp) builds its regions with as well
// In-place Cholesky factor (lower triangle) of the symmetric n x n matrix a; false when a pivot is not positive.
bool chol(std::vector<double> &a, int n) {
    for (int j = 0; j < n; ++j) {
        double d = a[static_cast<size_t>(j) * n + j];
        for (int t = 0; t < j; ++t) d -= a[static_cast<size_t>(j) * n + t] * a[static_cast<size_t>(j) * n + t];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double l = std::sqrt(d);
        a[static_cast<size_t>(j) * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double s = a[static_cast<size_t>(i) * n + j];
            for (int t = 0; t < j; ++t) s -= a[static_cast<size_t>(i) * n + t] * a[static_cast<size_t>(j) * n + t];
            a[static_cast<size_t>(i) * n + j] = s / l;
        }
    }
    return true;
}
// x := (L L')^-1 x for one column x of length n
void chol_solve(const std::vector<double> &L, int n, double *x) {
    for (int i = 0; i < n; ++i) {
        double s = x[i];
        for (int t = 0; t < i; ++t) s -= L[static_cast<size_t>(i) * n + t] * x[t];
        x[i] = s / L[static_cast<size_t>(i) * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = x[i];
        for (int t = i + 1; t < n; ++t) s -= L[static_cast<size_t>(t) * n + i] * x[t];
        x[i] = s / L[static_cast<size_t>(i) * n + i];
    }
}
// H^-1 of the symmetric part of the n x n matrix H, symmetrised; "" or what is wrong with H
std::string spd_inverse(const double *H, int n, std::vector<double> &Hinv) {
    const size_t nv = n;
    std::vector<double> L(H, H + nv * nv);
    for (size_t i = 0; i < nv; ++i)
        for (size_t j = 0; j < i; ++j) L[i * nv + j] = L[j * nv + i] = 0.5 * (H[i * nv + j] + H[j * nv + i]);
    for (size_t i = 0; i < nv * nv; ++i)
        if (!std::isfinite(H[i])) return "H has a non-finite entry";
    if (!chol(L, n)) return "H is not positive definite";
    Hinv.assign(nv * nv, 0.0);
    std::vector<double> col(nv);
    for (size_t j = 0; j < nv; ++j) {
        std::fill(col.begin(), col.end(), 0.0);
        col[j] = 1.0;
        chol_solve(L, n, col.data());
        for (size_t i = 0; i < nv; ++i) Hinv[i * nv + j] = col[i];
    }
    for (size_t i = 0; i < nv; ++i)
        for (size_t j = 0; j < i; ++j) Hinv[i * nv + j] = Hinv[j * nv + i] = 0.5 * (Hinv[i * nv + j] + Hinv[j * nv + i]);
    return std::string();
}

}  // namespace tmpc_host

namespace {

using tmpc::Mat;

// (A'A)^-1 A' of a matrix with independent columns; false when they are not
bool left_inverse(const Mat &A, Mat &out) {
    const int r = A.r, c = A.c;
    std::vector<double> N(static_cast<size_t>(c) * c, 0.0);
    for (int i = 0; i < c; ++i)
        for (int j = 0; j < c; ++j) {
            double s = 0.0;
            for (int t = 0; t < r; ++t) s += A(t, i) * A(t, j);
            N[static_cast<size_t>(i) * c + j] = s;
        }
    if (c > 0 && !chol(N, c)) return false;
    out = Mat(c, r);
    std::vector<double> col(static_cast<size_t>(c));
    for (int t = 0; t < r; ++t) {
        for (int i = 0; i < c; ++i) col[i] = A(t, i);
        chol_solve(N, c, col.data());
        for (int i = 0; i < c; ++i) out(i, t) = col[i];
    }
    return true;
}

// The host arrays of a model, raw condensed data: every pointer row-major, Rec may be NULL (z is given)
struct RawModel {
    int nv, nc, np, ny, nzin;
    const double *H, *F, *G, *g0, *Ebar, *Y, *Yp, *Rec;
};

// Computes H^-1, W, H^-1 F and uploads everything as one block ("" on success, else the message; rc says which error)
std::string upload_model(const RawModel &r, SensModel &m, int &rc) {
    const size_t nv = r.nv, nc = r.nc, np = r.np, ny = r.ny;
    rc = TMPC_E_INVALID;
    std::vector<double> Hinv;
    if (const std::string msg = spd_inverse(r.H, r.nv, Hinv); !msg.empty()) return msg;
    std::vector<double> W(nc * nv), HinvF(nv * np);
    for (size_t i = 0; i < nc; ++i)
        for (size_t j = 0; j < nv; ++j) {
            double s = 0.0;
            for (size_t t = 0; t < nv; ++t) s += r.G[i * nv + t] * Hinv[t * nv + j];
            W[i * nv + j] = s;
        }
    for (size_t i = 0; i < nv; ++i)
        for (size_t q = 0; q < np; ++q) {
            double s = 0.0;
            for (size_t t = 0; t < nv; ++t) s += Hinv[i * nv + t] * r.F[t * np + q];
            HinvF[i * np + q] = s;
        }
    std::vector<double> Gt(nc * nv), EbarT(nc * np);
    for (size_t i = 0; i < nc; ++i) {
        for (size_t j = 0; j < nv; ++j) Gt[j * nc + i] = r.G[i * nv + j];
        for (size_t q = 0; q < np; ++q) EbarT[q * nc + i] = r.Ebar[i * np + q];
    }
    // the block: H | Hinv | F | HinvF | G | W | g0 | Ebar | Y | Yp | Rec | Gt | EbarT
    const size_t nrec = r.Rec ? nv * (static_cast<size_t>(r.nzin) + np) : 0;
    const struct { const double *src; size_t n; } parts[] = {{r.H, nv * nv}, {Hinv.data(), nv * nv}, {r.F, nv * np}, {HinvF.data(), nv * np},
                                                              {r.G, nc * nv}, {W.data(), nc * nv}, {r.g0, nc}, {r.Ebar, nc * np},
                                                              {r.Y, ny * nv}, {r.Yp, ny * np}, {r.Rec, nrec},
                                                              {Gt.data(), nc * nv}, {EbarT.data(), nc * np}};
    std::vector<double> blob;
    size_t off[13];
    for (int k = 0; k < 13; ++k) {
        off[k] = blob.size();
        blob.insert(blob.end(), parts[k].src, parts[k].src + parts[k].n);
        blob.resize((blob.size() + 31) / 32 * 32, 0.0);
    }
    if (blob.empty()) blob.resize(32, 0.0);
    if (hipMalloc(reinterpret_cast<void **>(&m.block), blob.size() * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        m.block = nullptr;
        rc = TMPC_E_NOMEM;
        return "out of device memory";
    }
    if (const hipError_t e = hipMemcpy(m.block, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(m.block);
        m.block = nullptr;
        rc = TMPC_E_DEVICE;
        return std::string("upload: ") + hipGetErrorString(e);
    }
    const double *d = reinterpret_cast<const double *>(m.block);
    tmpc::SensArgs &a = m.a;
    a = tmpc::SensArgs{};
    a.nv = r.nv; a.nc = r.nc; a.np = r.np; a.ny = r.ny;
    a.H = d + off[0]; a.Hinv = d + off[1]; a.F = d + off[2]; a.HinvF = d + off[3]; a.G = d + off[4]; a.W = d + off[5]; a.g0 = d + off[6];
    a.Ebar = d + off[7]; a.Y = d + off[8]; a.Yp = d + off[9]; a.Rec = r.Rec ? d + off[10] : nullptr;
    a.Gt = d + off[11]; a.EbarT = d + off[12];
    m.ready = true;
    rc = TMPC_OK;
    return std::string();
}

// Workgroups of a launch over B instances on a card with n_cu compute units: as many as stay resident, at most eight per unit
unsigned sens_blocks(int64_t B, int n_cu, int nv, int np) {
    const size_t lds = tmpc::sens_lds_bytes(nv, np);
    const int64_t per_cu = std::clamp<int64_t>(static_cast<int64_t>((160u << 10) / std::max<size_t>(lds, 1)), 1, 8);
    return static_cast<unsigned>(std::clamp<int64_t>(B, 1, per_cu * std::max(n_cu, 1)));
}

}  // namespace

// The model of variant k of a handle from its condensed form: F = [F1 F2], Ebar = [E 0], the output map and the map back from the outputs
// (HostModel: tmpc_host.hpp)
std::string tmpc_host::host_model(const tmpc_handle *h, int k, HostModel &hm, int &rc) {
    const tmpc::Condensed &c = h->v[k].c;
    const int nx = c.nx, nu = c.nu, N = c.N, nv = c.nv, nc = c.nc, nvf = c.nvf, nth = c.nth, np = 2 * nx, ny = N * nu + 2 * nx + nu;
    rc = TMPC_E_UNSUPPORTED;
    if (c.off_aux >= 0) return "variant " + std::to_string(k) + " keeps the unpriced auxiliaries of the literal terminal row, which the outputs do not determine (give HTP / hTP)";
    if (nv > tmpc::SENS_MAX_NV) return "nv = " + std::to_string(nv) + " is beyond " + std::to_string(tmpc::SENS_MAX_NV);
    if (np > tmpc::SENS_MAX_NP || ny > tmpc::SENS_MAX_NY || nc > tmpc::SENS_MAX_NC) return "the problem is beyond the kernel's limits (2 nx <= 32, ny <= 4096, nc <= 2^20)";
    auto Tz = [&](int i, int j) { return c.Tz.a.empty() ? (i == j ? 1.0 : 0.0) : c.Tz(i, j); };
    auto Tx = [&](int i, int j) { return c.Tx.a.empty() ? 0.0 : c.Tx(i, j); };
    Mat &F = hm.F, &Eb = hm.Eb, &Y = hm.Y, &Yp = hm.Yp, &Rec = hm.Rec;
    F = Mat(nv, np); Eb = Mat(nc, np); Y = Mat(ny, nv); Yp = Mat(ny, np);
    for (int i = 0; i < nv; ++i)
        for (int j = 0; j < nx; ++j) { F(i, j) = c.F1(i, j); F(i, nx + j) = c.F2(i, j); }
    for (int i = 0; i < nc; ++i)
        for (int j = 0; j < nx; ++j) Eb(i, j) = c.E(i, j);
    // y = S z_full (+ x_k for x_nom0 of a fixed x_0), z_full = Tz z + Tx x_k
    Mat S(ny, nvf);
    for (int i = 0; i < N * nu; ++i) S(i, i) = 1.0;
    for (int i = 0; i < nx; ++i) {
        if (c.off_x0 >= 0) S(N * nu + i, c.off_x0 + i) = 1.0;
        else Yp(N * nu + i, i) = 1.0;
    }
    for (int i = 0; i < nx + nu; ++i)
        for (int j = 0; j < nth; ++j) S(N * nu + nx + i, c.off_theta + j) = c.Mth(i, j);
    for (int y = 0; y < ny; ++y)
        for (int t = 0; t < nvf; ++t) {
            const double s = S(y, t);
            if (s == 0.0) continue;
            for (int j = 0; j < nv; ++j) Y(y, j) += s * Tz(t, j);
            for (int j = 0; j < nx; ++j) Yp(y, j) += s * Tx(t, j);
        }
    // back: z_full = Sinv y (theta by least squares from xu_ss), z = Tz^+ (z_full - Tx x_k)
    Mat Mplus;
    rc = TMPC_E_INVALID;
    if (!left_inverse(c.Mth, Mplus)) return "the steady-state parametrisation is rank deficient";
    Mat Sinv(nvf, ny);
    for (int i = 0; i < N * nu; ++i) Sinv(i, i) = 1.0;
    if (c.off_x0 >= 0)
        for (int i = 0; i < nx; ++i) Sinv(c.off_x0 + i, N * nu + i) = 1.0;
    for (int j = 0; j < nth; ++j)
        for (int i = 0; i < nx + nu; ++i) Sinv(c.off_theta + j, N * nu + nx + i) = Mplus(j, i);
    Mat Tzm(nvf, nv), Tplus;
    for (int i = 0; i < nvf; ++i)
        for (int j = 0; j < nv; ++j) Tzm(i, j) = Tz(i, j);
    if (!left_inverse(Tzm, Tplus)) return "the parametrisation of z is rank deficient";
    Rec = Mat(nv, ny + np);
    for (int i = 0; i < nv; ++i)
        for (int t = 0; t < nvf; ++t) {
            const double s = Tplus(i, t);
            if (s == 0.0) continue;
            for (int y = 0; y < ny; ++y) Rec(i, y) += s * Sinv(t, y);
            for (int j = 0; j < nx; ++j) Rec(i, ny + j) -= s * Tx(t, j);
        }
    rc = TMPC_OK;
    return std::string();
}

namespace {

std::string handle_model(tmpc_handle *h, int k, int &rc) {
    HostModel hm;
    if (const std::string msg = host_model(h, k, hm, rc); !msg.empty()) return msg;
    const tmpc::Condensed &c = h->v[k].c;
    const RawModel r{c.nv, c.nc, 2 * c.nx, hm.Y.r, hm.Y.r, c.H.a.data(), hm.F.a.data(), c.G.a.data(), c.g0.data(), hm.Eb.a.data(), hm.Y.a.data(), hm.Yp.a.data(), hm.Rec.a.data()};
    return upload_model(r, h->sens->m[k], rc);
}

// The device arrays of one handle call
struct SensCall {
    int64_t B;
    const double *x_k, *ref;
    const uint8_t *variant;
    const double *u_nom, *x_nom0, *xu_ss;
    const int32_t *status;
    double act_tol;
    int mode;
    const double *ybar;
    double *out;
    int32_t *flag, *n_active;
    uint32_t *active;
    // tmpc_sens_vjp_weights*: the reduction over the batch runs behind each variant's launch, its results land here ([Hbar | Fbar] per variant)
    std::vector<double> *wgrad = nullptr;
};

// Workgroups of the reduction's first kernel: one wave per tile and chunk, as many as there are or a few per compute unit
unsigned wgrad_blocks(int64_t B, int n_cu, int nv, int np) {
    const int64_t work = static_cast<int64_t>(tmpc::sens_wgrad_chunks(B)) * ((nv + 15) / 16) * ((nv + np + 15) / 16);
    return static_cast<unsigned>(std::clamp<int64_t>(work, 1, 32 * static_cast<int64_t>(std::max(n_cu, 1))));
}

int nwords_of(const tmpc_handle *h) {
    int nc = 0;
    for (int k = 0; k < h->nvariants; ++k) nc = std::max(nc, h->v[k].c.nc);
    return (nc + 31) / 32;
}

// Refusals that need no device, in the order of include/tmpc.h; TMPC_OK with B == 0: nothing to do
int check_call(tmpc_handle *h, const char *who, const SensCall &c) {
    if (!h) return TMPC_E_INVALID;
    if (c.B < 0 || !c.x_k || !c.ref || !c.u_nom || !c.x_nom0 || !c.xu_ss || !c.out || !c.flag || !c.n_active || (c.mode == tmpc::SENS_MODE_VJP && !c.ybar)) {
        h->err = std::string(who) + (c.B < 0 ? ": B < 0" : ": NULL argument");
        return TMPC_E_INVALID;
    }
    if (session_bars(h, who)) return TMPC_E_INVALID;
    if (h->regulator) { h->err = std::string(who) + ": a regulator handle is not supported (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    for (int k = 0; k < (c.variant ? h->nvariants : 1); ++k)
        if (h->v[k].c.off_aux >= 0) {
            h->err = std::string(who) + ": variant " + std::to_string(k) + " keeps the unpriced auxiliaries of the literal terminal row, which the outputs do not determine (give HTP / hTP)";
            return TMPC_E_UNSUPPORTED;
        }
    if (c.B == 0) return TMPC_OK;
    if (h->device < 0) { h->err = "host-only handle (device < 0): nothing can be solved without the GPU"; return TMPC_E_DEVICE; }
    return TMPC_OK;
}

// The models of the variants the call uses (built by the first call that needs them), the lane's workspace, and one launch per variant
// on the lane's stream.
int enqueue_sens(tmpc_handle *h, Lane &lane, const char *who, const SensCall &c) {
    if (!h->sens) h->sens = new (std::nothrow) SensState;
    if (!h->sens) { h->err = std::string(who) + ": out of memory"; return TMPC_E_NOMEM; }
    SensState &s = *h->sens;
    DeviceBuffer &wsbuf = s.ws[&lane - h->lane];
    const int nvar = c.variant ? h->nvariants : 1;
    size_t ws = 0;
    for (int k = 0; k < nvar; ++k) {
        if (!s.m[k].ready) {
            int rc = TMPC_OK;
            if (const std::string msg = handle_model(h, k, rc); !msg.empty()) { h->err = std::string(who) + ": " + msg; return rc; }
        }
        const tmpc::SensArgs &a = s.m[k].a;
        if (c.mode == tmpc::SENS_MODE_JACOBIAN) ws = std::max(ws, static_cast<size_t>(sens_blocks(c.B, h->n_cu, a.nv, a.np)) * 2 * a.nv * a.np * sizeof(double));
    }
    if (ws) HIP_TRY(h, wsbuf.reserve(ws, lane.stream));      // (a buffer that grows waits for its lane alone, the only one whose launches use it)
    // the weight gradients' workspace: adj | zrec | partial tiles, used by one variant after the other, and [Hbar | Fbar] of each
    DeviceBuffer &wgbuf = s.wg[&lane - h->lane];
    size_t wg_part = 0, wg_res[2] = {0, 0}, wg_total = 0;
    if (c.wgrad) {
        size_t nvmax = 0, tile = 0;
        for (int k = 0; k < nvar; ++k) {
            const size_t nv = s.m[k].a.nv, N = nv + s.m[k].a.np;
            nvmax = std::max(nvmax, nv);
            tile = std::max(tile, nv * N);
        }
        const size_t vec = (static_cast<size_t>(c.B) * nvmax + 31) / 32 * 32;
        wg_part = 2 * vec;
        wg_total = wg_part + (tmpc::sens_wgrad_chunks(c.B) * tile + 31) / 32 * 32;
        for (int k = 0; k < nvar; ++k) {
            wg_res[k] = wg_total;
            wg_total += (static_cast<size_t>(s.m[k].a.nv) * (s.m[k].a.nv + s.m[k].a.np) + 31) / 32 * 32;
        }
        HIP_TRY(h, wgbuf.reserve(wg_total * sizeof(double), lane.stream));
    }
    const int nx = h->nx, nu = h->nu, N = h->N;
    if (const int rc = begin_timed_launch(h, lane)) return rc;       // (tmpc_last_kernel_ms reads the pair)
    for (int k = 0; k < nvar; ++k) {
        tmpc::SensArgs a = s.m[k].a;
        a.B = c.B;
        a.np0 = nx; a.P0 = c.x_k; a.P1 = c.ref;
        a.nz0 = N * nu; a.nz1 = nx; a.nz2 = nx + nu;
        a.Z0 = c.u_nom; a.Z1 = c.x_nom0; a.Z2 = c.xu_ss;
        a.status = c.status; a.variant = c.variant; a.my_variant = k; a.nvariants = h->nvariants;
        a.act_tol = c.act_tol > 0.0 ? c.act_tol : tmpc::SENS_ACT_TOL;
        a.mode = c.mode; a.ybar = c.ybar; a.out = c.out; a.flag = c.flag; a.n_active = c.n_active; a.active = c.active;
        a.nwords = nwords_of(h);
        a.ws = c.mode == tmpc::SENS_MODE_JACOBIAN ? wsbuf.as<double>() : nullptr;
        if (c.wgrad) {
            a.adj = wgbuf.as<double>();
            a.zrec = a.adj + wg_part / 2;
        }
        HIP_TRY(h, tmpc::launch_sens(a, sens_blocks(c.B, h->n_cu, a.nv, a.np), lane.stream));
        if (c.wgrad) {
            tmpc::SensWgradArgs g{};
            g.nv = a.nv; g.np = a.np; g.B = a.B; g.adj = a.adj; g.zrec = a.zrec; g.np0 = a.np0; g.P0 = a.P0; g.P1 = a.P1; g.flag = a.flag;
            g.variant = a.variant; g.my_variant = k; g.nvariants = a.nvariants;
            g.part = wgbuf.as<double>() + wg_part;
            g.Hbar = wgbuf.as<double>() + wg_res[k];
            g.Fbar = g.Hbar + static_cast<size_t>(a.nv) * a.nv;
            HIP_TRY(h, tmpc::launch_sens_wgrad(g, wgrad_blocks(c.B, h->n_cu, a.nv, a.np), lane.stream));
        }
    }
    HIP_TRY(h, hipEventRecord(h->ev1, lane.stream));
    h->timed = true;
    for (int k = 0; c.wgrad && k < nvar; ++k) {
        const size_t n = static_cast<size_t>(s.m[k].a.nv) * (s.m[k].a.nv + s.m[k].a.np);
        c.wgrad[k].resize(n);
        HIP_TRY(h, hipMemcpyAsync(c.wgrad[k].data(), wgbuf.as<double>() + wg_res[k], n * sizeof(double), hipMemcpyDeviceToHost, lane.stream));
    }
    return TMPC_OK;
}

// The primary lane behind what the secondary lane holds (every entry point that runs on the primary lane alone starts so)
int primary_behind_secondary(tmpc_handle *h) {
    return join_lanes(h);
}

// What a sensitivity call reads and writes, by byte range: the ordering contract of tmpc_solve_batch_device covers these calls too
tmpc::CallRanges sens_call_ranges(const tmpc_handle *h, const SensCall &c) {
    const size_t b = static_cast<size_t>(c.B), nx = h->nx, nu = h->nu, N = h->N, ny = N * nu + 2 * nx + nu, d = sizeof(double);
    tmpc::CallRanges r;
    static_assert(tmpc::CallRanges::NR >= 8 && tmpc::CallRanges::NW >= 4, "eight arrays read, four written");
    r.reads[0] = tmpc::byte_range(c.x_k, b * nx * d);
    r.reads[1] = tmpc::byte_range(c.ref, b * nx * d);
    r.reads[2] = tmpc::byte_range(c.variant, b);
    r.reads[3] = tmpc::byte_range(c.u_nom, b * N * nu * d);
    r.reads[4] = tmpc::byte_range(c.x_nom0, b * nx * d);
    r.reads[5] = tmpc::byte_range(c.xu_ss, b * (nx + nu) * d);
    r.reads[6] = tmpc::byte_range(c.status, b * sizeof(int32_t));
    r.reads[7] = tmpc::byte_range(c.ybar, b * ny * d);
    r.writes[0] = tmpc::byte_range(c.out, b * (c.mode == tmpc::SENS_MODE_VJP ? 2 * nx : ny * 2 * nx) * d);
    r.writes[1] = tmpc::byte_range(c.flag, b * sizeof(int32_t));
    r.writes[2] = tmpc::byte_range(c.n_active, b * sizeof(int32_t));
    r.writes[3] = tmpc::byte_range(c.active, b * static_cast<size_t>(nwords_of(h)) * sizeof(uint32_t));
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

// A _device call takes a launch lane as a tmpc_solve_batch_device call does: the other lane than the call before it when none of its
// arrays meets an unfinished call of that lane (RAW, WAW, WAR), else behind the call it depends on
int call_device(tmpc_handle *h, const char *who, const SensCall &c) {
    if (const int rc = check_call(h, who, c); rc || c.B == 0) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const tmpc::CallRanges call = sens_call_ranges(h, c);
    Lane *lane = nullptr;
    if (const int rc = pick_call_lane(h, call, &lane)) return rc;
    if (const int rc = enqueue_sens(h, *lane, who, c)) return rc;
    if (const int rc = note_call(h, *lane, call)) return rc;
    if (c.wgrad) HIP_TRY(h, hipStreamSynchronize(lane->stream));      // (the reduction's results are in host memory: the call's own lane alone)
    return TMPC_OK;
}

int call_host(tmpc_handle *h, const char *who, const SensCall &c) {
    if (const int rc = check_call(h, who, c); rc || c.B == 0) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (const int rc = primary_behind_secondary(h)) return rc;
    if (!h->sens) h->sens = new (std::nothrow) SensState;
    if (!h->sens) { h->err = std::string(who) + ": out of memory"; return TMPC_E_NOMEM; }
    const size_t b = static_cast<size_t>(c.B), nx = h->nx, nu = h->nu, N = h->N, ny = N * nu + 2 * nx + nu, d = sizeof(double);
    const size_t nw = static_cast<size_t>(nwords_of(h)), nout = c.mode == tmpc::SENS_MODE_VJP ? 2 * nx : ny * 2 * nx;
    // the staging block: inputs x_k | ref | u_nom | x_nom0 | xu_ss | ybar | status | variant, outputs out | flag | n_active | active
    struct Part { const void *host_in; void *host_out; size_t bytes; size_t off; };
    Part parts[] = {{c.x_k, nullptr, b * nx * d, 0}, {c.ref, nullptr, b * nx * d, 0}, {c.u_nom, nullptr, b * N * nu * d, 0}, {c.x_nom0, nullptr, b * nx * d, 0},
                    {c.xu_ss, nullptr, b * (nx + nu) * d, 0}, {c.ybar, nullptr, c.ybar ? b * ny * d : 0, 0}, {c.status, nullptr, c.status ? b * 4 : 0, 0},
                    {c.variant, nullptr, c.variant ? b : 0, 0}, {nullptr, c.out, b * nout * d, 0}, {nullptr, c.flag, b * 4, 0},
                    {nullptr, c.n_active, b * 4, 0}, {nullptr, c.active, c.active ? b * nw * 4 : 0, 0}};
    size_t total = 0;
    for (Part &p : parts) { p.off = total; total += (p.bytes + 255) / 256 * 256; }
    SensState &s = *h->sens;
    HIP_TRY(h, s.stage.reserve(std::max<size_t>(total, 256), h->stream));
    char *base = s.stage.p;
    for (const Part &p : parts)
        if (p.host_in && p.bytes) HIP_TRY(h, hipMemcpyAsync(base + p.off, p.host_in, p.bytes, hipMemcpyHostToDevice, h->stream));
    auto at = [&](int i) { return parts[i].bytes ? base + parts[i].off : nullptr; };
    SensCall dc = c;
    dc.x_k = reinterpret_cast<const double *>(at(0)); dc.ref = reinterpret_cast<const double *>(at(1));
    dc.u_nom = reinterpret_cast<const double *>(at(2)); dc.x_nom0 = reinterpret_cast<const double *>(at(3));
    dc.xu_ss = reinterpret_cast<const double *>(at(4)); dc.ybar = reinterpret_cast<const double *>(at(5));
    dc.status = reinterpret_cast<const int32_t *>(at(6)); dc.variant = reinterpret_cast<const uint8_t *>(at(7));
    dc.out = reinterpret_cast<double *>(at(8)); dc.flag = reinterpret_cast<int32_t *>(at(9));
    dc.n_active = reinterpret_cast<int32_t *>(at(10)); dc.active = reinterpret_cast<uint32_t *>(at(11));
    if (const int rc = enqueue_sens(h, h->lane[0], who, dc)) return rc;
    for (const Part &p : parts)
        if (p.host_out && p.bytes) HIP_TRY(h, hipMemcpyAsync(p.host_out, base + p.off, p.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sync_lanes(h));
    return TMPC_OK;
}

}  // namespace

// The adjoint of the cost assembly of condense() for variant k:  M[w] += 2 sum over the error signals priced with weight w of
// (L Hbar L' + L F1bar Dx' + L F2bar Dr'),  Fbar = [F1bar F2bar] ([nv][2 nx]).  M: Q [nx][nx], R [nu][nu], P [nx][nx], T [nx][nx].
void weight_map_add(const tmpc_handle *h, int k, const double *Hbar, const double *Fbar, std::vector<double> (&M)[4]) {
    const tmpc::Condensed &c = h->v[k].c;
    const int nx = c.nx, nv = c.nv;
    for (const tmpc::Condensed::CostSignal &e : c.cost) {
        const int d = e.L.r;
        std::vector<double> LH(static_cast<size_t>(d) * nv, 0.0), LF(static_cast<size_t>(d) * 2 * nx, 0.0);
        for (int i = 0; i < d; ++i)
            for (int t = 0; t < nv; ++t) {
                const double l = e.L(i, t);
                if (l == 0.0) continue;
                for (int j = 0; j < nv; ++j) LH[static_cast<size_t>(i) * nv + j] += l * Hbar[static_cast<size_t>(t) * nv + j];
                for (int j = 0; j < 2 * nx; ++j) LF[static_cast<size_t>(i) * 2 * nx + j] += l * Fbar[static_cast<size_t>(t) * 2 * nx + j];
            }
        std::vector<double> &m = M[e.w];
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) {
                double s = 0.0;
                for (int t = 0; t < nv; ++t) s += LH[static_cast<size_t>(i) * nv + t] * e.L(j, t);
                for (int t = 0; t < nx; ++t) s += LF[static_cast<size_t>(i) * 2 * nx + t] * e.Dx(j, t) + LF[static_cast<size_t>(i) * 2 * nx + nx + t] * e.Dr(j, t);
                m[static_cast<size_t>(i) * d + j] += 2.0 * s;
            }
    }
}

// The symmetric parts of M to the caller's matrices (any may be NULL): Wbar(i, j) and Wbar(j, i) are one number
void write_weights(const tmpc_handle *h, const std::vector<double> (&M)[4], double *const (&out)[4]) {
    const int dims[4] = {h->nx, h->nu, h->nx, h->nx};
    for (int w = 0; w < 4; ++w) {
        if (!out[w]) continue;
        const size_t d = dims[w];
        for (size_t i = 0; i < d; ++i)
            for (size_t j = 0; j <= i; ++j) out[w][i * d + j] = out[w][j * d + i] = 0.5 * (M[w][i * d + j] + M[w][j * d + i]);
    }
}

// tmpc_sens_vjp_weights[_device]: the VJP call with the reduction behind it, then the map to the weights on the host
int weights_call(tmpc_handle *h, const char *who, bool device, SensCall c, double *const (&out)[4]) {
    std::vector<double> res[2];
    c.wgrad = res;
    if (const int rc = device ? call_device(h, who, c) : call_host(h, who, c)) return rc;
    const int dims[4] = {h->nx, h->nu, h->nx, h->nx};
    std::vector<double> M[4];
    for (int w = 0; w < 4; ++w) M[w].assign(static_cast<size_t>(dims[w]) * dims[w], 0.0);
    for (int k = 0; k < (c.variant ? h->nvariants : 1); ++k)
        if (!res[k].empty()) weight_map_add(h, k, res[k].data(), res[k].data() + static_cast<size_t>(h->v[k].c.nv) * h->v[k].c.nv, M);
    write_weights(h, M, out);
    return TMPC_OK;
}

// The region signatures of a solved batch for tmpc_law_learn: the sensitivity kernel in its one-column mode with a zero ybar (HOST pointers)
int tmpc_host::sens_signatures(tmpc_handle *h, const char *who, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                               const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, int32_t *flag, int32_t *n_active, uint32_t *active) {
    const size_t b = static_cast<size_t>(std::max<int64_t>(B, 0)), nx = h ? h->nx : 0, ny = h ? h->N * h->nu + 2 * h->nx + h->nu : 0;
    std::vector<double> ybar(b * ny, 0.0), pbar(b * 2 * nx + 1);
    return call_host(h, who, {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, tmpc::SENS_MODE_VJP, ybar.data(), pbar.data(), flag, n_active, active});
}

extern "C" {

int tmpc_sens_jacobian(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                       const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, double *J, int32_t *flag,
                       int32_t *n_active, uint32_t *active) {
    return call_host(h, "tmpc_sens_jacobian", {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, tmpc::SENS_MODE_JACOBIAN, nullptr, J, flag, n_active, active});
}

int tmpc_sens_jacobian_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                              const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, double *J, int32_t *flag,
                              int32_t *n_active, uint32_t *active) {
    return call_device(h, "tmpc_sens_jacobian_device", {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, tmpc::SENS_MODE_JACOBIAN, nullptr, J, flag, n_active, active});
}

int tmpc_sens_vjp(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                  const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                  int32_t *flag, int32_t *n_active) {
    return call_host(h, "tmpc_sens_vjp", {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, tmpc::SENS_MODE_VJP, ybar, pbar, flag, n_active, nullptr});
}

int tmpc_sens_vjp_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                         const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                         int32_t *flag, int32_t *n_active) {
    return call_device(h, "tmpc_sens_vjp_device", {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, tmpc::SENS_MODE_VJP, ybar, pbar, flag, n_active, nullptr});
}

int tmpc_sens_vjp_weights(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                          const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                          double *Qbar, double *Rbar, double *Pbar, double *Tbar, int32_t *flag, int32_t *n_active) {
    return weights_call(h, "tmpc_sens_vjp_weights", false, {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, tmpc::SENS_MODE_VJP, ybar, pbar, flag, n_active, nullptr},
                        {Qbar, Rbar, Pbar, Tbar});
}

int tmpc_sens_vjp_weights_device(tmpc_handle *h, int64_t B, const double *x_k, const double *ref, const uint8_t *variant, const double *u_nom,
                                 const double *x_nom0, const double *xu_ss, const int32_t *status, double act_tol, const double *ybar, double *pbar,
                                 double *Qbar, double *Rbar, double *Pbar, double *Tbar, int32_t *flag, int32_t *n_active) {
    return weights_call(h, "tmpc_sens_vjp_weights_device", true, {B, x_k, ref, variant, u_nom, x_nom0, xu_ss, status, act_tol, tmpc::SENS_MODE_VJP, ybar, pbar, flag, n_active, nullptr},
                        {Qbar, Rbar, Pbar, Tbar});
}

int tmpc_sens_weight_map(tmpc_handle *h, int variant, const double *Hbar, const double *Fbar, double *Qbar, double *Rbar, double *Pbar, double *Tbar) {
    if (!h) return TMPC_E_INVALID;
    if (variant < 0 || variant >= h->nvariants) { h->err = "tmpc_sens_weight_map: variant out of range"; return TMPC_E_INVALID; }
    if (!Hbar || !Fbar) { h->err = "tmpc_sens_weight_map: NULL argument"; return TMPC_E_INVALID; }
    if (h->regulator) { h->err = "tmpc_sens_weight_map: a regulator handle is not supported (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    if (h->v[variant].c.off_aux >= 0) {
        h->err = "tmpc_sens_weight_map: variant " + std::to_string(variant) + " keeps the unpriced auxiliaries of the literal terminal row, which the outputs do not determine (give HTP / hTP)";
        return TMPC_E_UNSUPPORTED;
    }
    const int dims[4] = {h->nx, h->nu, h->nx, h->nx};
    std::vector<double> M[4];
    for (int w = 0; w < 4; ++w) M[w].assign(static_cast<size_t>(dims[w]) * dims[w], 0.0);
    weight_map_add(h, variant, Hbar, Fbar, M);
    write_weights(h, M, {Qbar, Rbar, Pbar, Tbar});
    return TMPC_OK;
}

int tmpc_sens_get_model(tmpc_handle *h, int variant, double *F, double *Ebar, double *Y, double *Yp, double *Rec) {
    if (!h) return TMPC_E_INVALID;
    if (variant < 0 || variant >= h->nvariants) { h->err = "tmpc_sens_get_model: variant out of range"; return TMPC_E_INVALID; }
    if (h->regulator) { h->err = "tmpc_sens_get_model: a regulator handle is not supported (tracking handles only)"; return TMPC_E_UNSUPPORTED; }
    HostModel hm;
    int rc = TMPC_OK;
    if (const std::string msg = host_model(h, variant, hm, rc); !msg.empty()) { h->err = "tmpc_sens_get_model: " + msg; return rc; }
    const struct { double *dst; const Mat *src; } parts[] = {{F, &hm.F}, {Ebar, &hm.Eb}, {Y, &hm.Y}, {Yp, &hm.Yp}, {Rec, &hm.Rec}};
    for (const auto &p : parts)
        if (p.dst && !p.src->a.empty()) std::memcpy(p.dst, p.src->a.data(), p.src->a.size() * sizeof(double));
    return TMPC_OK;
}

}  // extern "C"

namespace {

// tmpc_qp_sensitivity, and tmpc_qp_sensitivity_data (`data`: VJP mode, out may be NULL, with the reduction to Hbar and Fbar behind it)
int qp_sens(const char *name, bool data, int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G,
            const double *g0, const double *Ebar, const double *Y, const double *Yp, int64_t B, const double *P, const double *Z,
            const int32_t *status, double act_tol, int mode, const double *ybar, double *out, int32_t *flag, int32_t *n_active,
            uint32_t *active, double *Hbar, double *Fbar, double *adj) {
    const std::string who = std::string(name) + ": ";
    auto refuse = [&](int rc, const std::string &msg) { g_create_error = who + msg; return rc; };
    if (nv < 1 || nv > tmpc::SENS_MAX_NV) return refuse(TMPC_E_INVALID, "nv = " + std::to_string(nv) + " is not in [1, " + std::to_string(tmpc::SENS_MAX_NV) + "]");
    if (nc < 0 || nc > tmpc::SENS_MAX_NC) return refuse(TMPC_E_INVALID, "nc = " + std::to_string(nc) + " is not in [0, 2^20]");
    if (np < 1 || np > tmpc::SENS_MAX_NP) return refuse(TMPC_E_INVALID, "np = " + std::to_string(np) + " is not in [1, " + std::to_string(tmpc::SENS_MAX_NP) + "]");
    if (ny < 1 || ny > tmpc::SENS_MAX_NY) return refuse(TMPC_E_INVALID, "ny = " + std::to_string(ny) + " is not in [1, " + std::to_string(tmpc::SENS_MAX_NY) + "]");
    if (B < 0) return refuse(TMPC_E_INVALID, "B < 0");
    if (mode != TMPC_SENS_JACOBIAN && mode != TMPC_SENS_VJP) return refuse(TMPC_E_INVALID, "mode is TMPC_SENS_JACOBIAN or TMPC_SENS_VJP");
    if (!H || !F || (nc > 0 && (!G || !g0 || !Ebar)) || !Y || !Yp || !P || !Z || (!data && !out) || !flag || !n_active || (mode == TMPC_SENS_VJP && !ybar) ||
        (data && (!Hbar || !Fbar)))
        return refuse(TMPC_E_INVALID, "NULL argument");
    if (B == 0) {
        if (data) { std::fill(Hbar, Hbar + static_cast<size_t>(nv) * nv, 0.0); std::fill(Fbar, Fbar + static_cast<size_t>(nv) * np, 0.0); }
        return TMPC_OK;
    }
    if (device < 0) return refuse(TMPC_E_DEVICE, "device < 0: the kernel runs on the GPU");
    auto fail = [&](const char *what, hipError_t e) { return refuse(TMPC_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); };
    if (const hipError_t e = hipSetDevice(device); e != hipSuccess) return fail("hipSetDevice", e);
    int n_cu = 0;
    if (const hipError_t e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device); e != hipSuccess) return fail("hipDeviceGetAttribute", e);
    struct Owner {
        SensModel m;
        char *batch = nullptr;
        ~Owner() {
            if (m.block) (void)hipFree(m.block);
            if (batch) (void)hipFree(batch);
        }
    } own;
    const double zero = 0.0;
    const RawModel r{nv, nc, np, ny, nv, H, F, nc ? G : &zero, nc ? g0 : &zero, nc ? Ebar : &zero, Y, Yp, nullptr};
    int rc = TMPC_OK;
    if (const std::string msg = upload_model(r, own.m, rc); !msg.empty()) return refuse(rc, msg);
    const size_t b = static_cast<size_t>(B), d = sizeof(double), nw = (static_cast<size_t>(nc) + 31) / 32;
    const size_t nout = mode == TMPC_SENS_VJP ? static_cast<size_t>(np) : static_cast<size_t>(ny) * np;
    const unsigned blocks = sens_blocks(B, n_cu, nv, np);
    struct Part { const void *host_in; void *host_out; size_t bytes; size_t off; };
    Part parts[] = {{P, nullptr, b * np * d, 0}, {Z, nullptr, b * nv * d, 0}, {ybar, nullptr, mode == TMPC_SENS_VJP ? b * ny * d : 0, 0},
                    {status, nullptr, status ? b * 4 : 0, 0}, {nullptr, out, b * nout * d, 0}, {nullptr, flag, b * 4, 0}, {nullptr, n_active, b * 4, 0},
                    {nullptr, active, active ? b * nw * 4 : 0, 0},
                    {nullptr, nullptr, mode == TMPC_SENS_JACOBIAN ? static_cast<size_t>(blocks) * 2 * nv * np * d : 0, 0},
                    {nullptr, adj, data ? b * nv * d : 0, 0}, {nullptr, nullptr, data ? b * nv * d : 0, 0},
                    {nullptr, nullptr, data ? tmpc::sens_wgrad_chunks(B) * nv * (static_cast<size_t>(nv) + np) * d : 0, 0},
                    {nullptr, Hbar, data ? static_cast<size_t>(nv) * nv * d : 0, 0}, {nullptr, Fbar, data ? static_cast<size_t>(nv) * np * d : 0, 0}};
    size_t total = 0;
    for (Part &p : parts) { p.off = total; total += (p.bytes + 255) / 256 * 256; }
    if (hipMalloc(reinterpret_cast<void **>(&own.batch), total) != hipSuccess) {
        (void)hipGetLastError();
        own.batch = nullptr;
        return refuse(TMPC_E_NOMEM, "out of device memory");
    }
    for (const Part &p : parts)
        if (p.host_in && p.bytes)
            if (const hipError_t e = hipMemcpy(own.batch + p.off, p.host_in, p.bytes, hipMemcpyHostToDevice); e != hipSuccess) return fail("upload", e);
    auto at = [&](int i) { return parts[i].bytes ? own.batch + parts[i].off : nullptr; };
    tmpc::SensArgs a = own.m.a;
    a.B = B;
    a.np0 = np; a.P0 = reinterpret_cast<const double *>(at(0)); a.P1 = nullptr;
    a.nz0 = nv; a.nz1 = a.nz2 = 0; a.Z0 = reinterpret_cast<const double *>(at(1)); a.Z1 = a.Z2 = nullptr;
    a.ybar = reinterpret_cast<const double *>(at(2));
    a.status = reinterpret_cast<const int32_t *>(at(3));
    a.variant = nullptr; a.my_variant = 0; a.nvariants = 1;
    a.act_tol = act_tol > 0.0 ? act_tol : tmpc::SENS_ACT_TOL;
    a.mode = mode;
    a.out = reinterpret_cast<double *>(at(4)); a.flag = reinterpret_cast<int32_t *>(at(5)); a.n_active = reinterpret_cast<int32_t *>(at(6));
    a.active = reinterpret_cast<uint32_t *>(at(7)); a.nwords = static_cast<int>(nw);
    a.ws = reinterpret_cast<double *>(at(8));
    a.adj = reinterpret_cast<double *>(at(9)); a.zrec = reinterpret_cast<double *>(at(10));
    if (const hipError_t e = tmpc::launch_sens(a, blocks, nullptr); e != hipSuccess) return fail("launch", e);
    if (data) {
        tmpc::SensWgradArgs g{};
        g.nv = nv; g.np = np; g.B = B; g.adj = a.adj; g.zrec = a.zrec; g.np0 = np; g.P0 = a.P0; g.P1 = nullptr; g.flag = a.flag;
        g.variant = nullptr; g.my_variant = 0; g.nvariants = 1;
        g.part = reinterpret_cast<double *>(at(11)); g.Hbar = reinterpret_cast<double *>(at(12)); g.Fbar = reinterpret_cast<double *>(at(13));
        if (const hipError_t e = tmpc::launch_sens_wgrad(g, wgrad_blocks(B, n_cu, nv, np), nullptr); e != hipSuccess) return fail("launch", e);
    }
    if (const hipError_t e = hipDeviceSynchronize(); e != hipSuccess) return fail("hipDeviceSynchronize", e);
    for (const Part &p : parts)
        if (p.host_out && p.bytes)
            if (const hipError_t e = hipMemcpy(p.host_out, own.batch + p.off, p.bytes, hipMemcpyDeviceToHost); e != hipSuccess) return fail("copy-out", e);
    return TMPC_OK;
}

}  // namespace

extern "C" {

int tmpc_qp_sensitivity(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G,
                        const double *g0, const double *Ebar, const double *Y, const double *Yp, int64_t B, const double *P, const double *Z,
                        const int32_t *status, double act_tol, int mode, const double *ybar, double *out, int32_t *flag, int32_t *n_active,
                        uint32_t *active) {
    return qp_sens("tmpc_qp_sensitivity", false, device, nv, nc, np, ny, H, F, G, g0, Ebar, Y, Yp, B, P, Z, status, act_tol, mode, ybar, out, flag, n_active, active,
                   nullptr, nullptr, nullptr);
}

int tmpc_qp_sensitivity_data(int device, int32_t nv, int32_t nc, int32_t np, int32_t ny, const double *H, const double *F, const double *G,
                             const double *g0, const double *Ebar, const double *Y, const double *Yp, int64_t B, const double *P, const double *Z,
                             const int32_t *status, double act_tol, const double *ybar, double *pbar, double *Hbar, double *Fbar, double *adj,
                             int32_t *flag, int32_t *n_active) {
    return qp_sens("tmpc_qp_sensitivity_data", true, device, nv, nc, np, ny, H, F, G, g0, Ebar, Y, Yp, B, P, Z, status, act_tol, TMPC_SENS_VJP, ybar, pbar, flag, n_active,
                   nullptr, Hbar, Fbar, adj);
}

}  // extern "C"
