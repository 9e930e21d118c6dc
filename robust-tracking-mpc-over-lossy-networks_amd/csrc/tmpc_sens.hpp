// Sensitivity of the condensed QP's minimiser (tmpc_sens.hip): what tmpc_sens.cpp and the kernel share.  include/tmpc.h has the
// entry points (tmpc_sens_jacobian, tmpc_sens_vjp, tmpc_qp_sensitivity) and the meaning of the flags.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tmpc {

constexpr int SENS_MAX_NV = 128;         // decision variables, the limit of the solve paths
constexpr int SENS_MAX_NP = 32;          // parameters p (a controller has 2 nx <= 32)
constexpr int SENS_MAX_NY = 4096;        // outputs y
constexpr int SENS_MAX_NC = 1 << 20;     // inequality rows

// The tolerances of the flags (include/tmpc.h: TMPC_SENS_*), compile-time constants shared with the numpy twin
// (LinearMPCOverNetworks/sensitivity.py):
constexpr double SENS_RANK_TOL = 1e-10;  // a candidate row is dropped when its pivot is <= SENS_RANK_TOL * its diagonal entry of M
constexpr double SENS_MULT_TOL = 1e-9;   // WEAK: a kept row's multiplier <= SENS_MULT_TOL * max(1, |lambda|_inf)
constexpr double SENS_KKT_TOL = 1e-6;    // NOT_KKT: stationarity residual > SENS_KKT_TOL * (1 + |F p|_inf), or a multiplier below minus that
constexpr double SENS_ACT_TOL = 1e-7;    // the default act_tol

constexpr int SENS_MODE_JACOBIAN = 0, SENS_MODE_VJP = 1;

// One launch: the instances b of a batch whose variant id is `my_variant` (everything when variant == NULL).  All pointers are device
// pointers.  The model part does not depend on the instance and is computed once on the host (tmpc_sens.cpp).
struct SensArgs {
    // ---- model: min 1/2 z'Hz + (F p)'z  s.t.  G z <= g0 + Ebar p;  y = Y z + Yp p
    int nv, nc, np, ny;
    const double *H;         // [nv][nv]
    const double *Hinv;      // [nv][nv]
    const double *F;         // [nv][np]
    const double *HinvF;     // [nv][np]
    const double *G;         // [nc][nv]
    const double *W;         // [nc][nv]  G H^-1
    const double *g0;        // [nc]
    const double *Ebar;      // [nc][np]
    const double *Gt;        // [nv][nc]  G transposed: the row scan reads it a thread per row, neighbouring threads neighbouring words
    const double *EbarT;     // [np][nc]
    const double *Y;         // [ny][nv]
    const double *Yp;        // [ny][np]
    const double *Rec;       // [nv][nzin + np] or NULL: z = Rec [zin | p] (a handle: zin = the solve's outputs); NULL: z = zin, nzin = nv
    // ---- batch
    int64_t B;
    int np0;                 // p = [P0[b][0..np0) | P1[b][0..np - np0)]
    const double *P0, *P1;
    int nz0, nz1, nz2;       // zin = [Z0[b][0..nz0) | Z1[b][0..nz1) | Z2[b][0..nz2)]
    const double *Z0, *Z1, *Z2;
    const int32_t *status;   // or NULL
    const uint8_t *variant;  // or NULL
    int my_variant, nvariants;       // ids >= nvariants are flagged SKIPPED by the launch of variant 0
    double act_tol;
    int mode;                // SENS_MODE_*
    const double *ybar;      // [B][ny] (VJP)
    double *out;             // [B][ny][np] (Jacobian) or [B][np] (VJP)
    int32_t *flag;           // [B]
    int32_t *n_active;       // [B]
    uint32_t *active;        // [B][nwords] or NULL
    int nwords;
    double *ws;              // [blocks][2 nv np]  right-hand-side blocks of the Jacobian (NULL for the VJP)
    // ---- VJP mode, optional (NULL: not written): what the gradient with respect to H and F is made of (sens_wgrad below)
    double *adj = nullptr;   // [B][nv]  a_b = H^-1 v - W_A' q, the solution of [H G_A'; G_A 0] [a; q] = [v; 0], v = Y' ybar_b; zeros where SKIPPED
    double *zrec = nullptr;  // [B][nv]  the z_b the kernel worked on (rebuilt through Rec for a handle); zeros where SKIPPED
};

// The reduction over the batch behind the gradients with respect to H and F:  C [nv][nv + np] = sum_b a_b (x) [z_b | p_b]  over the
// instances of `my_variant` that are not SKIPPED, then  Hbar = -1/2 (C_H + C_H'),  Fbar = -C_F.  B is cut into chunks of
// SENS_WG_CHUNK instances -- a constant, so that the order of the sums depends on nothing but B: a wave per 16 x 16 tile and chunk
// writes its partial tile to `part` (v_mfma_f64_16x16x4_f64, four instances a step), a second kernel adds the partials in chunk order.
constexpr int SENS_WG_CHUNK = 256;
struct SensWgradArgs {
    int nv, np;
    int64_t B;
    const double *adj, *zrec;        // [B][nv] as sens_kernel wrote them
    int np0;                         // p as in SensArgs
    const double *P0, *P1;
    const int32_t *flag;             // [B] as sens_kernel wrote it
    const uint8_t *variant;          // or NULL
    int my_variant, nvariants;
    double *part;                    // [ceil(B / SENS_WG_CHUNK)][nv][nv + np]
    double *Hbar, *Fbar;             // [nv][nv], [nv][np]
};
inline size_t sens_wgrad_chunks(int64_t B) { return static_cast<size_t>((B + SENS_WG_CHUNK - 1) / SENS_WG_CHUNK); }
// `blocks`: workgroups of the first kernel (one wave each; they take the tile-chunk pairs round robin, the result does not depend on it)
hipError_t launch_sens_wgrad(const SensWgradArgs &a, unsigned blocks, hipStream_t stream);

// LDS of a workgroup in bytes, and its size in threads (one wave up to nv = 32, four beyond)
size_t sens_lds_bytes(int nv, int np);
int sens_threads(int nv);
hipError_t launch_sens(const SensArgs &a, unsigned blocks, hipStream_t stream);

}  // namespace tmpc
