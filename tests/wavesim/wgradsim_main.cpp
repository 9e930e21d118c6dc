// TEST INFRASTRUCTURE (not product code): the reverse mode of csrc/tmpc_sens.hip with its adj / zrec outputs, and the batch reduction
// behind the weight gradients (sens_wgrad_partial_kernel, sens_wgrad_sum_kernel; include/tmpc.h: tmpc_qp_sensitivity_data) -- the source
// text the GPU build compiles -- on the host execution model of hip_sim.hpp, for the sanitizers.  Every grid is ONE workgroup, which
// takes every instance, tile and chunk in turn.  Device memory is exact-size heap blocks; the outputs, adj, zrec and the partial tiles
// are left uninitialised.
//
//   wgradsim run <in> <out>
//     in:  int64 hd[5] = {nv, nc, np, ny, B}; double act_tol; then the model as tmpc_sens.cpp uploads it -- H[nv][nv], Hinv[nv][nv],
//          F[nv][np], HinvF[nv][np], G[nc][nv], W[nc][nv], g0[nc], Ebar[nc][np], Y[ny][nv], Yp[ny][np] -- and the batch: P[B][np], Z[B][nv],
//          int32 status[B], double ybar[B][ny]
//     out: double pbar[B][np]; double adj[B][nv]; double Hbar[nv][nv]; double Fbar[nv][np]; int32 flag[B]; int32 n_active[B]
#include "../../robust-tracking-mpc-over-lossy-networks_amd/csrc/tmpc_sens.hip"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

namespace {
void need(bool ok, const char *what) {
    if (!ok) { std::fprintf(stderr, "wgradsim: %s\n", what); std::exit(2); }
}
template <class T> void rd(FILE *f, T *p, size_t n) { need(std::fread(p, sizeof(T), n, f) == n, "short input file"); }
template <class T> void wr(FILE *f, const T *p, size_t n) { need(std::fwrite(p, sizeof(T), n, f) == n, "short write"); }
template <class T> std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }                      // uninitialised
template <class T> std::unique_ptr<T[]> read_block(FILE *f, size_t n) { auto p = block<T>(n); rd(f, p.get(), n); return p; }

int run_main(FILE *f, FILE *o) {
    int64_t hd[5];
    double act_tol;
    rd(f, hd, 5);
    rd(f, &act_tol, 1);
    need(hd[0] >= 1 && hd[0] <= tmpc::SENS_MAX_NV && hd[1] >= 0 && hd[2] >= 1 && hd[2] <= tmpc::SENS_MAX_NP && hd[3] >= 1 && hd[4] >= 1, "bad sizes");
    const size_t nv = hd[0], nc = hd[1], np = hd[2], ny = hd[3], nb = hd[4];
    auto H = read_block<double>(f, nv * nv), Hinv = read_block<double>(f, nv * nv), F = read_block<double>(f, nv * np), HinvF = read_block<double>(f, nv * np);
    auto G = read_block<double>(f, nc * nv), W = read_block<double>(f, nc * nv), g0 = read_block<double>(f, nc), Ebar = read_block<double>(f, nc * np);
    auto Y = read_block<double>(f, ny * nv), Yp = read_block<double>(f, ny * np);
    auto Gt = block<double>(nc * nv), EbarT = block<double>(nc * np);            // the transposed copies tmpc_sens.cpp adds
    for (size_t i = 0; i < nc; ++i) {
        for (size_t j = 0; j < nv; ++j) Gt[j * nc + i] = G[i * nv + j];
        for (size_t q = 0; q < np; ++q) EbarT[q * nc + i] = Ebar[i * np + q];
    }
    auto P = read_block<double>(f, nb * np), Z = read_block<double>(f, nb * nv);
    auto status = read_block<int32_t>(f, nb);
    auto ybar = read_block<double>(f, nb * ny);
    auto pbar = block<double>(nb * np), adj = block<double>(nb * nv), zrec = block<double>(nb * nv);
    auto flag = block<int32_t>(nb), nact = block<int32_t>(nb);
    auto part = block<double>(tmpc::sens_wgrad_chunks(hd[4]) * nv * (nv + np));
    auto Hbar = block<double>(nv * nv), Fbar = block<double>(nv * np);
    tmpc::SensArgs a{};
    a.nv = static_cast<int>(nv); a.nc = static_cast<int>(nc); a.np = static_cast<int>(np); a.ny = static_cast<int>(ny);
    a.H = H.get(); a.Hinv = Hinv.get(); a.F = F.get(); a.HinvF = HinvF.get(); a.G = G.get(); a.W = W.get(); a.g0 = g0.get(); a.Ebar = Ebar.get();
    a.Gt = Gt.get(); a.EbarT = EbarT.get();
    a.Y = Y.get(); a.Yp = Yp.get(); a.Rec = nullptr;
    a.B = hd[4];
    a.np0 = a.np; a.P0 = P.get(); a.P1 = nullptr;
    a.nz0 = a.nv; a.nz1 = a.nz2 = 0; a.Z0 = Z.get(); a.Z1 = a.Z2 = nullptr;
    a.status = status.get(); a.variant = nullptr; a.my_variant = 0; a.nvariants = 1;
    a.act_tol = act_tol;
    a.mode = tmpc::SENS_MODE_VJP; a.ybar = ybar.get();
    a.out = pbar.get(); a.flag = flag.get(); a.n_active = nact.get(); a.active = nullptr; a.nwords = 0;
    a.ws = nullptr;
    a.adj = adj.get(); a.zrec = zrec.get();
    need(tmpc::launch_sens(a, 1, nullptr) == hipSuccess, "launch failed");
    tmpc::SensWgradArgs g{};
    g.nv = a.nv; g.np = a.np; g.B = a.B; g.adj = a.adj; g.zrec = a.zrec; g.np0 = a.np; g.P0 = a.P0; g.P1 = nullptr; g.flag = a.flag;
    g.variant = nullptr; g.my_variant = 0; g.nvariants = 1;
    g.part = part.get(); g.Hbar = Hbar.get(); g.Fbar = Fbar.get();
    need(tmpc::launch_sens_wgrad(g, 1, nullptr) == hipSuccess, "launch of the reduction failed");
    wr(o, pbar.get(), nb * np);
    wr(o, adj.get(), nb * nv);
    wr(o, Hbar.get(), nv * nv);
    wr(o, Fbar.get(), nv * np);
    wr(o, flag.get(), nb);
    wr(o, nact.get(), nb);
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    need(argc == 4 && std::string(argv[1]) == "run", "usage: wgradsim run <in> <out>");
    FILE *f = std::fopen(argv[2], "rb");
    need(f != nullptr, "cannot open the input file");
    FILE *o = std::fopen(argv[3], "wb");
    need(o != nullptr, "cannot open the output file");
    const int rc = run_main(f, o);
    std::fclose(f);
    std::fclose(o);
    return rc;
}
