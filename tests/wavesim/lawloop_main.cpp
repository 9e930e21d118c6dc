// TEST INFRASTRUCTURE (not product code): the fused closed loop through the explicit law -- closed_loop_law, csrc/tmpc_kernels.hip with
// FUSED = 3, the source text the GPU build compiles in csrc/tmpc_fused_law.hip -- on the host execution model of hip_sim.hpp, for the
// sanitizers.  One workgroup; a wave keeps its trajectory for all T steps.  Device memory is exact-size heap blocks, what the kernel must
// write itself uninitialised.  Built with -DTMPC_SIM_LAW_LOOP (the lawloop line of the Makefile), the only binaries that hold this kernel.
//
//   lawloop <layout file> <loop file> <table file> <output file>
// layout file, loop file: as wavesim --loop (wavesim_main.cpp), one problem
// table file : int64 hd[6] = {np, ny, nrow, R, n_order, max_tries}, int64 miss_cap; S[R][np + 1][nrowp], K[R][np + 1][ny], int32 order[n_order]
//              (the layout tmpc_law.cpp uploads; law_case.pack_table)
// output file: err2 [B], x_final [B][nx], consistent [B] doubles; tube_viol [B], not_optimal [B], iters_sum [B] int32; region [B], hits [B] int32;
//              tries [B] int64; region hits [R] uint64; uint64 n_total; miss_p [min(n_total, miss_cap)][np] doubles; miss_var [same] bytes
#include "../../robust-tracking-mpc-over-lossy-networks_amd/csrc/tmpc_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

namespace {
void need(bool ok, const char *what) {
    if (!ok) { std::fprintf(stderr, "lawloop: %s\n", what); std::exit(2); }
}
template <class T> std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }          // uninitialised
struct Layout {
    tmpc::DeviceQP d;
    tmpc::KernelShape ks;
    std::vector<std::unique_ptr<char[]>> keep;
};
// (wavesim_main.cpp: read_layout) every array gets a heap block of exactly its size
void read_layout(const char *path, Layout &L) {
    FILE *f = std::fopen(path, "rb");
    need(f != nullptr, "cannot open layout file");
    int32_t shp[6], tag[2];
    uint64_t qb;
    need(std::fread(tag, 4, 2, f) == 2 && tag[0] == tmpc::DUMP_TAG && tag[1] == tmpc::DUMP_FORMAT, "layout file of another dump format");
    need(std::fread(shp, 4, 6, f) == 6 && std::fread(&qb, 8, 1, f) == 1 && qb == sizeof(tmpc::DeviceQP), "layout file written for another DeviceQP");
    need(std::fread(&L.d, sizeof L.d, 1, f) == 1, "short layout file");
    L.ks.nvp = shp[0]; L.ks.dp = shp[1]; L.ks.ds = shp[2]; L.ks.kcp = shp[3]; L.ks.cp = shp[4]; L.ks.cs = shp[5];
    const void **fields[] = {reinterpret_cast<const void **>(&L.d.Gt), reinterpret_cast<const void **>(&L.d.Hct), reinterpret_cast<const void **>(&L.d.Psi),
                             reinterpret_cast<const void **>(&L.d.Hs), reinterpret_cast<const void **>(&L.d.Hinv), reinterpret_cast<const void **>(&L.d.F1s),
                             reinterpret_cast<const void **>(&L.d.F2s), reinterpret_cast<const void **>(&L.d.g0p), reinterpret_cast<const void **>(&L.d.Esp),
                             reinterpret_cast<const void **>(&L.d.vmask), reinterpret_cast<const void **>(&L.d.row_of), reinterpret_cast<const void **>(&L.d.gp0),
                             reinterpret_cast<const void **>(&L.d.Ep), reinterpret_cast<const void **>(&L.d.Dv), reinterpret_cast<const void **>(&L.d.Tzs),
                             reinterpret_cast<const void **>(&L.d.Txf), reinterpret_cast<const void **>(&L.d.Mth), reinterpret_cast<const void **>(&L.d.A),
                             reinterpret_cast<const void **>(&L.d.B), reinterpret_cast<const void **>(&L.d.cip)};
    for (const void **fp : fields) {
        uint64_t n;
        need(std::fread(&n, 8, 1, f) == 1, "short layout file");
        if (n == 0) { *fp = nullptr; continue; }
        L.keep.emplace_back(new char[n]);
        need(std::fread(L.keep.back().get(), 1, n, f) == n, "short layout file");
        *fp = L.keep.back().get();
    }
    L.d.dbg = nullptr; L.d.save = nullptr; L.d.ticks = nullptr;
    std::fclose(f);
}
}  // namespace

int main(int argc, char **argv) {
    need(argc == 5, "usage: lawloop <layout> <loop file> <table file> <out>");
    Layout lay;
    read_layout(argv[1], lay);
    FILE *f = std::fopen(argv[2], "rb");
    need(f != nullptr, "cannot open loop file");
    int64_t hd[8];
    need(std::fread(hd, 8, 8, f) == 8, "short loop file");
    const int64_t B = hd[0], T = hd[1], nx = hd[2], nu = hd[3], rZ = hd[4];
    need(nx == lay.d.nx && nu == lay.d.nu && hd[5] == 0 && B > 0 && T > 0, "loop file does not belong to this layout");
    const int N = lay.d.N;
    auto rd = [&](size_t n) { std::vector<double> v(n); need(n == 0 || std::fread(v.data(), 8, n, f) == n, "short loop file"); return v; };
    const size_t b = static_cast<size_t>(B), t_ = static_cast<size_t>(T);
    std::vector<double> A = rd(nx * nx), Bm = rd(nx * nu), K = rd(nu * nx), Ka = rd(nu * nx), HZ = rd(rZ * nx), hZ = rd(rZ), pl = rd(b), ref = rd(t_),
                        th = rd(b * t_), ga = rd(b * t_), w = rd(b * t_ * nx), x0 = rd(b * nx);
    std::fclose(f);
    // the table
    f = std::fopen(argv[3], "rb");
    need(f != nullptr, "cannot open table file");
    int64_t th6[6], miss_cap;
    need(std::fread(th6, 8, 6, f) == 6 && std::fread(&miss_cap, 8, 1, f) == 1, "short table file");
    const size_t np = th6[0], ny = th6[1], nrow = th6[2], R = th6[3], n_order = th6[4], nrowp = (nrow + 63) / 64 * 64, cap = static_cast<size_t>(miss_cap);
    need(np == static_cast<size_t>(2 * nx) && ny == static_cast<size_t>(N * nu + 2 * nx + nu) && miss_cap >= 0, "table file does not belong to this layout");
    auto S = block<double>(R * (np + 1) * nrowp), Kt = block<double>(R * (np + 1) * ny);
    auto order = block<int32_t>(n_order);
    need(std::fread(S.get(), 8, R * (np + 1) * nrowp, f) == R * (np + 1) * nrowp && std::fread(Kt.get(), 8, R * (np + 1) * ny, f) == R * (np + 1) * ny &&
         std::fread(order.get(), 4, n_order, f) == n_order, "short table file");
    std::fclose(f);
    for (size_t i = 0; i < n_order; ++i) need(order[i] >= 0 && static_cast<size_t>(order[i]) < R, "order entry out of range");
    auto region_hits = block<unsigned long long>(R);
    std::memset(region_hits.get(), 0, R * sizeof(unsigned long long));
    // the law's record as tmpc_loops.cpp fills it (tracking_pieces): region -1, accumulators and counter 0, the log uninitialised
    auto ll = block<tmpc::LawLoop>(1);
    ll[0] = tmpc::LawLoop{};
    tmpc::LawTable &tab = ll[0].t[0];
    tab.nrow = static_cast<int>(nrow); tab.nrowp = static_cast<int>(nrowp); tab.R = static_cast<int>(R); tab.n_order = static_cast<int>(n_order);
    tab.S = R ? S.get() : nullptr; tab.K = R ? Kt.get() : nullptr; tab.order = n_order ? order.get() : nullptr; tab.hits = R ? region_hits.get() : nullptr;
    std::vector<int32_t> region(b, -1), hits(b, 0);
    std::vector<long long> tries(b, 0);
    unsigned long long miss_n = 0;
    auto miss_p = block<double>(cap * np);
    auto miss_var = block<uint8_t>(cap);
    ll[0].max_tries = static_cast<int>(th6[5]); ll[0].region = region.data(); ll[0].hits = hits.data(); ll[0].tries = tries.data();
    ll[0].miss_n = &miss_n; ll[0].miss_cap = miss_cap; ll[0].miss_p = miss_p.get(); ll[0].miss_var = miss_var.get();
    // the loop's state (wavesim_main.cpp: run_loop)
    tmpc::McFused mf{};
    tmpc::McModel &m = mf.m;
    tmpc::McState &st = mf.st;
    m.nx = static_cast<int>(nx); m.nu = static_cast<int>(nu); m.N = N; m.extended = 0; m.rZ = static_cast<int>(rZ);
    m.plant = TMPC_PLANT_LINEAR; m.substeps = 1; m.smart = static_cast<int>(hd[6]);
    m.A = A.data(); m.B = Bm.data(); m.K = K.data(); m.K_anc = Ka.data(); m.HZ = HZ.data(); m.hZ = hZ.data();
    std::vector<double> x(x0), xh(x0), xn(x0), Ub(b * (N + 1) * nu, 0.0), ul0(b * nu, 0.0), xn0l(b * nx, 0.0), refk(b * nx, 0.0), err2(b, 0.0), cons(b, 0.0);
    std::vector<int32_t> q_est(b, 0), q_act(b, 0), s_(b, 0), Th(b, 0), last_lost(b, -1), tube(b, 0), nopt(b, 0), itsum(b, 0);
    std::vector<uint8_t> gam(b, 1), dead(b, 0);
    for (size_t i = 0; i < b; ++i) refk[i * nx] = ref[0];
    st.x = x.data(); st.x_hat = xh.data(); st.x_nom = xn.data(); st.Ubuf = Ub.data(); st.u_latest0 = ul0.data(); st.x_nom0_latest = xn0l.data();
    st.ref_k = refk.data(); st.err2 = err2.data(); st.consistent = cons.data(); st.err2_phys = nullptr;
    st.q_est = q_est.data(); st.q_act = q_act.data(); st.s = s_.data(); st.Theta = Th.data(); st.last_lost = last_lost.data();
    st.tube_viol = tube.data(); st.not_optimal = nopt.data(); st.iters_sum = itsum.data(); st.gamma = gam.data(); st.dead = dead.data();
    st.p_loss = pl.data(); st.th_u = th.data(); st.ga_u = ga.data(); st.w = w.data();
    st.rng_on = 0; st.ticks = nullptr; st.tick_sum = st.tick_max = nullptr; st.cap_index = -1; st.cap = nullptr;
    st.rp_U = st.rp_xn0 = nullptr; st.trace_f = nullptr; st.trace_i = nullptr;
    mf.T = static_cast<int>(T);
    mf.ref_seq = ref.data();
    auto u = block<double>(b * N * nu), xo = block<double>(b * nx), ss = block<double>(b * (nx + nu));
    auto sst = block<int32_t>(b), it = block<int32_t>(b);
    std::vector<int32_t> ws(hd[7] ? b * tmpc::WS_STRIDE : 0, 0);
    unsigned long long word = 0;
    tmpc::WorkCounter wc{&word, 1, 0};
    const hipError_t e = tmpc::launch_solve_mc_law(lay.d, lay.ks, B, u.get(), xo.get(), ss.get(), sst.get(), it.get(), hd[7] ? ws.data() : nullptr, &mf, ll.get(), &wc,
                                                   1, nullptr);
    need(e == hipSuccess, "launch failed (shape not compiled into this build?)");
    FILE *o = std::fopen(argv[4], "wb");
    need(o != nullptr, "cannot open output file");
    const size_t kept = std::min<size_t>(static_cast<size_t>(miss_n), cap);
    const uint64_t n_total = miss_n;
    need(std::fwrite(err2.data(), 8, b, o) == b && std::fwrite(x.data(), 8, b * nx, o) == b * nx && std::fwrite(cons.data(), 8, b, o) == b &&
         std::fwrite(tube.data(), 4, b, o) == b && std::fwrite(nopt.data(), 4, b, o) == b && std::fwrite(itsum.data(), 4, b, o) == b &&
         std::fwrite(region.data(), 4, b, o) == b && std::fwrite(hits.data(), 4, b, o) == b && std::fwrite(tries.data(), 8, b, o) == b &&
         std::fwrite(region_hits.get(), 8, R, o) == R && std::fwrite(&n_total, 8, 1, o) == 1 && std::fwrite(miss_p.get(), 8, kept * np, o) == kept * np &&
         std::fwrite(miss_var.get(), 1, kept, o) == kept, "short write");
    std::fclose(o);
    return 0;
}
