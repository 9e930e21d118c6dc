// TEST INFRASTRUCTURE (not product code): the explicit-law kernel of csrc/tmpc_law.hip (include/tmpc.h: tmpc_qp_law_eval; the source text the
// GPU build compiles) on the host execution model of hip_sim.hpp, for the sanitizers.  The grid is ONE workgroup of four waves, which
// take the instances in turn.  Device memory is exact-size heap blocks, the outputs uninitialised.
//
// This driver runs the search with hops (tmpc_law_set_hops): the table comes with its keys and their hash, the six counters come back.
//
//   lawhop run <in> <out>
//     in:  int64 hd[12] = {np, ny, nrow, R, n_order, B, max_tries, has_hint, max_hops, nc, n_slot, 0}; then the table as tmpc_law.cpp uploads
//          it -- S[R][np + 1][nrowp] (nrowp = nrow rounded up to 64), K[R][np + 1][ny], int32 order[n_order] --, the batch: P[B][np], int32
//          hint[B] (has_hint only), and uint64 key[R], int32 slot[n_slot]
//     out: double y[B][ny]; int32 region[B]; int32 tries[B]; uint64 hits[R]; uint64 stats[6]
#include "../../robust-tracking-mpc-over-lossy-networks_amd/csrc/tmpc_law.hip"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

namespace {
void need(bool ok, const char *what) {
    if (!ok) { std::fprintf(stderr, "lawhop: %s\n", what); std::exit(2); }
}
template <class T> void rd(FILE *f, T *p, size_t n) { need(std::fread(p, sizeof(T), n, f) == n, "short input file"); }
template <class T> void wr(FILE *f, const T *p, size_t n) { need(std::fwrite(p, sizeof(T), n, f) == n, "short write"); }
template <class T> std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }                      // uninitialised
template <class T> std::unique_ptr<T[]> read_block(FILE *f, size_t n) { auto p = block<T>(n); rd(f, p.get(), n); return p; }

int run_main(FILE *f, FILE *o) {
    int64_t hd[12];
    rd(f, hd, 12);
    need(hd[0] >= 1 && hd[0] <= tmpc::LAW_MAX_NP && hd[1] >= 1 && hd[1] <= tmpc::LAW_MAX_NY && hd[2] >= 0 && hd[3] >= 0 && hd[4] >= 0 && hd[5] >= 1, "bad sizes");
    const size_t np = hd[0], ny = hd[1], nrow = hd[2], R = hd[3], n_order = hd[4], nb = hd[5], nrowp = (nrow + 63) / 64 * 64;
    auto S = read_block<double>(f, R * (np + 1) * nrowp), K = read_block<double>(f, R * (np + 1) * ny);
    auto order = read_block<int32_t>(f, n_order);
    auto P = read_block<double>(f, nb * np);
    auto hint = read_block<int32_t>(f, hd[7] ? nb : 0);
    need(hd[8] >= 0 && hd[9] >= 0 && hd[9] <= hd[2] && hd[10] >= 0 && (hd[10] & (hd[10] - 1)) == 0, "bad hop sizes");
    const size_t n_slot = hd[10];
    auto key = read_block<unsigned long long>(f, R);
    auto slot = read_block<int32_t>(f, n_slot);
    for (size_t i = 0; i < n_slot; ++i) need(slot[i] >= -1 && slot[i] < static_cast<int64_t>(R), "slot entry out of range");
    auto stats = block<unsigned long long>(tmpc::LAW_HOP_STATS);
    std::memset(stats.get(), 0, tmpc::LAW_HOP_STATS * sizeof(unsigned long long));
    for (size_t i = 0; i < n_order; ++i) need(order[i] >= 0 && static_cast<size_t>(order[i]) < R, "order entry out of range");
    auto y = block<double>(nb * ny);
    auto region = block<int32_t>(nb), tries = block<int32_t>(nb);
    auto hits = block<unsigned long long>(R);
    std::memset(hits.get(), 0, R * sizeof(unsigned long long));
    auto table = block<tmpc::LawTable>(1);
    table[0].nrow = static_cast<int>(nrow); table[0].nrowp = static_cast<int>(nrowp); table[0].R = static_cast<int>(R); table[0].n_order = static_cast<int>(n_order);
    table[0].S = S.get(); table[0].K = K.get(); table[0].order = order.get(); table[0].hits = hits.get();
    table[0].nc = static_cast<int>(hd[9]); table[0].key = key.get(); table[0].slot = slot.get(); table[0].n_slot = static_cast<int>(n_slot);
    tmpc::LawArgs a{};
    a.np = static_cast<int>(np); a.ny = static_cast<int>(ny); a.nvariants = 1; a.t = table.get();
    a.B = hd[5]; a.np0 = a.np; a.P0 = P.get(); a.P1 = nullptr; a.variant = nullptr; a.hint = hd[7] ? hint.get() : nullptr; a.max_tries = static_cast<int>(hd[6]);
    a.ny0 = a.ny; a.ny1 = 0; a.Y0 = y.get(); a.Y1 = a.Y2 = nullptr;
    a.region = region.get(); a.tries = tries.get();
    a.max_hops = static_cast<int>(hd[8]); a.hop_stats = stats.get();
    need(tmpc::launch_law(a, 1, nullptr) == hipSuccess, "launch failed");
    wr(o, y.get(), nb * ny);
    wr(o, region.get(), nb);
    wr(o, tries.get(), nb);
    wr(o, hits.get(), R);
    wr(o, stats.get(), static_cast<size_t>(tmpc::LAW_HOP_STATS));
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    need(argc == 4 && std::string(argv[1]) == "run", "usage: lawhop run <in> <out>");
    FILE *f = std::fopen(argv[2], "rb");
    need(f != nullptr, "cannot open the input file");
    FILE *o = std::fopen(argv[3], "wb");
    need(o != nullptr, "cannot open the output file");
    const int rc = run_main(f, o);
    std::fclose(f);
    std::fclose(o);
    return rc;
}
