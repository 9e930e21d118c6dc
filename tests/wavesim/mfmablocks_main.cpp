// TEST INFRASTRUCTURE (not product code): wv::gdg_blocks of csrc/tmpc_wave.hpp -- the G'DG pass of sweep A on 4 x 4 x 4 matrix blocks, with
// the host emulation of v_mfma_f64_4x4x4_4b_f64 -- on the host execution model of hip_sim.hpp.  tests/test_mfma_blocks_gpu.py builds it and
// compares what it writes with the device's (tests/wavecheck/mfmablocks.hip: the same staging).
//
//   mfmablocks_sim <nv> <nks> <np> <in.bin> <out.bin>
// in.bin, per problem: G[4 nks][nv], D[4 nks], t[4 nks].  out.bin, per problem: mf[nv][ldm] (pre-filled with the sentinel), gdr[nv].
#include "hip_sim.hpp"
#include "tmpc_wave.hpp"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

namespace {

constexpr int L = tmpc::wv::WAVE;
constexpr int ZERO_ROWS = 4;
constexpr double SENTINEL = -7.0e77;
constexpr int odd_up(int v) { return v | 1; }

template <int NV>
void run(int nks, const double *G, const double *D, const double *t, double *mf, double *gdr) {
    constexpr int LDG = 16 * ((NV + 1 + 15) / 16) + 1, LDM = odd_up(NV + 1);
    const int rows = 4 * nks;
    const size_t n_gt = static_cast<size_t>(rows + ZERO_ROWS) * LDG, n_dt = 2 * static_cast<size_t>(rows + ZERO_ROWS);
    sim::Dim3 bi, gd;
    bi.x = bi.y = bi.z = 0;
    sim::run_block(L, sizeof(double) * (n_gt + n_dt + NV * LDM + NV), bi, gd, [&]() {
        const int lane = static_cast<int>(threadIdx.x);
        double *Gt = sim::lds<double>(), *dtw = Gt + n_gt, *mt = dtw + n_dt, *gv = mt + NV * LDM;
        for (int e = lane; e < static_cast<int>(n_gt); e += L) {
            const int f = e / LDG, j = e - f * LDG;
            Gt[e] = (f < rows && j < NV) ? G[f * NV + j] : (f < rows && j == NV) ? 1.0 : 0.0;
        }
        for (int f = lane; f < rows + ZERO_ROWS; f += L) {
            dtw[2 * f] = f < rows ? D[f] : 0.0;
            dtw[2 * f + 1] = f < rows ? t[f] : 0.0;
        }
        for (int e = lane; e < NV * LDM; e += L) mt[e] = SENTINEL;
        if (lane < NV) gv[lane] = SENTINEL;
        __syncthreads();
        tmpc::wv::gdg_blocks<NV, LDG, LDM>(Gt, nks, dtw, mt, gv, lane);
        __syncthreads();
        for (int e = lane; e < NV * LDM; e += L) mf[e] = mt[e];
        if (lane < NV) gdr[lane] = gv[lane];
    });
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s nv nks np in.bin out.bin\n", argv[0]);
        return 2;
    }
    const int nv = std::atoi(argv[1]), nks = std::atoi(argv[2]), np = std::atoi(argv[3]);
    if ((nv != 8 && nv != 11 && nv != 12 && nv != 22) || nks < 1 || nks > 16 || np < 1 || np > 4096) return 2;
    const size_t rows = 4 * static_cast<size_t>(nks), per_in = rows * nv + 2 * rows, per_out = static_cast<size_t>(nv) * odd_up(nv + 1) + nv;
    std::vector<double> in(per_in * np), out(per_out * np);
    FILE *fi = std::fopen(argv[4], "rb");
    if (!fi || std::fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);
    for (int p = 0; p < np; ++p) {
        const double *G = in.data() + per_in * p, *D = G + rows * nv, *t = D + rows;
        double *mf = out.data() + per_out * p, *gdr = mf + static_cast<size_t>(nv) * odd_up(nv + 1);
        if (nv == 8) run<8>(nks, G, D, t, mf, gdr);
        else if (nv == 11) run<11>(nks, G, D, t, mf, gdr);
        else if (nv == 12) run<12>(nks, G, D, t, mf, gdr);
        else run<22>(nks, G, D, t, mf, gdr);
    }
    FILE *fo = std::fopen(argv[5], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 2;
    std::fclose(fo);
    return 0;
}
