// TEST INFRASTRUCTURE (not product code): the register wave sums of csrc/tmpc_wave.hpp -- wv::swap_reduce_to_lds (cross-half
// swaps, then one round of the transposition tile) and wv::wave_sum2 -- on the host execution model of hip_sim.hpp, for every
// count of values 1 ... 32 and both tile heights the kernels use (12 and 16 rows), and for 44 and 52 values on the 12-row tile
// (sweep B of the N = 20 shapes; 52 values take two rounds).  tests/test_wave_swap_reduce.py builds it and checks the totals.
//
//   swapsum <in.bin> <out.bin>
// in.bin: D data sets of [52][64] doubles (value c of lane l at c * 64 + l).  out.bin, per data set: for RR = 12, 16 and
// CNT = 1 ... 32, then RR = 12 and CNT = 44, 52, what every lane reads back from out[0 .. CNT) after the reduction ([64][CNT]
// doubles), then wave_sum2 of values 0 and 1 on every lane ([64][2]).
#include "hip_sim.hpp"
#include "tmpc_wave.hpp"

#include <cstdio>
#include <utility>
#include <vector>

namespace {

constexpr int MAXC = 52;
constexpr int L = tmpc::wv::WAVE;

template <int CNT, int RR>
void run_reduce(const double *in, std::vector<double> &res) {
    res.assign(static_cast<size_t>(L) * CNT, 0.0);
    const size_t lds = sizeof(double) * (static_cast<size_t>(RR) * tmpc::wv::RED_STRIDE + CNT);
    sim::Dim3 bi, gd;
    bi.x = bi.y = bi.z = 0;
    sim::run_block(L, lds, bi, gd, [&]() {
        const int lane = static_cast<int>(threadIdx.x);
        double *red = sim::lds<double>();
        double *out = red + RR * tmpc::wv::RED_STRIDE;
        double acc[CNT];
        for (int c = 0; c < CNT; ++c) acc[c] = in[c * L + lane];
        tmpc::wv::swap_reduce_to_lds<CNT, RR>(acc, red, out, lane);
        for (int c = 0; c < CNT; ++c) res[static_cast<size_t>(lane) * CNT + c] = out[c];
    });
}

void run_sum2(const double *in, std::vector<double> &res) {
    res.assign(2 * L, 0.0);
    sim::Dim3 bi, gd;
    bi.x = bi.y = bi.z = 0;
    sim::run_block(L, 0, bi, gd, [&]() {
        const int lane = static_cast<int>(threadIdx.x);
        double a = in[lane], b = in[L + lane];
        tmpc::wv::wave_sum2(a, b, lane);
        res[2 * lane] = a;
        res[2 * lane + 1] = b;
    });
}

template <int RR, int... C>
void all_counts(const double *in, FILE *f, std::integer_sequence<int, C...>) {
    std::vector<double> res;
    auto one = [&](auto cnt) {
        run_reduce<decltype(cnt)::value, RR>(in, res);
        std::fwrite(res.data(), sizeof(double), res.size(), f);
    };
    (one(std::integral_constant<int, C + 1>{}), ...);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    std::vector<double> data;
    double buf[MAXC * L];
    while (std::fread(buf, sizeof(double), MAXC * L, fi) == MAXC * L) data.insert(data.end(), buf, buf + MAXC * L);
    std::fclose(fi);
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    for (size_t off = 0; off < data.size(); off += MAXC * L) {
        const double *in = data.data() + off;
        all_counts<12>(in, fo, std::make_integer_sequence<int, 32>{});
        all_counts<16>(in, fo, std::make_integer_sequence<int, 32>{});
        std::vector<double> res;
        run_reduce<44, 12>(in, res);
        std::fwrite(res.data(), sizeof(double), res.size(), fo);
        run_reduce<52, 12>(in, res);
        std::fwrite(res.data(), sizeof(double), res.size(), fo);
        run_sum2(in, res);
        std::fwrite(res.data(), sizeof(double), res.size(), fo);
    }
    std::fclose(fo);
    return 0;
}
