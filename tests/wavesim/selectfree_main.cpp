// TEST INFRASTRUCTURE (not product code): the select-free factorisation and back substitution of csrc/tmpc_wave.hpp
// (wv::rows16_factor_masked, wv::rows16_backsub_lane_masked: the instructions that depend on a lane's place run under a constant
// EXEC pattern) against the forms with a select per use, on the host execution model of hip_sim.hpp.  The reference below is a COPY
// of the select forms as they stood when the masked forms were written -- it stays here whatever the header does later.
// tests/test_select_free_host.py builds this plain, under ASan + UBSan and under MSan; tests/test_select_free_gpu.py compares the
// device with the `select` half of the output.
//
//   selectfree <n> <in.bin> <out.bin>
// in.bin: P problems, the layout of wavecheck_lanes: rows[P][64][n] (the matrix row every lane holds), b1[P][64], b2[P][64].
// out.bin: for the reference, then for the masked forms: frows[P][64][n], dinv[P][64], x[P][64], x2[P][64], ok[P][64] (as doubles),
// from: factor with b1 carried, back substitution; forward substitution of b2, back substitution (k_lanes of wavecheck.hip).
// Exit code 1 if the two halves differ in any bit, 2 for a usage error.
#include "hip_sim.hpp"
#include "tmpc_wave.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace {

namespace wv = tmpc::wv;
constexpr int L = wv::WAVE;

// ---- the reference: the select forms (host model: fma of a DPP broadcast)
template <int N>
bool ref_factor(double (&row)[N], double &b, double &dinv, int lane) {
    const int l16 = lane & 15;
    bool ok = true;
    double pkk = wv::row_bcast_d<0>(row[0]);
    double pinv = wv::fast_rcp(pkk);
    wv::static_for_n<N>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        ok = ok && (pkk > 0.0);
        const double pinv_k = pinv;
        const double f = (l16 > k) ? row[k] * pinv_k : 0.0;
        const double nf = -f;
        constexpr int NU = N - 1 - k;
        wv::static_for_n<(NU < 3 ? NU : 3)>([&](auto j_) {
            constexpr int j = k + 1 + decltype(j_)::value;
            row[j] = fma(wv::row_bcast_d<k>(row[j]), nf, row[j]);
        });
        if constexpr (NU < 3) b = fma(wv::row_bcast_d<k>(b), nf, b);
        if constexpr (k + 1 < N) {
            pkk = wv::row_bcast_d<k + 1>(row[k + 1]);
            pinv = wv::fast_rcp(pkk);
        }
        if constexpr (NU >= 3) {
            wv::static_for_n<NU - 3>([&](auto j_) {
                constexpr int j = k + 4 + decltype(j_)::value;
                row[j] = fma(wv::row_bcast_d<k>(row[j]), nf, row[j]);
            });
            b = fma(wv::row_bcast_d<k>(b), nf, b);
        }
        if (l16 > k) row[k] = f;
        if (l16 == k) dinv = pinv_k;
    });
    return __builtin_amdgcn_readfirstlane(static_cast<int>(ok)) != 0;
}
template <int N>
void ref_forward(const double (&row)[N], double &b, int lane) {
    const int l16 = lane & 15;
    wv::static_for_n<N - 1>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        const double f = (l16 > k) ? row[k] : 0.0;
        b = fma(-f, wv::row_bcast_d<k>(b), b);
    });
}
template <int N>
double ref_backsub_lane(const double (&row)[N], double b, double dinv, int lane) {
    const int l16 = lane & 15;
    double xl = 0.0;
    wv::static_for_n<N>([&](auto r_) {
        constexpr int i = N - 1 - decltype(r_)::value;
        const double bi = b * dinv;
        const double xi = wv::row_bcast_d<i>(bi);
        xl = (l16 == i) ? bi : xl;
        b = fma(-row[i], xi, b);
    });
    return xl;
}

struct Out {
    std::vector<double> frows, dinv, x, x2, ok;
    void size(size_t P, int n) {
        frows.assign(P * L * n, 0.0);
        dinv.assign(P * L, 0.0);
        x.assign(P * L, 0.0);
        x2.assign(P * L, 0.0);
        ok.assign(P * L, 0.0);
    }
    void write(FILE *f) const {
        for (const auto *v : {&frows, &dinv, &x, &x2, &ok}) std::fwrite(v->data(), sizeof(double), v->size(), f);
    }
    bool same(const Out &o) const {
        auto eq = [](const std::vector<double> &a, const std::vector<double> &b) {
            return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
        };
        return eq(frows, o.frows) && eq(dinv, o.dinv) && eq(x, o.x) && eq(x2, o.x2) && eq(ok, o.ok);
    }
};

template <int N, bool MASKED>
void run(const double *rows, const double *b1, const double *b2, size_t P, Out &out) {
    out.size(P, N);
    for (size_t p = 0; p < P; ++p) {
        sim::Dim3 bi, gd;
        bi.x = bi.y = bi.z = 0;
        sim::run_block(L, 0, bi, gd, [&]() {
            const int lane = static_cast<int>(threadIdx.x);
            const size_t at = p * L + lane;
            double row[N];
            for (int j = 0; j < N; ++j) row[j] = rows[at * N + j];
            double b = b1[at], d = 1.0, bb = b2[at];
            bool o;
            double xl, xl2;
            if constexpr (MASKED) {
                o = wv::rows16_factor_masked<N>(row, b, d, lane);
                xl = wv::rows16_backsub_lane_masked<N>(row, b, d, lane);
                wv::rows16_forward<N>(row, bb, lane);
                xl2 = wv::rows16_backsub_lane_masked<N>(row, bb, d, lane);
            } else {
                o = ref_factor<N>(row, b, d, lane);
                xl = ref_backsub_lane<N>(row, b, d, lane);
                ref_forward<N>(row, bb, lane);
                xl2 = ref_backsub_lane<N>(row, bb, d, lane);
            }
            for (int j = 0; j < N; ++j) out.frows[at * N + j] = row[j];
            out.dinv[at] = d;
            out.x[at] = xl;
            out.x2[at] = xl2;
            out.ok[at] = o ? 1.0 : 0.0;
        });
    }
}

template <int N>
int both(const std::vector<double> &in, size_t P, FILE *fo) {
    const double *rows = in.data(), *b1 = rows + P * L * N, *b2 = b1 + P * L;
    Out ref, msk;
    run<N, false>(rows, b1, b2, P, ref);
    run<N, true>(rows, b1, b2, P, msk);
    ref.write(fo);
    msk.write(fo);
    return ref.same(msk) ? 0 : 1;
}

template <int... V>
int dispatch(int n, std::integer_sequence<int, V...>, const std::vector<double> &in, size_t P, FILE *fo) {
    int rc = 2;
    ((n == V ? (rc = both<V>(in, P, fo), 0) : 0), ...);
    return rc;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s n in.bin out.bin\n", argv[0]);
        return 2;
    }
    const int n = std::atoi(argv[1]);
    if (n < 1 || n > 16) return 2;
    FILE *fi = std::fopen(argv[2], "rb");
    if (!fi) return 2;
    std::vector<double> in;
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, fi)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(fi);
    const size_t per = static_cast<size_t>(L) * (n + 2);
    if (in.empty() || in.size() % per != 0) return 2;
    FILE *fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    const int rc = dispatch(n, std::integer_sequence<int, 1, 2, 8, 11, 12, 16>{}, in, in.size() / per, fo);
    std::fclose(fo);
    if (rc == 1) std::fprintf(stderr, "selectfree: the masked forms and the select forms differ (n = %d)\n", n);
    return rc;
}
