// Host simulation of the general-size wave FFT in aware_amd/csrc/fft_any.hpp: the 64 lanes of a wavefront run one
// after another between phase boundaries.  Built with hipcc (host code only) by tests/test_fft_any_host_sim.py; prints,
// per real length N, the max errors of rfft / irfft against a double-precision DFT:
//     N <n> rfft_maxerr <e> rfft_maxmag <m> irfft_maxerr <e>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../aware_amd/csrc/fft_any.hpp"

using namespace aware;

template <int M, int P, int DIR> struct SimStages {
    static void run(std::vector<std::vector<cf>>& V, cf* s, const cf* th) {
        constexpr int RAD = fa::stage_radix<M>(P);
        for (int l = 0; l < 64; ++l) fa::stage_load<M, RAD>(l, V[l].data(), s);
        for (int l = 0; l < 64; ++l) fa::stage_store<M, P, RAD, DIR>(l, V[l].data(), s, th);
        if constexpr (P * RAD < M) SimStages<M, P * RAD, DIR>::run(V, s, th);
    }
};

template <int M> static void run_size(unsigned seed) {
    constexpr int N = 2 * M;
    const double PI = 3.14159265358979323846;
    // plan tables as aware_plan_create builds them
    std::vector<cf> th(M / 2), twN(M + 1);
    for (int j = 0; j < M / 2; ++j) th[j] = mk((float)cos(2 * PI * j / M), (float)-sin(2 * PI * j / M));
    for (int k = 0; k <= M; ++k) twN[k] = mk((float)cos(2 * PI * k / N), (float)-sin(2 * PI * k / N));
    twN[0] = mk(1.f, 0.f);
    twN[M / 2] = mk(0.f, -1.f);
    twN[M] = mk(-1.f, 0.f);
    srand(seed);
    std::vector<double> x(N);
    for (auto& v : x) v = (rand() / (double)RAND_MAX) * 2 - 1;
    std::vector<std::vector<cf>> V(64, std::vector<cf>(M / 64));
    std::vector<cf> s(M + 8);

    // ---- forward ----
    for (int j = 0; j < M; ++j) s[j] = mk((float)x[2 * j], (float)x[2 * j + 1]);
    SimStages<M, 1, -1>::run(V, s.data(), th.data());
    std::vector<cf> X(M + 1);
    for (int k = 0; k <= M; ++k) X[k] = fa::rfft_bin<M>(k, s.data(), twN.data());
    double maxerr_f = 0, maxmag = 0;
    std::vector<double> Xr(M + 1), Xi(M + 1);
    for (int k = 0; k <= M; ++k) {
        double re = 0, im = 0;
        for (int n = 0; n < N; ++n) {
            const long kn = ((long)k * n) % N;
            re += x[n] * cos(2 * PI * kn / N);
            im -= x[n] * sin(2 * PI * kn / N);
        }
        Xr[k] = re;
        Xi[k] = im;
        maxerr_f = fmax(maxerr_f, fmax(fabs(re - X[k].x), fabs(im - X[k].y)));
        maxmag = fmax(maxmag, hypot(re, im));
    }

    // ---- inverse of the exact spectrum (imaginary parts of DC and Nyquist ignored, as irfft does) ----
    for (int k = 0; k <= M; ++k) s[k] = mk((float)Xr[k], (k == 0 || k == M) ? 0.f : (float)Xi[k]);
    for (int l = 0; l < 64; ++l) fa::irfft_merge_lane<M>(l, s.data(), twN.data());
    SimStages<M, 1, 1>::run(V, s.data(), th.data());
    double maxerr_i = 0;
    for (int n = 0; n < M; ++n) {
        const double a = s[n].x / (double)M, b = s[n].y / (double)M;
        maxerr_i = fmax(maxerr_i, fmax(fabs(a - x[2 * n]), fabs(b - x[2 * n + 1])));
    }
    printf("N %d rfft_maxerr %.3e rfft_maxmag %.3e irfft_maxerr %.3e\n", N, maxerr_f, maxmag, maxerr_i);
}

int main() {
    run_size<128>(11);
    run_size<256>(12);
    run_size<512>(13);
    run_size<1024>(14);
    run_size<2048>(15);
    return 0;
}
