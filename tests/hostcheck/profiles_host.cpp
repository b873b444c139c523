// Host build of the through-gap profile arithmetic (gapflow_amd/csrc/closures.hpp: profile_slip, profile_coefficients,
// profile_at) for the CPU sanitizer test tests/test_hostcheck_profiles.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all profiles_host.cpp -o profiles_host
// Reads little-endian doubles from stdin: [ncase], then per case [mode, nz, n, has_h, U, V], z [nz][n], q [3][n],
// (hh [3][n] if has_h), dqx [3][n], dqy [3][n], eta [n], zeta [n], Ls [n].  Writes per case u, v, tau_xx .. tau_xy as
// [8][nz][n] doubles to stdout.  Without hh the gap height is the cell's last z (get_velocity_profiles).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gapflow_amd/csrc/closures.hpp"

using namespace gpf;

static std::vector<double> rd(size_t n) {
    std::vector<double> v(n);
    if (n && std::fread(v.data(), sizeof(double), n, stdin) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return v;
}

int main() {
    const size_t ncase = (size_t)rd(1)[0];
    for (size_t c = 0; c < ncase; ++c) {
        const std::vector<double> hd = rd(6);
        const int mode = (int)hd[0], nz = (int)hd[1];
        const size_t n = (size_t)hd[2];
        const bool has_h = hd[3] != 0.0;
        const std::vector<double> z = rd((size_t)nz * n), q = rd(3 * n);
        const std::vector<double> hh = has_h ? rd(3 * n) : std::vector<double>();
        const std::vector<double> dqx = rd(3 * n), dqy = rd(3 * n), eta = rd(n), zeta = rd(n), Ls = rd(n);
        std::vector<double> out((size_t)8 * nz * n);
        for (size_t i = 0; i < n; ++i) {
            const double qq[3] = {q[i], q[n + i], q[2 * n + i]};
            const double h[3] = {has_h ? hh[i] : z[(size_t)(nz - 1) * n + i], has_h ? hh[n + i] : 0.0, has_h ? hh[2 * n + i] : 0.0};
            const double gx[3] = {dqx[i], dqx[n + i], dqx[2 * n + i]}, gy[3] = {dqy[i], dqy[n + i], dqy[2 * n + i]};
            double lo, hi;
            profile_slip(mode, Ls[i], lo, hi);
            ProfileCoef pc;
            profile_coefficients(qq, h, gx, gy, hd[4], hd[5], eta[i], zeta[i], lo, hi, pc);
            for (int k = 0; k < nz; ++k) {
                double o[8];
                profile_at(pc, z[(size_t)k * n + i], o);
                for (int f = 0; f < 8; ++f) out[((size_t)f * nz + k) * n + i] = o[f];
            }
        }
        std::fwrite(out.data(), sizeof(double), out.size(), stdout);
    }
    return 0;
}
