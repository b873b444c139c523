// Host build of the two Dowson-Higginson pressures of gapflow_amd/csrc/closures.hpp, for tests/test_integrals_host.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all film_pressure_host.cpp -o film_pressure_host
// Reads little-endian doubles from stdin: [n], the law's 8 parameters (rho0, P0, C1, C2, padding), n densities; writes
// eos_pressure<EOS_DH> of each, then film_pressure<EOS_DH> of each.  No GPU, no HIP: the same header the kernels compile.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gapflow_amd/csrc/phys_setup.hpp"

using namespace gpf;

static std::vector<double> rd(size_t n) {
    std::vector<double> v(n);
    if (n && std::fread(v.data(), sizeof(double), n, stdin) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return v;
}

int main() {
    const double zero4[4] = {0, 0, 0, 0};
    const size_t n = (size_t)rd(1)[0];
    const std::vector<double> par = rd(8), rho = rd(n);
    Phys P;
    setup_phys(P, 0.1, 0.0, 0.1, 0.0, 1e-5, 1e-5, EOS_DH, par.data(), PIEZO_NONE, zero4, THIN_NONE, zero4);
    std::vector<double> a(n), b(n);
    for (size_t i = 0; i < n; ++i) { a[i] = eos_pressure<EOS_DH>(rho[i], P); b[i] = film_pressure<EOS_DH>(rho[i], P); }
    std::fwrite(a.data(), sizeof(double), n, stdout);
    std::fwrite(b.data(), sizeof(double), n, stdout);
    return 0;
}
