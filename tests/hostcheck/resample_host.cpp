// Host build of the resampling arithmetic (gapflow_amd/csrc/resample.hpp: resample_axis, resample_cell), driven over whole
// grids the way k_resample drives it.  stdin, all doubles: nxs, nys, nxd, nyd, dxs, dys, dxd, dyd; the source's ghosted fields
// rho, jx, jy, h as [4][nxs + 2][nys + 2]; the destination's ghosted gap [nxd + 2][nyd + 2].  stdout: the destination's interior
// rho, jx, jy as [3][nxd][nyd].  tests/test_resample_host.py compares with NumPy under -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "../../gapflow_amd/csrc/resample.hpp"

int main() {
    double head[8];
    if (std::fread(head, sizeof(double), 8, stdin) != 8) return 2;
    const int nxs = (int)head[0], nys = (int)head[1], nxd = (int)head[2], nyd = (int)head[3];
    if (nxs < 1 || nys < 1 || nxd < 1 || nyd < 1) return 2;
    const double rx = head[6] / head[4], ry = head[7] / head[5];
    const size_t ws = (size_t)nys + 2, ns = ((size_t)nxs + 2) * ws, wd = (size_t)nyd + 2, nd = ((size_t)nxd + 2) * wd;
    std::vector<double> src(4 * ns), hd(nd), out((size_t)3 * nxd * nyd);
    if (std::fread(src.data(), sizeof(double), src.size(), stdin) != src.size()) return 2;
    if (std::fread(hd.data(), sizeof(double), hd.size(), stdin) != hd.size()) return 2;
    const bool unit_x = nxs == 1 && nxd == 1, unit_y = nys == 1 && nyd == 1;
    for (int ix = 1; ix <= nxd; ++ix) {
        const gpf::ResampleAxis ax = gpf::resample_axis(ix, rx, nxs, unit_x);
        for (int iy = 1; iy <= nyd; ++iy) {
            const gpf::ResampleAxis ay = gpf::resample_axis(iy, ry, nys, unit_y);
            const size_t o0 = (size_t)ax.i0 * ws + (size_t)ay.i0, o1 = o0 + ws;
            double f[4][4];
            for (int p = 0; p < 4; ++p) {
                const double* b = src.data() + (size_t)p * ns;
                f[p][0] = b[o0]; f[p][1] = b[o0 + 1]; f[p][2] = b[o1]; f[p][3] = b[o1 + 1];
            }
            const gpf::ResampleOut c = gpf::resample_cell(f[0], f[1], f[2], f[3], ax.w, ay.w, hd[(size_t)ix * wd + (size_t)iy]);
            const size_t k = (size_t)(ix - 1) * nyd + (size_t)(iy - 1), m = (size_t)nxd * nyd;
            out[k] = c.rho; out[m + k] = c.jx; out[2 * m + k] = c.jy;
        }
    }
    std::fwrite(out.data(), sizeof(double), out.size(), stdout);
    return 0;
}
