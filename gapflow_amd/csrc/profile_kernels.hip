// Through-gap velocity and stress profiles (models/profiles.py; entry points in api_profiles.inc).
//
// The kernel is store-bound by a wide margin: per (cell, level) it writes up to 9 doubles (72 B) from about 25 fp64
// operations, the per-cell work (slip parabola, chain-rule terms, viscosity) being folded once into the Horner
// coefficients of closures.hpp: profile_coefficients.  So the layout serves the stores: planes [field][level][cell], a lane
// owns two neighbouring cells and writes 16 bytes per plane (a wave: 1 KiB contiguous per plane), every store carries the
// non-temporal hint (nothing on the device reads the result again), and only the requested planes are written.  A thread
// covers PROFILE_LEVELS_PER_THREAD levels of its cell pair: the grid's y dimension runs over the level groups, so a chunk of a
// few dozen rows still puts thousands of waves on the device.
#pragma once

namespace gpf {

enum { PROFILE_F_Z = 1, PROFILE_F_U = 2, PROFILE_F_V = 4, PROFILE_F_TAU = 8 };
static constexpr int PROFILE_LEVELS_PER_THREAD = 4;

typedef double pf_d2 __attribute__((ext_vector_type(2)));

struct ProfileOut {
    double* out;            // planes of the requested fields, order z, u, v, xx, yy, zz, yz, xz, xy; each [level][cell]
    long long pitch;        // doubles per (field, level) plane: ncell rounded up to even (16-byte aligned pairs)
    long long ncell;
    int nlev, mask;
};

// Operator form: n cells from arrays.  Bit b of `per_cell` set: input b is [comp][n] (else one value for every cell);
// bits: 0 q, 1 hh, 2 dqx, 3 dqy, 4 eta, 5 zeta, 6 Ls, 7 z ([nz][n] instead of [nz]).  hh NULL: the gap height is the cell's
// last z and the slopes are zero (get_velocity_profiles, profiles.py:58); dqx / dqy NULL: zero gradients.
struct ProfileOpSource {
    const double *q, *hh, *dqx, *dqy, *eta, *zeta, *Ls, *z;
    long long n;
    int per_cell, nz, mode;
    double U, V;
    __device__ __forceinline__ double ld(const double* p, int bit, int comp, long long i) const {
        return (per_cell >> bit) & 1 ? p[comp * n + i] : p[comp];
    }
    __device__ __forceinline__ double zat(long long i, int k) const { return ld(z, 7, k, i); }
    __device__ __forceinline__ void cell(long long i, ProfileCoef& c) const {
        double qq[3], h[3], gx[3] = {0.0, 0.0, 0.0}, gy[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; ++k) {
            qq[k] = ld(q, 0, k, i);
            if (dqx) gx[k] = ld(dqx, 2, k, i);
            if (dqy) gy[k] = ld(dqy, 3, k, i);
        }
        if (hh) { for (int k = 0; k < 3; ++k) h[k] = ld(hh, 1, k, i); }
        else { h[0] = zat(i, nz - 1); h[1] = h[2] = 0.0; }
        double lo, hi;
        profile_slip(mode, ld(Ls, 6, 0, i), lo, hi);
        profile_coefficients(qq, h, gx, gy, U, V, ld(eta, 4, 0, i), ld(zeta, 5, 0, i), lo, hi, c);
    }
};

// Problem form: ghosted rows [ix0, ix0 + rows) of a handle's state and gap, levels k0.. of z_k = h k / (nz - 1).  The
// closures' own viscosity (cell_fields: piezo_eta of the EOS pressure, of the density for Bayada-Chupin), slip at the
// upper wall only (stress.py:328-345); gradients, when asked for, by np.gradient's stencil over the ghosted field.
template <int EOS>
struct ProfileGridSource {
    const double *q, *topo, *Ls;
    Layout L;
    Phys P;
    double dx, dy;
    int ix0, width, nz, k0, grad;
    __device__ __forceinline__ double zfrac(int k) const { return (double)(k0 + k) / (double)(nz - 1); }
    __device__ __forceinline__ void cell(long long i, ProfileCoef& c, double& h) const {
        const int ix = ix0 + (int)(i / width), iy = (int)(i % width);
        const long long o = L.at(ix, iy);
        double qq[3], hh[3], gx[3] = {0.0, 0.0, 0.0}, gy[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; ++k) { qq[k] = q[o + k * L.plane]; hh[k] = topo[o + k * L.plane]; }
        if (grad) {
            const int nxg = L.Nx + 2, nyg = L.Ny + 2;
            const int xl = ix > 0 ? ix - 1 : 0, xh = ix < nxg - 1 ? ix + 1 : nxg - 1;
            const int yl = iy > 0 ? iy - 1 : 0, yh = iy < nyg - 1 ? iy + 1 : nyg - 1;
            const double sx = (xh - xl == 2) ? 2.0 : 1.0, sy = (yh - yl == 2) ? 2.0 : 1.0;
            for (int k = 0; k < 3; ++k) {
                const double* f = q + k * L.plane;
                gx[k] = ((f[L.at(xh, iy)] - f[L.at(xl, iy)]) / sx) / dx;
                gy[k] = ((f[L.at(ix, yh)] - f[L.at(ix, yl)]) / sy) / dy;
            }
        }
        const double eta = P.piezo == PIEZO_NONE ? P.eta
                         : piezo_eta(P.eta, EOS == EOS_BAYADA ? qq[0] : eos_pressure<EOS>(qq[0], P), P);
        profile_coefficients(qq, hh, gx, gy, P.U, P.V, eta, P.zeta, 0.0, Ls ? Ls[o] : 0.0, c);
        h = hh[0];
    }
};

__device__ __forceinline__ void profile_put(const ProfileOut& o, int& f, int k, long long i, bool pair, double x, double y) {
    double* d = o.out + ((long long)f * o.nlev + k) * o.pitch + i;
    if (pair) __builtin_nontemporal_store(pf_d2{x, y}, reinterpret_cast<pf_d2*>(d));
    else __builtin_nontemporal_store(x, d);
    ++f;
}

__device__ __forceinline__ void profile_level(const ProfileOut& o, int k, long long i, bool pair, const ProfileCoef& c0,
                                              const ProfileCoef& c1, double z0, double z1) {
    double a[8], b[8];
    profile_at(c0, z0, a);
    profile_at(c1, z1, b);
    int f = 0;
    if (o.mask & PROFILE_F_Z) profile_put(o, f, k, i, pair, z0, z1);
    if (o.mask & PROFILE_F_U) profile_put(o, f, k, i, pair, a[0], b[0]);
    if (o.mask & PROFILE_F_V) profile_put(o, f, k, i, pair, a[1], b[1]);
    if (o.mask & PROFILE_F_TAU)
        for (int t = 0; t < 6; ++t) profile_put(o, f, k, i, pair, a[2 + t], b[2 + t]);
}

// grid: x over cell pairs, y over groups of PROFILE_LEVELS_PER_THREAD levels
__global__ __launch_bounds__(256) void k_gap_profiles_op(const ProfileOpSource s, const ProfileOut o) {
    const long long i = 2 * (blockIdx.x * 256ll + threadIdx.x);
    if (i >= o.ncell) return;
    const long long i1 = i + 1 < o.ncell ? i + 1 : i;
    ProfileCoef c0, c1;
    s.cell(i, c0);
    s.cell(i1, c1);
    const int k0 = blockIdx.y * PROFILE_LEVELS_PER_THREAD, k1 = min(k0 + PROFILE_LEVELS_PER_THREAD, o.nlev);
    for (int k = k0; k < k1; ++k) profile_level(o, k, i, i1 != i, c0, c1, s.zat(i, k), s.zat(i1, k));
}

template <int EOS>
__global__ __launch_bounds__(256) void k_gap_profiles(const ProfileGridSource<EOS> s, const ProfileOut o) {
    const long long i = 2 * (blockIdx.x * 256ll + threadIdx.x);
    if (i >= o.ncell) return;
    const long long i1 = i + 1 < o.ncell ? i + 1 : i;
    ProfileCoef c0, c1;
    double h0, h1;
    s.cell(i, c0, h0);
    s.cell(i1, c1, h1);
    const int k0 = blockIdx.y * PROFILE_LEVELS_PER_THREAD, k1 = min(k0 + PROFILE_LEVELS_PER_THREAD, o.nlev);
    for (int k = k0; k < k1; ++k) {
        const double t = s.zfrac(k);
        profile_level(o, k, i, i1 != i, c0, c1, h0 * t, h1 * t);
    }
}

// The yardstick of tools/profile_time.py: the same grid, the same planes and the same non-temporal 16-byte stores as
// k_gap_profiles, with no input and no arithmetic.
__global__ __launch_bounds__(256) void k_profile_store_only(const ProfileOut o, int nplanes) {
    const long long i = 2 * (blockIdx.x * 256ll + threadIdx.x);
    if (i >= o.ncell) return;
    const bool pair = i + 1 < o.ncell;
    const int k0 = blockIdx.y * PROFILE_LEVELS_PER_THREAD, k1 = min(k0 + PROFILE_LEVELS_PER_THREAD, o.nlev);
    for (int k = k0; k < k1; ++k) {
        int f = 0;
        for (int p = 0; p < nplanes; ++p) profile_put(o, f, k, i, pair, (double)k, (double)p);
    }
}

}  // namespace gpf
