// Shear-thinning series (entry points in api_thinning_series.inc): what a thinning film carries and what it costs its walls, per
// recorded step over the interior cells 1..Nx x 1..Ny of the COMMITTED state, with the gap and the slip length the handle holds.
// Per cell, as k_pressure + k_fields_thinning (aux_kernels.hip) evaluate an interior cell:
//   p      eos_pressure<EOS> of the density, at the cell and its four neighbours (ghost cells are neighbours), each rounded on
//          its own as the pressure plane there is
//   dpx    (p[ix + 1, iy] - p[ix - 1, iy]) / (2 dx),  dpy = (p[ix, iy + 1] - p[ix, iy - 1]) / (2 dy): np.gradient's central
//          difference; an interior cell has both neighbours, so the one-sided ends never occur
//   mu0    the Newtonian viscosity, piezo-viscosity included (of p; of the density for Bayada-Chupin)
//   rate   closures.hpp: shear_rate_avg(dpx, dpy, h, U, V, mu0)
//   eta    closures.hpp: thinning_eta(mu0, dpx, dpy, h, P) = mu0 * thinning_factor(rate, mu0)
// and cell_fields<EOS>(c, P, ., eta) for the thinned wall stresses, cell_fields<EOS>(c, P, .) for the Newtonian ones.
// A record is eleven sums times dx dy -- load (film_pressure<EOS>, the film integrals' load), tau_xz_bot, tau_yz_bot, tau_xz_top,
// tau_yz_top (lower[4], lower[3], upper[4], upper[3] with eta), the same four with mu0 (tau0_*: what the film would cost without
// thinning), eta_sum, rate_sum -- and eta_min, eta_max, rate_max, each with its cell (ix, iy) of the ghosted index space.
//
// The two launches per record, the guard, the fold tree and the row loop of the sums are series_rows.hpp's; the walk is its
// row_pairs_cross (row_pairs' pairs, order and loads, and the density's 5-point stencil); the three extrema -- their order,
// accumulator, folds and stores -- are series_first.hpp's:
//   k_thin_partial   one 256-thread workgroup per interior row; reads 6 planes (7 with a slip-length field) once and the density
//                    of the two neighbouring rows, which the workgroups of those rows read too (L2); six equations of state per
//                    cell, in registers; thread 0 stores the row's eleven sums and its three extrema with their columns.
//   k_thin_fold      one workgroup; thread 0 applies dx dy and stores the record.
// The sums go through block_sum and fold_rows: who adds what depends on (Nx, Ny) alone.  eta and rate are rounded on their own
// before they are added (weighted_kernels.hip: the canonicalize between product and sum), so a NumPy restatement of the terms
// from the device's leaf operators meets the device's.  A record is a pure function of (q, gap, Ls): no floating-point atomics,
// the same bits for every stride and for the wide and narrow loads.
#pragma once

#include "series_first.hpp"

namespace gpf {

constexpr int THIN_NSUM = 11;           // load tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top tau0_xz_bot tau0_yz_bot tau0_xz_top tau0_yz_top eta_sum rate_sum
constexpr int THIN_NEXT = 3;            // eta_min eta_max rate_max
constexpr int THIN_NREC = THIN_NSUM + THIN_NEXT;

struct ThinArgs {
    const double *qa, *qb, *topo, *Ls;
    const StepState* st;
    double* part;           // [Nx][THIN_NSUM]
    double* row_val;        // [Nx][3]: the row's eta_min, eta_max, rate_max
    int* row_iy;            // [Nx][3]: their columns
    double* rec;            // [cap + 1][THIN_NREC]: the eleven sums, eta_min, eta_max, rate_max
    int* cell;              // [cap + 1][3][2]: (ix, iy) of eta_min, of eta_max, of rate_max
    Layout L;
    double dx, dy;
    int wide;               // 16-byte pair loads are aligned
    long long slot, cap;    // record to write; slots the buffer holds
};

using ThinAcc = RowAcc<THIN_NSUM>;
using ThinExt = FirstAcc<THIN_NEXT, 0b001>;     // eta_min (k = 0), eta_max (k = 1), rate_max (k = 2)

// The pressure as k_pressure stores it: rounded before anything is done with it
template <int EOS> __device__ __forceinline__ double thin_pressure(double rho, const Phys& P) { return __builtin_canonicalize(eos_pressure<EOS>(rho, P)); }

// One cell's terms
template <int EOS>
__device__ __forceinline__ void thin_cell(ThinAcc& a, ThinExt& e, const ThinArgs& f, const Phys& P, const CellIn& c, const RhoCross& s, int ix, int iy) {
    const double pc = thin_pressure<EOS>(c.rho, P);
    double dpx, dpy;
    {
#pragma clang fp contract(off)
        dpx = (thin_pressure<EOS>(s.xp, P) - thin_pressure<EOS>(s.xm, P)) / (2 * f.dx);
        dpy = (thin_pressure<EOS>(s.yp, P) - thin_pressure<EOS>(s.ym, P)) / (2 * f.dy);
    }
    const double mu0 = (P.piezo == PIEZO_NONE) ? P.eta : piezo_eta(P.eta, (EOS == EOS_BAYADA) ? c.rho : pc, P);
    const double rate = __builtin_canonicalize(shear_rate_avg(dpx, dpy, c.h, P.U, P.V, mu0));
    const double eta = thinning_eta(mu0, dpx, dpy, c.h, P);
    CellFields thin, newt;
    cell_fields<EOS>(c, P, thin, eta);
    cell_fields<EOS>(c, P, newt);               // with the viscosity as cell_fields evaluates it: the film integrals' stresses
    a.v[0] += film_pressure<EOS>(c.rho, P);
    a.v[1] += thin.lower[4];
    a.v[2] += thin.lower[3];
    a.v[3] += thin.upper[4];
    a.v[4] += thin.upper[3];
    a.v[5] += newt.lower[4];
    a.v[6] += newt.lower[3];
    a.v[7] += newt.upper[4];
    a.v[8] += newt.upper[3];
    const double eta_r = __builtin_canonicalize(eta);
    a.v[9] += eta_r;
    a.v[10] += rate;
    e.take(0, eta_r, ix, iy);
    e.take(1, eta_r, ix, iy);
    e.take(2, rate, ix, iy);
}

template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(256) void k_thin_partial(const ThinArgs f, const Phys P, long long expect) {
    __shared__ double sm[4][THIN_NSUM];
    __shared__ ThinExt sme[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int ix = 1 + blockIdx.x;
    if (ix > f.L.Nx) return;
    ThinAcc a;
    a.zero();
    ThinExt e;
    e.none();
    row_pairs_cross<FilmPlanes<HAS_LS>>(f, ix, [&](const CellIn& c, const RhoCross& s, int iy) { thin_cell<EOS>(a, e, f, P, c, s, ix, iy); });
    const ThinAcc r = block_sum(a, sm);
    const ThinExt x = block_first(e, sme, 256);
    if (threadIdx.x == 0) {
        double* out = f.part + (long long)(ix - 1) * THIN_NSUM;
#pragma unroll
        for (int k = 0; k < THIN_NSUM; ++k) out[k] = r.v[k];
        store_row_first(f.row_val, f.row_iy, ix - 1, x);
    }
}

__global__ __launch_bounds__(256) void k_thin_fold(const ThinArgs f, long long expect) {
    __shared__ double sm[4][THIN_NSUM];
    __shared__ ThinExt sme[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int Nx = f.L.Nx;
    const ThinAcc r = fold_rows<THIN_NSUM>(f.part, 0, Nx, sm);
    const ThinExt x = block_first(first_of_rows<ThinExt>(f.row_val, f.row_iy, Nx), sme, 256);
    if (threadIdx.x != 0) return;
    double* out = f.rec + f.slot * THIN_NREC;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < THIN_NSUM; ++k) out[k] = r.v[k] * dA;
    store_first(f.rec + THIN_NSUM, f.cell, f.slot, x, THIN_NREC);
}

}  // namespace gpf
