// Weighted film integrals of the committed state (entry points in api_weighted.inc): for each of K <= 8 weight planes w_k the
// sums over the interior cells of w_k f dx dy for nine integrands f -- the pressure (closures.hpp: film_pressure, the function
// the integrals' `load` uses), h, rho h, jx h, jy h and the four wall shear stresses of closures.hpp: cell_fields<EOS> (lower[4],
// lower[3], upper[4], upper[3]: the terms integral_kernels.hip: film_cell adds).  Per-pad loads, windows and Fourier modes are all
// this reduction with another plane in front.
//
// The two launches per record, the pair walk, the fold tree and the guard are series_rows.hpp's, as for the film integrals:
//   k_wfilm_partial   grid (Nx, K): one workgroup per interior row ix and weight k; the cells' w f go to nine registers; lane 0
//                     stores the nine doubles to part[k][ix - 1][9].
//   k_wfilm_fold      grid (K): thread 0 applies dx dy and stores the nine values to the record's slot [K][9].
// The weight on blockIdx.y evaluates the closures K times and keeps nine accumulators per thread; the q / topo rows the first
// weight's workgroup brought in are read again by the others.
//
// The accumulate is acc += w * term with floating-point contraction OFF for that statement: the product is rounded on its own, so
// a weight of exactly 1.0 adds the term's own bits and a weight of exactly 0.0 adds a zero.  A plane of ones therefore goes
// through k_film_partial's additions in k_film_partial's order and k_wfilm_fold through k_film_fold's: p and the four stresses of
// that plane equal `load` and the tau_* of the film integrals in every bit.
// The product also passes through __builtin_canonicalize, the identity on every value a product of finite numbers can take: the
// library is compiled with -ffp-contract=fast, under which the backend fuses across the whole translation unit whatever a
// contract pragma says, and the canonicalize between the two operations is what it does not fuse across.  It costs no
// instruction: 18 v_fma_f64 of the loop body become 18 v_mul_f64 + 18 v_add_f64 in the ISA, nothing else.
// The weight planes must meet series_wide_ok's conditions for the 16-byte loads too.  Ghost cells never contribute.
#pragma once

#include "series_rows.hpp"

namespace gpf {

constexpr int WFILM_MAX_K = 8;
constexpr int WFILM_NQ = 9;             // p h rho_h jx_h jy_h tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top

struct WFilmArgs {
    const double *qa, *qb, *topo, *Ls;
    const double* w;        // [K] planes in the handle's Layout, ghost cells zero
    const StepState* st;
    double* part;           // [K][Nx][WFILM_NQ]
    double* rec;            // [cap + 1][K][WFILM_NQ]
    Layout L;
    double dx, dy;
    int K;
    int wide;               // 16-byte pair loads are aligned
    long long slot, cap;    // record to write; slots the buffer holds
};

using WFilmAcc = RowAcc<WFILM_NQ>;

// One cell's nine terms, each times the cell's weight
template <int EOS>
__device__ __forceinline__ void wfilm_cell(WFilmAcc& a, const Phys& P, const CellIn& c, double w) {
    CellFields o;
    cell_fields<EOS>(c, P, o);                  // wall stresses, with the viscosity as cell_fields evaluates it
    const double t[WFILM_NQ] = {film_pressure<EOS>(c.rho, P), c.h, c.rho * c.h, c.jx * c.h, c.jy * c.h,
                                o.lower[4], o.lower[3], o.upper[4], o.upper[3]};
#pragma unroll
    for (int k = 0; k < WFILM_NQ; ++k) {
#pragma clang fp contract(off)
        a.v[k] += __builtin_canonicalize(w * t[k]);
    }
}

template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(256) void k_wfilm_partial(const WFilmArgs f, const Phys P, long long expect) {
    __shared__ double sm[4][WFILM_NQ];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const Layout& L = f.L;
    const int ix = 1 + blockIdx.x, kw = blockIdx.y;
    if (ix > L.Nx || kw >= f.K) return;
    WFilmAcc a;
    a.zero();
    row_pairs<WFilmPlanes<HAS_LS>>(f, f.w + (long long)kw * L.plane, ix, [&](const CellIn& c, double w, int, double) { wfilm_cell<EOS>(a, P, c, w); });
    const WFilmAcc r = block_sum(a, sm);
    if (threadIdx.x == 0) {
        double* out = f.part + ((long long)kw * L.Nx + (ix - 1)) * WFILM_NQ;
#pragma unroll
        for (int k = 0; k < WFILM_NQ; ++k) out[k] = r.v[k];
    }
}

__global__ __launch_bounds__(256) void k_wfilm_fold(const WFilmArgs f, long long expect) {
    __shared__ double sm[4][WFILM_NQ];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int kw = blockIdx.x;
    if (kw >= f.K) return;
    const WFilmAcc r = fold_rows(f.part, kw, f.L.Nx, sm);
    if (threadIdx.x != 0) return;
    double* out = f.rec + (f.slot * f.K + kw) * WFILM_NQ;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < WFILM_NQ; ++k) out[k] = r.v[k] * dA;
}

}  // namespace gpf
