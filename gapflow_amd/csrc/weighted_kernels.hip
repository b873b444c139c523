// Weighted film integrals of the committed state (entry points in api_weighted.inc): for each of K <= 8 weight planes w_k the
// sums over the interior cells of w_k f dx dy for nine integrands f -- the pressure (closures.hpp: film_pressure, the function
// the integrals' `load` uses), h, rho h, jx h, jy h and the four wall shear stresses of closures.hpp: cell_fields<EOS> (lower[4],
// lower[3], upper[4], upper[3]: the terms integral_kernels.hip: film_cell adds).  Per-pad loads, windows and Fourier modes are all
// this reduction with another plane in front.
//
// Two launches per record, both guarded by the device's run state like k_film_partial / k_film_fold:
//   k_wfilm_partial   grid (Nx, K): one 256-thread workgroup per interior row ix and weight k, with k_film_partial's geometry.
//                     Thread t owns the column pairs (1 + 2j, 2 + 2j) for j = t, t + 256, ... and adds w f of their cells to its
//                     nine registers in that order, the lower column first; the workgroup folds the 256 register sets in
//                     film_block_sum's fixed tree (shuffles 32 .. 1 apart inside a wave, then waves 0, 1, 2, 3 in order) and
//                     lane 0 stores the nine doubles to part[k][ix - 1][9].
//   k_wfilm_fold      grid (K): thread t adds rows t, t + 256, ... in order, the same tree folds the threads, thread 0 applies
//                     dx dy and stores the nine values to the record's slot [K][9].
// The weight on blockIdx.y evaluates the closures K times and keeps nine accumulators per thread; the q / topo rows the first
// weight's workgroup brought in are read again by the others.  Who adds what, in which order, depends on (Nx, Ny) alone: no
// floating-point atomics, no arrival order, no ticket.
//
// The accumulate is acc += w * term with floating-point contraction OFF for that statement: the product is rounded on its own, so
// a weight of exactly 1.0 adds the term's own bits and a weight of exactly 0.0 adds a zero.  A plane of ones therefore goes
// through k_film_partial's additions in k_film_partial's order and k_wfilm_fold through k_film_fold's: p and the four stresses of
// that plane equal `load` and the tau_* of the film integrals in every bit.
// The product also passes through __builtin_canonicalize, the identity on every value a product of finite numbers can take: the
// library is compiled with -ffp-contract=fast, under which the backend fuses across the whole translation unit whatever a
// contract pragma says, and the canonicalize between the two operations is what it does not fuse across.  It costs no
// instruction: 18 v_fma_f64 of the loop body become 18 v_mul_f64 + 18 v_add_f64 in the ISA, nothing else.
// A pair is fetched with one 16-byte load per plane under film_wide_ok's conditions, which the weight planes must meet too, and
// with two 8-byte loads otherwise; the column Ny + 1 that the last pair of an odd Ny reaches is the row's ghost cell: it is loaded
// and never added.  Ghost cells never contribute.
#pragma once

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

struct WFilmAcc {
    double v[WFILM_NQ];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < WFILM_NQ; ++k) v[k] = 0.0;
    }
};

// film_block_sum's tree on nine values: lanes fold 32, 16, .. 1 apart, then waves 0, 1, 2, 3 in order; valid in thread 0
__device__ __forceinline__ WFilmAcc wfilm_block_sum(WFilmAcc a, double (*sm)[WFILM_NQ]) {
#pragma unroll
    for (int k = 0; k < WFILM_NQ; ++k)
        for (int s = 32; s >= 1; s >>= 1) a.v[k] += __shfl_down(a.v[k], s);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < WFILM_NQ; ++k) sm[w][k] = a.v[k];
    }
    __syncthreads();
    WFilmAcc r;
    r.zero();
    if (threadIdx.x == 0) {
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int k = 0; k < WFILM_NQ; ++k) r.v[k] += sm[i][k];
        }
    }
    return r;
}

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
    if (f.st->step != expect || f.st->invalid != 0) return;            // uniform: the step did not run, or was rolled back
    if (f.slot < 0 || f.slot > f.cap) return;
    const Layout& L = f.L;
    const int ix = 1 + blockIdx.x, kw = blockIdx.y;
    if (ix > L.Nx || kw >= f.K) return;
    const double* q = f.st->parity ? f.qb : f.qa;
    const double* wp = f.w + (long long)kw * L.plane;
    WFilmAcc a;
    a.zero();
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy);
        film_d2 in[8];
        if (f.wide) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                in[p] = *reinterpret_cast<const film_d2*>(q + p * L.plane + o);
                in[3 + p] = *reinterpret_cast<const film_d2*>(f.topo + p * L.plane + o);
            }
            in[6] = HAS_LS ? *reinterpret_cast<const film_d2*>(f.Ls + o) : film_d2{0.0, 0.0};
            in[7] = *reinterpret_cast<const film_d2*>(wp + o);
        } else {
            const long long o1 = two ? o + 1 : o;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                in[p] = film_d2{q[p * L.plane + o], q[p * L.plane + o1]};
                in[3 + p] = film_d2{f.topo[p * L.plane + o], f.topo[p * L.plane + o1]};
            }
            in[6] = HAS_LS ? film_d2{f.Ls[o], f.Ls[o1]} : film_d2{0.0, 0.0};
            in[7] = film_d2{wp[o], wp[o1]};
        }
        CellIn c;
        c.rho = in[0].x; c.jx = in[1].x; c.jy = in[2].x; c.h = in[3].x; c.hx = in[4].x; c.hy = in[5].x; c.Ls = in[6].x;
        wfilm_cell<EOS>(a, P, c, in[7].x);
        if (two) {
            c.rho = in[0].y; c.jx = in[1].y; c.jy = in[2].y; c.h = in[3].y; c.hx = in[4].y; c.hy = in[5].y; c.Ls = in[6].y;
            wfilm_cell<EOS>(a, P, c, in[7].y);
        }
    }
    const WFilmAcc r = wfilm_block_sum(a, sm);
    if (threadIdx.x == 0) {
        double* out = f.part + ((long long)kw * L.Nx + (ix - 1)) * WFILM_NQ;
#pragma unroll
        for (int k = 0; k < WFILM_NQ; ++k) out[k] = r.v[k];
    }
}

__global__ __launch_bounds__(256) void k_wfilm_fold(const WFilmArgs f, long long expect) {
    __shared__ double sm[4][WFILM_NQ];
    if (f.st->step != expect || f.st->invalid != 0) return;
    if (f.slot < 0 || f.slot > f.cap) return;
    const int kw = blockIdx.x;
    if (kw >= f.K) return;
    WFilmAcc a;
    a.zero();
    for (int row = threadIdx.x; row < f.L.Nx; row += 256) {
        const double* in = f.part + ((long long)kw * f.L.Nx + row) * WFILM_NQ;
#pragma unroll
        for (int k = 0; k < WFILM_NQ; ++k) a.v[k] += in[k];
    }
    const WFilmAcc r = wfilm_block_sum(a, sm);
    if (threadIdx.x != 0) return;
    double* out = f.rec + (f.slot * f.K + kw) * WFILM_NQ;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < WFILM_NQ; ++k) out[k] = r.v[k] * dA;
}

}  // namespace gpf
