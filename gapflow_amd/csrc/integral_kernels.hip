// Whole-film integrals of the committed state (entry points in api_integrals.inc): the load the film carries and its first
// moments, the pressure's in-plane push on the profiled wall, the shear force on each wall, and mass-flow rates through
// cross-sections.  Per cell the wall stresses come from closures.hpp: cell_fields<EOS> -- lower[], upper[], piezo-viscosity
// included -- and the pressure from closures.hpp: film_pressure, so the integrands are the fields the reference's pressure.py /
// viscous.py give for the same cell.
//
// The two launches per record, the pair walk, the fold tree and the guard are series_rows.hpp's:
//   k_film_partial   reads 6 planes (7 with a slip-length field) once; lane 0 stores the row's vector [FILM_NV] into the scratch
//                    buffer, 144 bytes per row.
//   k_film_fold      one workgroup; thread 0 applies dx dy (dy, dx for the flow rates) and stores the record.
//
// A third writer of the same record, film_record_block, runs inside the one-workgroup kernels (small_kernel.hip, mid_kernel.hip)
// after commit_step, on the dense planes the workgroup holds: it replays the order above on one workgroup and leaves the same
// bits (the argument is spelled out above the function and in DESIGN.md 3.3m).
#pragma once

#include "series_rows.hpp"

namespace gpf {

constexpr int FILM_MAX_SECTIONS = 8;
constexpr int FILM_NSUM = 9;                            // load load_x load_y p_hx p_hy tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top
constexpr int FILM_NV = FILM_NSUM + 1 + FILM_MAX_SECTIONS;      // + the row's sum of jx h + one slot per y-section (jy h of its column)

struct FilmArgs {
    const double *qa, *qb, *topo, *Ls;
    const StepState* st;
    double* part;           // [Nx][FILM_NV]
    double* rec;            // [cap + 1][9 + nsx + nsy]: flow_x behind the nine sums, flow_y behind flow_x
    Layout L;
    double dx, dy;
    int nsx, nsy;
    int sx[FILM_MAX_SECTIONS], sy[FILM_MAX_SECTIONS];       // interior rows / columns of the sections
    int wide;               // 16-byte pair loads are aligned
    long long slot, cap;    // record to write; slots the buffer holds
};

using FilmAcc = RowAcc<FILM_NV>;

// One cell's terms.  The load's pressure is closures.hpp: film_pressure -- Dowson-Higginson with the reference's own divisions,
// two more per cell in a pass that waits for HBM -- and NOT the p of cell_fields, which keeps eos_pressure for the viscosity.
// `f`: FilmArgs or FilmBlockArgs -- nsy and sy are read.
template <int EOS, class Args>
__device__ __forceinline__ void film_cell(FilmAcc& a, const Args& f, const Phys& P, const CellIn& c, double x, double y, int iy) {
    CellFields o;
    cell_fields<EOS>(c, P, o);                  // wall stresses, with the viscosity as cell_fields evaluates it
    const double p = film_pressure<EOS>(c.rho, P);
    a.v[0] += p;
    a.v[1] += p * x;
    a.v[2] += p * y;
    a.v[3] += p * c.hx;
    a.v[4] += p * c.hy;
    a.v[5] += o.lower[4];
    a.v[6] += o.lower[3];
    a.v[7] += o.upper[4];
    a.v[8] += o.upper[3];
    a.v[9] += c.jx * c.h;
    const double fy = c.jy * c.h;
#pragma unroll
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k)
        if (k < f.nsy && iy == f.sy[k]) a.v[FILM_NSUM + 1 + k] += fy;
}

template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(256) void k_film_partial(const FilmArgs f, const Phys P, long long expect) {
    __shared__ double sm[4][FILM_NV];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int ix = 1 + blockIdx.x;
    const double x = ((double)ix - 0.5) * f.dx;
    FilmAcc a;
    a.zero();
    row_pairs<FilmPlanes<HAS_LS>>(f, nullptr, ix, [&](const CellIn& c, double, int iy, double y) { film_cell<EOS>(a, f, P, c, x, y, iy); });
    const FilmAcc r = block_sum(a, sm);
    if (threadIdx.x == 0) {
        double* out = f.part + (long long)(ix - 1) * FILM_NV;
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) out[k] = r.v[k];
    }
}

__global__ __launch_bounds__(256) void k_film_fold(const FilmArgs f, long long expect) {
    __shared__ double sm[4][FILM_NV];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const FilmAcc r = fold_rows(f.part, 0, f.L.Nx, sm);
    if (threadIdx.x != 0) return;
    const int nrec = FILM_NSUM + f.nsx + f.nsy;
    double* out = f.rec + f.slot * nrec;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < FILM_NSUM; ++k) out[k] = r.v[k] * dA;
    for (int k = 0; k < f.nsx; ++k) out[FILM_NSUM + k] = f.part[(long long)(f.sx[k] - 1) * FILM_NV + FILM_NSUM] * f.dy;
#pragma unroll
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k)
        if (k < f.nsy) out[FILM_NSUM + f.nsx + k] = r.v[FILM_NSUM + 1 + k] * f.dx;
}

// ---------------------------------------------------------------------------------------------
// The same record from inside a one-workgroup kernel.
//
// What k_film_partial + k_film_fold compute is a fixed expression tree over the cells' terms: per row, virtual thread t of 256
// adds the pairs (1 + 2k, 2 + 2k), k = t, t + 256, ..., to a set that starts at +0.0; block_sum folds the 64 lanes of each
// of the four virtual waves 32, 16, .. 1 apart and adds the four wave sums in order to a set that starts at +0.0; over the rows,
// thread t adds the row vectors t, t + 256, ... to +0.0 and the same tree folds.  film_record_block evaluates that tree with
// another assignment of its nodes to threads, and leaves out only additions of +0.0:
//   * a set that starts at +0.0 and has terms added to it is never -0.0 (in round-to-nearest x + y is -0.0 only for
//     x = y = -0.0), so s + (+0.0) == s in every bit for every partial sum s the tree holds;
//   * a virtual thread without a pair (t >= npair), a virtual wave without one (64 w >= npair) and a fold thread without a row
//     (t >= Nx) hold +0.0 in all slots, and so does every sum of such sets: the stages of the lane fold that would only add
//     them (lane distance >= P, the power of two >= the lanes in use) and the wave sums of empty waves are skipped.
// The per-cell terms are film_cell<EOS> itself on the same operands, x and y spelled as k_film_partial spells them.
//
// Phase 1, all waves of the workgroup: rows with npair <= 64 are packed 64 / P to a wave (lane = row slot * P + virtual thread),
// wider rows take one wave per (row, virtual wave).  Lane 0 of each segment stores the wave sum to `W` [Nx][nvw][FILM_NV] --
// the flux planes, dead between commit_step and the next closure pass, 6 nc >= 18 Nx nvw doubles (nvw > 1 needs Ny > 128).
// Phase 2, threads 0..255: thread t forms the row vectors t, t + 256, ... (+0.0 + wave sums in order), stores flow_x where the
// row is a section, adds them up; the waves that hold rows fold their lanes and stage the result in `sm`.
// Phase 3, thread 0: the wave sums in order, the factors dx dy and dx, the record.
// Block-uniform; two barriers, the second of which also orders every read of W before the next step's closure pass writes it.
// q, T, W are plain pointers (no const, no __restrict__): in the workspace tier they are device memory handed from wave to wave
// across barriers (mid_kernel.hip).
struct FilmBlockArgs {
    double* rec;            // [cap][9 + nsx + nsy]
    long long every, cap;   // recording stride; records the buffer holds
    double dx, dy;
    int nsx, nsy;
    int sx[FILM_MAX_SECTIONS], sy[FILM_MAX_SECTIONS];
};

template <int EOS>
__device__ __forceinline__ void film_record_block(const FilmBlockArgs* args, double* q, double* T, double* W, double (*sm)[FILM_NV], int Nx, int Ny,
                                                  int nc, int w, long long slot, const Phys& P) {
    const FilmBlockArgs x = *args;
    if (slot < 0 || slot >= x.cap) return;             // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int npair = (Ny + 1) / 2;
    const int nvw = npair > 64 ? (npair > 192 ? 4 : (npair + 63) / 64) : 1;    // virtual waves of a row that hold pairs
    int Pw = 64;                                        // lanes of a segment: one row's virtual threads within a wave
    if (nvw == 1) { Pw = 1; while (Pw < npair) Pw <<= 1; }
    const int G = 64 / Pw;                              // rows per wave (1 when nvw > 1)
    const int ntask = nvw == 1 ? (Nx + G - 1) / G : Nx * nvw;
    for (int task = wave; task < ntask; task += nwaves) {       // wave-uniform
        int row, vw, vt;
        if (nvw == 1) { row = task * G + lane / Pw; vw = 0; vt = lane % Pw; }
        else { row = task / nvw; vw = task % nvw; vt = vw * 64 + lane; }
        FilmAcc a;
        a.zero();
        if (row < Nx) {
            const int ix = 1 + row;
            const double xc = ((double)ix - 0.5) * x.dx;
            for (int k = vt; k < npair; k += 256) {
                const int iy = 1 + 2 * k;
                const int ncol = iy + 1 <= Ny ? 2 : 1;
#pragma nounroll
                for (int j = 0; j < ncol; ++j) {            // lower column first; one instance of film_cell keeps the registers of the host kernel
                    const int o = ix * w + iy + j;
                    CellIn c;
                    c.rho = q[o]; c.jx = q[nc + o]; c.jy = q[2 * nc + o]; c.h = T[o]; c.hx = T[nc + o]; c.hy = T[2 * nc + o]; c.Ls = T[3 * nc + o];
                    const double yc = j == 0 ? ((double)iy - 0.5) * x.dy : ((double)iy + 0.5) * x.dy;
                    film_cell<EOS>(a, x, P, c, xc, yc, iy + j);
                }
            }
        }
        for (int s = Pw >> 1; s >= 1; s >>= 1) {
#pragma unroll
            for (int k = 0; k < FILM_NV; ++k) a.v[k] += __shfl_down(a.v[k], s);
        }
        if (row < Nx && (lane & (Pw - 1)) == 0) {
            double* out = W + (row * nvw + vw) * FILM_NV;
#pragma unroll
            for (int k = 0; k < FILM_NV; ++k) out[k] = a.v[k];
        }
    }
    __syncthreads();
    const int nrec = FILM_NSUM + x.nsx + x.nsy;
    double* out = x.rec + slot * nrec;
    const int nfold = Nx < 256 ? Nx : 256;              // fold threads that hold rows
    if ((wave << 6) < nfold) {                          // wave-uniform
        FilmAcc a;
        a.zero();
        for (int row = tid; row < Nx; row += 256) {
            FilmAcc r;
            r.zero();
            for (int i = 0; i < nvw; ++i) {
                const double* in = W + (row * nvw + i) * FILM_NV;
#pragma unroll
                for (int k = 0; k < FILM_NV; ++k) r.v[k] += in[k];
            }
#pragma unroll
            for (int k = 0; k < FILM_MAX_SECTIONS; ++k)
                if (k < x.nsx && x.sx[k] == row + 1) out[FILM_NSUM + k] = r.v[FILM_NSUM] * x.dy;
#pragma unroll
            for (int k = 0; k < FILM_NV; ++k) a.v[k] += r.v[k];
        }
        int Pf = 64;
        if (nfold < 64) { Pf = 1; while (Pf < nfold) Pf <<= 1; }
        for (int s = Pf >> 1; s >= 1; s >>= 1) {
#pragma unroll
            for (int k = 0; k < FILM_NV; ++k) a.v[k] += __shfl_down(a.v[k], s);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < FILM_NV; ++k) sm[wave][k] = a.v[k];
        }
    }
    __syncthreads();
    if (tid != 0) return;
    FilmAcc r;
    r.zero();
    const int nw = (nfold + 63) >> 6;
    for (int i = 0; i < nw; ++i) {
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) r.v[k] += sm[i][k];
    }
    const double dA = x.dx * x.dy;
#pragma unroll
    for (int k = 0; k < FILM_NSUM; ++k) out[k] = r.v[k] * dA;
#pragma unroll
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k)
        if (k < x.nsy) out[FILM_NSUM + x.nsx + k] = r.v[FILM_NSUM + 1 + k] * x.dx;
}

}  // namespace gpf
