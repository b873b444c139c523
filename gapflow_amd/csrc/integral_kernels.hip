// Whole-film integrals of the committed state (entry points in api_integrals.inc): the load the film carries and its first
// moments, the pressure's in-plane push on the profiled wall, the shear force on each wall, and mass-flow rates through
// cross-sections.  Per cell the wall stresses come from closures.hpp: cell_fields<EOS> -- lower[], upper[], piezo-viscosity
// included -- and the pressure from closures.hpp: film_pressure, so the integrands are the fields the reference's pressure.py /
// viscous.py give for the same cell.
//
// Two launches per record, both guarded by the device's run state like k_probe_record:
//   k_film_partial   one 256-thread workgroup per interior row ix.  Thread t owns the column pairs (1 + 2k, 2 + 2k) for
//                    k = t, t + 256, ... and adds their terms to its registers in that order, the lower column first; the
//                    workgroup folds the 256 register sets in a fixed tree (shuffles inside a wave, the four waves in order)
//                    and lane 0 stores the row's vector [FILM_NV] into the scratch buffer.
//   k_film_fold      one workgroup.  Thread t adds rows 1 + t, 1 + t + 256, ... in order, the same tree folds the threads,
//                    thread 0 applies dx dy (dy, dx for the flow rates) and stores the record.
// Who adds what, and in which order, depends on (Nx, Ny) alone: a record is a pure function of the state, the gap and the
// sections -- no floating-point atomics, no arrival order.  A pair is fetched with one 16-byte load per plane where the
// buffers allow it (Layout::at puts column 1 at element off + 1 = 16 of a row whose pitch is a multiple of 16 doubles; the
// host checks this, the parity of `plane` and the base pointers, see film_wide_ok) and with two 8-byte loads otherwise; the
// column Ny + 1 that the last pair of an odd Ny reaches is the row's ghost cell: it is loaded and never added.
// The pass reads 6 planes (7 with a slip-length field) once and writes 144 bytes per row.
//
// A third writer of the same record, film_record_block, runs inside the one-workgroup kernels (small_kernel.hip, mid_kernel.hip)
// after commit_step, on the dense planes the workgroup holds: it replays the order above on one workgroup and leaves the same
// bits (the argument is spelled out above the function and in DESIGN.md 3.3m).
#pragma once

namespace gpf {

constexpr int FILM_MAX_SECTIONS = 8;
constexpr int FILM_NSUM = 9;                            // load load_x load_y p_hx p_hy tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top
constexpr int FILM_NV = FILM_NSUM + 1 + FILM_MAX_SECTIONS;      // + the row's sum of jx h + one slot per y-section (jy h of its column)

typedef double film_d2 __attribute__((ext_vector_type(2)));

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

struct FilmAcc {
    double v[FILM_NV];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) v[k] = 0.0;
    }
};

// Sum of the 256 threads' sets, valid in thread 0: lanes fold 32, 16, .. 1 apart, then waves 0, 1, 2, 3 in order.
__device__ __forceinline__ FilmAcc film_block_sum(FilmAcc a, double (*sm)[FILM_NV]) {
#pragma unroll
    for (int k = 0; k < FILM_NV; ++k)
        for (int s = 32; s >= 1; s >>= 1) a.v[k] += __shfl_down(a.v[k], s);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) sm[w][k] = a.v[k];
    }
    __syncthreads();
    FilmAcc r;
    r.zero();
    if (threadIdx.x == 0) {
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int k = 0; k < FILM_NV; ++k) r.v[k] += sm[i][k];
        }
    }
    return r;
}

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
    if (f.st->step != expect || f.st->invalid != 0) return;            // uniform: the step did not run, or was rolled back
    if (f.slot < 0 || f.slot > f.cap) return;
    const Layout& L = f.L;
    const int ix = 1 + blockIdx.x;
    const double* q = f.st->parity ? f.qb : f.qa;
    const double x = ((double)ix - 0.5) * f.dx;
    FilmAcc a;
    a.zero();
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy);
        film_d2 in[7];
        if (f.wide) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                in[p] = *reinterpret_cast<const film_d2*>(q + p * L.plane + o);
                in[3 + p] = *reinterpret_cast<const film_d2*>(f.topo + p * L.plane + o);
            }
            in[6] = HAS_LS ? *reinterpret_cast<const film_d2*>(f.Ls + o) : film_d2{0.0, 0.0};
        } else {
            const long long o1 = two ? o + 1 : o;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                in[p] = film_d2{q[p * L.plane + o], q[p * L.plane + o1]};
                in[3 + p] = film_d2{f.topo[p * L.plane + o], f.topo[p * L.plane + o1]};
            }
            in[6] = HAS_LS ? film_d2{f.Ls[o], f.Ls[o1]} : film_d2{0.0, 0.0};
        }
        CellIn c;
        c.rho = in[0].x; c.jx = in[1].x; c.jy = in[2].x; c.h = in[3].x; c.hx = in[4].x; c.hy = in[5].x; c.Ls = in[6].x;
        film_cell<EOS>(a, f, P, c, x, ((double)iy - 0.5) * f.dy, iy);
        if (two) {
            c.rho = in[0].y; c.jx = in[1].y; c.jy = in[2].y; c.h = in[3].y; c.hx = in[4].y; c.hy = in[5].y; c.Ls = in[6].y;
            film_cell<EOS>(a, f, P, c, x, ((double)iy + 0.5) * f.dy, iy + 1);
        }
    }
    const FilmAcc r = film_block_sum(a, sm);
    if (threadIdx.x == 0) {
        double* out = f.part + (long long)(ix - 1) * FILM_NV;
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) out[k] = r.v[k];
    }
}

__global__ __launch_bounds__(256) void k_film_fold(const FilmArgs f, long long expect) {
    __shared__ double sm[4][FILM_NV];
    if (f.st->step != expect || f.st->invalid != 0) return;
    if (f.slot < 0 || f.slot > f.cap) return;
    FilmAcc a;
    a.zero();
    for (int row = threadIdx.x; row < f.L.Nx; row += 256) {
        const double* in = f.part + (long long)row * FILM_NV;
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) a.v[k] += in[k];
    }
    const FilmAcc r = film_block_sum(a, sm);
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
// adds the pairs (1 + 2k, 2 + 2k), k = t, t + 256, ..., to a set that starts at +0.0; film_block_sum folds the 64 lanes of each
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

// Which step a one-workgroup kernel records next and where (as ExtremaCursor): the first multiple of the stride beyond the
// count the launch starts at, and its rank among the multiples in (base, .]; each record moves both on.
// (Only the stride is kept beside them: the record fetches its arguments when it is due, so that nothing of them stays in
// registers over the steps in between.)
struct FilmCursor {
    long long every, next, slot;
    __device__ __forceinline__ void begin(const FilmBlockArgs* args, long long step, long long base) {
        every = args->every;
        next = (step / every + 1) * every;
        slot = next / every - base / every - 1;
    }
    __device__ __forceinline__ bool due(long long step) const { return step == next; }
    __device__ __forceinline__ void advance() { next += every; slot += 1; }
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
