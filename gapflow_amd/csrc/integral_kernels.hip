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
template <int EOS>
__device__ __forceinline__ void film_cell(FilmAcc& a, const FilmArgs& f, const Phys& P, const CellIn& c, double x, double y, int iy) {
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

}  // namespace gpf
