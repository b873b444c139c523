// The workspace tier of the ensembles: members too large for one workgroup's LDS (small_kernel.hip: 1200 cells) and of at most
// MID_GRID_MAX_CELLS = 16384 cells, ghost cells included -- the reference's 2-D set-ups, 40 x 40 to 100 x 100.  One member, one
// workgroup of 512 threads, whole batches of steps in one launch, as there; the planes live in the member's workspace in device
// memory (mid_layout.hpp) instead of LDS.  Phase order, per-cell arithmetic and the thread-to-cell map (t = tid; t < nc; t += 512)
// are those of small_steps_body, and so are its parts: cell_closure<EOS, true, HAS_LS, true>, ghost_x / ghost_y with the corner
// rule, Acc::cell, block_reduce, commit_step, the final write-back.
//
// What differs: the update of a stage goes to a THIRD state buffer instead of through registers (stage 1 reads q0 and writes q1,
// stage 2 reads q1 and writes q2, the average goes into q2, then q2 becomes q0) -- at up to 32 cells per thread the LDS body's
// nv[3][3] staging would live in scratch, and with a buffer of its own the update needs no barrier between its loads and stores.
//
// Memory ordering: a workgroup lives on one CU, all its waves load and store through that CU's one vector L1, and __syncthreads()
// is a workgroup-scope release / acquire (every wave's stores have left it before any wave passes the barrier).  That is all the
// hand-offs between phases need: nobody outside the workgroup reads the workspace, ever.  The workspace pointers carry no
// `const` / `__restrict__`, so that no loaded value is carried over a barrier.
#pragma once

#include "mid_layout.hpp"

namespace gpf {

// The whole batch of one member on one workgroup of 512 threads.  The workgroup's only stores to global memory go to its own
// workspace `ws`, a.qa, a.qb, a.st, a.log and the film records (a.film: film_record_block, whose row vectors pass through the
// workspace's flux planes under the barriers' release / acquire like everything else here), the probe records (a.probe:
// probe_record_block) and the extrema records (a.extrema: extrema_record_wide) -- the ensemble's own series, in slots it owns; a
// member with a series armed on itself is still refused by gpf_ensemble_create.  All three are written behind the commit and
// only read the state: the committed field q0 was stored to device memory by other threads than those that read it here, and
// what makes those stores visible is the workgroup barrier behind commit_step (with the one that ends ghosts(q2) before it).
// Returns the run state the batch ended on (in LDS; thread 0 alone may read it without a barrier).
template <int EOS, bool HAS_LS>
__device__ __forceinline__ const StepState* mid_steps_body(const SmallArgs& a, const Phys& P, double* ws) {
    __shared__ Acc sm[16];
    __shared__ int sh_flags[2];
    __shared__ StepState sst;                       // the run state stays on-chip for the whole batch
    __shared__ double film_sm[4][FILM_NV];          // film_record_block's wave staging
    __shared__ ExtAcc ext_sm[MID_THREADS / 64];     // extrema_record_wide's: one candidate set per wave
    const Layout& G = a.L;                          // layout of the member's own planes
    const int w = G.Ny + 2, nc = (G.Nx + 2) * w;
    Layout D;                                       // dense layout of the workspace planes
    D.Nx = G.Nx; D.Ny = G.Ny; D.pitch = w; D.off = 0; D.plane = nc;
    double* q0 = ws + mid_plane_offset(MID_PLANE_Q, nc);
    double* q1 = ws + mid_plane_offset(MID_PLANE_Q + 3, nc);
    double* q2 = ws + mid_plane_offset(MID_PLANE_Q + 6, nc);
    double* F = ws + mid_plane_offset(MID_PLANE_F, nc);
    double* T = ws + mid_plane_offset(MID_PLANE_T, nc);    // h, hx, hy, Ls
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) sst = *a.st;
    __syncthreads();
    StepState* st = &sst;

    {   // current field and topography -> workspace
        const double* src = st->parity ? a.qb : a.qa;
        MidCursor k(tid, nt, w);
        for (int t = tid; t < nc; t += nt, k.next()) {
            const long long o = G.at(k.ix, k.iy);
            for (int c = 0; c < 3; ++c) { q0[c * nc + t] = src[c * G.plane + o]; T[c * nc + t] = a.topo[c * G.plane + o]; }
            T[3 * nc + t] = HAS_LS ? a.Ls[o] : 0.0;
        }
    }
    __syncthreads();

    // every ghost cell from interior values directly, in ONE phase (small_kernel.hip: a corner is rule_y(rule_x(.)))
    auto ghosts = [&](double* f) {
        const int nrow = 2 * w, ncol = 2 * D.Nx;
        for (int t = tid; t < nrow + ncol; t += nt) {
            double v[3];
            int cell;
            if (t < nrow) {
                const int e = t / w, iy = t % w;
                cell = (int)D.at(e == 0 ? 0 : D.Nx + 1, iy);
                if (iy >= 1 && iy <= D.Ny) {
                    for (int c = 0; c < 3; ++c) v[c] = ghost_x(f, D, a.E, e, c, iy);
                } else {
                    const int ey = iy == 0 ? 2 : 3;
                    const int src = (a.E.rule[ey][0] == BC_P) ? (ey == 2 ? D.Ny : 1) : (ey == 2 ? 1 : D.Ny);
                    for (int c = 0; c < 3; ++c) {
                        const double gx = ghost_x(f, D, a.E, e, c, src);
                        v[c] = a.E.rule[ey][c] == BC_D ? 2.0 * a.E.value[ey] - gx : gx;
                    }
                }
            } else {
                const int u = t - nrow, e = 2 + u / D.Nx, ix = 1 + u % D.Nx;
                cell = (int)D.at(ix, e == 2 ? 0 : D.Ny + 1);
                for (int c = 0; c < 3; ++c) v[c] = ghost_y(f, D, a.E, e, c, ix);
            }
            for (int c = 0; c < 3; ++c) f[c * nc + cell] = v[c];
        }
        __syncthreads();
    };

    int committed = 0;                              // steps this launch has committed (block-uniform)
    SeriesCursor ext, film;
    if (a.extrema) ext.begin(a.extrema->every, st->step, a.log_base);
    if (a.film) film.begin(a.film->every, st->step, a.log_base);
    for (int step = 0; step < a.nsteps; ++step) {
        if (st->invalid != 0 || (a.honor_stop && (st->converged || st->step >= st->max_it))) break;     // block-uniform
        const double dt = st->dt;
        const int dir0 = direction_of_step(st, st->step);
        for (int stage = 0; stage < 2; ++stage) {
            double* qin = stage == 0 ? q0 : q1;             // stage 1 reads the current field,
            double* qout = stage == 0 ? q1 : q2;            // ... each stage writes a buffer of its own
            const int dir = stage == 0 ? dir0 : -dir0;
            // Pressure / WallStress / BulkStress.update on the whole array, ghost cells included (problem.py:536-540)
            for (int t = tid; t < nc; t += nt) {
                CellIn c;
                c.rho = qin[t]; c.jx = qin[nc + t]; c.jy = qin[2 * nc + t];
                c.h = T[t]; c.hx = T[nc + t]; c.hy = T[2 * nc + t]; c.Ls = T[3 * nc + t];
                CellFlux f;
                cell_closure<EOS, true, HAS_LS, true>(c, P, f);
                F[t] = f.fx1; F[nc + t] = f.fx2; F[2 * nc + t] = f.fy2; F[3 * nc + t] = f.s0; F[4 * nc + t] = f.s1; F[5 * nc + t] = f.s2;
            }
            __syncthreads();
            // predictor_corrector + source + update (integrate.py:38-130, problem.py:558) on interior cells; every ghost cell
            // of qout is written right after
            const double cx = (double)dir * P.inv_dx, cy = (double)dir * P.inv_dy;
            MidCursor k(tid, nt, w);
            for (int t = tid; t < nc; t += nt, k.next()) {
                if (k.ix < 1 || k.ix > D.Nx || k.iy < 1 || k.iy > D.Ny) continue;
                const int xu = t - dir * w, yu = t - dir;          // upwind neighbours in x and y
                qout[t] = qin[t] - dt * (cx * (qin[nc + t] - qin[nc + xu]) + cy * (qin[2 * nc + t] - qin[2 * nc + yu]) - F[3 * nc + t]);
                qout[nc + t] = qin[nc + t] - dt * (cx * (F[t] - F[xu]) + cy * (F[nc + t] - F[nc + yu]) - F[4 * nc + t]);
                qout[2 * nc + t] = qin[2 * nc + t] - dt * (cx * (F[nc + t] - F[nc + xu]) + cy * (F[2 * nc + t] - F[2 * nc + yu]) - F[5 * nc + t]);
            }
            __syncthreads();
            ghosts(qout);
        }
        // second-order temporal averaging over the whole array (problem.py:563); validity before the ghost update (:565)
        int pre = 0;
        for (int t = tid; t < nc; t += nt) {
            for (int c = 0; c < 3; ++c) q2[c * nc + t] = 0.5 * (q2[c * nc + t] + q0[c * nc + t]);
            const double r = q2[t], jx = q2[nc + t], jy = q2[2 * nc + t];
            if (r != r || jx != jx || jy != jy) pre |= 1;
            if (r < 0.0) pre |= 2;
        }
        if (tid == 0) sh_flags[0] = 0;
        __syncthreads();
        if (pre) atomicOr(&sh_flags[0], pre);
        __syncthreads();
        ghosts(q2);
        Acc acc; acc.zero();
        for (int t = tid; t < nc; t += nt) acc.cell<EOS>(q2[t], q2[nc + t], q2[2 * nc + t], T[t], P);
        acc = block_reduce(acc, sm);
        if (tid == 0) {
            const int flags = (sh_flags[0] & 3) | (acc.flags & 4);
            commit_step(st, acc.ekin, acc.v2, acc.c2, flags, a.log, a.log_base, a.log_cap);
            sh_flags[1] = st->invalid;
        }
        __syncthreads();
        if (sh_flags[1]) break;                     // rolled back: q0 still holds the last valid state
        double* tmp = q0; q0 = q2; q2 = tmp;        // the averaged field is the current one now, q2 the state before this step
        committed += 1;
        // the records: block-uniform, reads of q0 and T only, behind the barrier above (q0 is not written again before the
        // commit after next; ext_sm not before the next record, a step's barriers later)
        if (a.probe) probe_record_block<EOS>(*a.probe, q0, nc, w, st->step - 1 - a.log_base, a.log_cap, P);
        if (a.extrema && ext.due(st->step)) {           // the arguments are fetched when a record is due, as the film's
#ifdef GPF_MID_EXTREMA_PER_WAVE                         // diagnostic build (tools/ensemble_series_time.py): the LDS tier's one wave per quantity
            extrema_record_block<EOS>(*a.extrema, q0, T, D.Nx, D.Ny, nc, w, ext.slot, P);
#else
            extrema_record_wide<EOS>(*a.extrema, q0, T, D.Nx, D.Ny, nc, w, ext.slot, P, ext_sm);
#endif
            ext.advance();
        }
        if (a.film && film.due(st->step)) {             // block-uniform; F is free until the next closure pass
            film_record_block<EOS>(a.film, q0, T, F, film_sm, D.Nx, D.Ny, nc, w, film.slot, P);
            film.advance();
        }
    }
    // the current state -> the buffer the (final) parity designates, the state before the last committed step -> the other one
    // (where the launch-per-step kernels leave it too); the run state back to global memory
    __syncthreads();
    if (tid == 0) *a.st = sst;
    double* dst = st->parity ? a.qb : a.qa;
    double* prev = st->parity ? a.qa : a.qb;
    const bool with_prev = committed > 0 && st->invalid == 0;
    MidCursor k(tid, nt, w);
    for (int t = tid; t < nc; t += nt, k.next()) {
        const long long o = G.at(k.ix, k.iy);
        for (int c = 0; c < 3; ++c) dst[c * G.plane + o] = q0[c * nc + t];
        if (with_prev)
            for (int c = 0; c < 3; ++c) prev[c * G.plane + o] = q2[c * nc + t];
    }
    return st;
}

// Workgroup m advances the member of launch slot m on workspace ws[m]; arguments as k_small_ensemble's.
template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(MID_THREADS) void k_mid_ensemble(const SmallArgs* __restrict__ args, const Phys* __restrict__ phys,
                                                              double* const* __restrict__ ws, StepState* __restrict__ states_out) {
    const StepState* st = mid_steps_body<EOS, HAS_LS>(args[blockIdx.x], phys[blockIdx.x], ws[blockIdx.x]);
    if (threadIdx.x == 0) states_out[blockIdx.x] = *st;
}

}  // namespace gpf
