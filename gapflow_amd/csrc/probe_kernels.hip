// Point probes: rho, jx, jy (and the EOS pressure) of a few cells after every committed step (entry points in api_probes.inc).
//
// Records live on the device as [step][probe][value] doubles, the record of the step that took the count to s at index
// s - 1 - base -- the slot commit_step gives that step's scalar record -- and leave it once per batch, with the scalar log.
// Three writers, one layout:
//   k_probe_record       one launch behind every launch-per-step step (k_step2 fused or split) and behind gpf_close_step
//   probe_record_block   inside k_small_steps, after commit_step, from the field the workgroup holds in LDS
// Both only read the state.  `p` is eos_pressure of the COMMITTED density, not the corrector-stage pressure plane of the
// derived fields (GPF_FIELD_PRESSURE).
#pragma once

namespace gpf {

constexpr int PROBE_MAX = 256;

struct ProbeArgs {
    const int* cells;       // [nprobe][2]: ix, iy in the ghosted index space
    double* out;            // [cap][nprobe][nv]
    int nprobe, nv;         // nv 3: rho jx jy; 4: + p
    long long base, cap;    // step count before the batch's first step, records the buffer holds
};

__device__ __forceinline__ void probe_put(const ProbeArgs& r, long long k, int p, int v, double x) {
    r.out[(k * r.nprobe + p) * r.nv + v] = x;
}

// One thread per (probe, value).  `expect` is the step count the launch ahead of this one produces IF it commits: a step
// that did not run (converged / max_it under honor_stop, or behind a rollback) leaves st->step below it, a rolled-back one
// leaves it below AND raises st->invalid -- either way nothing is written, and nothing depends on when the host looks.
template <int EOS>
__global__ __launch_bounds__(256) void k_probe_record(const double* qa, const double* qb, const StepState* st, const Layout L,
                                                      const Phys P, const ProbeArgs r, long long expect) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= r.nprobe * r.nv) return;
    if (st->step != expect || st->invalid != 0) return;
    const long long k = expect - 1 - r.base;
    if (k < 0 || k >= r.cap) return;
    const int p = t / r.nv, v = t - p * r.nv;
    const double* q = st->parity ? qb : qa;
    const long long o = L.at(r.cells[2 * p], r.cells[2 * p + 1]);
    probe_put(r, k, p, v, v < 3 ? q[v * L.plane + o] : eos_pressure<EOS>(q[o], P));
}

// The same record from a dense LDS field of k_small_steps (planes of nc cells, rows of w): the whole block calls it after
// the commit with the record's index k (that of the step's scalar record) and the batch's capacity; r.base and r.cap are not used.
template <int EOS>
__device__ __forceinline__ void probe_record_block(const ProbeArgs& r, const double* q, int nc, int w, long long k, long long cap, const Phys& P) {
    if (k < 0 || k >= cap) return;
    for (int t = threadIdx.x; t < r.nprobe * r.nv; t += blockDim.x) {
        const int p = t / r.nv, v = t - p * r.nv;
        const int cell = r.cells[2 * p] * w + r.cells[2 * p + 1];
        probe_put(r, k, p, v, v < 3 ? q[v * nc + cell] : eos_pressure<EOS>(q[cell], P));
    }
}

// The yardstick of tools/probe_time.py: a launch in k_probe_record's place in the stream that does nothing.
__global__ void k_probe_empty() {}

}  // namespace gpf
