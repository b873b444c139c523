// Part of api.hip (included there, not compiled on its own): the step-change series -- per conserved field the squared L2 norm of
// q^n - q^(n-1) and of q^n, the largest |q^n - q^(n-1)| with its cell, the mass defect sum (rho^n - rho^(n-1)) h dx dy and the
// step size -- recorded on the device behind the committed steps whose count is a multiple of the armed stride, and handed out
// once per call.  Kernels: change_kernels.hip.
// The series rests on one invariant: after a committed fused step the OTHER q buffer holds the state before it (k_step2 reads one
// buffer and writes the other; k_small_steps leaves both on exit).  Inside a batch stream order keeps it: the record of step n is
// enqueued behind step n and before step n + 1, which overwrites q^(n-1).  Between calls the handle's prev_state_valid says
// whether it still holds (gpf_changes_now asks).  A handle that steps through k_small_steps has its batch cut at every recorded
// step (small_batch_cut), as for the weighted integrals: the kernel's exit leaves both buffers.

// The cases the series does not cover: series_refusal's, with its error classes.  Surrogate, shear-thinning and elastic
// handles step stage-wise, and a closed stage-wise step leaves no previous state the series could rely on.
static int changes_refusal(const gpf_handle* h, const std::string& who) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; changes are not available on slabs");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set)
        return fail(GPF_ERR_INVALID, who + ": surrogate closures step stage-wise, which keeps no previous state for the changes (not supported)");
    if (h->cfg.thinning != GPF_THINNING_NONE)
        return fail(GPF_ERR_INVALID, who + ": shear thinning steps stage-wise, which keeps no previous state for the changes (not supported)");
    if (h->el.on || h->els.on)
        return fail(GPF_ERR_INVALID, who + ": an elastic handle steps stage-wise, which keeps no previous state for the changes (not supported)");
    return GPF_OK;
}

// 16-byte pair loads of k_change_partial: series_wide_ok's conditions on the planes it reads (GPF_FILM_NARROW, read when the
// buffers are allocated, asks for the 8-byte loads regardless)
static bool changes_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->chg.narrow, false); }

// The record buffers (log_cap slots for a batch + one for gpf_changes_now) and the row scratch, on first use
static int changes_buffers(gpf_handle* h) {
    const size_t slots = (size_t)h->log_cap + 1, nx = (size_t)h->L.Nx;
    if (!h->chg.rec) {
        h->chg.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
        DBG("changes_buffers: k_change_partial takes %s pair loads", changes_wide_ok(h) ? "16-byte" : "8-byte");       // (GPF_DEBUG: the narrow-load test reads this)
        HIP_TRY(hipMalloc(&h->chg.rec, slots * CHANGE_NREC * sizeof(double)));
    }
    if (!h->chg.part) HIP_TRY(hipMalloc(&h->chg.part, nx * CHANGE_NSUM * sizeof(double)));
    return series_first_buffers(h, CHANGE_NMAX, h->chg.cell, h->chg.row_val, h->chg.row_iy);
}

// A stepping call begins: its records replace those of the call before
static int changes_begin(gpf_handle* h) {
    if (!h->chg.armed()) return GPF_OK;
    GPF_TRY(changes_refusal(h, "gpf_step with changes armed"));
    h->chg.forget();
    return changes_buffers(h);
}

// The two launches on the handle's stream: the record of the committed state against the other buffer into `slot` if the step
// count is `expect`
static int changes_enqueue(gpf_handle* h, long long expect, long long slot) {
    ChangeArgs f;
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.st = h->st;
    f.part = h->chg.part; f.row_val = h->chg.row_val; f.row_iy = h->chg.row_iy; f.rec = h->chg.rec; f.cell = h->chg.cell;
    f.L = h->L; f.dx = h->cfg.dx; f.dy = h->cfg.dy;
    f.wide = changes_wide_ok(h) ? 1 : 0;
    f.slot = slot; f.cap = h->log_cap;
    hipLaunchKernelGGL(k_change_partial, dim3(h->L.Nx), dim3(256), 0, h->stream, f, expect);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_change_fold, dim3(1), dim3(256), 0, h->stream, f, expect);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without changes armed.
static int changes_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->chg.every, expect)) return GPF_OK;
    return changes_enqueue(h, expect, series_slot(base, expect, h->chg.every));
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host
static int changes_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->chg.every, h->chg.steps, base, ran, series_channel(h->chg.host, h->chg.rec, (size_t)CHANGE_NREC),
                          series_channel(h->chg.cells, h->chg.cell, (size_t)2 * CHANGE_NMAX));
}

static SeriesBuffers changes_owned(gpf_handle* h) {
    return {(void**)&h->chg.rec, (void**)&h->chg.cell, (void**)&h->chg.part, (void**)&h->chg.row_val, (void**)&h->chg.row_iy};
}

static int changes_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(changes_owned(h)));
    h->chg.disarm();
    return GPF_OK;
}

extern "C" int gpf_changes_set(gpf_handle* h, int64_t every) {
    GPF_TRY(series_set_checks(h, SERIES[S_CHANGES], every, changes_refusal));
    GPF_TRY(series_disarm(h, SERIES[S_CHANGES]));
    h->chg.every = every;
    return GPF_OK;
}

extern "C" int gpf_changes_clear(gpf_handle* h) { return series_clear(h, SERIES[S_CHANGES]); }

extern "C" int gpf_changes_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->chg.armed()) return fail(GPF_ERR_STATE, "gpf_changes_read: no changes are armed (gpf_changes_set)");
    series_read(h->chg.steps, capacity_records, steps_out, n_records, series_channel(h->chg.host, values, (size_t)CHANGE_NREC),
                series_channel(h->chg.cells, cells, (size_t)2 * CHANGE_NMAX));
    return GPF_OK;
}

extern "C" int gpf_changes_now(gpf_handle* h, double values[11], int32_t cells[6]) {
    GPF_TRY(series_now_checks(h, SERIES[S_CHANGES], values && cells, changes_refusal));
    GPF_TRY(enter(h, true));
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_CHANGES], s));
    if (!h->prev_state_valid) {
        const char* why = h->prev_lost == PREV_LOST_CLOSURES ? "gpf_update_closures has reused the buffer for the predictor's field"
                        : h->prev_lost == PREV_LOST_STAGEWISE ? "the last step was stage-wise"
                        : h->prev_lost == PREV_LOST_PLAN ? "the step plan's timing launches have reused the buffer"
                        : "no step has been committed since gpf_pre_run, an upload of q or the topography, a resampled start or a checkpoint without it";
        return fail(GPF_ERR_STATE, std::string("gpf_changes_now: the state before the last step is not on the device: ") + why);
    }
    GPF_TRY(changes_buffers(h));
    GPF_TRY(changes_enqueue(h, s.step, h->log_cap));            // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(values, h->chg.rec + (size_t)h->log_cap * CHANGE_NREC, CHANGE_NREC * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(cells, h->chg.cell + (size_t)h->log_cap * 2 * CHANGE_NMAX, 2 * CHANGE_NMAX * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/changes_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed changes are put aside
// for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream (series_time).
extern "C" int gpf_changes_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_CHANGES], n, mode, 1, ms, "armed changes (gpf_changes_set)", changes_refusal));
    return series_time_fused(h, SERIES[S_CHANGES], n, mode, ms);
}
