// Part of api.hip (included there, not compiled on its own): the deformation series of an elastic handle -- displaced volume,
// squared deflection, p d, film volume, the largest and smallest deflection with their cells -- reduced on the device behind the
// gpf_elastic_update that follows a committed step whose count is a multiple of the armed stride, and handed out once per call.
// Kernels: elastic_series_kernels.hip.  The gap deforms after the step closes, so a record written at gpf_close_step would pair
// the new state with the gap of the step before: every record waits for the update (SERIES_BEHIND_UPDATE, as the extrema's and
// the film integrals' on such a handle) and holds the state, the gap and the deformation the handle then holds.

// The cases the series does not cover
static int eldef_refusal(const gpf_handle* h, const std::string& who) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; the deformation series is not available on slabs");
    if (!h->el.on) return fail(GPF_ERR_STATE, who + ": no elastic gap (gpf_elastic_setup)");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set) return fail(GPF_ERR_INVALID, who + ": p d needs the EOS pressure, this handle's pressure comes from a surrogate");
    return GPF_OK;
}

// 16-byte pair loads of k_eldef_partial: series_wide_ok's conditions on the planes it reads, the deformation plane among them
static bool eldef_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->eldef.narrow, false, h->el.deformation); }

// The record buffers (log_cap slots + one for gpf_elastic_series_now) and the row scratch, on first use
static int eldef_buffers(gpf_handle* h) {
    auto& d = h->eldef;
    const size_t slots = (size_t)h->log_cap + 1, nx = (size_t)h->L.Nx;
    if (!d.rec) {
        d.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
        DBG("eldef_buffers: k_eldef_partial takes %s pair loads", eldef_wide_ok(h) ? "16-byte" : "8-byte");     // (GPF_DEBUG: the narrow-load test reads this)
        HIP_TRY(hipMalloc(&d.rec, slots * ELDEF_NREC * sizeof(double)));
    }
    if (!d.part) HIP_TRY(hipMalloc(&d.part, nx * ELDEF_NSUM * sizeof(double)));
    return series_first_buffers(h, ELDEF_NEXT, d.cell, d.row_val, d.row_iy);
}

// A stepping call begins: its records replace those of the call before
static int eldef_begin(gpf_handle* h) {
    h->eldef.pending = false;
    if (!h->eldef.armed()) return GPF_OK;
    GPF_TRY(eldef_refusal(h, "a stepping call with the deformation series armed"));
    h->eldef.forget();
    return eldef_buffers(h);
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int eldef_enqueue(gpf_handle* h, long long expect, long long slot) {
    const auto& d = h->eldef;
    ElDefArgs f;
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.d = h->el.deformation; f.st = h->st;
    f.part = d.part; f.row_val = d.row_val; f.row_iy = d.row_iy; f.rec = d.rec; f.cell = d.cell;
    f.L = h->L; f.dx = h->cfg.dx; f.dy = h->cfg.dy;
    f.wide = eldef_wide_ok(h) ? 1 : 0;
    f.slot = slot; f.cap = h->log_cap;
    EOS_DISPATCH(h->cfg.eos, { hipLaunchKernelGGL((k_eldef_partial<EOS_>), dim3(h->L.Nx), dim3(256), 0, h->stream, f, h->P, expect); });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_eldef_fold, dim3(1), dim3(256), 0, h->stream, f, expect);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// Behind gpf_elastic_update's launches (series_after_elastic_update): the record of the step that took the count to `expect`
static int eldef_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->eldef.every, expect)) return GPF_OK;
    return eldef_enqueue(h, expect, series_slot(base, expect, h->eldef.every));
}

static int eldef_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->eldef.every, h->eldef.steps, base, ran, series_channel(h->eldef.host, h->eldef.rec, (size_t)ELDEF_NREC),
                          series_channel(h->eldef.cells, h->eldef.cell, (size_t)2 * ELDEF_NEXT));
}

static SeriesBuffers eldef_owned(gpf_handle* h) {
    auto& d = h->eldef;
    return {(void**)&d.rec, (void**)&d.cell, (void**)&d.part, (void**)&d.row_val, (void**)&d.row_iy};
}

static int eldef_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(eldef_owned(h)));
    h->eldef.disarm();
    return GPF_OK;
}

extern "C" int gpf_elastic_series_set(gpf_handle* h, int64_t every) {
    GPF_TRY(series_set_checks(h, SERIES[S_ELDEF], every, eldef_refusal));
    GPF_TRY(series_disarm(h, SERIES[S_ELDEF]));
    h->eldef.every = every;
    return GPF_OK;
}

extern "C" int gpf_elastic_series_clear(gpf_handle* h) { return series_clear(h, SERIES[S_ELDEF]); }

extern "C" int gpf_elastic_series_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->eldef.armed()) return fail(GPF_ERR_STATE, "gpf_elastic_series_read: the deformation series is not armed (gpf_elastic_series_set)");
    series_read(h->eldef.steps, capacity_records, steps_out, n_records, series_channel(h->eldef.host, values, (size_t)ELDEF_NREC),
                series_channel(h->eldef.cells, cells, (size_t)2 * ELDEF_NEXT));
    return GPF_OK;
}

extern "C" int gpf_elastic_series_now(gpf_handle* h, double values[6], int32_t cells[4]) {
    GPF_TRY(series_now_checks(h, SERIES[S_ELDEF], values && cells, eldef_refusal));
    GPF_TRY(enter(h, true));
    GPF_TRY(eldef_buffers(h));
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_ELDEF], s));
    GPF_TRY(eldef_enqueue(h, s.step, h->log_cap));              // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(values, h->eldef.rec + (size_t)h->log_cap * ELDEF_NREC, ELDEF_NREC * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(cells, h->eldef.cell + (size_t)h->log_cap * 2 * ELDEF_NEXT, 2 * ELDEF_NEXT * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/elastic_series_time.py): n steps as a host takes them on an elastic handle -- the stage-wise calls and
// gpf_elastic_update (series_time_stagewise_steps) --, with `mode` 0 nothing (the armed series is put aside for the call), 1
// recording at the armed stride; *ms = first launch to last on the handle's stream, the host's share of such steps included
// (series_time).
extern "C" int gpf_elastic_series_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_ELDEF], n, mode, 1, ms, "the armed series (gpf_elastic_series_set)", eldef_refusal));
    GPF_TRY(enter(h));
    SeriesAside aside(h, mode == 1 ? &h->eldef.every : nullptr);
    std::vector<double> host;
    std::vector<int32_t> cells;
    std::vector<long long> steps;
    const int rc = series_time(h, "gpf_elastic_series_time", aside,
                               [&](long long) {
                                   return series_time_stagewise_steps(h, n, [&] {
                                       cells.insert(cells.end(), h->eldef.cells.begin(), h->eldef.cells.end());
                                       h->eldef.cells.clear();
                                       series_time_keep(h->eldef.host, h->eldef.steps, host, steps);
                                   });
                               },
                               [&](long long, long long) { h->eldef.host.swap(host); h->eldef.cells.swap(cells); h->eldef.steps.swap(steps); return (int)GPF_OK; }, ms);
    prev_state_lost(h, PREV_LOST_STAGEWISE);    // (series_resync speaks of fused steps: a closed step leaves its working field in the other buffer)
    return rc;
}
