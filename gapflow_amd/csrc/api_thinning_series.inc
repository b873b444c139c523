// Part of api.hip (included there, not compiled on its own): the shear-thinning series of a handle with properties.thinning --
// the load, the wall friction with the thinned and with the Newtonian viscosity, the sums of the viscosity and of the shear
// rate, the smallest and largest viscosity and the largest shear rate with their cells -- reduced on the device behind the
// gpf_close_step that commits a step whose count is a multiple of the armed stride, and handed out once per call.
// Kernels: thinning_series_kernels.hip.  A thinning handle steps stage-wise; where its gap is elastic too the gap deforms after
// the step closes, and the record waits for gpf_elastic_update as the extrema's does (SERIES_AT_CLOSE_UNLESS_ELASTIC): it holds
// the state and the gap the handle then holds.

// The cases the series does not cover
static int thin_refusal(const gpf_handle* h, const std::string& who) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; the thinning series is not available on slabs");
    if (h->cfg.thinning == GPF_THINNING_NONE) return fail(GPF_ERR_STATE, who + ": no shear thinning (gpf_config.thinning)");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set)
        return fail(GPF_ERR_INVALID, who + ": surrogate closures: the thinning series evaluates the analytic pressure and wall stress, which this handle replaces");
    return GPF_OK;
}

// 16-byte pair loads of k_thin_partial: series_wide_ok's conditions on the planes it reads, the slip-length plane among them
static bool thin_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->thin.narrow, true); }

// The record buffers (log_cap slots + one for gpf_thinning_series_now) and the row scratch, on first use
static int thin_buffers(gpf_handle* h) {
    auto& d = h->thin;
    const size_t slots = (size_t)h->log_cap + 1, nx = (size_t)h->L.Nx;
    if (!d.rec) {
        d.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
        DBG("thin_buffers: k_thin_partial takes %s pair loads", thin_wide_ok(h) ? "16-byte" : "8-byte");     // (GPF_DEBUG: the narrow-load test reads this)
        HIP_TRY(hipMalloc(&d.rec, slots * THIN_NREC * sizeof(double)));
    }
    if (!d.part) HIP_TRY(hipMalloc(&d.part, nx * THIN_NSUM * sizeof(double)));
    return series_first_buffers(h, THIN_NEXT, d.cell, d.row_val, d.row_iy);
}

// A stepping call begins: its records replace those of the call before
static int thin_begin(gpf_handle* h) {
    h->thin.pending = false;
    if (!h->thin.armed()) return GPF_OK;
    GPF_TRY(thin_refusal(h, "a stepping call with the thinning series armed"));
    h->thin.forget();
    return thin_buffers(h);
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int thin_enqueue(gpf_handle* h, long long expect, long long slot) {
    const auto& d = h->thin;
    ThinArgs f;
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.Ls = h->Ls; f.st = h->st;
    f.part = d.part; f.row_val = d.row_val; f.row_iy = d.row_iy; f.rec = d.rec; f.cell = d.cell;
    f.L = h->L; f.dx = h->cfg.dx; f.dy = h->cfg.dy;
    f.wide = thin_wide_ok(h) ? 1 : 0;
    f.slot = slot; f.cap = h->log_cap;
    const dim3 grid(h->L.Nx, 1);
    SERIES_ROWS_ENQUEUE(h, k_thin_partial, k_thin_fold, grid, f, expect);
    return GPF_OK;
}

// Behind gpf_close_step's launches, or gpf_elastic_update's on an elastic handle: the record of the step that took the count to `expect`
static int thin_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->thin.every, expect)) return GPF_OK;
    return thin_enqueue(h, expect, series_slot(base, expect, h->thin.every));
}

static int thin_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->thin.every, h->thin.steps, base, ran, series_channel(h->thin.host, h->thin.rec, (size_t)THIN_NREC),
                          series_channel(h->thin.cells, h->thin.cell, (size_t)2 * THIN_NEXT));
}

static SeriesBuffers thin_owned(gpf_handle* h) {
    auto& d = h->thin;
    return {(void**)&d.rec, (void**)&d.cell, (void**)&d.part, (void**)&d.row_val, (void**)&d.row_iy};
}

static int thin_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(thin_owned(h)));
    h->thin.disarm();
    return GPF_OK;
}

extern "C" int gpf_thinning_series_set(gpf_handle* h, int64_t every) {
    GPF_TRY(series_set_checks(h, SERIES[S_THIN], every, thin_refusal));
    GPF_TRY(series_disarm(h, SERIES[S_THIN]));
    h->thin.every = every;
    return GPF_OK;
}

extern "C" int gpf_thinning_series_clear(gpf_handle* h) { return series_clear(h, SERIES[S_THIN]); }

extern "C" int gpf_thinning_series_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->thin.armed()) return fail(GPF_ERR_STATE, "gpf_thinning_series_read: the thinning series is not armed (gpf_thinning_series_set)");
    series_read(h->thin.steps, capacity_records, steps_out, n_records, series_channel(h->thin.host, values, (size_t)THIN_NREC),
                series_channel(h->thin.cells, cells, (size_t)2 * THIN_NEXT));
    return GPF_OK;
}

extern "C" int gpf_thinning_series_now(gpf_handle* h, double values[14], int32_t cells[6]) {
    GPF_TRY(series_now_checks(h, SERIES[S_THIN], values && cells, thin_refusal));
    GPF_TRY(enter(h, true));
    GPF_TRY(thin_buffers(h));
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_THIN], s));
    GPF_TRY(thin_enqueue(h, s.step, h->log_cap));               // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(values, h->thin.rec + (size_t)h->log_cap * THIN_NREC, THIN_NREC * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(cells, h->thin.cell + (size_t)h->log_cap * 2 * THIN_NEXT, 2 * THIN_NEXT * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/thinning_series_time.py): n steps as a host takes them on a thinning handle -- the stage-wise calls, and
// gpf_elastic_update where the gap is elastic (series_time_stagewise_steps) --, with `mode` 0 nothing (the armed series is put
// aside for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream, the host's share of
// such steps included (series_time).
extern "C" int gpf_thinning_series_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_THIN], n, mode, 1, ms, "the armed series (gpf_thinning_series_set)", thin_refusal));
    GPF_TRY(enter(h));
    SeriesAside aside(h, mode == 1 ? &h->thin.every : nullptr);
    std::vector<double> host;
    std::vector<int32_t> cells;
    std::vector<long long> steps;
    const int rc = series_time(h, "gpf_thinning_series_time", aside,
                               [&](long long) {
                                   return series_time_stagewise_steps(h, n, [&] {
                                       cells.insert(cells.end(), h->thin.cells.begin(), h->thin.cells.end());
                                       h->thin.cells.clear();
                                       series_time_keep(h->thin.host, h->thin.steps, host, steps);
                                   });
                               },
                               [&](long long, long long) { h->thin.host.swap(host); h->thin.cells.swap(cells); h->thin.steps.swap(steps); return (int)GPF_OK; }, ms);
    prev_state_lost(h, PREV_LOST_STAGEWISE);    // (series_resync speaks of fused steps: a closed step leaves its working field in the other buffer)
    return rc;
}
