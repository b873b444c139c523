// Part of api.hip (included there, not compiled on its own): whole-film integrals -- load, its moments, the pressure's push on
// the profiled wall, wall friction and flow rates through cross-sections -- reduced on the device behind the committed steps
// whose count is a multiple of the armed stride, and handed out once per call.  Kernels: integral_kernels.hip.
// A handle that steps through k_small_steps records inside the batch (film_record_block, told where by integ.dev): same buffer,
// same slots, same bits, no launch.

static int integrals_nrec(const gpf_handle* h) { return FILM_NSUM + h->integ.nsx + h->integ.nsy; }

// The cases the reduction does not cover: series_refusal's, with its classes and texts, except the elastic gap of one handle
// (el.on).  Its gap is h->topo, the planes the kernels read anyway; only the moment of the record differs: it waits for
// gpf_elastic_update (SERIES_BEHIND_UPDATE), and other handles' closed steps leave no film-integral record.  An elastic slab is
// refused as a slab.
static int integrals_refusal(const gpf_handle* h, const std::string& who) { return series_refusal(h, who, "film integrals", "the film integrals", true); }

// First and last interior row / column; a direction of extent 1 has the one section
static void integrals_default_sections(gpf_handle* h) {
    h->integ.nsx = h->L.Nx > 1 ? 2 : 1; h->integ.sx[0] = 1; h->integ.sx[1] = h->L.Nx;
    h->integ.nsy = h->L.Ny > 1 ? 2 : 1; h->integ.sy[0] = 1; h->integ.sy[1] = h->L.Ny;
}

// 16-byte pair loads of k_film_partial: series_wide_ok's conditions on the planes it reads (GPF_FILM_NARROW, read when the
// buffers are allocated, i.e. at the first record after gpf_integrals_set / _clear, asks for the 8-byte loads regardless, which
// is how tests/test_gpu_integrals.py holds them bit for bit against the wide loads)
static bool film_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->integ.narrow, true); }

static FilmBlockArgs film_block_args(double* rec, long long every, long long cap, double dx, double dy, int nsx, const int* sx, int nsy, const int* sy) {
    FilmBlockArgs b;
    b.rec = rec; b.every = every; b.cap = cap; b.dx = dx; b.dy = dy; b.nsx = nsx; b.nsy = nsy;
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k) { b.sx[k] = k < nsx ? sx[k] : 1; b.sy[k] = k < nsy ? sy[k] : 1; }
    return b;
}

// The record buffer (log_cap slots for a batch + one for gpf_integrals_now) and the row scratch, on first use; armed, also the
// arguments' copy in device memory that k_small_steps reads
static int integrals_buffers(gpf_handle* h) {
    if (!h->integ.nsx) integrals_default_sections(h);
    if (!h->integ.part) {
        h->integ.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
        HIP_TRY(hipMalloc(&h->integ.part, (size_t)h->L.Nx * FILM_NV * sizeof(double)));
    }
    if (!h->integ.rec) HIP_TRY(hipMalloc(&h->integ.rec, (size_t)(h->log_cap + 1) * integrals_nrec(h) * sizeof(double)));
    if (!h->integ.dev && h->integ.every) {      // what k_small_steps records by: stride and sections are fixed until gpf_integrals_set / _clear frees this
        FilmBlockArgs b = film_block_args(h->integ.rec, h->integ.every, h->log_cap, h->cfg.dx, h->cfg.dy, h->integ.nsx, h->integ.sx, h->integ.nsy, h->integ.sy);
        FilmBlockArgs* dev = nullptr;
        HIP_TRY(hipMalloc(&dev, sizeof(b)));
        hipError_t e = hipMemcpy(dev, &b, sizeof(b), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(dev); HIP_TRY(e); }
        h->integ.dev = dev;
    }
    return GPF_OK;
}

// A stepping call begins: its records replace those of the call before
static int integrals_begin(gpf_handle* h) {
    h->integ.pending = false;
    if (!h->integ.armed()) return GPF_OK;
    GPF_TRY(integrals_refusal(h, "gpf_step with film integrals armed"));
    h->integ.forget();
    return integrals_buffers(h);
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int integrals_enqueue(gpf_handle* h, long long expect, long long slot) {
    FilmArgs f;
    series_row_args(h, film_wide_ok(h), slot, f);
    f.part = h->integ.part; f.rec = h->integ.rec;
    f.nsx = h->integ.nsx; f.nsy = h->integ.nsy;
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k) { f.sx[k] = k < f.nsx ? h->integ.sx[k] : 1; f.sy[k] = k < f.nsy ? h->integ.sy[k] : 1; }
    const dim3 grid(h->L.Nx);
    SERIES_ROWS_ENQUEUE(h, k_film_partial, k_film_fold, grid, f, expect);
    return GPF_OK;
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without integrals armed.
static int integrals_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->integ.every, expect)) return GPF_OK;
    return integrals_enqueue(h, expect, series_slot(base, expect, h->integ.every));
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host
static int integrals_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->integ.every, h->integ.steps, base, ran, series_channel(h->integ.host, h->integ.rec, (size_t)integrals_nrec(h)));
}

static SeriesBuffers integrals_owned(gpf_handle* h) { return {(void**)&h->integ.rec, (void**)&h->integ.part, (void**)&h->integ.dev}; }

static int integrals_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(integrals_owned(h)));
    h->integ.disarm(); h->integ.nsx = h->integ.nsy = 0;
    return GPF_OK;
}

extern "C" int gpf_integrals_set(gpf_handle* h, int64_t every, int nsx, const int32_t* ix, int nsy, const int32_t* iy) {
    GPF_TRY(series_set_checks(h, SERIES[S_INTEGRALS], every, integrals_refusal));
    if (nsx > FILM_MAX_SECTIONS || nsy > FILM_MAX_SECTIONS)
        return fail(GPF_ERR_INVALID, "gpf_integrals_set: section " + std::to_string(FILM_MAX_SECTIONS) + " is one too many (" +
                                     std::to_string(std::max(nsx, nsy)) + " given, at most " + std::to_string(FILM_MAX_SECTIONS) + " per direction)");
    for (int k = 0; ix && k < nsx; ++k)
        if (ix[k] < 1 || ix[k] > h->L.Nx)
            return fail(GPF_ERR_INVALID, "gpf_integrals_set: x-section " + std::to_string(k) + " at row " + std::to_string(ix[k]) +
                                         " lies outside the interior rows 1.." + std::to_string(h->L.Nx));
    for (int k = 0; iy && k < nsy; ++k)
        if (iy[k] < 1 || iy[k] > h->L.Ny)
            return fail(GPF_ERR_INVALID, "gpf_integrals_set: y-section " + std::to_string(k) + " at column " + std::to_string(iy[k]) +
                                         " lies outside the interior columns 1.." + std::to_string(h->L.Ny));
    GPF_TRY(series_disarm(h, SERIES[S_INTEGRALS]));
    integrals_default_sections(h);
    if (ix && nsx > 0) { h->integ.nsx = nsx; for (int k = 0; k < nsx; ++k) h->integ.sx[k] = ix[k]; }
    if (iy && nsy > 0) { h->integ.nsy = nsy; for (int k = 0; k < nsy; ++k) h->integ.sy[k] = iy[k]; }
    h->integ.every = every;
    return GPF_OK;
}

extern "C" int gpf_integrals_clear(gpf_handle* h) { return series_clear(h, SERIES[S_INTEGRALS]); }

extern "C" int gpf_integrals_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->integ.armed()) return fail(GPF_ERR_STATE, "gpf_integrals_read: no integrals are armed (gpf_integrals_set)");
    series_read(h->integ.steps, capacity_records, steps_out, n_records, series_channel(h->integ.host, out, (size_t)integrals_nrec(h)));
    return GPF_OK;
}

extern "C" int gpf_integrals_in_batch(gpf_handle* h, int* yes) {
    if (!h || !yes) return fail(GPF_ERR_INVALID, "gpf_integrals_in_batch: null argument");
    *yes = h->integ.armed() && small_grid_eligible(h) ? 1 : 0;
    return GPF_OK;
}

extern "C" int gpf_integrals_now(gpf_handle* h, double* out, int64_t count) {
    GPF_TRY(series_now_checks(h, SERIES[S_INTEGRALS], out != nullptr, integrals_refusal));
    GPF_TRY(enter(h, true));
    GPF_TRY(integrals_buffers(h));
    const int nrec = integrals_nrec(h);
    if (count < nrec) return fail(GPF_ERR_INVALID, "gpf_integrals_now: room for " + std::to_string(nrec) + " doubles required, " + std::to_string(count) + " given");
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_INTEGRALS], s));
    GPF_TRY(integrals_enqueue(h, s.step, h->log_cap));          // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(out, h->integ.rec + (size_t)h->log_cap * nrec, (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/integrals_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed integrals are put
// aside for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream (series_time).
extern "C" int gpf_integrals_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_INTEGRALS], n, mode, 1, ms, "armed integrals (gpf_integrals_set)", integrals_refusal));
    if (h->el.on) {         // an elastic handle: n stage-wise steps, each with its gpf_elastic_update and the record behind it
        GPF_TRY(enter(h));
        SeriesAside aside(h, mode == 1 ? &h->integ.every : nullptr);
        std::vector<double> host;
        std::vector<long long> steps;
        const int rc = series_time(h, "gpf_integrals_time", aside,
                                   [&](long long) { return series_time_stagewise_steps(h, n, [&] { series_time_keep(h->integ.host, h->integ.steps, host, steps); }); },
                                   [&](long long, long long) { h->integ.host.swap(host); h->integ.steps.swap(steps); return (int)GPF_OK; }, ms);
        prev_state_lost(h, PREV_LOST_STAGEWISE);    // (series_resync speaks of fused steps: a closed step leaves its working field in the other buffer)
        return rc;
    }
    return series_time_fused(h, SERIES[S_INTEGRALS], n, mode, ms);
}
