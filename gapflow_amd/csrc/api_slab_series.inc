// Part of api.hip (included there, not compiled on its own): the domain series of an x-slab -- the film integrals and the field
// extrema of the WHOLE domain, recorded by every rank behind the committed steps whose count is a multiple of the series' stride
// and handed out once per stepping call.  Kernels: slab_series_kernels.hip; the cut and the message geometry: slab_rows.hpp.
//
// The host steps a slab (gapflow_amd/slab.py: SlabDriver), so a record is two calls around the host's collective:
//   gpf_slab_series_local   the partials of the series due at the step count `expect`, into this rank's message
//   (one all-gather of the message)
//   gpf_slab_series_fold    the folds of those series over the gathered messages, into the records
// between gpf_slab_series_begin (a stepping call begins: the step count it begins at, the records of the call before forgotten)
// and gpf_slab_series_end (the state read, the records of the committed steps -> host).  All launches go to the handle's stream.
//
// What is api_series.inc's and what is not: the arithmetic of a stride's records (series_due, series_slot), the record store
// (one SeriesStore per series), the way to the host and out of it (series_collect, series_read, series_channel), the alignment
// test of the pair loads, series_row_args and series_free are used as they are.  The recorder has NO row in the table SERIES and
// its state lies beside the nine recorders' (gpf_handle::sser): a row is one stride and one launch hook behind a step that
// gpf_step, gpf_close_step or gpf_elastic_update enqueues, all of which refuse a slab, while this recorder has two strides under
// one name, its launches are split around a collective that only the host can run, and its stepping call is the host's loop --
// nothing that walks the table could call it, and the table's walks stay what they were for the nine.

static int slab_series_nrec(const gpf_handle* h) { return FILM_NSUM + h->sser.nsx + h->sser.nsy; }
static bool slab_series_is_set(const gpf_handle* h) { return h->sser.nranks > 0; }

// The cases the domain series do not cover.  These handles step stage-wise on slabs (gapflow_amd/slab.py: _stagewise_step), and
// the film integrals evaluate the analytic closures without grad p.  A slip-length plane: SlabProblem never uploads one, so no
// kernel is instantiated for it.
static int slab_series_refusal(const gpf_handle* h, const std::string& who) {
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set)
        return fail(GPF_ERR_INVALID, who + ": surrogate closures: the domain series evaluate the analytic pressure and wall stress, which this handle replaces "
                                           "(and a slab with surrogates steps stage-wise)");
    if (h->cfg.thinning != GPF_THINNING_NONE) return fail(GPF_ERR_INVALID, who + ": shear thinning needs grad p and steps stage-wise on slabs (not supported)");
    if (h->el.on || h->els.on) return fail(GPF_ERR_INVALID, who + ": an elastic gap steps stage-wise on slabs and deforms between steps (not supported)");
    if (h->Ls) return fail(GPF_ERR_INVALID, who + ": this handle holds a slip-length plane (not supported on slabs)");
    return GPF_OK;
}

static SeriesBuffers slab_series_film_owned(gpf_handle* h) { return {(void**)&h->sser.msg, (void**)&h->sser.rec, (void**)&h->sser.film_t}; }
static SeriesBuffers slab_series_ext_owned(gpf_handle* h) { return {(void**)&h->sser.val, (void**)&h->sser.cell, (void**)&h->sser.ext_t}; }

static int slab_series_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(slab_series_film_owned(h)));
    GPF_TRY(series_free(slab_series_ext_owned(h)));
    h->sser.film.disarm(); h->sser.ext.disarm();
    h->sser.film_time.clear(); h->sser.ext_time.clear();
    h->sser.nranks = 0; h->sser.nsx = h->sser.nsy = 0; h->sser.now_step = -1;
    return GPF_OK;
}

// gpf_destroy (the stream has been drained; errors are not reported there)
static void slab_series_destroy(gpf_handle* h) {
    for (const SeriesBuffers& owned : {slab_series_film_owned(h), slab_series_ext_owned(h)})
        for (void** p : owned)
            if (p && *p) (void)hipFree(*p);
}

extern "C" int gpf_slab_series_set(gpf_handle* h, int row0, int nx_global, int nranks, int64_t every_integrals, int nsx, const int32_t* ix,
                                   int nsy, const int32_t* iy, int64_t every_extrema) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    const std::string who = "gpf_slab_series_set";
    GPF_TRY(slab_series_refusal(h, who));
    if (h->p2p.on) return fail(GPF_ERR_STATE, who + ": this handle steps over the peer-to-peer transport, whose batches have no host between steps (not supported)");
    if (every_integrals < 0 || every_extrema < 0)
        return fail(GPF_ERR_INVALID, who + ": every >= 0 required (0: that series is off; gpf_slab_series_clear disarms), got " +
                                     std::to_string(every_integrals < 0 ? every_integrals : every_extrema));
    switch (slab_check(row0, h->L.Nx, nx_global, nranks)) {
    case 1: return fail(GPF_ERR_INVALID, who + ": " + std::to_string(nx_global) + " rows cannot be cut into " + std::to_string(nranks) + " slabs");
    case 2: return fail(GPF_ERR_INVALID, who + ": " + std::to_string(h->L.Nx) + " rows from global row " + std::to_string(row0 + 1) + " are no rank's slab of " +
                                         std::to_string(nx_global) + " rows cut into " + std::to_string(nranks));
    }
    if (nsx > FILM_MAX_SECTIONS || nsy > FILM_MAX_SECTIONS)
        return fail(GPF_ERR_INVALID, who + ": section " + std::to_string(FILM_MAX_SECTIONS) + " is one too many (" + std::to_string(std::max(nsx, nsy)) +
                                     " given, at most " + std::to_string(FILM_MAX_SECTIONS) + " per direction)");
    for (int k = 0; ix && k < nsx; ++k)
        if (ix[k] < 1 || ix[k] > nx_global)
            return fail(GPF_ERR_INVALID, who + ": x-section " + std::to_string(k) + " at row " + std::to_string(ix[k]) + " lies outside the interior rows 1.." +
                                         std::to_string(nx_global));
    for (int k = 0; iy && k < nsy; ++k)
        if (iy[k] < 1 || iy[k] > h->L.Ny)
            return fail(GPF_ERR_INVALID, who + ": y-section " + std::to_string(k) + " at column " + std::to_string(iy[k]) +
                                         " lies outside the interior columns 1.." + std::to_string(h->L.Ny));
    GPF_TRY(enter(h, true));
    GPF_TRY(slab_series_release(h));
    auto& s = h->sser;
    // first and last interior row / column of the DOMAIN; a direction of extent 1 has the one section
    s.nsx = nx_global > 1 ? 2 : 1; s.sx[0] = 1; s.sx[1] = nx_global;
    s.nsy = h->L.Ny > 1 ? 2 : 1; s.sy[0] = 1; s.sy[1] = h->L.Ny;
    if (ix && nsx > 0) { s.nsx = nsx; for (int k = 0; k < nsx; ++k) s.sx[k] = ix[k]; }
    if (iy && nsy > 0) { s.nsy = nsy; for (int k = 0; k < nsy; ++k) s.sy[k] = iy[k]; }
    const int max_nx = slab_max_nx(nx_global, nranks);
    const size_t slots = (size_t)h->log_cap + 1;
    s.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
    HIP_TRY(hipMalloc(&s.msg, (size_t)max_nx * SLAB_SERIES_W * sizeof(double)));
    HIP_TRY(hipMemset(s.msg, 0, (size_t)max_nx * SLAB_SERIES_W * sizeof(double)));     // (the padding rows travel, unread)
    HIP_TRY(hipMalloc(&s.rec, slots * (size_t)(FILM_NSUM + s.nsx + s.nsy) * sizeof(double)));
    HIP_TRY(hipMalloc(&s.film_t, slots * sizeof(double)));
    HIP_TRY(hipMalloc(&s.val, slots * EXTREMA_NQ * sizeof(double)));
    HIP_TRY(hipMalloc(&s.cell, slots * 2 * EXTREMA_NQ * sizeof(int)));
    HIP_TRY(hipMalloc(&s.ext_t, slots * sizeof(double)));
    s.row0 = row0; s.nx_global = nx_global; s.max_nx = max_nx;
    s.film.every = every_integrals; s.ext.every = every_extrema;
    s.base = h->host_step;
    s.nranks = nranks;      // last: the series is set once everything it describes is in place
    return GPF_OK;
}

extern "C" int gpf_slab_series_clear(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (h->step_open) return fail(GPF_ERR_STATE, "gpf_slab_series_clear: a stage-wise step is open; close it first");
    GPF_TRY(enter(h, true));
    return slab_series_release(h);
}

extern "C" int gpf_slab_series_message(gpf_handle* h, void** message, size_t* count) {
    if (!h || !message || !count) return fail(GPF_ERR_INVALID, "gpf_slab_series_message: null argument");
    if (!slab_series_is_set(h)) return fail(GPF_ERR_STATE, "gpf_slab_series_message: no domain series are set (gpf_slab_series_set)");
    *message = h->sser.msg;
    *count = (size_t)h->sser.max_nx * SLAB_SERIES_W;
    return GPF_OK;
}

// What every recording call checks: the series set, the cases it refuses (a model or a plane may have come since), and for a
// fold the gathered buffer's size
static int slab_series_call_checks(gpf_handle* h, const std::string& who, bool fold, const void* gathered, size_t count) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!slab_series_is_set(h)) return fail(GPF_ERR_STATE, who + ": no domain series are set (gpf_slab_series_set)");
    if (!h->has_q || !h->has_topo) return fail(GPF_ERR_STATE, who + ": upload q and topography first");
    GPF_TRY(slab_series_refusal(h, who));
    if (fold) {
        if (!gathered) return fail(GPF_ERR_INVALID, who + ": null argument");
        const size_t want = (size_t)h->sser.nranks * h->sser.max_nx * SLAB_SERIES_W;
        if (count != want) return fail(GPF_ERR_INVALID, who + ": the gathered messages hold " + std::to_string(want) + " doubles (ranks x longest slab x " +
                                                         std::to_string(SLAB_SERIES_W) + "), " + std::to_string(count) + " given");
    }
    return GPF_OK;
}

static void slab_series_film_args(gpf_handle* h, const double* gathered, long long slot, SlabFilmArgs& f) {
    const auto& s = h->sser;
    series_row_args(h, series_wide_ok(h, s.narrow, false), slot, f);
    f.msg = s.msg; f.gathered = gathered; f.rec = s.rec; f.time = s.film_t;
    f.nsx = s.nsx; f.nsy = s.nsy;
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k) { f.sx[k] = k < f.nsx ? s.sx[k] : 1; f.sy[k] = k < f.nsy ? s.sy[k] : 1; }
    f.row0 = s.row0; f.nx_global = s.nx_global; f.nranks = s.nranks;
}

static void slab_series_ext_args(gpf_handle* h, const double* gathered, long long slot, SlabExtremaArgs& e) {
    const auto& s = h->sser;
    e.qa = h->q[0]; e.qb = h->q[1]; e.topo = h->topo; e.st = h->st;
    e.msg = s.msg; e.gathered = gathered; e.time = s.ext_t;
    e.x = ExtremaArgs{};
    e.x.val = s.val; e.x.cell = s.cell; e.x.cap = h->log_cap;
    e.L = h->L; e.wide = series_wide_ok(h, s.narrow, false) ? 1 : 0;
    e.nx_global = s.nx_global; e.nranks = s.nranks; e.slot = slot;
}

// The partials (gathered null) or the folds of the series `film` / `ext` name, the record of the committed state into the slots
// given if the step count is `expect`
static int slab_series_enqueue(gpf_handle* h, const double* gathered, long long expect, bool film, long long film_slot, bool ext, long long ext_slot) {
    if (film) {
        SlabFilmArgs f;
        slab_series_film_args(h, gathered, film_slot, f);
        if (gathered) hipLaunchKernelGGL(k_slab_film_fold, dim3(1), dim3(256), 0, h->stream, f, expect);
        else EOS_DISPATCH(h->cfg.eos, { hipLaunchKernelGGL((k_slab_film_partial<EOS_>), dim3(h->L.Nx), dim3(256), 0, h->stream, f, h->P, expect); });
        HIP_TRY(hipGetLastError());
    }
    if (ext) {
        SlabExtremaArgs e;
        slab_series_ext_args(h, gathered, ext_slot, e);
        if (gathered) hipLaunchKernelGGL(k_slab_extrema_fold, dim3(1), dim3(256), 0, h->stream, e, expect);
        else EOS_DISPATCH(h->cfg.eos, { hipLaunchKernelGGL((k_slab_extrema_partial<EOS_>), dim3(h->L.Nx), dim3(256), 0, h->stream, e, h->P, expect); });
        HIP_TRY(hipGetLastError());
    }
    return GPF_OK;
}

// ... of a stepping call that began at sser.base: the series due at `expect`, each into the slot of its rank among the call's records
static int slab_series_step(gpf_handle* h, const std::string& who, const double* gathered, long long expect) {
    auto& s = h->sser;
    if (expect <= s.base) return fail(GPF_ERR_INVALID, who + ": step " + std::to_string(expect) + " does not lie behind the step count " +
                                                       std::to_string(s.base) + " the stepping call began at (gpf_slab_series_begin)");
    const bool film = series_due(s.film.every, expect), ext = series_due(s.ext.every, expect);
    const long long fs = film ? series_slot(s.base, expect, s.film.every) : 0, es = ext ? series_slot(s.base, expect, s.ext.every) : 0;
    if (fs >= h->log_cap || es >= h->log_cap)
        return fail(GPF_ERR_INVALID, who + ": more than " + std::to_string(h->log_cap) + " records in one stepping call; end it and begin another");
    GPF_TRY(enter(h, true));
    return slab_series_enqueue(h, gathered, expect, film, fs, ext, es);
}

extern "C" int gpf_slab_series_begin(gpf_handle* h, int64_t* base) {
    GPF_TRY(slab_series_call_checks(h, "gpf_slab_series_begin", false, nullptr, 0));
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_slab_series_begin: call gpf_pre_run first");
    GPF_TRY(enter(h, true));
    StepState st;
    GPF_TRY(read_state(h, st));
    auto& s = h->sser;
    h->host_step = st.step; h->next_step = st.step;
    s.base = st.step;
    s.film.forget(); s.ext.forget(); s.film_time.clear(); s.ext_time.clear();
    if (base) *base = st.step;
    return GPF_OK;
}

extern "C" int gpf_slab_series_local(gpf_handle* h, int64_t expect) {
    GPF_TRY(slab_series_call_checks(h, "gpf_slab_series_local", false, nullptr, 0));
    return slab_series_step(h, "gpf_slab_series_local", nullptr, expect);
}

extern "C" int gpf_slab_series_fold(gpf_handle* h, const void* gathered, size_t count, int64_t expect) {
    GPF_TRY(slab_series_call_checks(h, "gpf_slab_series_fold", true, gathered, count));
    return slab_series_step(h, "gpf_slab_series_fold", (const double*)gathered, expect);
}

extern "C" int gpf_slab_series_end(gpf_handle* h, int64_t* ran) {
    GPF_TRY(slab_series_call_checks(h, "gpf_slab_series_end", false, nullptr, 0));
    GPF_TRY(enter(h, true));
    StepState st;
    GPF_TRY(read_state(h, st));
    auto& s = h->sser;
    const long long n = st.step - s.base;
    GPF_TRY(series_collect(s.film.every, s.film.steps, s.base, n, series_channel(s.film.host, s.rec, (size_t)slab_series_nrec(h)),
                           series_channel(s.film_time, s.film_t, 1)));
    GPF_TRY(series_collect(s.ext.every, s.ext.steps, s.base, n, series_channel(s.ext.host, s.val, (size_t)EXTREMA_NQ),
                           series_channel(s.ext.cells, s.cell, (size_t)2 * EXTREMA_NQ), series_channel(s.ext_time, s.ext_t, 1)));
    h->host_step = st.step; h->next_step = st.step;
    s.base = st.step;       // (a call that goes on without another begin would write over slots already collected: local / fold say so)
    if (ran) *ran = n;
    return GPF_OK;
}

extern "C" int gpf_slab_series_read(gpf_handle* h, int which, double* values, int32_t* cells, double* times, int64_t capacity_records, int64_t* steps_out,
                                    int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (which < 0 || which > 1) return fail(GPF_ERR_INVALID, "gpf_slab_series_read: which must be 0 (film integrals) or 1 (field extrema)");
    auto& s = h->sser;
    SeriesStore& store = which == 0 ? s.film : s.ext;
    if (!slab_series_is_set(h) || !store.armed())
        return fail(GPF_ERR_STATE, std::string("gpf_slab_series_read: the domain ") + (which == 0 ? "film integrals" : "field extrema") + " are not armed (gpf_slab_series_set)");
    if (which == 0)
        series_read(store.steps, capacity_records, steps_out, n_records, series_channel(store.host, values, (size_t)slab_series_nrec(h)),
                    series_channel(s.film_time, times, 1));
    else
        series_read(store.steps, capacity_records, steps_out, n_records, series_channel(store.host, values, (size_t)EXTREMA_NQ),
                    series_channel(store.cells, cells, (size_t)2 * EXTREMA_NQ), series_channel(s.ext_time, times, 1));
    return GPF_OK;
}

extern "C" int gpf_slab_series_now_local(gpf_handle* h) {
    GPF_TRY(slab_series_call_checks(h, "gpf_slab_series_now_local", false, nullptr, 0));
    GPF_TRY(enter(h, true));
    StepState st;
    GPF_TRY(read_state(h, st));
    if (st.invalid) return fail(GPF_ERR_STATE, "gpf_slab_series_now_local: the run state is flagged invalid (the last step was rolled back)");
    h->sser.now_step = st.step;
    return slab_series_enqueue(h, nullptr, st.step, true, h->log_cap, true, h->log_cap);        // the slot behind a call's
}

extern "C" int gpf_slab_series_now_fold(gpf_handle* h, const void* gathered, size_t count, double* integrals, int64_t integrals_count, double values[7],
                                        int32_t cells[14]) {
    GPF_TRY(slab_series_call_checks(h, "gpf_slab_series_now_fold", true, gathered, count));
    if (!integrals || !values || !cells) return fail(GPF_ERR_INVALID, "gpf_slab_series_now_fold: null argument");
    auto& s = h->sser;
    const int nrec = slab_series_nrec(h);
    if (integrals_count < nrec)
        return fail(GPF_ERR_INVALID, "gpf_slab_series_now_fold: room for " + std::to_string(nrec) + " doubles required, " + std::to_string(integrals_count) + " given");
    if (s.now_step < 0) return fail(GPF_ERR_STATE, "gpf_slab_series_now_fold without gpf_slab_series_now_local");
    GPF_TRY(enter(h, true));
    const long long at = s.now_step, cap = h->log_cap;
    s.now_step = -1;
    GPF_TRY(slab_series_enqueue(h, (const double*)gathered, at, true, cap, true, cap));
    HIP_TRY(hipMemcpyAsync(integrals, s.rec + (size_t)cap * nrec, (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(values, s.val + (size_t)cap * EXTREMA_NQ, EXTREMA_NQ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(cells, s.cell + (size_t)cap * 2 * EXTREMA_NQ, 2 * EXTREMA_NQ * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}
