// Part of api.hip (included there, not compiled on its own): field extrema -- the largest and smallest pressure and density, the
// smallest gap, the largest velocity components, each with its cell -- recorded on the device behind the committed steps whose
// count is a multiple of the armed stride, and handed out once per call.  Kernels: extrema_kernels.hip.

// The cases the records do not cover, with the error classes gpf_probes_set gives them
static int extrema_refusal(const gpf_handle* h, const std::string& who) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; extrema are not available on slabs");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set) return fail(GPF_ERR_INVALID, who + ": no EOS pressure to take the extrema of, this handle's pressure comes from a surrogate");
    return GPF_OK;
}

// 16-byte pair loads of k_extrema_partial: series_wide_ok's conditions on the planes it reads (GPF_FILM_NARROW, read when the
// buffers are allocated, asks for the 8-byte loads regardless)
static bool extrema_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->extr.narrow, false); }

// The record buffers (log_cap slots for a batch + one for gpf_extrema_now), the row scratch and the arguments' copy in device
// memory, on first use.  `dev` is set last, once everything it describes is in place.
static int extrema_buffers(gpf_handle* h) {
    ExtremaArgs& a = h->extr.a;
    const size_t slots = (size_t)h->log_cap + 1;
    if (!a.val) {
        h->extr.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
        DBG("extrema_buffers: k_extrema_partial takes %s pair loads", extrema_wide_ok(h) ? "16-byte" : "8-byte");      // (GPF_DEBUG: the narrow-load test reads this)
        HIP_TRY(hipMalloc(&a.val, slots * EXTREMA_NQ * sizeof(double)));
    }
    GPF_TRY(series_first_buffers(h, EXTREMA_NQ, a.cell, a.row_val, a.row_iy));
    a.cap = h->log_cap;
    if (!h->extr.dev) {
        ExtremaArgs* dev = nullptr;
        HIP_TRY(hipMalloc(&dev, sizeof(ExtremaArgs)));
        h->extr.dev = dev;
    }
    const long long every = std::max<long long>(1, h->extr.every);      // (1 while not armed: k_small_steps does not read the copy then)
    if (a.every != every) {                 // the copy k_small_steps reads follows the armed stride; extrema_release zeroes a.every
        a.every = every;
        HIP_TRY(hipMemcpy(h->extr.dev, &a, sizeof(a), hipMemcpyHostToDevice));
    }
    return GPF_OK;
}

// A stepping call begins: its records replace those of the call before
static int extrema_begin(gpf_handle* h) {
    h->extr.pending = false;
    if (!h->extr.armed()) return GPF_OK;
    GPF_TRY(extrema_refusal(h, "a stepping call with extrema armed"));
    h->extr.forget();
    return extrema_buffers(h);
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int extrema_enqueue(gpf_handle* h, long long expect, long long slot) {
    const ExtremaArgs& a = h->extr.a;
    const int wide = extrema_wide_ok(h) ? 1 : 0;
    EOS_DISPATCH(h->cfg.eos, {
        hipLaunchKernelGGL((k_extrema_partial<EOS_>), dim3(h->L.Nx), dim3(256), 0, h->stream, (const double*)h->q[0], (const double*)h->q[1],
                           (const double*)h->topo, (const StepState*)h->st, h->L, h->P, a, wide, expect, slot);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_extrema_fold, dim3(1), dim3(256), 0, h->stream, (const StepState*)h->st, a, h->L.Nx, expect, slot);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without extrema armed.
static int extrema_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->extr.every, expect)) return GPF_OK;
    return extrema_enqueue(h, expect, series_slot(base, expect, h->extr.every));
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host
static int extrema_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->extr.every, h->extr.steps, base, ran, series_channel(h->extr.host, h->extr.a.val, (size_t)EXTREMA_NQ),
                          series_channel(h->extr.cells, h->extr.a.cell, (size_t)2 * EXTREMA_NQ));
}

static SeriesBuffers extrema_owned(gpf_handle* h) {
    ExtremaArgs& a = h->extr.a;
    return {(void**)&a.val, (void**)&a.cell, (void**)&a.row_val, (void**)&a.row_iy, (void**)&h->extr.dev};
}

static int extrema_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(extrema_owned(h)));
    h->extr.a.every = 0; h->extr.a.cap = 0;
    h->extr.disarm();
    return GPF_OK;
}

extern "C" int gpf_extrema_set(gpf_handle* h, int64_t every) {
    GPF_TRY(series_set_checks(h, SERIES[S_EXTREMA], every, extrema_refusal));
    GPF_TRY(series_disarm(h, SERIES[S_EXTREMA]));
    h->extr.every = every;
    return GPF_OK;
}

extern "C" int gpf_extrema_clear(gpf_handle* h) { return series_clear(h, SERIES[S_EXTREMA]); }

extern "C" int gpf_extrema_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->extr.armed()) return fail(GPF_ERR_STATE, "gpf_extrema_read: no extrema are armed (gpf_extrema_set)");
    series_read(h->extr.steps, capacity_records, steps_out, n_records, series_channel(h->extr.host, values, (size_t)EXTREMA_NQ),
                series_channel(h->extr.cells, cells, (size_t)2 * EXTREMA_NQ));
    return GPF_OK;
}

extern "C" int gpf_extrema_now(gpf_handle* h, double values[7], int32_t cells[14]) {
    GPF_TRY(series_now_checks(h, SERIES[S_EXTREMA], values && cells, extrema_refusal));
    GPF_TRY(enter(h, true));
    GPF_TRY(extrema_buffers(h));
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_EXTREMA], s));
    GPF_TRY(extrema_enqueue(h, s.step, h->log_cap));            // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(values, h->extr.a.val + (size_t)h->log_cap * EXTREMA_NQ, EXTREMA_NQ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(cells, h->extr.a.cell + (size_t)h->log_cap * 2 * EXTREMA_NQ, 2 * EXTREMA_NQ * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/extrema_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed extrema are put aside
// for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream (series_time).
extern "C" int gpf_extrema_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_EXTREMA], n, mode, 1, ms, "armed extrema (gpf_extrema_set)", [](const gpf_handle* h, const std::string& who) {
        GPF_TRY(extrema_refusal(h, who));
        if (h->cfg.thinning != GPF_THINNING_NONE || h->el.on || h->gp[1].set || h->gp[2].set)
            return fail(GPF_ERR_STATE, who + ": handles that gpf_step advances only (this one steps stage-wise)");
        return (int)GPF_OK;
    }));
    return series_time_fused(h, SERIES[S_EXTREMA], n, mode, ms);
}
