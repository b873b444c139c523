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

// 16-byte pair loads of k_extrema_partial: film_wide_ok's conditions on the planes it reads (GPF_FILM_NARROW, read when the
// buffers are allocated, asks for the 8-byte loads regardless)
static bool extrema_wide_ok(const gpf_handle* h) {
    const Layout& L = h->L;
    auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    return ((L.off + 1) & 1) == 0 && (L.pitch & 1) == 0 && (L.plane & 1) == 0 && a16(h->q[0]) && a16(h->q[1]) && a16(h->topo) && !h->extr.narrow;
}

// The record buffers (log_cap slots for a batch + one for gpf_extrema_now), the row scratch and the arguments' copy in device
// memory, on first use.  `dev` is set last, once everything it describes is in place.
static int extrema_buffers(gpf_handle* h) {
    ExtremaArgs& a = h->extr.a;
    const size_t slots = (size_t)h->log_cap + 1, nx = (size_t)h->L.Nx;
    if (!a.val) {
        h->extr.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
        DBG("extrema_buffers: k_extrema_partial takes %s pair loads", extrema_wide_ok(h) ? "16-byte" : "8-byte");      // (GPF_DEBUG: the narrow-load test reads this)
        HIP_TRY(hipMalloc(&a.val, slots * EXTREMA_NQ * sizeof(double)));
    }
    if (!a.cell) HIP_TRY(hipMalloc(&a.cell, slots * 2 * EXTREMA_NQ * sizeof(int)));
    if (!a.row_val) HIP_TRY(hipMalloc(&a.row_val, nx * EXTREMA_NQ * sizeof(double)));
    if (!a.row_iy) HIP_TRY(hipMalloc(&a.row_iy, nx * EXTREMA_NQ * sizeof(int)));
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
    if (!h->extr.every) return GPF_OK;
    GPF_TRY(extrema_refusal(h, "a stepping call with extrema armed"));
    h->extr.host.clear(); h->extr.cells.clear(); h->extr.steps.clear();
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
    const long long every = h->extr.every;
    if (!every || expect % every != 0) return GPF_OK;
    return extrema_enqueue(h, expect, integrals_count(base, expect - base, every) - 1);
}

// After the batch's state has been read (the stream is idle): a batch that stopped on the device ran a prefix of its steps,
// so the records written are those of the multiples of the stride in (base, base + ran]
static int extrema_collect(gpf_handle* h, long long base, long long ran) {
    const long long every = h->extr.every;
    if (!every) return GPF_OK;
    const long long cnt = integrals_count(base, ran, every);
    if (cnt <= 0) return GPF_OK;
    const size_t at = h->extr.steps.size();
    h->extr.host.resize((at + (size_t)cnt) * EXTREMA_NQ);
    h->extr.cells.resize((at + (size_t)cnt) * 2 * EXTREMA_NQ);
    HIP_TRY(hipMemcpy(h->extr.host.data() + at * EXTREMA_NQ, h->extr.a.val, (size_t)cnt * EXTREMA_NQ * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->extr.cells.data() + at * 2 * EXTREMA_NQ, h->extr.a.cell, (size_t)cnt * 2 * EXTREMA_NQ * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (long long k = 1; k <= cnt; ++k) h->extr.steps.push_back((base / every + k) * every);
    return GPF_OK;
}

// gpf_close_step: the closed step's record, if it commits.  An elastic handle's gap deforms after the step closes
// (gpf_elastic_update); its record waits for that call, so that it holds the gap the handle holds with that state.
static int extrema_close_step_launch(gpf_handle* h) {
    GPF_TRY(extrema_begin(h));
    if (!h->extr.every) return GPF_OK;
    if (h->el.on) { h->extr.pending = true; h->extr.pending_base = h->host_step; return GPF_OK; }
    return extrema_launch(h, h->host_step + 1, h->host_step);
}

static int extrema_close_step_collect(gpf_handle* h, long long ran) {
    if (h->extr.pending) { if (ran < 1) h->extr.pending = false; return GPF_OK; }
    return extrema_collect(h, h->host_step, ran);
}

// gpf_elastic_update, behind its launches: the record of the step gpf_close_step committed just before
static int extrema_after_elastic_update(gpf_handle* h) {
    if (!h->extr.pending) return GPF_OK;
    h->extr.pending = false;
    const long long base = h->extr.pending_base;
    if (!h->extr.every || h->host_step != base + 1) return GPF_OK;
    GPF_TRY(extrema_launch(h, h->host_step, base));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return extrema_collect(h, base, 1);
}

static int extrema_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    ExtremaArgs& a = h->extr.a;
    if (a.val) HIP_TRY(hipFree(a.val));
    a.val = nullptr;
    if (a.cell) HIP_TRY(hipFree(a.cell));
    a.cell = nullptr;
    if (a.row_val) HIP_TRY(hipFree(a.row_val));
    a.row_val = nullptr;
    if (a.row_iy) HIP_TRY(hipFree(a.row_iy));
    a.row_iy = nullptr;
    if (h->extr.dev) HIP_TRY(hipFree(h->extr.dev));
    h->extr.dev = nullptr;
    a.every = 0; a.cap = 0;
    h->extr.every = 0; h->extr.pending = false;
    h->extr.host.clear(); h->extr.cells.clear(); h->extr.steps.clear();
    return GPF_OK;
}

extern "C" int gpf_extrema_set(gpf_handle* h, int64_t every) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    GPF_TRY(extrema_refusal(h, "gpf_extrema_set"));
    if (every < 1) return fail(GPF_ERR_INVALID, "gpf_extrema_set: every >= 1 required (gpf_extrema_clear disarms), got " + std::to_string(every));
    GPF_TRY(enter(h, true));
    GPF_TRY(extrema_release(h));
    h->extr.every = every;
    return GPF_OK;
}

extern "C" int gpf_extrema_clear(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (h->step_open) return fail(GPF_ERR_STATE, "gpf_extrema_clear: a stage-wise step is open; close it first");
    GPF_TRY(enter(h, true));
    return extrema_release(h);
}

extern "C" int gpf_extrema_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->extr.every) return fail(GPF_ERR_STATE, "gpf_extrema_read: no extrema are armed (gpf_extrema_set)");
    const int64_t have = (int64_t)h->extr.steps.size(), take = std::max<int64_t>(0, std::min(have, capacity_records));
    if (n_records) *n_records = have;
    if (values && take > 0) std::memcpy(values, h->extr.host.data(), (size_t)take * EXTREMA_NQ * sizeof(double));
    if (cells && take > 0) std::memcpy(cells, h->extr.cells.data(), (size_t)take * 2 * EXTREMA_NQ * sizeof(int32_t));
    for (int64_t k = 0; steps_out && k < take; ++k) steps_out[k] = h->extr.steps[(size_t)k];
    return GPF_OK;
}

extern "C" int gpf_extrema_now(gpf_handle* h, double values[7], int32_t cells[14]) {
    if (!h || !values || !cells) return fail(GPF_ERR_INVALID, "gpf_extrema_now: null argument");
    if (!h->has_q || !h->has_topo) return fail(GPF_ERR_STATE, "gpf_extrema_now: upload q and topography first");
    GPF_TRY(extrema_refusal(h, "gpf_extrema_now"));
    GPF_TRY(enter(h, true));
    GPF_TRY(extrema_buffers(h));
    StepState s;
    GPF_TRY(read_state(h, s));
    if (s.invalid) return fail(GPF_ERR_STATE, "gpf_extrema_now: the run state is flagged invalid (the last step was rolled back)");
    GPF_TRY(extrema_enqueue(h, s.step, h->log_cap));            // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(values, h->extr.a.val + (size_t)h->log_cap * EXTREMA_NQ, EXTREMA_NQ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(cells, h->extr.a.cell + (size_t)h->log_cap * 2 * EXTREMA_NQ, 2 * EXTREMA_NQ * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/extrema_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed extrema are put aside
// for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream.  Probes and film
// integrals are put aside in both modes; armed statistics begin a new window after the call.
extern "C" int gpf_extrema_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    if (!h || !ms) return fail(GPF_ERR_INVALID, "gpf_extrema_time: null argument");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_extrema_time: call gpf_pre_run first");
    GPF_TRY(extrema_refusal(h, "gpf_extrema_time"));
    if (h->cfg.thinning != GPF_THINNING_NONE || h->el.on || h->gp[1].set || h->gp[2].set)
        return fail(GPF_ERR_STATE, "gpf_extrema_time: handles that gpf_step advances only (this one steps stage-wise)");
    if (n < 1 || n > h->log_cap || mode < 0 || mode > 1)
        return fail(GPF_ERR_INVALID, "gpf_extrema_time: 1 <= n <= " + std::to_string(h->log_cap) + " and mode in 0..1 required");
    if (mode == 1 && !h->extr.every) return fail(GPF_ERR_STATE, "gpf_extrema_time: mode 1 needs armed extrema (gpf_extrema_set)");
    const bool small = small_grid_eligible(h);
    GPF_TRY(enter(h));
    h->integ.host.clear(); h->integ.steps.clear();
    h->probes.host.clear(); h->probes.first_step = h->host_step + 1;
    const long long keep_every = h->extr.every, keep_integ = h->integ.every;
    const int keep_probes = h->probes.n;
    h->probes.n = 0; h->integ.every = 0;
    int rc = extrema_begin(h);          // (buffers and the device copy of the arguments while the stride is still the armed one)
    if (mode != 1) { h->extr.every = 0; h->extr.host.clear(); h->extr.cells.clear(); h->extr.steps.clear(); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    const long long base = h->host_step;
    float t = 0.f;
    if (rc == GPF_OK && e == hipSuccess) e = hipEventRecord(e0, h->stream);
    if (rc == GPF_OK && e == hipSuccess) {
        if (small) rc = enqueue_small_steps(h, (int)n, 0, base);
        for (int64_t i = 0; i < n && rc == GPF_OK && !small; ++i) {
            rc = enqueue_step(h, 0, base, nullptr);
            if (rc == GPF_OK) rc = extrema_launch(h, base + i + 1, base);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(e1, h->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    // steps may have been queued whatever went wrong after them: the host's counters follow the device's
    StepState s;
    const int rs = read_state(h, s);
    if (rs == GPF_OK) {
        h->prev_state_valid = s.step > base && !s.invalid;
        h->host_step = s.step; h->next_step = s.step;
    }
    int rcol = GPF_OK;
    if (rc == GPF_OK && e == hipSuccess && rs == GPF_OK) rcol = extrema_collect(h, base, s.step - base);
    h->extr.every = keep_every; h->integ.every = keep_integ; h->probes.n = keep_probes;
    if (rs == GPF_OK && rcol == GPF_OK) rcol = stats_restart(h, s.step);
    GPF_TRY(rc);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_extrema_time: ") + hipGetErrorString(e));
    GPF_TRY(rs);
    GPF_TRY(rcol);
    *ms = t;
    return GPF_OK;
}
