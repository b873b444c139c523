// Part of api.hip (included there, not compiled on its own): whole-film integrals -- load, its moments, the pressure's push on
// the profiled wall, wall friction and flow rates through cross-sections -- reduced on the device behind the committed steps
// whose count is a multiple of the armed stride, and handed out once per call.  Kernels: integral_kernels.hip.
// A handle that steps through k_small_steps records inside the batch (film_record_block, told where by integ.dev): same buffer,
// same slots, same bits, no launch.

// Records a stepping call leaves for the steps (base, base + ran]: the multiples of `every` among them.
static long long integrals_count(long long base, long long ran, long long every) {
    return ran > 0 ? (base + ran) / every - base / every : 0;
}

static int integrals_nrec(const gpf_handle* h) { return FILM_NSUM + h->integ.nsx + h->integ.nsy; }

// The cases the reduction does not cover, with the error class gpf_probes_set / gpf_gap_profiles give them
static int integrals_refusal(const gpf_handle* h, const std::string& who) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; film integrals are not available on slabs");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set)
        return fail(GPF_ERR_INVALID, who + ": surrogate closures: the film integrals evaluate the analytic pressure and wall stress, which this handle replaces");
    if (h->cfg.thinning != GPF_THINNING_NONE) return fail(GPF_ERR_INVALID, who + ": shear thinning needs grad p (not supported)");
    if (h->el.on || h->els.on) return fail(GPF_ERR_INVALID, who + ": an elastic handle steps stage-wise and deforms its gap between steps (not supported)");
    return GPF_OK;
}

// First and last interior row / column; a direction of extent 1 has the one section
static void integrals_default_sections(gpf_handle* h) {
    h->integ.nsx = h->L.Nx > 1 ? 2 : 1; h->integ.sx[0] = 1; h->integ.sx[1] = h->L.Nx;
    h->integ.nsy = h->L.Ny > 1 ? 2 : 1; h->integ.sy[0] = 1; h->integ.sy[1] = h->L.Ny;
}

// 16-byte pair loads of k_film_partial: every pair (1 + 2k, 2 + 2k) of every row of every plane must start on 16 bytes.
// Layout and hipMalloc give that today, so the 8-byte loads are otherwise out of reach: the environment variable GPF_FILM_NARROW
// (any value; read when the buffers are allocated, i.e. at the first record after gpf_integrals_set / _clear) asks for them,
// which is how tests/test_gpu_integrals.py holds them bit for bit against the wide loads.
static bool film_wide_ok(const gpf_handle* h) {
    const Layout& L = h->L;
    auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    return ((L.off + 1) & 1) == 0 && (L.pitch & 1) == 0 && (L.plane & 1) == 0 && a16(h->q[0]) && a16(h->q[1]) && a16(h->topo) &&
           (!h->Ls || a16(h->Ls)) && !h->integ.narrow;
}

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
    if (!h->integ.every) return GPF_OK;
    GPF_TRY(integrals_refusal(h, "gpf_step with film integrals armed"));
    h->integ.host.clear(); h->integ.steps.clear();
    return integrals_buffers(h);
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int integrals_enqueue(gpf_handle* h, long long expect, long long slot) {
    FilmArgs f;
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.Ls = h->Ls; f.st = h->st;
    f.part = h->integ.part; f.rec = h->integ.rec; f.L = h->L; f.dx = h->cfg.dx; f.dy = h->cfg.dy;
    f.nsx = h->integ.nsx; f.nsy = h->integ.nsy;
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k) { f.sx[k] = k < f.nsx ? h->integ.sx[k] : 1; f.sy[k] = k < f.nsy ? h->integ.sy[k] : 1; }
    f.wide = film_wide_ok(h) ? 1 : 0;
    f.slot = slot; f.cap = h->log_cap;
    EOS_DISPATCH(h->cfg.eos, {
        if (h->Ls) hipLaunchKernelGGL((k_film_partial<EOS_, true>), dim3(h->L.Nx), dim3(256), 0, h->stream, f, h->P, expect);
        else hipLaunchKernelGGL((k_film_partial<EOS_, false>), dim3(h->L.Nx), dim3(256), 0, h->stream, f, h->P, expect);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_film_fold, dim3(1), dim3(256), 0, h->stream, f, expect);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without integrals armed.
static int integrals_launch(gpf_handle* h, long long expect, long long base) {
    const long long every = h->integ.every;
    if (!every || expect % every != 0) return GPF_OK;
    return integrals_enqueue(h, expect, integrals_count(base, expect - base, every) - 1);
}

// After the batch's state has been read (the stream is idle): a batch that stopped on the device ran a prefix of its steps,
// so the records written are those of the multiples of the stride in (base, base + ran]
static int integrals_collect(gpf_handle* h, long long base, long long ran) {
    const long long every = h->integ.every;
    if (!every) return GPF_OK;
    const long long cnt = integrals_count(base, ran, every);
    if (cnt <= 0) return GPF_OK;
    const size_t nrec = (size_t)integrals_nrec(h), at = h->integ.host.size();
    h->integ.host.resize(at + (size_t)cnt * nrec);
    HIP_TRY(hipMemcpy(h->integ.host.data() + at, h->integ.rec, (size_t)cnt * nrec * sizeof(double), hipMemcpyDeviceToHost));
    for (long long k = 1; k <= cnt; ++k) h->integ.steps.push_back((base / every + k) * every);
    return GPF_OK;
}

static int integrals_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    if (h->integ.rec) HIP_TRY(hipFree(h->integ.rec));
    h->integ.rec = nullptr;
    if (h->integ.part) HIP_TRY(hipFree(h->integ.part));
    h->integ.part = nullptr;
    if (h->integ.dev) HIP_TRY(hipFree(h->integ.dev));
    h->integ.dev = nullptr;
    h->integ.every = 0; h->integ.nsx = h->integ.nsy = 0;
    h->integ.host.clear(); h->integ.steps.clear();
    return GPF_OK;
}

extern "C" int gpf_integrals_set(gpf_handle* h, int64_t every, int nsx, const int32_t* ix, int nsy, const int32_t* iy) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    GPF_TRY(integrals_refusal(h, "gpf_integrals_set"));
    if (every < 1) return fail(GPF_ERR_INVALID, "gpf_integrals_set: every >= 1 required (gpf_integrals_clear disarms), got " + std::to_string(every));
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
    GPF_TRY(enter(h, true));
    GPF_TRY(integrals_release(h));
    integrals_default_sections(h);
    if (ix && nsx > 0) { h->integ.nsx = nsx; for (int k = 0; k < nsx; ++k) h->integ.sx[k] = ix[k]; }
    if (iy && nsy > 0) { h->integ.nsy = nsy; for (int k = 0; k < nsy; ++k) h->integ.sy[k] = iy[k]; }
    h->integ.every = every;
    return GPF_OK;
}

extern "C" int gpf_integrals_clear(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (h->step_open) return fail(GPF_ERR_STATE, "gpf_integrals_clear: a stage-wise step is open; close it first");
    GPF_TRY(enter(h, true));
    return integrals_release(h);
}

extern "C" int gpf_integrals_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->integ.every) return fail(GPF_ERR_STATE, "gpf_integrals_read: no integrals are armed (gpf_integrals_set)");
    const size_t nrec = (size_t)integrals_nrec(h);
    const int64_t have = (int64_t)h->integ.steps.size(), take = std::max<int64_t>(0, std::min(have, capacity_records));
    if (n_records) *n_records = have;
    if (out && take > 0) std::memcpy(out, h->integ.host.data(), (size_t)take * nrec * sizeof(double));
    for (int64_t k = 0; steps_out && k < take; ++k) steps_out[k] = h->integ.steps[(size_t)k];
    return GPF_OK;
}

extern "C" int gpf_integrals_in_batch(gpf_handle* h, int* yes) {
    if (!h || !yes) return fail(GPF_ERR_INVALID, "gpf_integrals_in_batch: null argument");
    *yes = h->integ.every && small_grid_eligible(h) ? 1 : 0;
    return GPF_OK;
}

extern "C" int gpf_integrals_now(gpf_handle* h, double* out, int64_t count) {
    if (!h || !out) return fail(GPF_ERR_INVALID, "gpf_integrals_now: null argument");
    if (!h->has_q || !h->has_topo) return fail(GPF_ERR_STATE, "gpf_integrals_now: upload q and topography first");
    GPF_TRY(integrals_refusal(h, "gpf_integrals_now"));
    GPF_TRY(enter(h, true));
    GPF_TRY(integrals_buffers(h));
    const int nrec = integrals_nrec(h);
    if (count < nrec) return fail(GPF_ERR_INVALID, "gpf_integrals_now: room for " + std::to_string(nrec) + " doubles required, " + std::to_string(count) + " given");
    StepState s;
    GPF_TRY(read_state(h, s));
    if (s.invalid) return fail(GPF_ERR_STATE, "gpf_integrals_now: the run state is flagged invalid (the last step was rolled back)");
    GPF_TRY(integrals_enqueue(h, s.step, h->log_cap));          // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(out, h->integ.rec + (size_t)h->log_cap * nrec, (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/integrals_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed integrals are put
// aside for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream.  Probes, weighted
// integrals and statistics are put aside in both modes (armed statistics begin a new window after the call).
extern "C" int gpf_integrals_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    if (!h || !ms) return fail(GPF_ERR_INVALID, "gpf_integrals_time: null argument");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_integrals_time: call gpf_pre_run first");
    GPF_TRY(integrals_refusal(h, "gpf_integrals_time"));
    if (n < 1 || n > h->log_cap || mode < 0 || mode > 1)
        return fail(GPF_ERR_INVALID, "gpf_integrals_time: 1 <= n <= " + std::to_string(h->log_cap) + " and mode in 0..1 required");
    if (mode == 1 && !h->integ.every) return fail(GPF_ERR_STATE, "gpf_integrals_time: mode 1 needs armed integrals (gpf_integrals_set)");
    const bool small = small_grid_eligible(h);
    GPF_TRY(enter(h));
    h->integ.host.clear(); h->integ.steps.clear();
    h->probes.host.clear(); h->probes.first_step = h->host_step + 1;
    const long long keep_every = h->integ.every, keep_weighted = h->weighted.every, keep_stats = h->stats.every, keep_regions = h->regions.every,
                    keep_lines = h->lines.every;
    const int keep_probes = h->probes.n;
    h->probes.n = 0; h->weighted.every = 0; h->stats.every = 0; h->regions.every = 0; h->lines.every = 0;
    if (mode != 1) h->integ.every = 0;
    int rc = integrals_begin(h);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    const long long base = h->host_step;
    float t = 0.f;
    if (rc == GPF_OK && e == hipSuccess) e = hipEventRecord(e0, h->stream);
    if (rc == GPF_OK && e == hipSuccess) {
        if (small) rc = small_batch_cut(h, n, 0, base);
        for (int64_t i = 0; i < n && rc == GPF_OK && !small; ++i) {
            rc = enqueue_step(h, 0, base, nullptr);
            if (rc == GPF_OK) rc = integrals_launch(h, base + i + 1, base);
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
    if (rc == GPF_OK && e == hipSuccess && rs == GPF_OK) rcol = integrals_collect(h, base, s.step - base);
    h->integ.every = keep_every; h->weighted.every = keep_weighted; h->stats.every = keep_stats; h->regions.every = keep_regions; h->lines.every = keep_lines; h->probes.n = keep_probes;
    if (rs == GPF_OK && rcol == GPF_OK) rcol = stats_restart(h, s.step);
    GPF_TRY(rc);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_integrals_time: ") + hipGetErrorString(e));
    GPF_TRY(rs);
    GPF_TRY(rcol);
    *ms = t;
    return GPF_OK;
}
