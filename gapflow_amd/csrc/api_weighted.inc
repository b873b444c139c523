// Part of api.hip (included there, not compiled on its own): weighted film integrals -- the film integrals' pressure, gap, mass,
// flow and wall-friction sums with up to 8 weight planes in front (pads, windows, Fourier modes) -- reduced on the device behind
// the committed steps whose count is a multiple of the armed stride, and handed out once per call.  Kernels: weighted_kernels.hip.

// The cases the reduction does not cover: the film integrals' (integrals_refusal), with their error classes
static int weighted_refusal(const gpf_handle* h, const std::string& who) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; weighted film integrals are not available on slabs");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set)
        return fail(GPF_ERR_INVALID, who + ": surrogate closures: the weighted integrals evaluate the analytic pressure and wall stress, which this handle replaces");
    if (h->cfg.thinning != GPF_THINNING_NONE) return fail(GPF_ERR_INVALID, who + ": shear thinning needs grad p (not supported)");
    if (h->el.on || h->els.on) return fail(GPF_ERR_INVALID, who + ": an elastic handle steps stage-wise and deforms its gap between steps (not supported)");
    return GPF_OK;
}

static size_t weighted_nrec(const gpf_handle* h) { return (size_t)h->weighted.K * WFILM_NQ; }

// 16-byte pair loads of k_wfilm_partial: film_wide_ok's conditions on the planes it reads, the weight planes among them
// (GPF_FILM_NARROW, read by gpf_weighted_set, asks for the 8-byte loads regardless)
static bool weighted_wide_ok(const gpf_handle* h) {
    const Layout& L = h->L;
    auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    return ((L.off + 1) & 1) == 0 && (L.pitch & 1) == 0 && (L.plane & 1) == 0 && a16(h->q[0]) && a16(h->q[1]) && a16(h->topo) &&
           (!h->Ls || a16(h->Ls)) && a16(h->weighted.w) && !h->weighted.narrow;
}

// A stepping call begins: its records replace those of the call before
static int weighted_begin(gpf_handle* h) {
    if (!h->weighted.every) return GPF_OK;
    GPF_TRY(weighted_refusal(h, "gpf_step with weighted integrals armed"));
    h->weighted.host.clear(); h->weighted.steps.clear();
    return GPF_OK;
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int weighted_enqueue(gpf_handle* h, long long expect, long long slot) {
    WFilmArgs f;
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.Ls = h->Ls; f.w = h->weighted.w; f.st = h->st;
    f.part = h->weighted.part; f.rec = h->weighted.rec; f.L = h->L; f.dx = h->cfg.dx; f.dy = h->cfg.dy;
    f.K = h->weighted.K; f.wide = weighted_wide_ok(h) ? 1 : 0;
    f.slot = slot; f.cap = h->log_cap;
    const dim3 grid(h->L.Nx, f.K);
    EOS_DISPATCH(h->cfg.eos, {
        if (h->Ls) hipLaunchKernelGGL((k_wfilm_partial<EOS_, true>), grid, dim3(256), 0, h->stream, f, h->P, expect);
        else hipLaunchKernelGGL((k_wfilm_partial<EOS_, false>), grid, dim3(256), 0, h->stream, f, h->P, expect);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_wfilm_fold, dim3(f.K), dim3(256), 0, h->stream, f, expect);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without weighted integrals armed.
static int weighted_launch(gpf_handle* h, long long expect, long long base) {
    const long long every = h->weighted.every;
    if (!every || expect % every != 0) return GPF_OK;
    return weighted_enqueue(h, expect, integrals_count(base, expect - base, every) - 1);
}

// After the batch's state has been read (the stream is idle): the records written are those of the multiples of the stride in
// (base, base + ran]
static int weighted_collect(gpf_handle* h, long long base, long long ran) {
    const long long every = h->weighted.every;
    if (!every) return GPF_OK;
    const long long cnt = integrals_count(base, ran, every);
    if (cnt <= 0) return GPF_OK;
    const size_t nrec = weighted_nrec(h), at = h->weighted.host.size();
    h->weighted.host.resize(at + (size_t)cnt * nrec);
    HIP_TRY(hipMemcpy(h->weighted.host.data() + at, h->weighted.rec, (size_t)cnt * nrec * sizeof(double), hipMemcpyDeviceToHost));
    for (long long k = 1; k <= cnt; ++k) h->weighted.steps.push_back((base / every + k) * every);
    return GPF_OK;
}

static int weighted_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    for (double** p : {&h->weighted.w, &h->weighted.part, &h->weighted.rec}) {
        if (*p) HIP_TRY(hipFree(*p));
        *p = nullptr;
    }
    h->weighted.every = 0; h->weighted.K = 0;
    h->weighted.host.clear(); h->weighted.steps.clear();
    return GPF_OK;
}

extern "C" int gpf_weighted_set(gpf_handle* h, int64_t every, int K, const double* weights) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    GPF_TRY(weighted_refusal(h, "gpf_weighted_set"));
    if (every < 1) return fail(GPF_ERR_INVALID, "gpf_weighted_set: every >= 1 required (gpf_weighted_clear disarms), got " + std::to_string(every));
    if (K < 1 || K > WFILM_MAX_K)
        return fail(GPF_ERR_INVALID, "gpf_weighted_set: 1 to " + std::to_string(WFILM_MAX_K) + " weight planes required, got " + std::to_string(K));
    if (!weights) return fail(GPF_ERR_INVALID, "gpf_weighted_set: null weights");
    const Layout& L = h->L;
    const int nx = L.Nx + 2, ny = L.Ny + 2;
    const size_t ncell = (size_t)nx * ny;
    for (int k = 0; k < K; ++k)
        for (int ix = 1; ix <= L.Nx; ++ix)
            for (int iy = 1; iy <= L.Ny; ++iy)
                if (!std::isfinite(weights[(size_t)k * ncell + (size_t)ix * ny + iy]))
                    return fail(GPF_ERR_INVALID, "gpf_weighted_set: weight plane " + std::to_string(k) + " is not finite at cell (" +
                                                 std::to_string(ix) + ", " + std::to_string(iy) + ")");
    GPF_TRY(enter(h, true));
    GPF_TRY(weighted_release(h));
    auto undo = [&](int code) { (void)weighted_release(h); return code; };
#define HIP_TRY_W(expr)                                                                                 \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return undo(fail(GPF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)));      \
    } while (0)
    const size_t wbytes = (size_t)K * L.plane * sizeof(double) + PLANE_PAD_BYTES;
    HIP_TRY_W(hipMalloc(&h->weighted.w, wbytes));
    HIP_TRY_W(hipMemsetAsync(h->weighted.w, 0, wbytes, h->stream));
    HIP_TRY_W(hipMalloc(&h->weighted.part, (size_t)K * L.Nx * WFILM_NQ * sizeof(double)));
    HIP_TRY_W(hipMalloc(&h->weighted.rec, (size_t)(h->log_cap + 1) * K * WFILM_NQ * sizeof(double)));
    // gpf_upload's way into Layout planes -- the contiguous staging buffer, then k_pack -- one plane at a time, so that the staging
    // stays at one plane whatever K is.  The plane as it goes to the device: ghost cells zero whatever the caller holds there
    const int rs = ensure_stage(h, ncell);
    if (rs != GPF_OK) return undo(rs);
    std::vector<double> plane(ncell);
    for (int k = 0; k < K; ++k) {
        std::fill(plane.begin(), plane.end(), 0.0);
        for (int ix = 1; ix <= L.Nx; ++ix)
            std::memcpy(&plane[(size_t)ix * ny + 1], &weights[(size_t)k * ncell + (size_t)ix * ny + 1], (size_t)L.Ny * sizeof(double));
        HIP_TRY_W(hipMemcpyAsync(h->stage, plane.data(), ncell * sizeof(double), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_pack, dim3(blocks_for((long long)ncell)), dim3(256), 0, h->stream, (const double*)h->stage,
                           h->weighted.w + (size_t)k * L.plane, L, 1);
        HIP_TRY_W(hipGetLastError());
        HIP_TRY_W(hipStreamSynchronize(h->stream));     // `plane` and the staging buffer are used again for the next one
    }
#undef HIP_TRY_W
    h->weighted.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
    h->weighted.K = K;
    h->weighted.every = every;
    return GPF_OK;
}

extern "C" int gpf_weighted_clear(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (h->step_open) return fail(GPF_ERR_STATE, "gpf_weighted_clear: a stage-wise step is open; close it first");
    GPF_TRY(enter(h, true));
    return weighted_release(h);
}

extern "C" int gpf_weighted_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->weighted.every) return fail(GPF_ERR_STATE, "gpf_weighted_read: no weighted integrals are armed (gpf_weighted_set)");
    const size_t nrec = weighted_nrec(h);
    const int64_t have = (int64_t)h->weighted.steps.size(), take = std::max<int64_t>(0, std::min(have, capacity_records));
    if (n_records) *n_records = have;
    if (out && take > 0) std::memcpy(out, h->weighted.host.data(), (size_t)take * nrec * sizeof(double));
    for (int64_t k = 0; steps_out && k < take; ++k) steps_out[k] = h->weighted.steps[(size_t)k];
    return GPF_OK;
}

extern "C" int gpf_weighted_now(gpf_handle* h, double* out, int64_t count) {
    if (!h || !out) return fail(GPF_ERR_INVALID, "gpf_weighted_now: null argument");
    if (!h->has_q || !h->has_topo) return fail(GPF_ERR_STATE, "gpf_weighted_now: upload q and topography first");
    GPF_TRY(weighted_refusal(h, "gpf_weighted_now"));
    if (!h->weighted.every) return fail(GPF_ERR_STATE, "gpf_weighted_now: no weighted integrals are armed (gpf_weighted_set holds the weights)");
    GPF_TRY(enter(h, true));
    const size_t nrec = weighted_nrec(h);
    if (count < (int64_t)nrec) return fail(GPF_ERR_INVALID, "gpf_weighted_now: room for " + std::to_string(nrec) + " doubles required, " + std::to_string(count) + " given");
    StepState s;
    GPF_TRY(read_state(h, s));
    if (s.invalid) return fail(GPF_ERR_STATE, "gpf_weighted_now: the run state is flagged invalid (the last step was rolled back)");
    GPF_TRY(weighted_enqueue(h, s.step, h->log_cap));           // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(out, h->weighted.rec + (size_t)h->log_cap * nrec, nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/weighted_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed weighted integrals are
// put aside for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream.  Probes, film
// integrals, extrema and statistics are put aside in both modes (armed statistics begin a new window after the call).
extern "C" int gpf_weighted_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    if (!h || !ms) return fail(GPF_ERR_INVALID, "gpf_weighted_time: null argument");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_weighted_time: call gpf_pre_run first");
    GPF_TRY(weighted_refusal(h, "gpf_weighted_time"));
    if (n < 1 || n > h->log_cap || mode < 0 || mode > 1)
        return fail(GPF_ERR_INVALID, "gpf_weighted_time: 1 <= n <= " + std::to_string(h->log_cap) + " and mode in 0..1 required");
    if (mode == 1 && !h->weighted.every) return fail(GPF_ERR_STATE, "gpf_weighted_time: mode 1 needs armed weighted integrals (gpf_weighted_set)");
    const bool small = small_grid_eligible(h);
    GPF_TRY(enter(h));
    h->integ.host.clear(); h->integ.steps.clear();
    h->extr.host.clear(); h->extr.cells.clear(); h->extr.steps.clear();
    h->probes.host.clear(); h->probes.first_step = h->host_step + 1;
    const long long keep_every = h->weighted.every, keep_integ = h->integ.every, keep_extr = h->extr.every, keep_stats = h->stats.every, keep_regions = h->regions.every,
                    keep_lines = h->lines.every;
    const int keep_probes = h->probes.n;
    h->probes.n = 0; h->integ.every = 0; h->extr.every = 0; h->stats.every = 0; h->regions.every = 0; h->lines.every = 0;
    if (mode != 1) h->weighted.every = 0;
    int rc = weighted_begin(h);
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
            if (rc == GPF_OK) rc = weighted_launch(h, base + i + 1, base);
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
    if (rc == GPF_OK && e == hipSuccess && rs == GPF_OK) rcol = weighted_collect(h, base, s.step - base);
    h->weighted.every = keep_every; h->integ.every = keep_integ; h->extr.every = keep_extr; h->stats.every = keep_stats; h->regions.every = keep_regions; h->lines.every = keep_lines; h->probes.n = keep_probes;
    if (rs == GPF_OK && rcol == GPF_OK) rcol = stats_restart(h, s.step);
    GPF_TRY(rc);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_weighted_time: ") + hipGetErrorString(e));
    GPF_TRY(rs);
    GPF_TRY(rcol);
    *ms = t;
    return GPF_OK;
}
