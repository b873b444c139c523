// Part of api.hip (included there, not compiled on its own): weighted film integrals -- the film integrals' pressure, gap, mass,
// flow and wall-friction sums with up to 8 weight planes in front (pads, windows, Fourier modes) -- reduced on the device behind
// the committed steps whose count is a multiple of the armed stride, and handed out once per call.  Kernels: weighted_kernels.hip.

// The cases the reduction does not cover: the film integrals' (series_refusal), with their error classes
static int weighted_refusal(const gpf_handle* h, const std::string& who) { return series_refusal(h, who, "weighted film integrals", "the weighted integrals"); }

static size_t weighted_nrec(const gpf_handle* h) { return (size_t)h->weighted.K * WFILM_NQ; }

// 16-byte pair loads of k_wfilm_partial: series_wide_ok's conditions on the planes it reads, the weight planes among them
// (GPF_FILM_NARROW, read by gpf_weighted_set, asks for the 8-byte loads regardless)
static bool weighted_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->weighted.narrow, true, h->weighted.w); }

// A stepping call begins: its records replace those of the call before
static int weighted_begin(gpf_handle* h) {
    if (!h->weighted.armed()) return GPF_OK;
    GPF_TRY(weighted_refusal(h, "gpf_step with weighted integrals armed"));
    h->weighted.forget();
    return GPF_OK;
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int weighted_enqueue(gpf_handle* h, long long expect, long long slot) {
    WFilmArgs f;
    series_row_args(h, weighted_wide_ok(h), slot, f);
    f.w = h->weighted.w; f.part = h->weighted.part; f.rec = h->weighted.rec; f.K = h->weighted.K;
    const dim3 grid(h->L.Nx, f.K);
    SERIES_ROWS_ENQUEUE(h, k_wfilm_partial, k_wfilm_fold, grid, f, expect);
    return GPF_OK;
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without weighted integrals armed.
static int weighted_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->weighted.every, expect)) return GPF_OK;
    return weighted_enqueue(h, expect, series_slot(base, expect, h->weighted.every));
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host
static int weighted_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->weighted.every, h->weighted.steps, base, ran, series_channel(h->weighted.host, h->weighted.rec, weighted_nrec(h)));
}

static SeriesBuffers weighted_owned(gpf_handle* h) { return {(void**)&h->weighted.w, (void**)&h->weighted.part, (void**)&h->weighted.rec}; }

static int weighted_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(weighted_owned(h)));
    h->weighted.disarm(); h->weighted.K = 0;
    return GPF_OK;
}

extern "C" int gpf_weighted_set(gpf_handle* h, int64_t every, int K, const double* weights) {
    GPF_TRY(series_set_checks(h, SERIES[S_WEIGHTED], every, weighted_refusal));
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
    GPF_TRY(series_disarm(h, SERIES[S_WEIGHTED]));
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

extern "C" int gpf_weighted_clear(gpf_handle* h) { return series_clear(h, SERIES[S_WEIGHTED]); }

extern "C" int gpf_weighted_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->weighted.armed()) return fail(GPF_ERR_STATE, "gpf_weighted_read: no weighted integrals are armed (gpf_weighted_set)");
    series_read(h->weighted.steps, capacity_records, steps_out, n_records, series_channel(h->weighted.host, out, weighted_nrec(h)));
    return GPF_OK;
}

extern "C" int gpf_weighted_now(gpf_handle* h, double* out, int64_t count) {
    GPF_TRY(series_now_checks(h, SERIES[S_WEIGHTED], out != nullptr, weighted_refusal));
    if (!h->weighted.armed()) return fail(GPF_ERR_STATE, "gpf_weighted_now: no weighted integrals are armed (gpf_weighted_set holds the weights)");
    GPF_TRY(enter(h, true));
    const size_t nrec = weighted_nrec(h);
    if (count < (int64_t)nrec) return fail(GPF_ERR_INVALID, "gpf_weighted_now: room for " + std::to_string(nrec) + " doubles required, " + std::to_string(count) + " given");
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_WEIGHTED], s));
    GPF_TRY(weighted_enqueue(h, s.step, h->log_cap));           // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(out, h->weighted.rec + (size_t)h->log_cap * nrec, nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/weighted_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed weighted integrals are
// put aside for the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream (series_time).
extern "C" int gpf_weighted_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_WEIGHTED], n, mode, 1, ms, "armed weighted integrals (gpf_weighted_set)", weighted_refusal));
    return series_time_fused(h, SERIES[S_WEIGHTED], n, mode, ms);
}
