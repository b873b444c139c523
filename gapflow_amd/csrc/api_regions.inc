// Part of api.hip (included there, not compiled on its own): region series -- the weighted film integrals' nine sums over zones
// the state itself defines (a field inside [lo, hi), inside a box), with the zone's exact cell count and bounding box -- reduced on
// the device behind the committed steps whose count is a multiple of the armed stride, and handed out once per call.
// Kernels: region_kernels.hip; the predicate: regions.hpp.

// The cases the reduction does not cover: the weighted integrals' (series_refusal), with their error classes
static int regions_refusal(const gpf_handle* h, const std::string& who) { return series_refusal(h, who, "regions", "the regions"); }

static size_t regions_nsum(const gpf_handle* h) { return (size_t)h->regions.K * WFILM_NQ; }
static size_t regions_nint(const gpf_handle* h) { return (size_t)h->regions.K * REGION_NI; }

// 16-byte pair loads of k_region_partial: series_wide_ok's conditions on the planes it reads (GPF_FILM_NARROW, read by
// gpf_regions_set, asks for the 8-byte loads regardless)
static bool regions_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->regions.narrow, true); }

// A stepping call begins: its records replace those of the call before
static int regions_begin(gpf_handle* h) {
    if (!h->regions.armed()) return GPF_OK;
    GPF_TRY(regions_refusal(h, "gpf_step with regions armed"));
    h->regions.forget();
    return GPF_OK;
}

// The two launches on the handle's stream: the record of the committed state into `slot` if the step count is `expect`
static int regions_enqueue(gpf_handle* h, long long expect, long long slot) {
    RegionArgs f;
    series_row_args(h, regions_wide_ok(h), slot, f);
    f.regions = h->regions.defs; f.part = h->regions.part; f.ipart = h->regions.ipart; f.rec = h->regions.rec; f.irec = h->regions.irec;
    f.K = h->regions.K;
    const dim3 grid(h->L.Nx, f.K);
    SERIES_ROWS_ENQUEUE(h, k_region_partial, k_region_fold, grid, f, expect);
    return GPF_OK;
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without regions armed.
static int regions_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->regions.every, expect)) return GPF_OK;
    return regions_enqueue(h, expect, series_slot(base, expect, h->regions.every));
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host
static int regions_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->regions.every, h->regions.steps, base, ran, series_channel(h->regions.host, h->regions.rec, regions_nsum(h)),
                          series_channel(h->regions.ints, h->regions.irec, regions_nint(h)));
}

static SeriesBuffers regions_owned(gpf_handle* h) {
    return {(void**)&h->regions.defs, (void**)&h->regions.part, (void**)&h->regions.ipart, (void**)&h->regions.rec, (void**)&h->regions.irec};
}

static int regions_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(regions_owned(h)));
    h->regions.disarm(); h->regions.K = 0;
    return GPF_OK;
}

extern "C" int gpf_regions_set(gpf_handle* h, int64_t every, int K, const gpf_region* regions) {
    static const char* const field_names = "0 (p), 1 (rho), 2 (h), 3 (jx), 4 (jy)";
    GPF_TRY(series_set_checks(h, SERIES[S_REGIONS], every, regions_refusal));
    if (K < 1 || K > REGION_MAX_K)
        return fail(GPF_ERR_INVALID, "gpf_regions_set: 1 to " + std::to_string(REGION_MAX_K) + " regions required, got " + std::to_string(K));
    if (!regions) return fail(GPF_ERR_INVALID, "gpf_regions_set: null regions");
    const Layout& L = h->L;
    Region defs[REGION_MAX_K];
    for (int k = 0; k < K; ++k) {
        const gpf_region& g = regions[k];
        Region& r = defs[k];
        r.lo = g.lo; r.hi = g.hi; r.field = g.field; r.pad_ = 0;
        const bool whole = !g.box[0] && !g.box[1] && !g.box[2] && !g.box[3];       // all zeros: the whole interior
        r.ix0 = whole ? 1 : g.box[0]; r.ix1 = whole ? L.Nx : g.box[1]; r.iy0 = whole ? 1 : g.box[2]; r.iy1 = whole ? L.Ny : g.box[3];
        const std::string who = "gpf_regions_set: region " + std::to_string(k);
        switch (region_check(r.field, r.lo, r.hi, r.ix0, r.ix1, r.iy0, r.iy1, L.Nx, L.Ny)) {
            case 0: break;
            case 1: return fail(GPF_ERR_INVALID, who + ": unknown field " + std::to_string(g.field) + "; one of " + field_names + " required");
            case 2: return fail(GPF_ERR_INVALID, who + ": lo < hi required, neither a NaN (lo inclusive, hi exclusive; -inf / +inf leave a side open), got lo = " +
                                                 std::to_string(g.lo) + ", hi = " + std::to_string(g.hi));
            default: return fail(GPF_ERR_INVALID, who + ": box (" + std::to_string(g.box[0]) + ", " + std::to_string(g.box[1]) + ", " + std::to_string(g.box[2]) + ", " +
                                                  std::to_string(g.box[3]) + ") must be ix0 <= ix1 within 1.." + std::to_string(L.Nx) + " and iy0 <= iy1 within 1.." +
                                                  std::to_string(L.Ny) + " (inclusive interior indices; all zeros: the whole interior)");
        }
    }
    GPF_TRY(series_disarm(h, SERIES[S_REGIONS]));
    auto undo = [&](int code) { (void)regions_release(h); return code; };
#define HIP_TRY_R(expr)                                                                                 \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return undo(fail(GPF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)));      \
    } while (0)
    const size_t slots = (size_t)(h->log_cap + 1) * K;
    HIP_TRY_R(hipMalloc(&h->regions.defs, (size_t)K * sizeof(Region)));
    HIP_TRY_R(hipMalloc(&h->regions.part, (size_t)K * L.Nx * WFILM_NQ * sizeof(double)));
    HIP_TRY_R(hipMalloc(&h->regions.ipart, (size_t)K * L.Nx * REGION_NROW * sizeof(int)));
    HIP_TRY_R(hipMalloc(&h->regions.rec, slots * WFILM_NQ * sizeof(double)));
    HIP_TRY_R(hipMalloc(&h->regions.irec, slots * REGION_NI * sizeof(long long)));
    HIP_TRY_R(hipMemcpyAsync(h->regions.defs, defs, (size_t)K * sizeof(Region), hipMemcpyHostToDevice, h->stream));
    HIP_TRY_R(hipStreamSynchronize(h->stream));         // `defs` is on this call's stack
#undef HIP_TRY_R
    h->regions.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
    h->regions.K = K;
    h->regions.every = every;
    return GPF_OK;
}

extern "C" int gpf_regions_clear(gpf_handle* h) { return series_clear(h, SERIES[S_REGIONS]); }

extern "C" int gpf_regions_read(gpf_handle* h, double* sums, int64_t* ints, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->regions.armed()) return fail(GPF_ERR_STATE, "gpf_regions_read: no regions are armed (gpf_regions_set)");
    series_read(h->regions.steps, capacity_records, steps_out, n_records, series_channel(h->regions.host, sums, regions_nsum(h)),
                series_channel(h->regions.ints, (long long*)ints, regions_nint(h)));
    return GPF_OK;
}

extern "C" int gpf_regions_now(gpf_handle* h, double* sums, int64_t* ints, int64_t count) {
    GPF_TRY(series_now_checks(h, SERIES[S_REGIONS], sums && ints, regions_refusal));
    if (!h->regions.armed()) return fail(GPF_ERR_STATE, "gpf_regions_now: no regions are armed (gpf_regions_set holds the region list)");
    GPF_TRY(enter(h, true));
    if (count < h->regions.K) return fail(GPF_ERR_INVALID, "gpf_regions_now: room for " + std::to_string(h->regions.K) + " regions required, " + std::to_string(count) + " given");
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_REGIONS], s));
    const size_t ns = regions_nsum(h), ni = regions_nint(h);
    GPF_TRY(regions_enqueue(h, s.step, h->log_cap));            // the slot behind a batch's
    HIP_TRY(hipMemcpyAsync(sums, h->regions.rec + (size_t)h->log_cap * ns, ns * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(ints, h->regions.irec + (size_t)h->log_cap * ni, ni * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/regions_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed regions are put aside for
// the call), 1 recording at the armed stride; *ms = first launch to last on the handle's stream (series_time).
extern "C" int gpf_regions_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_REGIONS], n, mode, 1, ms, "armed regions (gpf_regions_set)", regions_refusal));
    return series_time_fused(h, SERIES[S_REGIONS], n, mode, ms);
}
