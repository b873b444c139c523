// Part of api.hip (included there, not compiled on its own): running field statistics -- per cell of the ghosted grid the mean,
// the sum of squared deviations, the smallest and the largest p, rho, jx, jy over the recorded steps -- folded into accumulator
// planes on the device behind the committed steps whose count is a multiple of the armed stride and greater than `after`, and
// read on request.  Kernel: stats_kernels.hip.

// The cases the statistics do not cover, with the error classes gpf_extrema_set gives them
static int stats_refusal(const gpf_handle* h, const std::string& who, int mask) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; statistics are not available on slabs");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if ((mask & 1) && h->gp[0].set)
        return fail(GPF_ERR_INVALID, who + ": no EOS pressure to take the statistics of, this handle's pressure comes from a surrogate (rho, jx, jy are available)");
    return GPF_OK;
}

// Records count from here: the step count at arming (or at the last restart of the window) or `after`, whichever is later
static long long stats_floor(const gpf_handle* h) { return std::max(h->stats.arm_step, h->stats.after); }

// Rank (1, 2, ...) of the record of the step that takes the count to `expect`, a multiple of `every` above `floor`
static long long stats_rank(long long expect, long long every, long long floor) { return expect / every - floor / every; }

// Records the window holds once the step count stands at `step`
static long long stats_count(const gpf_handle* h, long long step) {
    return std::max<long long>(0, stats_rank(step, h->stats.every, stats_floor(h)));
}

static int stats_nfields(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1); }

// 16-byte pair accesses of k_stats_update: series_wide_ok's conditions on the planes it reads and the accumulator planes
// (GPF_FILM_NARROW, read by gpf_stats_set, asks for the 8-byte accesses regardless)
static bool stats_wide_ok(const gpf_handle* h) { return series_wide_ok(h, h->stats.narrow, false, h->stats.acc); }

// A stepping call begins
static int stats_begin(gpf_handle* h) {
    if (!h->stats.every) return GPF_OK;
    return stats_refusal(h, "a stepping call with statistics armed", h->stats.mask);
}

static StatsArgs stats_args(gpf_handle* h) {
    StatsArgs a;
    a.qa = h->q[0]; a.qb = h->q[1]; a.st = h->st; a.acc = h->stats.acc; a.rec = h->stats.rec; a.L = h->L;
    a.mask = h->stats.mask; a.wide = stats_wide_ok(h) ? 1 : 0;
    return a;
}

// Eight workgroups per CU at most; the threads of the grid take the items in turn
static int stats_grid(const gpf_handle* h) { return blocks_for((long long)(h->L.Nx + 2) * (h->L.Ny + 2) / 2 + 1, 256, 2048); }

// The launch on the handle's stream: record number n from the committed state if the step count is `expect`
static int stats_enqueue(gpf_handle* h, long long expect, long long n) {
    const StatsArgs a = stats_args(h);
    EOS_DISPATCH(h->cfg.eos, {
        hipLaunchKernelGGL((k_stats_update<EOS_>), dim3(stats_grid(h)), dim3(256), 0, h->stream, a, h->P, expect, n);
    });
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// Behind the launches of one step: record it if it takes the count to a multiple of the stride above the floor.  No launch
// otherwise, and none without statistics armed.
static int stats_launch(gpf_handle* h, long long expect, long long) {
    const long long every = h->stats.every;
    if (!every || expect % every != 0 || expect <= stats_floor(h)) return GPF_OK;
    return stats_enqueue(h, expect, stats_rank(expect, every, stats_floor(h)));
}

// After the state has been read (the stream is idle; the step count stands at `step` = base + ran): the device's record of the
// window, held against the host's own count -- the records applied are a prefix, so the two can differ only if a launch was lost
static int stats_collect(gpf_handle* h, long long base, long long ran) {
    if (!h->stats.every) return GPF_OK;
    const long long step = base + ran;
    HIP_TRY(hipMemcpy(&h->stats.host, h->stats.rec, sizeof(StatsRecord), hipMemcpyDeviceToHost));
    const long long want = stats_count(h, step);
    if (h->stats.host.count != want)
        return fail(GPF_ERR_STATE, "statistics: the device holds " + std::to_string(h->stats.host.count) + " records, " + std::to_string(want) +
                                   " expected at step " + std::to_string(step) + " (stride " + std::to_string(h->stats.every) + ", counted from step " +
                                   std::to_string(stats_floor(h)) + ")");
    return GPF_OK;
}

// The step count starts over or the state was replaced (gpf_pre_run, gpf_resample, gpf_checkpoint_load): a new window begins at
// `step`; stride, `after` and the fields stay
static int stats_restart(gpf_handle* h, long long step) {
    if (!h->stats.every) return GPF_OK;
    HIP_TRY(hipMemsetAsync(h->stats.rec, 0, sizeof(StatsRecord), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->stats.host = StatsRecord{};
    h->stats.arm_step = step;
    return GPF_OK;
}

// Where the statistics cut a one-workgroup batch: at the next step after `at` they record, which lies above their floor
static long long stats_next_record(gpf_handle* h, const Series&, long long at) {
    const long long every = h->stats.every;
    return every ? (std::max(at, stats_floor(h)) / every + 1) * every : LLONG_MAX;
}

static SeriesBuffers stats_owned(gpf_handle* h) { return {(void**)&h->stats.acc, (void**)&h->stats.rec}; }

static int stats_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(stats_owned(h)));
    h->stats.every = 0; h->stats.after = 0; h->stats.mask = 0; h->stats.arm_step = 0;
    h->stats.host = StatsRecord{};
    return GPF_OK;
}

extern "C" int gpf_stats_set(gpf_handle* h, int64_t every, int64_t after, int field_mask) {
    GPF_TRY(series_set_checks(h, SERIES[S_STATS], every, [&](const gpf_handle* h, const std::string& who) { return stats_refusal(h, who, field_mask); }));
    if (after < 0) return fail(GPF_ERR_INVALID, "gpf_stats_set: after >= 0 required, got " + std::to_string(after));
    if (field_mask < 1 || field_mask >= (1 << STATS_NF))
        return fail(GPF_ERR_INVALID, "gpf_stats_set: the field mask must hold at least one of the bits 1 (p), 2 (rho), 4 (jx), 8 (jy) and no other, got " +
                                     std::to_string(field_mask));
    GPF_TRY(series_disarm(h, SERIES[S_STATS]));
    auto undo = [&](int code) { (void)stats_release(h); return code; };
    hipError_t e = hipMalloc(&h->stats.acc, (size_t)stats_nfields(field_mask) * STATS_NQ * h->L.plane * sizeof(double) + PLANE_PAD_BYTES);
    if (e == hipSuccess) e = hipMalloc(&h->stats.rec, sizeof(StatsRecord));
    if (e == hipSuccess) e = hipMemsetAsync(h->stats.rec, 0, sizeof(StatsRecord), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return undo(fail(GPF_ERR_HIP, std::string("gpf_stats_set: ") + hipGetErrorString(e)));
    h->stats.narrow = std::getenv("GPF_FILM_NARROW") != nullptr;
    DBG("gpf_stats_set: k_stats_update takes %s pair accesses", stats_wide_ok(h) ? "16-byte" : "8-byte");
    h->stats.every = every; h->stats.after = after; h->stats.mask = field_mask;
    h->stats.arm_step = h->host_step;
    return GPF_OK;
}

extern "C" int gpf_stats_clear(gpf_handle* h) { return series_clear(h, SERIES[S_STATS]); }

extern "C" int gpf_stats_info(gpf_handle* h, int64_t* count, int64_t* first_step, int64_t* last_step, double* t_first, double* t_last) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->stats.every) return fail(GPF_ERR_STATE, "gpf_stats_info: no statistics are armed (gpf_stats_set)");
    const StatsRecord& r = h->stats.host;
    if (count) *count = r.count;
    if (first_step) *first_step = r.first_step;
    if (last_step) *last_step = r.last_step;
    if (t_first) *t_first = r.t_first;
    if (t_last) *t_last = r.t_last;
    return GPF_OK;
}

extern "C" int gpf_stats_read(gpf_handle* h, int field, int quantity, double* out, size_t n_doubles) {
    if (!h || !out) return fail(GPF_ERR_INVALID, "gpf_stats_read: null argument");
    if (!h->stats.every) return fail(GPF_ERR_STATE, "gpf_stats_read: no statistics are armed (gpf_stats_set)");
    if (field < 0 || field >= STATS_NF || !((h->stats.mask >> field) & 1))
        return fail(GPF_ERR_INVALID, "gpf_stats_read: field " + std::to_string(field) + " (0 p, 1 rho, 2 jx, 3 jy) is not among the armed ones (mask " +
                                     std::to_string(h->stats.mask) + ")");
    if (quantity < 0 || quantity >= STATS_NQ) return fail(GPF_ERR_INVALID, "gpf_stats_read: quantity must be 0 (mean), 1 (m2), 2 (min) or 3 (max)");
    const Layout& L = h->L;
    const size_t ncell = (size_t)(L.Nx + 2) * (L.Ny + 2);
    if (n_doubles != ncell) return fail(GPF_ERR_INVALID, "gpf_stats_read: n_doubles does not match (Nx+2)*(Ny+2)");
    if (h->stats.host.count == 0) return fail(GPF_ERR_STATE, "gpf_stats_read: nothing has been recorded yet in this window");
    GPF_TRY(enter(h, true));
    const int slot = stats_nfields(h->stats.mask & ((1 << field) - 1));
    const double* src = h->stats.acc + ((size_t)slot * STATS_NQ + quantity) * L.plane;
    GPF_TRY(ensure_stage(h, ncell));
    hipLaunchKernelGGL(k_unpack, dim3(blocks_for((long long)ncell)), dim3(256), 0, h->stream, src, h->stage, L, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->stage, ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPF_OK;
}

// Diagnostic (tools/stats_time.py): with `mode` 0 and 1, n steps as gpf_step enqueues them -- 0 nothing recorded (armed
// statistics are put aside for the call), 1 recording at the armed stride and `after`; with `mode` 2, n launches of
// k_stats_stream, the elementwise kernel that moves a record's bytes over the same planes, and no step (the window restarts:
// its accumulators have been written over).  *ms = first launch to last on the handle's stream (series_time).
extern "C" int gpf_stats_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_STATS], n, mode, 2, ms, nullptr, [](const gpf_handle* h, const std::string& who) {
        GPF_TRY(stats_refusal(h, who, h->stats.mask));
        if (h->cfg.thinning != GPF_THINNING_NONE || h->el.on || h->gp[0].set || h->gp[1].set || h->gp[2].set)
            return fail(GPF_ERR_STATE, who + ": handles that gpf_step advances only (this one steps stage-wise)");
        return (int)GPF_OK;
    }));
    if (mode >= 1 && !h->stats.every) return fail(GPF_ERR_STATE, "gpf_stats_time: modes 1 and 2 need armed statistics (gpf_stats_set)");
    GPF_TRY(enter(h));
    SeriesAside aside(h, mode == 1 ? &h->stats.every : nullptr);
    return series_time(h, "gpf_stats_time", aside,
                       [&](long long base) {
                           if (mode != 2) return series_time_steps(h, n, base, [&](long long expect) { return stats_launch(h, expect, base); });
                           int par = 0;
                           GPF_TRY(current_parity(h, &par));
                           const int mask = h->stats.mask, nin = ((mask & 3) ? 1 : 0) + ((mask >> 2) & 1) + ((mask >> 3) & 1);
                           for (int64_t i = 0; i < n; ++i)
                               hipLaunchKernelGGL(k_stats_stream, dim3(stats_grid(h)), dim3(256), 0, h->stream, (const double*)h->q[par], h->stats.acc, h->L.plane, nin,
                                                  stats_nfields(mask));
                           return (int)GPF_OK;
                       },
                       [&](long long base, long long ran) { return stats_collect(h, base, ran); }, ms);
}
