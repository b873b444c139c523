// Part of api.hip (included there, not compiled on its own): line profiles -- the nine fields rho, jx, jy, p, h and the four wall
// shear stresses along interior rows or columns, at one index or averaged over a band -- recorded on the device behind the
// committed steps whose count is a multiple of the armed stride, and handed out once per call.  Kernels: line_kernels.hip; the
// record's layout, the order of a band's additions and the batch limit: lines.hpp.

// The cases the recording does not cover: the regions' (series_refusal), with their error classes
static int lines_refusal(const gpf_handle* h, const std::string& who) { return series_refusal(h, who, "lines", "the lines"); }

// gpf_line entries checked against the handle's grid and laid out (lines.hpp: lines_layout); i0 = i1 = 0 is the centre line
static int lines_parse(const gpf_handle* h, const std::string& who, int K, const gpf_line* lines, Line* defs, long long* rec_doubles, long long* scratch_doubles) {
    if (K < 1 || K > LINE_MAX_K) return fail(GPF_ERR_INVALID, who + ": 1 to " + std::to_string(LINE_MAX_K) + " lines required, got " + std::to_string(K));
    if (!lines) return fail(GPF_ERR_INVALID, who + ": null lines");
    const Layout& L = h->L;
    for (int k = 0; k < K; ++k) {
        const gpf_line& g = lines[k];
        Line& l = defs[k];
        const bool centre = !g.i0 && !g.i1;
        l.along = g.along;
        l.i0 = centre ? line_centre(g.along == 1 ? 1 : 0, L.Nx, L.Ny) : g.i0;
        l.i1 = centre ? l.i0 : g.i1;
        const std::string which = who + ": line " + std::to_string(k);
        switch (line_check(l.along, l.i0, l.i1, L.Nx, L.Ny)) {
            case 0: break;
            case 1: return fail(GPF_ERR_INVALID, which + ": along must be 0 (x) or 1 (y), got " + std::to_string(g.along));
            default: return fail(GPF_ERR_INVALID, which + ": indices (" + std::to_string(g.i0) + ", " + std::to_string(g.i1) + ") must be i0 <= i1 within 1.." +
                                                  std::to_string(l.along == 0 ? L.Ny : L.Nx) + " (inclusive interior " + (l.along == 0 ? "columns" : "rows") +
                                                  "; both zero: the centre line)");
        }
    }
    *rec_doubles = lines_layout(defs, K, L.Nx, L.Ny, scratch_doubles);
    return GPF_OK;
}

// A stepping call begins: its records replace those of the call before
static int lines_begin(gpf_handle* h) {
    if (!h->lines.armed()) return GPF_OK;
    GPF_TRY(lines_refusal(h, "gpf_step with lines armed"));
    h->lines.forget();
    return GPF_OK;
}

// The launches on the handle's stream: the record of the committed state, if the step count is `expect`, into `slot` of `rec`
// (`cap`: the last slot `rec` holds)
static int lines_enqueue_to(gpf_handle* h, const Line* defs, int K, long long rec_doubles, double* rec, double* scratch, long long expect, long long slot,
                            long long cap) {
    LineArgs f;
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.Ls = h->Ls; f.st = h->st;
    f.rec = rec; f.scratch = scratch; f.L = h->L; f.K = K; f.rec_doubles = rec_doubles; f.slot = slot; f.cap = cap;
    long long npoint = 0, nband_x = 0, nband_y = 0, npartial = 0;       // threads along grid.x of each kind: its longest line
    for (int k = 0; k < LINE_MAX_K; ++k) {
        f.lines[k] = k < K ? defs[k] : Line{0, 1, 1, 0, 0, 0};
        if (k >= K) continue;
        const Line& l = defs[k];
        if (!line_is_band(l)) npoint = std::max<long long>(npoint, l.len);
        else if (l.along == 0) nband_x = std::max<long long>(nband_x, l.len);
        else {
            nband_y = std::max<long long>(nband_y, l.len);
            npartial = std::max<long long>(npartial, (long long)line_chunks(line_band_cells(l)) * l.len);
        }
    }
    auto blocks = [](long long n, int per) { return (unsigned)((n + per - 1) / per); };
    EOS_DISPATCH(h->cfg.eos, {
        if (npoint) {
            const dim3 grid(blocks(npoint, 256), K);
            if (h->Ls) hipLaunchKernelGGL((k_line_point<EOS_, true>), grid, dim3(256), 0, h->stream, f, h->P, expect);
            else hipLaunchKernelGGL((k_line_point<EOS_, false>), grid, dim3(256), 0, h->stream, f, h->P, expect);
        }
        if (nband_x) {
            const dim3 grid(blocks(nband_x, 4), K);         // four waves, four rows, per workgroup
            if (h->Ls) hipLaunchKernelGGL((k_line_band_x<EOS_, true>), grid, dim3(256), 0, h->stream, f, h->P, expect);
            else hipLaunchKernelGGL((k_line_band_x<EOS_, false>), grid, dim3(256), 0, h->stream, f, h->P, expect);
        }
        if (nband_y) {
            const dim3 grid(blocks(npartial, 256), K);
            if (h->Ls) hipLaunchKernelGGL((k_line_band_y_partial<EOS_, true>), grid, dim3(256), 0, h->stream, f, h->P, expect);
            else hipLaunchKernelGGL((k_line_band_y_partial<EOS_, false>), grid, dim3(256), 0, h->stream, f, h->P, expect);
        }
    });
    HIP_TRY(hipGetLastError());
    if (nband_y) {
        hipLaunchKernelGGL(k_line_band_y_fold, dim3(blocks(nband_y, 256), K), dim3(256), 0, h->stream, f, expect);
        HIP_TRY(hipGetLastError());
    }
    return GPF_OK;
}

static int lines_enqueue(gpf_handle* h, long long expect, long long slot) {
    return lines_enqueue_to(h, h->lines.defs, h->lines.K, h->lines.rec_doubles, h->lines.rec, h->lines.scratch, expect, slot, h->lines.capacity);
}

// The longest batch a stepping call may enqueue from step count `base`: with lines armed, no more steps than leave `capacity`
// records (lines.hpp: lines_batch_limit); unchanged without
static long long lines_batch(const gpf_handle* h, long long batch, long long base) {
    if (!h->lines.armed()) return batch;
    return std::min(batch, lines_batch_limit(base, h->lines.every, h->lines.capacity));
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without lines armed.
static int lines_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->lines.every, expect)) return GPF_OK;
    const long long slot = lines_count(base, expect - base, h->lines.every) - 1;
    if (slot >= h->lines.capacity) return fail(GPF_ERR_STATE, "lines: a batch would leave more than the " + std::to_string(h->lines.capacity) + " records the buffer holds");
    return lines_enqueue(h, expect, slot);
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host (series_count
// is lines.hpp's lines_count)
static int lines_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->lines.every, h->lines.steps, base, ran, series_channel(h->lines.host, h->lines.rec, (size_t)h->lines.rec_doubles));
}

static SeriesBuffers lines_owned(gpf_handle* h) { return {(void**)&h->lines.rec, (void**)&h->lines.scratch}; }

static int lines_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(lines_owned(h)));
    h->lines.disarm(); h->lines.K = 0; h->lines.capacity = 0; h->lines.rec_doubles = 0;
    return GPF_OK;
}

extern "C" int gpf_lines_set(gpf_handle* h, int64_t every, int K, const gpf_line* lines, int64_t capacity) {
    GPF_TRY(series_set_checks(h, SERIES[S_LINES], every, lines_refusal));
    if (capacity < 0) return fail(GPF_ERR_INVALID, "gpf_lines_set: capacity >= 1 required (0: the default), got " + std::to_string(capacity));
    Line defs[LINE_MAX_K];
    long long rec_doubles = 0, scratch_doubles = 0;
    GPF_TRY(lines_parse(h, "gpf_lines_set", K, lines, defs, &rec_doubles, &scratch_doubles));
    long long mb = 64;
    if (const char* s = std::getenv("GPF_LINES_MB")) mb = std::max<long long>(1, std::atoll(s));
    const long long most = (h->log_cap + every - 1) / every;        // what the longest batch can leave: more is never used
    const long long cap = capacity ? std::min<long long>(capacity, most) : lines_default_capacity(mb << 20, rec_doubles, h->log_cap, every);
    GPF_TRY(series_disarm(h, SERIES[S_LINES]));
    hipError_t e = hipMalloc(&h->lines.rec, (size_t)(cap + 1) * rec_doubles * sizeof(double));       // + the slot of gpf_lines_now
    if (e == hipSuccess && scratch_doubles) e = hipMalloc(&h->lines.scratch, (size_t)scratch_doubles * sizeof(double));
    if (e != hipSuccess) {
        (void)lines_release(h);
        return fail(GPF_ERR_HIP, std::string("gpf_lines_set: ") + hipGetErrorString(e));
    }
    for (int k = 0; k < K; ++k) h->lines.defs[k] = defs[k];
    h->lines.K = K; h->lines.rec_doubles = rec_doubles; h->lines.capacity = cap;
    h->lines.every = every;
    return GPF_OK;
}

extern "C" int gpf_lines_clear(gpf_handle* h) { return series_clear(h, SERIES[S_LINES]); }

extern "C" int gpf_lines_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->lines.armed()) return fail(GPF_ERR_STATE, "gpf_lines_read: no lines are armed (gpf_lines_set)");
    series_read(h->lines.steps, capacity_records, steps_out, n_records, series_channel(h->lines.host, out, (size_t)h->lines.rec_doubles));
    return GPF_OK;
}

extern "C" int gpf_lines_now(gpf_handle* h, int K, const gpf_line* lines, double* out, int64_t count) {
    GPF_TRY(series_now_checks(h, SERIES[S_LINES], out != nullptr, lines_refusal));
    const bool armed = K == 0 && !lines;            // the armed lines, into the slot behind a batch's
    if (armed && !h->lines.armed()) return fail(GPF_ERR_STATE, "gpf_lines_now: no lines are armed (gpf_lines_set), and none are given");
    Line defs[LINE_MAX_K];
    long long rec_doubles = h->lines.rec_doubles, scratch_doubles = 0;
    if (!armed) GPF_TRY(lines_parse(h, "gpf_lines_now", K, lines, defs, &rec_doubles, &scratch_doubles));
    if (count < rec_doubles) return fail(GPF_ERR_INVALID, "gpf_lines_now: room for " + std::to_string(rec_doubles) + " doubles required, " + std::to_string(count) + " given");
    GPF_TRY(enter(h, true));
    StepState s;
    GPF_TRY(series_now_state(h, SERIES[S_LINES], s));
    if (armed) {
        GPF_TRY(lines_enqueue(h, s.step, h->lines.capacity));
        HIP_TRY(hipMemcpyAsync(out, h->lines.rec + (size_t)h->lines.capacity * rec_doubles, (size_t)rec_doubles * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return GPF_OK;
    }
    // a list of its own: buffers for this call alone, nothing armed or disarmed
    double *rec = nullptr, *scratch = nullptr;
    hipError_t e = hipMalloc(&rec, (size_t)rec_doubles * sizeof(double));
    if (e == hipSuccess && scratch_doubles) e = hipMalloc(&scratch, (size_t)scratch_doubles * sizeof(double));
    int rc = e == hipSuccess ? lines_enqueue_to(h, defs, K, rec_doubles, rec, scratch, s.step, 0, 0) : GPF_OK;
    if (e == hipSuccess && rc == GPF_OK) e = hipMemcpyAsync(out, rec, (size_t)rec_doubles * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);      // whatever was queued has run before the buffers go
    if (e == hipSuccess) e = es;
    if (rec) (void)hipFree(rec);
    if (scratch) (void)hipFree(scratch);
    GPF_TRY(rc);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_lines_now: ") + hipGetErrorString(e));
    return GPF_OK;
}

// Diagnostic (tools/lines_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed lines are put aside for the
// call), 1 recording at the armed stride (n at most what one batch may hold: lines_batch); *ms = first launch to last on the
// handle's stream (series_time).
extern "C" int gpf_lines_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_LINES], n, mode, 1, ms, "armed lines (gpf_lines_set)", lines_refusal));
    if (mode == 1 && n > lines_batch(h, n, h->host_step))
        return fail(GPF_ERR_INVALID, "gpf_lines_time: " + std::to_string(n) + " steps leave more records than the buffer holds (" + std::to_string(h->lines.capacity) +
                                     " at stride " + std::to_string(h->lines.every) + ")");
    return series_time_fused(h, SERIES[S_LINES], n, mode, ms);
}
