// Part of api.hip (included there, not compiled on its own): reduced frames -- for each selected field of the lines' nine one
// (mx, my) array over a window of the interior, sampled or block-averaged on an sx x sy lattice, as float or double -- recorded on
// the device behind the committed steps whose count is a multiple of the armed stride, and handed out once per call.  Kernels:
// frame_kernels.hip; the argument check, the blocks with their ragged ends, the record's layout and the batch limit: frames.hpp.

// The cases the recording does not cover: the regions' (series_refusal), with their error classes
static int frames_refusal(const gpf_handle* h, const std::string& who) { return series_refusal(h, who, "frames", "the frames"); }

// A gpf_frame_spec checked against the handle's grid and normalised (frames.hpp: frame_check, frame_normalise); a window of four
// zeros is the whole interior
static int frames_parse(const gpf_handle* h, const std::string& who, const gpf_frame_spec* g, FrameSpec& s) {
    if (!g) return fail(GPF_ERR_INVALID, who + ": null spec");
    const Layout& L = h->L;
    const bool whole = !g->ix0 && !g->ix1 && !g->iy0 && !g->iy1;
    s.mask = g->fields;
    s.ix0 = whole ? 1 : g->ix0; s.ix1 = whole ? L.Nx : g->ix1; s.iy0 = whole ? 1 : g->iy0; s.iy1 = whole ? L.Ny : g->iy1;
    s.sx = g->sx; s.sy = g->sy; s.reduce = g->reduce; s.f4 = g->dtype;
    switch (frame_check(s, L.Nx, L.Ny)) {
        case 0: break;
        case 1: return fail(GPF_ERR_INVALID, who + ": fields must be a non-empty mask of the nine fields (bits 0..8), got " + std::to_string(g->fields));
        case 2: return fail(GPF_ERR_INVALID, who + ": window (" + std::to_string(g->ix0) + ", " + std::to_string(g->ix1) + ", " + std::to_string(g->iy0) + ", " +
                                             std::to_string(g->iy1) + ") must be ix0 <= ix1 within 1.." + std::to_string(L.Nx) + " and iy0 <= iy1 within 1.." +
                                             std::to_string(L.Ny) + " (inclusive interior indices; four zeros: the whole interior)");
        case 3: return fail(GPF_ERR_INVALID, who + ": stride (" + std::to_string(g->sx) + ", " + std::to_string(g->sy) + ") must lie within 1.." +
                                             std::to_string(FRAME_MAX_STRIDE));
        case 4: return fail(GPF_ERR_INVALID, who + ": reduce must be 0 (sample) or 1 (mean), got " + std::to_string(g->reduce));
        default: return fail(GPF_ERR_INVALID, who + ": dtype must be 0 (f8) or 1 (f4), got " + std::to_string(g->dtype));
    }
    if (frame_mx(s) > 65535) return fail(GPF_ERR_INVALID, who + ": " + std::to_string(frame_mx(s)) + " output rows, at most 65535 (a larger sx, or a narrower window)");
    frame_normalise(s);
    return GPF_OK;
}

// A stepping call begins: its records replace those of the call before
static int frames_begin(gpf_handle* h) {
    if (!h->frames.armed()) return GPF_OK;
    GPF_TRY(frames_refusal(h, "gpf_step with frames armed"));
    h->frames.forget();
    return GPF_OK;
}

// The launch on the handle's stream: the record of the committed state, if the step count is `expect`, into `slot` of `rec`
// (`cap`: the last slot `rec` holds)
static int frames_enqueue_to(gpf_handle* h, const FrameSpec& s, char* rec, long long expect, long long slot, long long cap) {
    FrameArgs f;
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.Ls = h->Ls; f.st = h->st;
    f.rec = rec; f.L = h->L; f.s = s; f.mx = frame_mx(s); f.my = frame_my(s); f.record_bytes = frame_record_bytes(s); f.slot = slot; f.cap = cap;
    const bool tau = (s.mask & FRAME_TAU) != 0, ls = tau && h->Ls;      // (the slip length enters the wall stresses alone)
    const bool mean = s.reduce == FRAME_MEAN;
    const dim3 grid(mean ? (unsigned)frame_groups(s) : (unsigned)((f.my + FRAME_THREADS - 1) / FRAME_THREADS), (unsigned)f.mx);
#define FRAME_LAUNCH(LS, TAU)                                                                                                    \
    do {                                                                                                                        \
        if (mean) hipLaunchKernelGGL((k_frame_mean<EOS_, LS, TAU>), grid, dim3(FRAME_THREADS), 0, h->stream, f, h->P, expect);  \
        else hipLaunchKernelGGL((k_frame_sample<EOS_, LS, TAU>), grid, dim3(FRAME_THREADS), 0, h->stream, f, h->P, expect);     \
    } while (0)
    EOS_DISPATCH(h->cfg.eos, {
        if (!tau) FRAME_LAUNCH(false, false);
        else if (ls) FRAME_LAUNCH(true, true);
        else FRAME_LAUNCH(false, true);
    });
#undef FRAME_LAUNCH
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

static int frames_enqueue(gpf_handle* h, long long expect, long long slot) {
    return frames_enqueue_to(h, h->frames.spec, h->frames.rec, expect, slot, h->frames.capacity);
}

// The longest batch a stepping call may enqueue from step count `base`: with frames armed, no more steps than leave `capacity`
// records (frames.hpp: frames_batch_limit); unchanged without
static long long frames_batch(const gpf_handle* h, long long batch, long long base) {
    if (!h->frames.armed()) return batch;
    return std::min(batch, frames_batch_limit(base, h->frames.every, h->frames.capacity));
}

// Behind the launches of one step of a batch that began at step count `base`: record it if it takes the count to a multiple
// of the stride.  No launch otherwise, and none without frames armed.
static int frames_launch(gpf_handle* h, long long expect, long long base) {
    if (!series_due(h->frames.every, expect)) return GPF_OK;
    const long long slot = series_slot(base, expect, h->frames.every);
    if (slot >= h->frames.capacity) return fail(GPF_ERR_STATE, "frames: a batch would leave more than the " + std::to_string(h->frames.capacity) + " records the buffer holds");
    return frames_enqueue(h, expect, slot);
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host
static int frames_collect(gpf_handle* h, long long base, long long ran) {
    return series_collect(h->frames.every, h->frames.steps, base, ran,
                          series_channel(h->frames.bytes, (unsigned char*)h->frames.rec, (size_t)h->frames.record_bytes));
}

static SeriesBuffers frames_owned(gpf_handle* h) { return {(void**)&h->frames.rec}; }

static int frames_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(frames_owned(h)));
    h->frames.disarm(); h->frames.capacity = 0; h->frames.record_bytes = 0;
    return GPF_OK;
}

extern "C" int gpf_frames_set(gpf_handle* h, int64_t every, const gpf_frame_spec* spec, int64_t capacity) {
    GPF_TRY(series_set_checks(h, SERIES[S_FRAMES], every, frames_refusal));
    if (capacity < 0) return fail(GPF_ERR_INVALID, "gpf_frames_set: capacity >= 1 required (0: the default), got " + std::to_string(capacity));
    FrameSpec s;
    GPF_TRY(frames_parse(h, "gpf_frames_set", spec, s));
    const long long bytes = frame_record_bytes(s);
    long long mb = 64;
    if (const char* e = std::getenv("GPF_FRAMES_MB")) mb = std::max<long long>(1, std::atoll(e));
    const long long most = (h->log_cap + every - 1) / every;        // what the longest batch can leave: more is never used
    const long long cap = capacity ? std::min<long long>(capacity, most) : frames_default_capacity(mb << 20, bytes, h->log_cap, every);
    GPF_TRY(series_disarm(h, SERIES[S_FRAMES]));
    const hipError_t e = hipMalloc(&h->frames.rec, (size_t)(cap + 1) * bytes);       // + the slot of gpf_frames_now
    if (e != hipSuccess) {
        (void)frames_release(h);
        return fail(GPF_ERR_HIP, std::string("gpf_frames_set: ") + hipGetErrorString(e));
    }
    h->frames.spec = s; h->frames.record_bytes = bytes; h->frames.capacity = cap;
    h->frames.every = every;
    return GPF_OK;
}

extern "C" int gpf_frames_clear(gpf_handle* h) { return series_clear(h, SERIES[S_FRAMES]); }

extern "C" int gpf_frames_read(gpf_handle* h, void* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->frames.armed()) return fail(GPF_ERR_STATE, "gpf_frames_read: no frames are armed (gpf_frames_set)");
    series_read(h->frames.steps, capacity_records, steps_out, n_records, series_channel(h->frames.bytes, (unsigned char*)out, (size_t)h->frames.record_bytes));
    return GPF_OK;
}

extern "C" int gpf_frames_shape(gpf_handle* h, const gpf_frame_spec* spec, int32_t* mx, int32_t* my, int64_t* record_bytes) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    FrameSpec s;
    GPF_TRY(frames_parse(h, "gpf_frames_shape", spec, s));
    if (mx) *mx = frame_mx(s);
    if (my) *my = frame_my(s);
    if (record_bytes) *record_bytes = frame_record_bytes(s);
    return GPF_OK;
}

extern "C" int gpf_frames_now(gpf_handle* h, const gpf_frame_spec* spec, void* out, int64_t bytes) {
    GPF_TRY(series_now_checks(h, SERIES[S_FRAMES], out != nullptr, frames_refusal));
    const bool armed = !spec;                       // the armed frame, into the slot behind a batch's
    if (armed && !h->frames.armed()) return fail(GPF_ERR_STATE, "gpf_frames_now: no frames are armed (gpf_frames_set), and no spec is given");
    FrameSpec s = h->frames.spec;
    if (!armed) GPF_TRY(frames_parse(h, "gpf_frames_now", spec, s));
    const long long need = frame_record_bytes(s);
    if (bytes < need) return fail(GPF_ERR_INVALID, "gpf_frames_now: room for " + std::to_string(need) + " bytes required, " + std::to_string(bytes) + " given");
    GPF_TRY(enter(h, true));
    StepState st;
    GPF_TRY(series_now_state(h, SERIES[S_FRAMES], st));
    if (armed) {
        GPF_TRY(frames_enqueue(h, st.step, h->frames.capacity));
        HIP_TRY(hipMemcpyAsync(out, h->frames.rec + (size_t)h->frames.capacity * need, (size_t)need, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return GPF_OK;
    }
    // a spec of its own: a buffer for this call alone, nothing armed or disarmed
    char* rec = nullptr;
    hipError_t e = hipMalloc(&rec, (size_t)need);
    const int rc = e == hipSuccess ? frames_enqueue_to(h, s, rec, st.step, 0, 0) : GPF_OK;
    if (e == hipSuccess && rc == GPF_OK) e = hipMemcpyAsync(out, rec, (size_t)need, hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);      // whatever was queued has run before the buffer goes
    if (e == hipSuccess) e = es;
    if (rec) (void)hipFree(rec);
    GPF_TRY(rc);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_frames_now: ") + hipGetErrorString(e));
    return GPF_OK;
}

// Diagnostic (tools/frames_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing (armed frames are put aside for the
// call), 1 recording at the armed stride (n at most what one batch may hold: frames_batch); *ms = first launch to last on the
// handle's stream (series_time).
extern "C" int gpf_frames_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_FRAMES], n, mode, 1, ms, "armed frames (gpf_frames_set)", frames_refusal));
    if (mode == 1 && n > frames_batch(h, n, h->host_step))
        return fail(GPF_ERR_INVALID, "gpf_frames_time: " + std::to_string(n) + " steps leave more records than the buffer holds (" + std::to_string(h->frames.capacity) +
                                     " at stride " + std::to_string(h->frames.every) + ")");
    return series_time_fused(h, SERIES[S_FRAMES], n, mode, ms);
}
