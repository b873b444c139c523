// Part of api.hip (included there, not compiled on its own): what the per-step recorders of a handle -- probes, film integrals,
// weighted integrals, regions, lines, extrema, statistics, an elastic handle's deformation series, step changes (api_<name>.inc, included
// behind this file) -- have in common: the
// arithmetic of a stride's records, their way to the host and out of it, the alignment test of the 16-byte loads, the arguments
// and the two launches of the row-reduced series (device side: series_rows.hpp), the cases the film reductions refuse, how
// series are put aside for a call, the frame of the gpf_*_time diagnostics, and the cut of a small-grid batch.  A new series is named here in SeriesAside, series_forget_records and, if it cuts, small_batch_cut.

// ---- records of a stride -----------------------------------------------------------------------------------------------------
// Records a stepping call leaves for the steps (base, base + ran]: the multiples of `every` among them.
static long long series_count(long long base, long long ran, long long every) {
    return ran > 0 ? (base + ran) / every - base / every : 0;
}

// Slot of the record of step `expect`, a multiple of `every`, in a batch that began at step count `base`
static long long series_slot(long long base, long long expect, long long every) { return series_count(base, expect - base, every) - 1; }

// Does the step that takes the count to `expect` leave a record?  Not without the series armed, nor off its stride.
static bool series_due(long long every, long long expect) { return every && expect % every == 0; }

// One channel of a series' records: `per` values of T per record, on the host, and the buffer they come from (the device's
// records of the batch, series_collect) or go to (the caller's, series_read; may be null)
template <class T> struct SeriesChannel { std::vector<T>& host; T* other; size_t per; };
template <class T> static SeriesChannel<T> series_channel(std::vector<T>& host, T* other, size_t per) { return {host, other, per}; }

template <class T> static int series_append(const SeriesChannel<T>& c, size_t have, size_t cnt) {
    c.host.resize((have + cnt) * c.per);
    HIP_TRY(hipMemcpy(c.host.data() + have * c.per, c.other, cnt * c.per * sizeof(T), hipMemcpyDeviceToHost));
    return GPF_OK;
}

// After the batch's state has been read (the stream is idle): a batch that stopped on the device ran a prefix of its steps,
// so the records written are those of the multiples of the stride in (base, base + ran]: every channel's -> host, and their
// step counts
template <class... T> static int series_collect(long long every, std::vector<long long>& steps, long long base, long long ran, const SeriesChannel<T>&... channels) {
    if (!every) return GPF_OK;
    const long long cnt = series_count(base, ran, every);
    if (cnt <= 0) return GPF_OK;
    const size_t have = steps.size();
    int rc = GPF_OK;
    ((rc = rc != GPF_OK ? rc : series_append(channels, have, (size_t)cnt)), ...);
    GPF_TRY(rc);
    for (long long k = 1; k <= cnt; ++k) steps.push_back((base / every + k) * every);
    return GPF_OK;
}

template <class T> static void series_hand_out(const SeriesChannel<T>& c, int64_t take) {
    if (c.other && take > 0) std::memcpy(c.other, c.host.data(), (size_t)take * c.per * sizeof(T));
}

// The records of the last stepping call: how many there are, and as many as the caller has room for
template <class... T> static void series_read(const std::vector<long long>& steps, int64_t capacity_records, int64_t* steps_out, int64_t* n_records,
                                              const SeriesChannel<T>&... channels) {
    const int64_t have = (int64_t)steps.size(), take = std::max<int64_t>(0, std::min(have, capacity_records));
    if (n_records) *n_records = have;
    (series_hand_out(channels, take), ...);
    for (int64_t k = 0; steps_out && k < take; ++k) steps_out[k] = steps[(size_t)k];
}

// hipFree what is there and forget it (the *_release of a series, once the stream is idle)
static int series_free(std::initializer_list<void**> buffers) {
    for (void** p : buffers) {
        if (*p) HIP_TRY(hipFree(*p));
        *p = nullptr;
    }
    return GPF_OK;
}

// ---- 16-byte pair loads ------------------------------------------------------------------------------------------------------
// Every pair (1 + 2k, 2 + 2k) of every row of every plane a recording kernel reads must start on 16 bytes: the state, the gap,
// the slip-length plane if the kernel reads it (`with_Ls`) and there is one, and the series' own planes (`own`, or null).
// Layout and hipMalloc give that today, so the 8-byte loads are otherwise out of reach: the environment variable GPF_FILM_NARROW
// (any value; each series reads it when its buffers are allocated and passes what it found as `narrow`) asks for them, which is
// how the narrow-load tests hold them bit for bit against the wide loads.
static bool series_wide_ok(const gpf_handle* h, bool narrow, bool with_Ls, const void* own = nullptr) {
    const Layout& L = h->L;
    auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    return ((L.off + 1) & 1) == 0 && (L.pitch & 1) == 0 && (L.plane & 1) == 0 && a16(h->q[0]) && a16(h->q[1]) && a16(h->topo) &&
           (!with_Ls || !h->Ls || a16(h->Ls)) && a16(own) && !narrow;
}

// ---- the row-reduced series' launches (series_rows.hpp) ----------------------------------------------------------------------
// What their kernels are told about the handle, the leading part of FilmArgs, WFilmArgs and RegionArgs by name (each keeps its
// own layout): the record of the committed state goes into `slot`
template <class Args> static void series_row_args(const gpf_handle* h, bool wide, long long slot, Args& f) {
    f.qa = h->q[0]; f.qb = h->q[1]; f.topo = h->topo; f.Ls = h->Ls; f.st = h->st;
    f.L = h->L; f.dx = h->cfg.dx; f.dy = h->cfg.dy;
    f.wide = wide ? 1 : 0;
    f.slot = slot; f.cap = h->log_cap;
}

// The two launches on the handle's stream, partial<EOS, HAS_LS> on `grid` (x: the interior rows) and fold on grid.y workgroups:
// the record if the step count is `expect`.  Returns from the calling function on a launch error.  `grid` and `f`: variables.
#define SERIES_ROWS_ENQUEUE(h, partial, fold, grid, f, expect)                                                                   \
    do {                                                                                                                        \
        EOS_DISPATCH((h)->cfg.eos, {                                                                                            \
            if ((h)->Ls) hipLaunchKernelGGL((partial<EOS_, true>), (grid), dim3(256), 0, (h)->stream, (f), (h)->P, (expect));   \
            else hipLaunchKernelGGL((partial<EOS_, false>), (grid), dim3(256), 0, (h)->stream, (f), (h)->P, (expect));          \
        });                                                                                                                     \
        HIP_TRY(hipGetLastError());                                                                                             \
        hipLaunchKernelGGL(fold, dim3((grid).y), dim3(256), 0, (h)->stream, (f), (expect));                                     \
        HIP_TRY(hipGetLastError());                                                                                             \
    } while (0)

// ---- refusals ----------------------------------------------------------------------------------------------------------------
// The cases the film reductions (film integrals, weighted integrals, regions, lines) do not cover, with the error class
// gpf_probes_set / gpf_gap_profiles give them.  `what` names the series as a whole, `the_what` where it evaluates.
// `elastic_gap_ok`: the series records an elastic handle's closed step behind gpf_elastic_update (the film integrals alone).
static int series_refusal(const gpf_handle* h, const std::string& who, const char* what, const char* the_what, bool elastic_gap_ok = false) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; " + what + " are not available on slabs");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set)
        return fail(GPF_ERR_INVALID, who + ": surrogate closures: " + the_what + " evaluate the analytic pressure and wall stress, which this handle replaces");
    if (h->cfg.thinning != GPF_THINNING_NONE) return fail(GPF_ERR_INVALID, who + ": shear thinning needs grad p (not supported)");
    if ((h->el.on && !elastic_gap_ok) || h->els.on) return fail(GPF_ERR_INVALID, who + ": an elastic handle steps stage-wise and deforms its gap between steps (not supported)");
    return GPF_OK;
}

// ---- series put aside for a call ---------------------------------------------------------------------------------------------
// What arms each of the nine series -- the probes' count and the eight strides -- remembered, and all of them disarmed except
// `keep` (the address of one of these fields, or null: none).  restore() puts the values back; the destructor does if nobody
// asked.  Every recorder returns at once while its series is disarmed, so this is all it takes to step without it.
struct SeriesAside {
    gpf_handle* const h;
    const void* const keep;
    const int probes;
    long long every[8];
    bool restored = false;
    std::array<long long*, 8> strides() const {
        return {&h->integ.every, &h->weighted.every, &h->regions.every, &h->lines.every, &h->extr.every, &h->stats.every, &h->eldef.every, &h->chg.every};
    }
    SeriesAside(gpf_handle* handle, const void* keep_armed) : h(handle), keep(keep_armed), probes(handle->probes.n) {
        if (keep != &h->probes.n) h->probes.n = 0;
        int k = 0;
        for (long long* e : strides()) {
            every[k++] = *e;
            if (e != keep) *e = 0;
        }
    }
    SeriesAside(const SeriesAside&) = delete;
    SeriesAside& operator=(const SeriesAside&) = delete;
    ~SeriesAside() { restore(); }
    void restore() {
        if (restored) return;
        restored = true;
        h->probes.n = probes;
        int k = 0;
        for (long long* e : strides()) *e = every[k++];
    }
    bool keeps_statistics() const { return keep == &h->stats.every; }
};

// The records every series holds on the host for _read go: a stepping call in which a series records nothing leaves none.
// (The statistics hold a window, not a call's records: stats_restart.)
static void series_forget_records(gpf_handle* h) {
    h->probes.host.clear(); h->probes.first_step = h->host_step + 1;
    h->integ.host.clear(); h->integ.steps.clear();
    h->weighted.host.clear(); h->weighted.steps.clear();
    h->regions.host.clear(); h->regions.ihost.clear(); h->regions.steps.clear();
    h->lines.host.clear(); h->lines.steps.clear();
    h->extr.host.clear(); h->extr.cells.clear(); h->extr.steps.clear();
    h->eldef.host.clear(); h->eldef.cells.clear(); h->eldef.steps.clear();
    h->chg.host.clear(); h->chg.cells.clear(); h->chg.steps.clear();
}

// ---- the gpf_*_time diagnostics ----------------------------------------------------------------------------------------------
// A call stepped from step count `base` outside gpf_step's loop: the host's counters follow the device's
static int series_resync(gpf_handle* h, long long base, StepState& s) {
    GPF_TRY(read_state(h, s));
    prev_state_after(h, s.step > base && !s.invalid);
    h->host_step = s.step; h->next_step = s.step;
    return GPF_OK;
}

// The frame of a gpf_*_time call (include/gapflow_hip.h: "the gpf_*_time diagnostics").  `aside` holds every series but the
// one the call records, if any.  *ms = what `enqueue(base)` puts on the handle's stream from step count `base`, first launch
// to last; `collect(base, ran)` takes the records of the `ran` steps to the host while the series' stride is still set; then
// the series come back, and armed statistics begin a new window unless the call recorded into it.  No other series keeps
// records from before the call.  Errors: enqueue's, then HIP's under the caller's name `who`, then the state read's, then
// collect's.
template <class Enqueue, class Collect>
static int series_time(gpf_handle* h, const char* who, SeriesAside& aside, Enqueue&& enqueue, Collect&& collect, double* ms) {
    series_forget_records(h);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    const long long base = h->host_step;
    int rc = GPF_OK;
    float t = 0.f;
    if (e == hipSuccess) e = hipEventRecord(e0, h->stream);
    if (e == hipSuccess) {
        rc = enqueue(base);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(e1, h->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    // steps may have been queued whatever went wrong after them: the host's counters follow the device's
    StepState s;
    const int rs = series_resync(h, base, s);
    int rcol = GPF_OK;
    if (rc == GPF_OK && e == hipSuccess && rs == GPF_OK) rcol = collect(base, s.step - base);
    aside.restore();
    if (rs == GPF_OK && rcol == GPF_OK && !aside.keeps_statistics()) rcol = stats_restart(h, s.step);     // steps went by unrecorded: a new window
    GPF_TRY(rc);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    GPF_TRY(rs);
    GPF_TRY(rcol);
    *ms = t;
    return GPF_OK;
}

// n steps from step count `base` as gpf_step enqueues them, `behind(expect)` behind each step of a grid that takes a launch
// per step (the armed series' own _launch, as a rule); a small grid's batch records or is cut by what is armed
template <class Behind> static int series_time_steps(gpf_handle* h, int64_t n, long long base, Behind&& behind) {
    if (small_grid_eligible(h)) return small_batch_cut(h, n, 0, base);
    for (int64_t i = 0; i < n; ++i) {
        GPF_TRY(enqueue_step(h, 0, base, nullptr));
        GPF_TRY(behind(base + i + 1));
    }
    return GPF_OK;
}

// n steps of an elastic handle as a host takes them: the stage-wise calls, then gpf_elastic_update, behind whose launches the
// film integrals and the deformation series write the closed step's record (every call synchronises, so *ms of series_time is
// the host's time too).  Every gpf_close_step begins its series' records afresh: `keep()` behind each update moves what the step
// left to where the call's collect finds it.  Stops at a step that did not commit.
template <class Keep> static int series_time_elastic_steps(gpf_handle* h, int64_t n, Keep&& keep) {
    for (int64_t i = 0; i < n; ++i) {
        GPF_TRY(gpf_open_step(h));
        for (int stage = 0; stage < 2; ++stage) {
            GPF_TRY(gpf_stage_closures(h));
            GPF_TRY(gpf_stage_advance(h, stage));
        }
        gpf_scalars_t sc;
        GPF_TRY(gpf_close_step(h, &sc));
        if (sc.invalid) break;
        GPF_TRY(gpf_elastic_update(h));
        keep();
    }
    return GPF_OK;
}

// keep() of a series whose record is a channel of doubles and the step counts: appended to `host`, `steps` of the call
static void series_time_keep(std::vector<double>& from, std::vector<long long>& from_steps, std::vector<double>& host, std::vector<long long>& steps) {
    host.insert(host.end(), from.begin(), from.end());
    steps.insert(steps.end(), from_steps.begin(), from_steps.end());
    from.clear(); from_steps.clear();
}

// ---- a small grid's batch ----------------------------------------------------------------------------------------------------
static int weighted_launch(gpf_handle* h, long long expect, long long base);
static int regions_launch(gpf_handle* h, long long expect, long long base);
static int lines_launch(gpf_handle* h, long long expect, long long base);
static int stats_launch(gpf_handle* h, long long expect);
static int changes_launch(gpf_handle* h, long long expect, long long base);
static long long stats_floor(const gpf_handle* h);

// A batch of the small-grid kernel, cut at the union of the steps that the series which cut it record (weighted integrals,
// regions, lines, statistics, changes), each series' kernels launched at its own steps.  k_small_steps itself knows nothing of them, and a
// batch in pieces is bitwise the batch in one: every piece starts from the state and the run state the piece before left.
// With none of them armed this is the one launch.  Probes, extrema and film integrals do not cut: k_small_steps records them.
static int small_batch_cut(gpf_handle* h, long long batch, int honor_stop, long long base) {
    const long long end = base + batch;
    for (long long at = base; at < end;) {
        long long next = end;
        for (long long every : {h->weighted.every, h->regions.every, h->lines.every, h->chg.every})
            if (every) next = std::min(next, (at / every + 1) * every);
        if (h->stats.every) next = std::min(next, (std::max(at, stats_floor(h)) / h->stats.every + 1) * h->stats.every);
        GPF_TRY(enqueue_small_steps(h, (int)(next - at), honor_stop, base));
        GPF_TRY(weighted_launch(h, next, base));
        GPF_TRY(regions_launch(h, next, base));
        GPF_TRY(lines_launch(h, next, base));
        GPF_TRY(stats_launch(h, next));
        GPF_TRY(changes_launch(h, next, base));     // (k_small_steps' exit has left q^(n-1) in the other buffer)
        at = next;
    }
    return GPF_OK;
}
