// Part of api.hip (included there, not compiled on its own): what the per-step recorders of a handle -- probes, film integrals,
// weighted integrals, regions, lines, extrema, statistics, step changes, reduced frames, an elastic handle's deformation series,
// a thinning handle's series
// (api_<name>.inc, included behind this file) -- have in common: the arithmetic of a stride's records, their way to the host and out of it, the
// alignment test of the 16-byte loads, the arguments and the two launches of the row-reduced series (device side:
// series_rows.hpp), the cases the film reductions refuse, the table of the series (SERIES) and every walk over it -- the records
// forgotten, the buffers freed, the series put aside for a call, the cut of a small-grid batch, the closed stage-wise step and the
// records that wait for gpf_elastic_update --, the shared checks of the gpf_<name>_set / _clear / _now / _time entry points and
// the frame of the gpf_*_time diagnostics.  A new series is its api_<name>.inc, its struct in gpf_handle and a row of SERIES:
// add a row (DESIGN.md 3.3n).

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

// The device buffers a series owns, by address (null: unused entry)
using SeriesBuffers = std::array<void**, 5>;

// hipFree what is there and forget it (the *_release of a series, once the stream is idle)
static int series_free(const SeriesBuffers& buffers) {
    for (void** p : buffers) {
        if (!p) continue;
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

// What a series with n first candidates (series_first.hpp) keeps beside its values, on first use: the cells of its records,
// cell [log_cap + 1][n][2], and the row scratch its row kernel hands its fold, row_val [Nx][n] and row_iy [Nx][n]
static int series_first_buffers(const gpf_handle* h, size_t n, int*& cell, double*& row_val, int*& row_iy) {
    const size_t slots = (size_t)h->log_cap + 1, nx = (size_t)h->L.Nx;
    if (!cell) HIP_TRY(hipMalloc(&cell, slots * 2 * n * sizeof(int)));
    if (!row_val) HIP_TRY(hipMalloc(&row_val, nx * n * sizeof(double)));
    if (!row_iy) HIP_TRY(hipMalloc(&row_iy, nx * n * sizeof(int)));
    return GPF_OK;
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

// ---- the table of the series ---------------------------------------------------------------------------------------------------
// When a series records a closed stage-wise step (gpf_close_step): not at all; behind the close's launches; there unless the
// handle's gap is elastic, behind gpf_elastic_update then (the gap deforms after the step closes: the record holds the gap the
// handle holds with that state); or behind gpf_elastic_update alone (no record on other handles)
enum { SERIES_NOT_STAGEWISE = 0, SERIES_AT_CLOSE, SERIES_AT_CLOSE_UNLESS_ELASTIC, SERIES_BEHIND_UPDATE };

// One row per series.  name: as the entry points spell it (gpf_<name>_set, ...).  arming: the word that arms it, 0 while it is
// not.  forget: the records the host holds for _read go (null: it keeps none per call).  store: its SeriesStore (null: none).
// begin, launch, collect, release, owned: its api_<name>.inc's -- a stepping call begins; behind the launches of the step that
// takes the count to `expect` in a batch that began at `base`; after the batch's state has been read, `ran` steps committed; the
// series disarmed, the stream drained, its buffers freed; those buffers.  Each returns at once while the series is not armed.
// fused: gpf_step records it.  next_record: the next step after `at` it records, for the series that cut a one-workgroup batch
// there (null: k_small_steps records it itself, or it is not fused).  stagewise: SERIES_* above.
struct Series {
    const char* name;
    long long* (*arming)(gpf_handle*);
    void (*forget)(gpf_handle*);
    SeriesStore* (*store)(gpf_handle*);
    int (*begin)(gpf_handle*);
    int (*launch)(gpf_handle*, long long expect, long long base);
    int (*collect)(gpf_handle*, long long base, long long ran);
    int (*release)(gpf_handle*);
    SeriesBuffers (*owned)(gpf_handle*);
    bool fused;
    long long (*next_record)(gpf_handle*, const Series&, long long at);
    int stagewise;
};

// The next multiple of the armed stride after `at` (never, while not armed)
static long long series_next_record(gpf_handle* h, const Series& r, long long at) {
    const long long every = *r.arming(h);
    return every ? (at / every + 1) * every : LLONG_MAX;
}
static long long stats_next_record(gpf_handle* h, const Series& r, long long at);

#define SERIES_HOOKS(x)                                                                                                          \
    static int x##_begin(gpf_handle*); static int x##_launch(gpf_handle*, long long, long long);                                \
    static int x##_collect(gpf_handle*, long long, long long); static int x##_release(gpf_handle*); static SeriesBuffers x##_owned(gpf_handle*);
SERIES_HOOKS(probes) SERIES_HOOKS(integrals) SERIES_HOOKS(weighted) SERIES_HOOKS(regions) SERIES_HOOKS(lines) SERIES_HOOKS(extrema)
SERIES_HOOKS(stats) SERIES_HOOKS(changes) SERIES_HOOKS(frames) SERIES_HOOKS(eldef) SERIES_HOOKS(thin)
#undef SERIES_HOOKS
// The first columns of a row whose struct in gpf_handle derives from SeriesStore; the hooks' columns
#define SERIES_STORE(field) [](gpf_handle* h) { return &h->field.every; }, [](gpf_handle* h) { h->field.forget(); }, [](gpf_handle* h) -> SeriesStore* { return &h->field; }
#define SERIES_HOOKS(x) x##_begin, x##_launch, x##_collect, x##_release, x##_owned

// In gpf_step's order -- of the refusals a caller sees first, and of the recording launches on the stream --, the deformation
// series and the thinning series, which gpf_step does not record, behind them
enum { S_PROBES, S_INTEGRALS, S_WEIGHTED, S_REGIONS, S_LINES, S_EXTREMA, S_STATS, S_CHANGES, S_FRAMES, S_ELDEF, S_THIN };
static const Series SERIES[] = {
    {"probes", [](gpf_handle* h) { return &h->probes.n; }, [](gpf_handle* h) { h->probes.host.clear(); h->probes.first_step = h->host_step + 1; }, nullptr,
     SERIES_HOOKS(probes), true, nullptr, SERIES_AT_CLOSE},
    {"integrals", SERIES_STORE(integ), SERIES_HOOKS(integrals), true, nullptr, SERIES_BEHIND_UPDATE},
    {"weighted", SERIES_STORE(weighted), SERIES_HOOKS(weighted), true, series_next_record, SERIES_NOT_STAGEWISE},
    {"regions", SERIES_STORE(regions), SERIES_HOOKS(regions), true, series_next_record, SERIES_NOT_STAGEWISE},
    {"lines", SERIES_STORE(lines), SERIES_HOOKS(lines), true, series_next_record, SERIES_NOT_STAGEWISE},
    {"extrema", SERIES_STORE(extr), SERIES_HOOKS(extrema), true, nullptr, SERIES_AT_CLOSE_UNLESS_ELASTIC},
    // (the statistics hold a window, not a call's records: stats_restart; their floor decides where they cut)
    {"stats", [](gpf_handle* h) { return &h->stats.every; }, nullptr, nullptr, SERIES_HOOKS(stats), true, stats_next_record, SERIES_AT_CLOSE},
    {"changes", SERIES_STORE(chg), SERIES_HOOKS(changes), true, series_next_record, SERIES_NOT_STAGEWISE},
    {"frames", SERIES_STORE(frames), SERIES_HOOKS(frames), true, series_next_record, SERIES_NOT_STAGEWISE},
    {"elastic_series", SERIES_STORE(eldef), SERIES_HOOKS(eldef), false, nullptr, SERIES_BEHIND_UPDATE},
    {"thinning_series", SERIES_STORE(thin), SERIES_HOOKS(thin), false, nullptr, SERIES_AT_CLOSE_UNLESS_ELASTIC},
};
#undef SERIES_STORE
#undef SERIES_HOOKS
// gpf_close_step's order, and gpf_elastic_update's: extrema before film integrals, where gpf_step has them the other way round
// (kept apart: the order decides which of two refusals a caller sees)
static const int SERIES_STAGEWISE[] = {S_PROBES, S_EXTREMA, S_INTEGRALS, S_ELDEF, S_STATS, S_THIN};

// The records every series holds on the host for _read go: a stepping call in which a series records nothing leaves none
static void series_forget_records(gpf_handle* h) {
    for (const Series& r : SERIES)
        if (r.forget) r.forget(h);
}

// gpf_destroy: the series' device buffers (the stream has been drained; errors are not reported there)
static void series_destroy(gpf_handle* h) {
    for (const Series& r : SERIES)
        for (void** p : r.owned(h))
            if (p && *p) (void)hipFree(*p);
}

// ---- series put aside for a call ---------------------------------------------------------------------------------------------
// What arms each series remembered, and all of them disarmed except `keep` (the address of one's arming word, or null: none).
// restore() puts the values back; the destructor does if nobody asked.  Every recorder returns at once while its series is
// disarmed, so this is all it takes to step without it.
struct SeriesAside {
    gpf_handle* const h;
    const long long* const keep;
    long long armed[sizeof(SERIES) / sizeof(SERIES[0])];
    bool restored = false;
    SeriesAside(gpf_handle* handle, const long long* keep_armed) : h(handle), keep(keep_armed) {
        int k = 0;
        for (const Series& r : SERIES) {
            long long* word = r.arming(h);
            armed[k++] = *word;
            if (word != keep) *word = 0;
        }
    }
    SeriesAside(const SeriesAside&) = delete;
    SeriesAside& operator=(const SeriesAside&) = delete;
    ~SeriesAside() { restore(); }
    void restore() {
        if (restored) return;
        restored = true;
        int k = 0;
        for (const Series& r : SERIES) *r.arming(h) = armed[k++];
    }
    bool keeps_statistics() const { return keep == SERIES[S_STATS].arming(h); }
};

// ---- a small grid's batch ----------------------------------------------------------------------------------------------------
// A batch of the small-grid kernel, cut at the union of the steps that the series which cut it record (the rows with a
// next_record), each series' kernels launched at its own steps.  k_small_steps itself knows nothing of them, and a batch in
// pieces is bitwise the batch in one: every piece starts from the state and the run state the piece before left.  With none of
// them armed this is the one launch.  Probes, extrema and film integrals do not cut: k_small_steps records them.
static int small_batch_cut(gpf_handle* h, long long batch, int honor_stop, long long base) {
    const long long end = base + batch;
    for (long long at = base; at < end;) {
        long long next = end;
        for (const Series& r : SERIES)
            if (r.next_record) next = std::min(next, r.next_record(h, r, at));
        GPF_TRY(enqueue_small_steps(h, (int)(next - at), honor_stop, base));
        for (const Series& r : SERIES)      // (the changes': k_small_steps' exit has left q^(n-1) in the other buffer)
            if (r.next_record) GPF_TRY(r.launch(h, next, base));
        at = next;
    }
    return GPF_OK;
}

// ---- the closed stage-wise step --------------------------------------------------------------------------------------------------
// Does the record of a closed step of this handle wait for gpf_elastic_update?
static bool series_waits_for_update(const gpf_handle* h, const Series& r) {
    return r.stagewise == SERIES_BEHIND_UPDATE || (r.stagewise == SERIES_AT_CLOSE_UNLESS_ELASTIC && h->el.on);
}

// gpf_close_step, behind its launches: the closed step's record, if it commits -- or, where the record waits, the note that it
// does (`pending`) and of the step count the step began at.  Only an elastic handle has the update to wait for.
static int series_close_launch(gpf_handle* h, const Series& r) {
    const long long base = h->host_step;
    if (!series_waits_for_update(h, r)) {
        GPF_TRY(r.begin(h));
        return r.launch(h, base + 1, base);
    }
    SeriesStore& s = *r.store(h);
    s.pending = false;
    if (!h->el.on) return GPF_OK;
    GPF_TRY(r.begin(h));
    s.pending = s.armed(); s.pending_base = base;
    return GPF_OK;
}

// ... after the state has been read: the record to the host; a step that did not commit leaves nothing to wait for
static int series_close_collect(gpf_handle* h, const Series& r, long long ran) {
    if (!series_waits_for_update(h, r)) return r.collect(h, h->host_step, ran);
    if (ran < 1) r.store(h)->pending = false;
    return GPF_OK;
}

// gpf_elastic_update, behind its launches: the record of the step gpf_close_step committed just before, at the armed stride, with
// the gap the handle now holds
static int series_after_elastic_update(gpf_handle* h, const Series& r) {
    SeriesStore& s = *r.store(h);
    if (!s.pending) return GPF_OK;
    s.pending = false;
    const long long base = s.pending_base;
    if (h->host_step != base + 1 || !series_due(s.every, h->host_step)) return GPF_OK;
    GPF_TRY(r.launch(h, h->host_step, base));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return r.collect(h, base, 1);
}

// ---- what the entry points of the series share -------------------------------------------------------------------------------
// Each takes the series' row and builds the caller's name from it, "gpf_<name>_<call>"; `refusal(h, who)` is the series' own.
static std::string series_entry(const Series& r, const char* call) { return std::string("gpf_") + r.name + "_" + call; }

// gpf_<name>_set up to the series' own arguments: the handle, the series' refusal, the stride
template <class Refusal> static int series_set_checks(gpf_handle* h, const Series& r, int64_t every, Refusal&& refusal) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    const std::string who = series_entry(r, "set");
    GPF_TRY(refusal(h, who));
    if (every < 1) return fail(GPF_ERR_INVALID, who + ": every >= 1 required (" + series_entry(r, "clear") + " disarms), got " + std::to_string(every));
    return GPF_OK;
}

// ... and once they have passed: what was armed goes, with its buffers and records (the caller arms last, when all is in place)
static int series_disarm(gpf_handle* h, const Series& r) {
    GPF_TRY(enter(h, true));
    return r.release(h);
}

// gpf_<name>_clear
static int series_clear(gpf_handle* h, const Series& r) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (h->step_open) return fail(GPF_ERR_STATE, series_entry(r, "clear") + ": a stage-wise step is open; close it first");
    return series_disarm(h, r);
}

// gpf_<name>_now up to the series' own arguments (`have_args`: none of the caller's pointers is null)
template <class Refusal> static int series_now_checks(gpf_handle* h, const Series& r, bool have_args, Refusal&& refusal) {
    const std::string who = series_entry(r, "now");
    if (!h || !have_args) return fail(GPF_ERR_INVALID, who + ": null argument");
    if (!h->has_q || !h->has_topo) return fail(GPF_ERR_STATE, who + ": upload q and topography first");
    return refusal(h, who);
}

// ... and the run state whose step count the record is taken at: a rolled-back one has no record
static int series_now_state(gpf_handle* h, const Series& r, StepState& s) {
    GPF_TRY(read_state(h, s));
    if (s.invalid) return fail(GPF_ERR_STATE, series_entry(r, "now") + ": the run state is flagged invalid (the last step was rolled back)");
    return GPF_OK;
}

// gpf_<name>_time up to the series' own checks: modes 0..max_mode, of which mode 1 records and `needs` the series armed (the end
// of that sentence; null: the caller says it)
template <class Refusal> static int series_time_checks(gpf_handle* h, const Series& r, int64_t n, int mode, int max_mode, double* ms, const char* needs, Refusal&& refusal) {
    const std::string who = series_entry(r, "time");
    if (!h || !ms) return fail(GPF_ERR_INVALID, who + ": null argument");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, who + ": call gpf_pre_run first");
    GPF_TRY(refusal(h, who));
    if (n < 1 || n > h->log_cap || mode < 0 || mode > max_mode)
        return fail(GPF_ERR_INVALID, who + ": 1 <= n <= " + std::to_string(h->log_cap) + " and mode in 0.." + std::to_string(max_mode) + " required");
    if (needs && mode == 1 && !*r.arming(h)) return fail(GPF_ERR_STATE, who + ": mode 1 needs " + needs);
    return GPF_OK;
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

// n steps of a handle that steps stage-wise as a host takes them: the stage-wise calls, then, on an elastic handle,
// gpf_elastic_update, behind whose launches the film integrals and the deformation series write the closed step's record (every
// call synchronises, so *ms of series_time is the host's time too).  Every gpf_close_step begins its series' records afresh:
// `keep()` behind each step moves what it left to where the call's collect finds it.  Stops at a step that did not commit.
template <class Keep> static int series_time_stagewise_steps(gpf_handle* h, int64_t n, Keep&& keep) {
    for (int64_t i = 0; i < n; ++i) {
        GPF_TRY(gpf_open_step(h));
        for (int stage = 0; stage < 2; ++stage) {
            GPF_TRY(gpf_stage_closures(h));
            GPF_TRY(gpf_stage_advance(h, stage));
        }
        gpf_scalars_t sc;
        GPF_TRY(gpf_close_step(h, &sc));
        if (sc.invalid) break;
        if (h->el.on) GPF_TRY(gpf_elastic_update(h));
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

// The rest of a gpf_<name>_time whose modes are 0 -- nothing recorded, the armed series put aside for the call -- and 1 --
// recording at the armed stride --: n steps as gpf_step enqueues them with the row's hooks
static int series_time_fused(gpf_handle* h, const Series& r, int64_t n, int mode, double* ms) {
    GPF_TRY(enter(h));
    SeriesAside aside(h, mode == 1 ? r.arming(h) : nullptr);
    GPF_TRY(r.begin(h));        // (returns at once in mode 0)
    return series_time(h, series_entry(r, "time").c_str(), aside,
                       [&](long long base) { return series_time_steps(h, n, base, [&](long long expect) { return r.launch(h, expect, base); }); },
                       [&](long long base, long long ran) { return r.collect(h, base, ran); }, ms);
}
