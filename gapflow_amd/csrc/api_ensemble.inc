// Ensembles (gpf_ensemble_*): many small problems advanced by one launch per kernel instantiation, one workgroup per member.
// Two tiers: a member that fits one workgroup's LDS runs k_small_ensemble (small_kernel.hip); one of up to MID_GRID_MAX_CELLS
// cells runs k_mid_ensemble (mid_kernel.hip) on a workspace in device memory that the ensemble owns.  Part of api.hip's
// translation unit.
//
// A member is a handle of its own, borrowed: everything a solo gpf_step of the same count would leave in it -- buffers, run
// state, log, host_step / next_step, prev_state_valid, g1_ready -- is left in it here, so that it can go on alone.
//
// The series -- film integrals (gpf_ensemble_integrals_*), field extrema (gpf_ensemble_extrema_*), point probes
// (gpf_ensemble_probes_*) -- belong to the ENSEMBLE, not to its members: both kernels record them inside the batch, behind each
// commit (film_record_block, extrema_record_block / extrema_record_wide, probe_record_block), into per-member slots that the
// ensemble owns, so nothing cuts a launch.  All three are one EnsembleSeries: where a member's records lie is
// ensemble_slots.hpp's to say, every gpf_ensemble_*_set ends in ensemble_series_install, every release is
// ensemble_series_release, a call's records come to the host through series_collect and leave through series_read
// (api_series.inc), as a handle's do.  A further series is its _set's checks and argument image, its _clear and _read shells, an
// entry in gpf_ensemble::series() and a pointer in SmallArgs; ensemble_collect takes a second channel of int32 as it is, any
// other kind of channel needs its arm there.

#include "ensemble_slots.hpp"

// One series of an ensemble: `what` an error message calls its records; the stride that arms it (0: not armed; the probes' is
// 1); `cap`, the records every member's slots hold -- what a call of at most LOG_CAPACITY steps can leave at the stride; 0 for the
// probes, whose capacity is each member's own log's and lives in `at` alone --; ONE device allocation `rec` for every member's
// records, laid out by `at`; the members' argument structs in device memory (`dev`: [m], and whatever the series keeps behind
// them), which point into `rec`; per member what the last gpf_ensemble_step left on the host (of each SeriesStore the records and
// their steps alone: the stride is `every` here, and nothing is ever pending).
struct EnsembleSeries {
    const char* what = "";
    long long every = 0, cap = 0;
    char* rec = nullptr;
    char* dev = nullptr;
    EnsembleSlots at;
    std::vector<SeriesStore> last;
    SeriesBuffers owned() { return {(void**)&rec, (void**)&dev}; }
    // member i's argument struct for the kernels (null while not armed)
    template <class Args> Args* args(int i) const { return every ? (Args*)dev + i : nullptr; }
    // channel c of member i's records: on the device, and where a call's come to rest
    template <class T> SeriesChannel<T> device_channel(int c, int i, std::vector<T>& host) const {
        return series_channel(host, (T*)(rec + at.at(c, i)), at.record_bytes(c, i) / sizeof(T));
    }
    template <class T> SeriesChannel<T> read_channel(int c, int i, std::vector<T>& host, T* out) const {
        return series_channel(host, out, at.record_bytes(c, i) / sizeof(T));
    }
};

struct gpf_ensemble {
    std::vector<gpf_handle*> members;
    int device = 0;
    // one device allocation and its pinned mirror, in launch-slot order: StepState[m] | SmallArgs[k] | Phys[k] for the k members a
    // call launches -- the arguments adjacent, so that ONE copy per call fills them; the states come back with one
    char* dev = nullptr;
    char* host = nullptr;
    // ... and behind them double*[k], the launched members' workspaces (null for a member of the LDS tier)
    std::vector<int> slot_member;           // launch slot -> member, of the last call
    std::vector<long long> entries;         // per member: log records the last call left (0: not launched)
    int flags = 0;                          // of gpf_ensemble_create2
    std::vector<int> tier;                  // per member: GPF_ENSEMBLE_TIER_LDS / _WORKSPACE, fixed at create
    std::vector<long long> ws_off;          // per member of the workspace tier: where its workspace starts in `ws`, in bytes
    char* ws = nullptr;                     // one device allocation for all workspaces (mid_layout.hpp)
    // the three series; the probes keep per member the step count of the first record of the last call beside theirs
    EnsembleSeries film, ext, probes;
    std::vector<long long> probes_first;
    std::array<EnsembleSeries*, 3> series() { return {&film, &ext, &probes}; }
    size_t args_off() const { return members.size() * sizeof(StepState); }
    size_t bytes() const { return args_off() + members.size() * (sizeof(SmallArgs) + sizeof(Phys) + sizeof(double*)); }
};
static_assert(sizeof(StepState) % 8 == 0 && sizeof(SmallArgs) % 8 == 0 && sizeof(Phys) % 8 == 0, "the four arrays share one allocation");

// The tier a member gets in an ensemble made with `flags`; -1, and the reason in *why, for one that no tier takes.
static int ensemble_member_tier(gpf_handle* h, int flags, std::string* why) {
    if (const char* no = one_workgroup_refusal(h)) { *why = no; return -1; }
    if (!(flags & GPF_ENSEMBLE_FORCE_WORKSPACE) && small_grid_fits_lds(h)) return GPF_ENSEMBLE_TIER_LDS;
    if (mid_cells(h->L.Nx, h->L.Ny) <= MID_GRID_MAX_CELLS) return GPF_ENSEMBLE_TIER_WORKSPACE;
    *why = "its grid does not fit one workgroup's LDS (16 doubles per cell, ghost cells included, in 150 KB) nor the workspace tier (at most " +
           std::to_string(MID_GRID_MAX_CELLS) + " cells, ghost cells included)";
    return -1;
}

// Why a member cannot be stepped in an ensemble right now; empty: it can.
static std::string ensemble_member_refusal(gpf_handle* h, gpf_handle* first, int flags) {
    std::string why;
    if (ensemble_member_tier(h, flags, &why) < 0) return why;
    if (h->cfg.device != first->cfg.device) return "it lives on device " + std::to_string(h->cfg.device) + ", member 0 on device " +
                                                   std::to_string(first->cfg.device) + " (one launch needs one device)";
    if (h->stream != first->stream) return "its stream differs from member 0's (one launch needs one stream)";
    // (spelled out, not walked from SERIES: the order differs from the table's, and the host tests of the series read these lines)
    if (h->integ.every) return "film integrals are armed on it (they cut the batch per member; gpf_integrals_clear, or step it alone)";
    if (h->weighted.every) return "weighted integrals are armed on it (they cut the batch per member; gpf_weighted_clear, or step it alone)";
    if (h->stats.every) return "statistics are armed on it (they cut the batch per member; gpf_stats_clear, or step it alone)";
    if (h->regions.every) return "regions are armed on it (they cut the batch per member; gpf_regions_clear, or step it alone)";
    if (h->lines.every) return "lines are armed on it (they cut the batch per member; gpf_lines_clear, or step it alone)";
    if (h->probes.n) return "probes are armed on it (their records need per-member slots; gpf_probes_clear, or step it alone)";
    if (h->extr.every) return "extrema are armed on it (their records need per-member slots; gpf_extrema_clear, or step it alone)";
    if (h->chg.every) return "changes are armed on it (they cut the batch per member; gpf_changes_clear, or step it alone)";
    if (h->frames.every) return "frames are armed on it (they cut the batch per member; gpf_frames_clear, or step it alone)";
    return "";
}

static int ensemble_member_check(const gpf_ensemble* e, int member, const char* who) {
    if (member >= 0 && member < (int)e->members.size()) return GPF_OK;
    return fail(GPF_ERR_INVALID, std::string(who) + ": member " + std::to_string(member) + " outside 0 .. " + std::to_string(e->members.size() - 1));
}

// ---- the ensemble's series ---------------------------------------------------------------------------------------------------------
// What is armed goes, with its buffers and the records on the host
static int ensemble_series_release(gpf_ensemble* e, EnsembleSeries& s) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->members[0]->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(s.owned()));
    s = EnsembleSeries();
    return GPF_OK;
}

// What every gpf_ensemble_*_set ends in, its checks passed: `fresh` holds the stride, the capacity and the layout; `image` is what
// `dev` shall hold -- the members' argument structs and whatever lies behind them --, complete but for the device addresses,
// which `patch(fresh)` writes into it once they are known.  Built first and swapped in last: on an error the ensemble stays as
// it was, the series that was armed included.
template <class Patch> static int ensemble_series_install(gpf_ensemble* e, EnsembleSeries& s, EnsembleSeries&& fresh, const char* who, void* image,
                                                          size_t image_bytes, Patch&& patch) {
    HIP_TRY(hipSetDevice(e->device));
    fresh.last.resize(e->members.size());
    hipError_t err = hipMalloc(&fresh.rec, fresh.at.total);
    if (err == hipSuccess) err = hipMalloc(&fresh.dev, image_bytes);
    if (err == hipSuccess) {
        patch(fresh);
        err = hipMemcpy(fresh.dev, image, image_bytes, hipMemcpyHostToDevice);
    }
    const int rc = err == hipSuccess ? ensemble_series_release(e, s) : fail(GPF_ERR_HIP, std::string(who) + ": " + hipGetErrorString(err));
    if (rc != GPF_OK) {
        (void)series_free(fresh.owned());
        return rc;
    }
    s = std::move(fresh);
    return GPF_OK;
}

// After a call's states have been read: member i's records of the `ran` steps it committed from step count `base` -> host.  The
// multiples of each stride in (base, base + ran], by its own ran (a member that stopped on the device ran a prefix of its steps;
// a rolled-back step left none); a probe record per committed step.  One copy per channel, each series whatever became of the others.
static int ensemble_collect(gpf_ensemble* e, int i, long long base, long long ran) {
    int rc = GPF_OK;
    for (EnsembleSeries* s : e->series()) {
        if (!s->every) continue;
        SeriesStore& r = s->last[i];
        // channel 0: doubles -> `host`; a series laid out with a second channel has int32 there -> `cells`
        const int got = s->at.channels() == 2 ? series_collect(s->every, r.steps, base, ran, s->device_channel(0, i, r.host), s->device_channel(1, i, r.cells))
                                              : series_collect(s->every, r.steps, base, ran, s->device_channel(0, i, r.host));
        if (got == GPF_OK) continue;
        r.forget();                                 // (series_append made room before the copy that failed)
        if (rc == GPF_OK) rc = fail(got, std::string("gpf_ensemble_step: ") + s->what + " record copy: " + g_err);
    }
    return rc;
}

extern "C" int gpf_ensemble_create(gpf_handle* const* members, int m, gpf_ensemble** out) {
    return gpf_ensemble_create2(members, m, 0, out);
}

extern "C" int gpf_ensemble_create2(gpf_handle* const* members, int m, int flags, gpf_ensemble** out) {
    if (!members || !out) return fail(GPF_ERR_INVALID, "gpf_ensemble_create: null argument");
    if (flags & ~GPF_ENSEMBLE_FORCE_WORKSPACE) return fail(GPF_ERR_INVALID, "gpf_ensemble_create2: flags = " + std::to_string(flags) + ", 0 or GPF_ENSEMBLE_FORCE_WORKSPACE required");
    if (m < 1) return fail(GPF_ERR_INVALID, "gpf_ensemble_create: an ensemble needs at least one member (m = " + std::to_string(m) + ")");
    for (int i = 0; i < m; ++i) {
        if (!members[i]) return fail(GPF_ERR_INVALID, "gpf_ensemble_create: member " + std::to_string(i) + " is a null handle");
        for (int j = 0; j < i; ++j)
            if (members[j] == members[i])
                return fail(GPF_ERR_INVALID, "gpf_ensemble_create: member " + std::to_string(i) + " is the same handle as member " +
                                             std::to_string(j) + " (two workgroups would write the same buffers)");
        const std::string why = ensemble_member_refusal(members[i], members[0], flags);
        if (!why.empty()) return fail(GPF_ERR_INVALID, "gpf_ensemble_create: member " + std::to_string(i) + ": " + why);
    }
    HIP_TRY(hipSetDevice(members[0]->cfg.device));
    gpf_ensemble* e = new gpf_ensemble();
    e->members.assign(members, members + m);
    e->device = members[0]->cfg.device;
    e->entries.assign(m, 0);
    e->probes_first.assign(m, 0);
    e->flags = flags;
    e->tier.assign(m, GPF_ENSEMBLE_TIER_LDS);
    e->ws_off.assign(m, 0);
    long long ws_bytes = 0;                 // every workspace a multiple of 256 bytes: each starts 256-byte aligned
    for (int i = 0; i < m; ++i) {
        std::string unused;
        e->tier[i] = ensemble_member_tier(members[i], flags, &unused);
        if (e->tier[i] != GPF_ENSEMBLE_TIER_WORKSPACE) continue;
        e->ws_off[i] = ws_bytes;
        ws_bytes += mid_workspace_bytes(mid_cells(members[i]->L.Nx, members[i]->L.Ny));
    }
    for (gpf_handle* h : e->members) ensemble_members_add(h);
    hipError_t err = hipMalloc(&e->dev, e->bytes());
    if (err == hipSuccess && ws_bytes > 0) err = hipMalloc(&e->ws, (size_t)ws_bytes);
    if (err == hipSuccess) err = hipHostMalloc((void**)&e->host, e->bytes(), hipHostMallocDefault);
    if (err != hipSuccess) {
        gpf_ensemble_destroy(e);
        return fail(GPF_ERR_HIP, std::string("gpf_ensemble_create: ") + hipGetErrorString(err));
    }
    *out = e;
    return GPF_OK;
}

extern "C" int gpf_ensemble_destroy(gpf_ensemble* e) {
    if (!e) return GPF_OK;
    for (gpf_handle* h : e->members) ensemble_members_drop(h, false);
    hipSetDevice(e->device);
    hipStreamSynchronize(e->members[0]->stream);        // a launch that records into the buffers below may still be queued
    for (EnsembleSeries* s : e->series())               // (errors are not reported here: series_destroy)
        for (void** p : s->owned())
            if (p && *p) (void)hipFree(*p);
    if (e->dev) hipFree(e->dev);
    if (e->ws) hipFree(e->ws);
    if (e->host) hipHostFree(e->host);
    delete e;
    return GPF_OK;
}

extern "C" int gpf_ensemble_step(gpf_ensemble* e, const int64_t* n, int honor_stop, int64_t* n_executed) {
    if (!e || !n) return fail(GPF_ERR_INVALID, "gpf_ensemble_step: null argument");
    const int m = (int)e->members.size();
    // every refusal before anything is touched: a call that fails leaves every member as it was
    for (int i = 0; i < m; ++i) {
        gpf_handle* h = e->members[i];
        const std::string who = "gpf_ensemble_step: member " + std::to_string(i) + ": ";
        if (n[i] < 0 || n[i] > h->log_cap)
            return fail(GPF_ERR_INVALID, who + "n = " + std::to_string((long long)n[i]) + ", 0 .. " + std::to_string(h->log_cap) + " (the log's capacity) required");
        if (n[i] == 0) continue;
        const std::string why = ensemble_member_refusal(h, e->members[0], e->flags);
        if (!why.empty()) return fail(GPF_ERR_INVALID, who + why);
        if (!h->pre_run_done) return fail(GPF_ERR_STATE, who + "call gpf_pre_run first (Problem._pre_run, problem.py:412)");
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t stream = e->members[0]->stream;
    // launch slots: the members to advance, grouped by kernel (tier) and instantiation (EOS, slip-length field or not), member
    // order within
    auto key = [&](int i) { return (e->tier[i] * 64 + e->members[i]->cfg.eos) * 2 + (e->members[i]->Ls ? 1 : 0); };
    std::vector<int>& slots = e->slot_member;
    slots.clear();
    for (int i = 0; i < m; ++i) {
        e->entries[i] = 0;
        if (n[i] > 0) slots.push_back(i);
        for (EnsembleSeries* s : e->series())
            if (s->every) s->last[i].forget();          // the records of the call before go
        if (e->probes.every) e->probes_first[i] = e->members[i]->host_step + 1;
    }
    std::stable_sort(slots.begin(), slots.end(), [&](int a, int b) { return key(a) < key(b); });
    const int nslots = (int)slots.size();
    const size_t args_bytes = (size_t)nslots * sizeof(SmallArgs), phys_bytes = (size_t)nslots * sizeof(Phys), ws_bytes = (size_t)nslots * sizeof(double*);
    StepState* hs = (StepState*)e->host;
    SmallArgs* ha = (SmallArgs*)(e->host + e->args_off());
    Phys* hp = (Phys*)(e->host + e->args_off() + args_bytes);
    double** hw = (double**)(e->host + e->args_off() + args_bytes + phys_bytes);
    StepState* ds = (StepState*)e->dev;
    SmallArgs* da = (SmallArgs*)(e->dev + e->args_off());
    Phys* dp = (Phys*)(e->dev + e->args_off() + args_bytes);
    double** dw = (double**)(e->dev + e->args_off() + args_bytes + phys_bytes);
    for (int s = 0; s < nslots; ++s) {
        gpf_handle* h = e->members[slots[s]];
        GPF_TRY(enter(h));
        SmallArgs& a = ha[s];
        a.qa = h->q[0]; a.qb = h->q[1]; a.topo = h->topo; a.Ls = h->Ls; a.st = h->st;
        a.log = h->log; a.log_base = h->host_step; a.log_cap = h->log_cap; a.L = h->L; a.E = h->E;
        a.nsteps = (int)n[slots[s]]; a.honor_stop = honor_stop;
        a.probe = e->probes.args<ProbeArgs>(slots[s]);
        a.extrema = e->ext.args<ExtremaArgs>(slots[s]);
        a.film = e->film.args<FilmBlockArgs>(slots[s]);
        hp[s] = h->P;
        hw[s] = e->tier[slots[s]] == GPF_ENSEMBLE_TIER_WORKSPACE ? (double*)(e->ws + e->ws_off[slots[s]]) : nullptr;
    }
    // Once a group has been launched its members have moved on the device, whatever happens next on the host: an error from
    // then on does not return at once.  No further group is launched, the states of the launched slots are read back and
    // those handles brought up to date as after a good call; then the error is returned.
    int rc = GPF_OK, launched = 0;
    auto hip_ok = [&](hipError_t err, const char* what) {
        if (err != hipSuccess && rc == GPF_OK) rc = fail(GPF_ERR_HIP, std::string("gpf_ensemble_step: ") + what + ": " + hipGetErrorString(err));
        return err == hipSuccess;
    };
    if (nslots > 0 && hip_ok(hipMemcpyAsync(da, ha, args_bytes + phys_bytes + ws_bytes, hipMemcpyHostToDevice, stream), "argument copy")) {   // one copy per call
        for (int s0 = 0; s0 < nslots && rc == GPF_OK;) {
            int s1 = s0;
            size_t lds = 0;
            while (s1 < nslots && key(slots[s1]) == key(slots[s0])) {
                const Layout& L = e->members[slots[s1]]->L;
                lds = std::max(lds, (size_t)(L.Nx + 2) * (L.Ny + 2) * SMALL_DOUBLES_PER_CELL * 8);     // the largest member's need
                ++s1;
            }
            gpf_handle* h0 = e->members[slots[s0]];
            const dim3 grid(s1 - s0);
            if (e->tier[slots[s0]] == GPF_ENSEMBLE_TIER_WORKSPACE) {
                EOS_DISPATCH(h0->cfg.eos, {
                    if (h0->Ls) hipLaunchKernelGGL((k_mid_ensemble<EOS_, true>), grid, dim3(MID_THREADS), 0, stream, da + s0, dp + s0, dw + s0, ds + s0);
                    else hipLaunchKernelGGL((k_mid_ensemble<EOS_, false>), grid, dim3(MID_THREADS), 0, stream, da + s0, dp + s0, dw + s0, ds + s0);
                });
            } else {
                EOS_DISPATCH(h0->cfg.eos, {
                    if (h0->Ls) {
                        if (hip_ok(hipFuncSetAttribute((const void*)k_small_ensemble<EOS_, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "LDS attribute"))
                            hipLaunchKernelGGL((k_small_ensemble<EOS_, true>), grid, dim3(512), lds, stream, da + s0, dp + s0, ds + s0);
                    } else {
                        if (hip_ok(hipFuncSetAttribute((const void*)k_small_ensemble<EOS_, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "LDS attribute"))
                            hipLaunchKernelGGL((k_small_ensemble<EOS_, false>), grid, dim3(512), lds, stream, da + s0, dp + s0, ds + s0);
                    }
                });
            }
            if (rc == GPF_OK && hip_ok(hipGetLastError(), "launch")) launched = s1;
            s0 = s1;
        }
        if (launched > 0) {
            const bool back = hip_ok(hipMemcpyAsync(hs, ds, (size_t)launched * sizeof(StepState), hipMemcpyDeviceToHost, stream), "state copy") &&
                              hip_ok(hipStreamSynchronize(stream), "synchronise");
            if (!back) launched = 0;            // the device no longer answers: gpf_state re-reads a member's count if it recovers
        }
    }
    // what gpf_step leaves in a handle after one batch (api.hip)
    for (int s = 0; s < launched; ++s) {
        const int i = slots[s];
        gpf_handle* h = e->members[i];
        const StepState& st = hs[s];
        const long long ran = st.step - h->host_step;
        e->entries[i] = ran + ((st.invalid && ran < n[i]) ? 1 : 0);
        const int rcol = ensemble_collect(e, i, h->host_step, ran);
        if (rc == GPF_OK) rc = rcol;
        h->host_step = st.step; h->next_step = st.step;
        prev_state_after(h, ran >= 1 && !st.invalid);
        h->g1_ready = false;
    }
    if (n_executed)
        for (int i = 0; i < m; ++i) n_executed[i] = e->members[i]->host_step;
    return rc;
}

extern "C" int gpf_ensemble_limits(int64_t* lds_bytes, int32_t* doubles_per_cell, int64_t* max_steps) {
    if (lds_bytes) *lds_bytes = SMALL_GRID_LDS_BYTES;
    if (doubles_per_cell) *doubles_per_cell = SMALL_DOUBLES_PER_CELL;
    if (max_steps) *max_steps = LOG_CAPACITY;
    return GPF_OK;
}

extern "C" int gpf_ensemble_limits2(int64_t* mid_max_cells, int32_t* mid_doubles_per_cell) {
    if (mid_max_cells) *mid_max_cells = MID_GRID_MAX_CELLS;
    if (mid_doubles_per_cell) *mid_doubles_per_cell = MID_DOUBLES_PER_CELL;
    return GPF_OK;
}

extern "C" int gpf_ensemble_member_info(gpf_ensemble* e, int member, int32_t* tier, int64_t* workspace_bytes) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_member_info: null argument");
    GPF_TRY(ensemble_member_check(e, member, "gpf_ensemble_member_info"));
    const bool ws = e->tier[member] == GPF_ENSEMBLE_TIER_WORKSPACE;
    if (tier) *tier = e->tier[member];
    if (workspace_bytes) *workspace_bytes = ws ? mid_workspace_bytes(mid_cells(e->members[member]->L.Nx, e->members[member]->L.Ny)) : 0;
    return GPF_OK;
}

extern "C" int gpf_ensemble_log(gpf_ensemble* e, int member, gpf_scalars_t* log, int64_t log_capacity, int64_t* n_entries) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_log: null argument");
    GPF_TRY(ensemble_member_check(e, member, "gpf_ensemble_log"));
    const long long have = e->entries[member];
    if (n_entries) *n_entries = have;
    const long long take = std::min<long long>(have, log ? log_capacity : 0);
    if (take > 0) {
        gpf_handle* h = e->members[member];
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipMemcpy(log, h->log, (size_t)take * sizeof(LogEntry), hipMemcpyDeviceToHost));
    }
    return GPF_OK;
}

// ---- film integrals (the record of gpf_integrals_*), extrema (that of gpf_extrema_*), point probes (that of gpf_probes_*) -------------
// k_small_ensemble records them on its LDS planes -- in every bit what the member's solo batch records --, k_mid_ensemble on its
// workspace planes.

extern "C" int gpf_ensemble_integrals_set(gpf_ensemble* e, int64_t every, int nsx, const int32_t* ix, int nsy, const int32_t* iy) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_set: null argument");
    if (every < 1) return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_set: every >= 1 required (gpf_ensemble_integrals_clear disarms), got " + std::to_string(every));
    if (nsx > FILM_MAX_SECTIONS || nsy > FILM_MAX_SECTIONS)
        return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_set: " + std::to_string(std::max(nsx, nsy)) + " sections given, at most " +
                                     std::to_string(FILM_MAX_SECTIONS) + " per direction");
    const int m = (int)e->members.size();
    // explicit sections are the same for everyone: they must lie inside every member's interior
    for (int i = 0; i < m; ++i) {
        const gpf_handle* h = e->members[i];
        const std::string who = "gpf_ensemble_integrals_set: member " + std::to_string(i);
        GPF_TRY(integrals_refusal(h, who));
        for (int k = 0; ix && k < nsx; ++k)
            if (ix[k] < 1 || ix[k] > h->L.Nx)
                return fail(GPF_ERR_INVALID, who + ": x-section " + std::to_string(k) + " at row " + std::to_string(ix[k]) +
                                             " lies outside its interior rows 1.." + std::to_string(h->L.Nx));
        for (int k = 0; iy && k < nsy; ++k)
            if (iy[k] < 1 || iy[k] > h->L.Ny)
                return fail(GPF_ERR_INVALID, who + ": y-section " + std::to_string(k) + " at column " + std::to_string(iy[k]) +
                                             " lies outside its interior columns 1.." + std::to_string(h->L.Ny));
    }
    EnsembleSeries f;
    f.what = "film";
    f.every = every;
    f.cap = LOG_CAPACITY / every + 1;               // series_count(base, ran, every) <= ran / every + 1
    std::vector<FilmBlockArgs> args(m);
    std::vector<size_t> record_bytes(m);
    for (int i = 0; i < m; ++i) {
        const gpf_handle* h = e->members[i];
        // default: first and last interior row / column, one where the extent is 1 (integrals_default_sections)
        int sx[FILM_MAX_SECTIONS] = {1, h->L.Nx}, sy[FILM_MAX_SECTIONS] = {1, h->L.Ny};
        int mx = h->L.Nx > 1 ? 2 : 1, my = h->L.Ny > 1 ? 2 : 1;
        if (ix && nsx > 0) { mx = nsx; for (int k = 0; k < nsx; ++k) sx[k] = ix[k]; }
        if (iy && nsy > 0) { my = nsy; for (int k = 0; k < nsy; ++k) sy[k] = iy[k]; }
        args[i] = film_block_args(nullptr, every, f.cap, h->cfg.dx, h->cfg.dy, mx, sx, my, sy);
        record_bytes[i] = (size_t)(FILM_NSUM + mx + my) * sizeof(double);
    }
    f.at = ensemble_slots({record_bytes}, std::vector<long long>(m, f.cap));
    return ensemble_series_install(e, e->film, std::move(f), "gpf_ensemble_integrals_set", args.data(), args.size() * sizeof(FilmBlockArgs),
                                   [&](const EnsembleSeries& s) { for (int i = 0; i < m; ++i) args[i].rec = (double*)(s.rec + s.at.at(0, i)); });
}

extern "C" int gpf_ensemble_integrals_clear(gpf_ensemble* e) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_clear: null argument");
    return ensemble_series_release(e, e->film);
}

extern "C" int gpf_ensemble_integrals_read(gpf_ensemble* e, int member, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!e || !n_records) return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_read: null argument (e and n_records are required)");
    GPF_TRY(ensemble_member_check(e, member, "gpf_ensemble_integrals_read"));
    if (!e->film.every) return fail(GPF_ERR_STATE, "gpf_ensemble_integrals_read: no integrals are armed (gpf_ensemble_integrals_set)");
    SeriesStore& r = e->film.last[member];
    series_read(r.steps, capacity_records, steps_out, n_records, e->film.read_channel(0, member, r.host, out));
    return GPF_OK;
}

extern "C" int gpf_ensemble_extrema_set(gpf_ensemble* e, int64_t every) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_set: null argument");
    if (every < 1) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_set: every >= 1 required (gpf_ensemble_extrema_clear disarms), got " + std::to_string(every));
    const int m = (int)e->members.size();
    for (int i = 0; i < m; ++i) GPF_TRY(extrema_refusal(e->members[i], "gpf_ensemble_extrema_set: member " + std::to_string(i)));
    EnsembleSeries x;
    x.what = "extrema";
    x.every = every;
    x.cap = LOG_CAPACITY / every + 1;               // series_count(base, ran, every) <= ran / every + 1
    // the values of all members ([m][cap][7] doubles), then their cells ([m][cap][7][2] ints)
    x.at = ensemble_slots({std::vector<size_t>(m, EXTREMA_NQ * sizeof(double)), std::vector<size_t>(m, 2 * EXTREMA_NQ * sizeof(int))},
                          std::vector<long long>(m, x.cap));
    std::vector<ExtremaArgs> args(m);
    for (ExtremaArgs& a : args) {
        a.row_val = nullptr; a.row_iy = nullptr;    // k_extrema_partial's: no launch of it here (both kernels fold inside the workgroup)
        a.every = every; a.cap = x.cap;
    }
    return ensemble_series_install(e, e->ext, std::move(x), "gpf_ensemble_extrema_set", args.data(), args.size() * sizeof(ExtremaArgs),
                                   [&](const EnsembleSeries& s) {
                                       for (int i = 0; i < m; ++i) { args[i].val = (double*)(s.rec + s.at.at(0, i)); args[i].cell = (int*)(s.rec + s.at.at(1, i)); }
                                   });
}

extern "C" int gpf_ensemble_extrema_clear(gpf_ensemble* e) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_clear: null argument");
    return ensemble_series_release(e, e->ext);
}

extern "C" int gpf_ensemble_extrema_read(gpf_ensemble* e, int member, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out,
                                         int64_t* n_records) {
    if (!e || !n_records) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_read: null argument (e and n_records are required)");
    GPF_TRY(ensemble_member_check(e, member, "gpf_ensemble_extrema_read"));
    if (!e->ext.every) return fail(GPF_ERR_STATE, "gpf_ensemble_extrema_read: no extrema are armed (gpf_ensemble_extrema_set)");
    SeriesStore& r = e->ext.last[member];
    series_read(r.steps, capacity_records, steps_out, n_records, e->ext.read_channel(0, member, r.host, values), e->ext.read_channel(1, member, r.cells, cells));
    return GPF_OK;
}

// The most bytes the probe records of an ensemble may take on the device: GPF_ENSEMBLE_PROBES_MB (MiB, read at every set), 256
static size_t ensemble_probes_budget() {
    const char* s = std::getenv("GPF_ENSEMBLE_PROBES_MB");
    const long long mb = s ? std::atoll(s) : 0;
    return (size_t)(mb > 0 ? mb : 256) << 20;
}

extern "C" int gpf_ensemble_probes_set(gpf_ensemble* e, int per_member, const int32_t* nprobe, const int32_t* cells, int with_pressure) {
    if (!e || !nprobe || !cells) return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_set: null argument");
    const int m = (int)e->members.size();
    const int nv = with_pressure ? 4 : 3;
    std::vector<int> count(m);
    std::vector<size_t> first_cell(m), record_bytes(m);     // where member i's cells start in `cells`, in cells; its n x nv doubles
    std::vector<long long> cap(m);                          // a record per step of the longest call
    size_t ncells = 0;
    for (int i = 0; i < m; ++i) {
        const gpf_handle* h = e->members[i];
        const std::string who = "gpf_ensemble_probes_set: member " + std::to_string(i);
        GPF_TRY(probes_refusal(h, who));
        if (with_pressure) GPF_TRY(probes_pressure_refusal(h, who));
        const int n = nprobe[per_member ? i : 0];
        if (n < 1) return fail(GPF_ERR_INVALID, who + ": n >= 1 cells required (gpf_ensemble_probes_clear removes them), got " + std::to_string(n));
        if (n > PROBE_MAX)
            return fail(GPF_ERR_INVALID, who + ": probe " + std::to_string(PROBE_MAX) + " is one too many (" + std::to_string(n) + " given, at most " +
                                         std::to_string(PROBE_MAX) + " per member)");
        first_cell[i] = per_member ? ncells : 0;
        const int32_t* c = cells + 2 * first_cell[i];
        for (int k = 0; k < n; ++k)
            if (c[2 * k] < 0 || c[2 * k] > h->L.Nx + 1 || c[2 * k + 1] < 0 || c[2 * k + 1] > h->L.Ny + 1)
                return fail(GPF_ERR_INVALID, who + ": probe " + std::to_string(k) + " at cell (" + std::to_string(c[2 * k]) + ", " + std::to_string(c[2 * k + 1]) +
                                             ") lies outside 0.." + std::to_string(h->L.Nx + 1) + " x 0.." + std::to_string(h->L.Ny + 1));
        count[i] = n;
        ncells = per_member ? ncells + (size_t)n : (size_t)n;
        record_bytes[i] = (size_t)n * (size_t)nv * sizeof(double);
        cap[i] = h->log_cap;
    }
    EnsembleSeries p;
    p.what = "probe";
    p.every = 1;                                    // (cap stays 0: per member, below)
    p.at = ensemble_slots({record_bytes}, cap);
    const size_t need = p.at.total, budget = ensemble_probes_budget();
    if (need > budget)
        return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_set: the records of one call need " + std::to_string(need) + " bytes of device memory (" +
                                     std::to_string(LOG_CAPACITY) + " steps x probes x values x 8 per member), more than the budget of " +
                                     std::to_string(budget) + " bytes (GPF_ENSEMBLE_PROBES_MB, in MiB; default 256)");
    // ProbeArgs[m], then the cells: one small allocation, one copy
    std::vector<char> image((size_t)m * sizeof(ProbeArgs) + ncells * 2 * sizeof(int));
    ProbeArgs* args = (ProbeArgs*)image.data();
    for (int i = 0; i < m; ++i) {
        args[i].nprobe = count[i]; args[i].nv = nv;
        args[i].base = 0; args[i].cap = cap[i];     // (the one-workgroup kernels take both from their own arguments)
    }
    std::memcpy(image.data() + (size_t)m * sizeof(ProbeArgs), cells, ncells * 2 * sizeof(int));
    GPF_TRY(ensemble_series_install(e, e->probes, std::move(p), "gpf_ensemble_probes_set", image.data(), image.size(), [&](const EnsembleSeries& s) {
        const int* dev_cells = (const int*)(s.dev + (size_t)m * sizeof(ProbeArgs));
        for (int i = 0; i < m; ++i) { args[i].cells = dev_cells + 2 * first_cell[i]; args[i].out = (double*)(s.rec + s.at.at(0, i)); }
    }));
    e->probes_first.assign(m, 0);
    return GPF_OK;
}

extern "C" int gpf_ensemble_probes_clear(gpf_ensemble* e) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_clear: null argument");
    return ensemble_series_release(e, e->probes);
}

extern "C" int gpf_ensemble_probes_read(gpf_ensemble* e, int member, double* out, int64_t capacity_records, int64_t* first_step, int64_t* n_records) {
    if (!e || !n_records) return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_read: null argument (e and n_records are required)");
    GPF_TRY(ensemble_member_check(e, member, "gpf_ensemble_probes_read"));
    if (!e->probes.every) return fail(GPF_ERR_STATE, "gpf_ensemble_probes_read: no probes are set (gpf_ensemble_probes_set)");
    SeriesStore& r = e->probes.last[member];
    series_read(r.steps, capacity_records, nullptr, n_records, e->probes.read_channel(0, member, r.host, out));
    if (first_step) *first_step = e->probes_first[member];      // the member's step count at the start of the call + 1, record or none
    return GPF_OK;
}
