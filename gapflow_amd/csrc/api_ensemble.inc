// Ensembles (gpf_ensemble_*): many small problems advanced by one launch per kernel instantiation, one workgroup per member.
// Two tiers: a member that fits one workgroup's LDS runs k_small_ensemble (small_kernel.hip); one of up to MID_GRID_MAX_CELLS
// cells runs k_mid_ensemble (mid_kernel.hip) on a workspace in device memory that the ensemble owns.  Part of api.hip's
// translation unit.
//
// A member is a handle of its own, borrowed: everything a solo gpf_step of the same count would leave in it -- buffers, run
// state, log, host_step / next_step, prev_state_valid, g1_ready -- is left in it here, so that it can go on alone.
//
// Film-integral series (gpf_ensemble_integrals_*) belong to the ENSEMBLE, not to its members: both kernels record them inside
// the batch (integral_kernels.hip: film_record_block) into per-member slots that the ensemble owns, so nothing cuts a launch.

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
    // film-integral series: stride (0: not armed); per member its sections, doubles per record and where its records start in
    // `rec` (one device allocation, `cap` records per member: what a call of at most LOG_CAPACITY steps can leave at the stride);
    // the members' FilmBlockArgs in device memory ([m]); the records of the last gpf_ensemble_step and their step counts on the host
    struct Film {
        long long every = 0, cap = 0;
        std::vector<FilmBlockArgs> args;
        std::vector<size_t> off;
        double* rec = nullptr;
        FilmBlockArgs* dev = nullptr;
        std::vector<std::vector<double>> host;
        std::vector<std::vector<long long>> steps;
        int nrec(int i) const { return FILM_NSUM + args[i].nsx + args[i].nsy; }
    } film;
    // field-extrema series, the same way: stride (0: not armed), `cap` records per member in ONE device allocation `rec` -- the
    // values of all members ([m][cap][7] doubles), then their cells ([m][cap][7][2] ints) --, the members' ExtremaArgs in device
    // memory ([m]; no row scratch: both kernels fold inside the workgroup), the records of the last gpf_ensemble_step on the host
    struct Extrema {
        long long every = 0, cap = 0;
        char* rec = nullptr;
        ExtremaArgs* dev = nullptr;
        std::vector<std::vector<double>> host;
        std::vector<std::vector<int32_t>> cells;
        std::vector<std::vector<long long>> steps;
        double* val(int i) const { return (double*)rec + (size_t)i * cap * EXTREMA_NQ; }
        int* cell(size_t m, int i) const { return (int*)((double*)rec + m * cap * EXTREMA_NQ) + (size_t)i * cap * 2 * EXTREMA_NQ; }
    } ext;
    // point probes: per member its count (empty: not armed) and where its records start in `out` (ONE device allocation, log_cap
    // records of n[i] x nv doubles per member: a record per committed step); `dev`: the members' ProbeArgs ([m]) and behind them
    // everyone's cells, in device memory; the records of the last gpf_ensemble_step on the host and the step count of the first
    struct Probes {
        std::vector<int> n;
        int nv = 0;
        std::vector<size_t> off;
        double* out = nullptr;
        ProbeArgs* dev = nullptr;
        std::vector<std::vector<double>> host;
        std::vector<long long> first;
        bool armed() const { return !n.empty(); }
    } probes;
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
    if (e->film.rec) hipFree(e->film.rec);
    if (e->film.dev) hipFree(e->film.dev);
    if (e->ext.rec) hipFree(e->ext.rec);
    if (e->ext.dev) hipFree(e->ext.dev);
    if (e->probes.out) hipFree(e->probes.out);
    if (e->probes.dev) hipFree(e->probes.dev);
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
        if (e->film.every) { e->film.host[i].clear(); e->film.steps[i].clear(); }      // the records of the call before go
        if (e->ext.every) { e->ext.host[i].clear(); e->ext.cells[i].clear(); e->ext.steps[i].clear(); }
        if (e->probes.armed()) { e->probes.host[i].clear(); e->probes.first[i] = e->members[i]->host_step + 1; }
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
        a.probe = e->probes.armed() ? e->probes.dev + slots[s] : nullptr;
        a.extrema = e->ext.every ? e->ext.dev + slots[s] : nullptr;
        a.film = e->film.every ? e->film.dev + slots[s] : nullptr;
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
        // the member's film records: the multiples of the stride in (base, base + ran], by its own ran (a member that stopped on
        // the device ran a prefix of its steps; a rolled-back step left none)
        const long long cnt = e->film.every ? series_count(h->host_step, ran, e->film.every) : 0;
        if (cnt > 0) {
            const size_t nrec = (size_t)e->film.nrec(i);
            std::vector<double> got((size_t)cnt * nrec);
            if (hip_ok(hipMemcpy(got.data(), e->film.rec + e->film.off[i], got.size() * sizeof(double), hipMemcpyDeviceToHost), "film record copy")) {
                e->film.host[i].swap(got);
                for (long long k = 1; k <= cnt; ++k) e->film.steps[i].push_back((h->host_step / e->film.every + k) * e->film.every);
            }
        }
        // its extrema records likewise (values and cells), and a probe record per committed step
        const long long ecnt = e->ext.every ? series_count(h->host_step, ran, e->ext.every) : 0;
        if (ecnt > 0) {
            std::vector<double> val((size_t)ecnt * EXTREMA_NQ);
            std::vector<int32_t> cell((size_t)ecnt * 2 * EXTREMA_NQ);
            if (hip_ok(hipMemcpy(val.data(), e->ext.val(i), val.size() * sizeof(double), hipMemcpyDeviceToHost), "extrema record copy") &&
                hip_ok(hipMemcpy(cell.data(), e->ext.cell((size_t)m, i), cell.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "extrema record copy")) {
                e->ext.host[i].swap(val);
                e->ext.cells[i].swap(cell);
                for (long long k = 1; k <= ecnt; ++k) e->ext.steps[i].push_back((h->host_step / e->ext.every + k) * e->ext.every);
            }
        }
        if (e->probes.armed() && ran > 0) {
            std::vector<double> got((size_t)ran * e->probes.n[i] * e->probes.nv);
            if (hip_ok(hipMemcpy(got.data(), e->probes.out + e->probes.off[i], got.size() * sizeof(double), hipMemcpyDeviceToHost), "probe record copy"))
                e->probes.host[i].swap(got);
        }
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
    if (member < 0 || member >= (int)e->members.size())
        return fail(GPF_ERR_INVALID, "gpf_ensemble_member_info: member " + std::to_string(member) + " outside 0 .. " + std::to_string(e->members.size() - 1));
    const bool ws = e->tier[member] == GPF_ENSEMBLE_TIER_WORKSPACE;
    if (tier) *tier = e->tier[member];
    if (workspace_bytes) *workspace_bytes = ws ? mid_workspace_bytes(mid_cells(e->members[member]->L.Nx, e->members[member]->L.Ny)) : 0;
    return GPF_OK;
}

extern "C" int gpf_ensemble_log(gpf_ensemble* e, int member, gpf_scalars_t* log, int64_t log_capacity, int64_t* n_entries) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_log: null argument");
    if (member < 0 || member >= (int)e->members.size())
        return fail(GPF_ERR_INVALID, "gpf_ensemble_log: member " + std::to_string(member) + " outside 0 .. " + std::to_string(e->members.size() - 1));
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

static int ensemble_film_release(gpf_ensemble* e) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->members[0]->stream));       // a recording launch may still be queued
    if (e->film.rec) HIP_TRY(hipFree(e->film.rec));
    e->film.rec = nullptr;
    if (e->film.dev) HIP_TRY(hipFree(e->film.dev));
    e->film.dev = nullptr;
    e->film = gpf_ensemble::Film();
    return GPF_OK;
}

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
    GPF_TRY(ensemble_film_release(e));
    gpf_ensemble::Film f;
    f.every = every;
    f.cap = LOG_CAPACITY / every + 1;               // series_count(base, ran, every) <= ran / every + 1
    f.args.resize(m); f.off.resize(m); f.host.resize(m); f.steps.resize(m);
    size_t total = 0;
    for (int i = 0; i < m; ++i) {
        const gpf_handle* h = e->members[i];
        // default: first and last interior row / column, one where the extent is 1 (integrals_default_sections)
        int sx[FILM_MAX_SECTIONS] = {1, h->L.Nx}, sy[FILM_MAX_SECTIONS] = {1, h->L.Ny};
        int mx = h->L.Nx > 1 ? 2 : 1, my = h->L.Ny > 1 ? 2 : 1;
        if (ix && nsx > 0) { mx = nsx; for (int k = 0; k < nsx; ++k) sx[k] = ix[k]; }
        if (iy && nsy > 0) { my = nsy; for (int k = 0; k < nsy; ++k) sy[k] = iy[k]; }
        f.args[i] = film_block_args(nullptr, every, f.cap, h->cfg.dx, h->cfg.dy, mx, sx, my, sy);
        f.off[i] = total;
        total += (size_t)f.cap * (size_t)(FILM_NSUM + mx + my);
    }
    hipError_t err = hipMalloc(&f.rec, total * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&f.dev, (size_t)m * sizeof(FilmBlockArgs));
    for (int i = 0; i < m; ++i) f.args[i].rec = f.rec ? f.rec + f.off[i] : nullptr;
    if (err == hipSuccess) err = hipMemcpy(f.dev, f.args.data(), (size_t)m * sizeof(FilmBlockArgs), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        if (f.rec) (void)hipFree(f.rec);
        if (f.dev) (void)hipFree(f.dev);
        return fail(GPF_ERR_HIP, std::string("gpf_ensemble_integrals_set: ") + hipGetErrorString(err));
    }
    e->film = std::move(f);
    return GPF_OK;
}

extern "C" int gpf_ensemble_integrals_clear(gpf_ensemble* e) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_clear: null argument");
    return ensemble_film_release(e);
}

extern "C" int gpf_ensemble_integrals_read(gpf_ensemble* e, int member, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records) {
    if (!e || !n_records) return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_read: null argument (e and n_records are required)");
    if (member < 0 || member >= (int)e->members.size())
        return fail(GPF_ERR_INVALID, "gpf_ensemble_integrals_read: member " + std::to_string(member) + " outside 0 .. " + std::to_string(e->members.size() - 1));
    if (!e->film.every) return fail(GPF_ERR_STATE, "gpf_ensemble_integrals_read: no integrals are armed (gpf_ensemble_integrals_set)");
    const size_t nrec = (size_t)e->film.nrec(member);
    const int64_t have = (int64_t)e->film.steps[member].size(), take = std::max<int64_t>(0, std::min(have, capacity_records));
    *n_records = have;
    if (out && take > 0) std::memcpy(out, e->film.host[member].data(), (size_t)take * nrec * sizeof(double));
    for (int64_t k = 0; steps_out && k < take; ++k) steps_out[k] = e->film.steps[member][(size_t)k];
    return GPF_OK;
}

// ---- the ensemble's extrema series (the record of gpf_extrema_*) and point probes (that of gpf_probes_*) -------------------------
// Both kernels write them inside the batch, behind each commit: k_small_ensemble through extrema_record_block / probe_record_block
// on its LDS planes -- in every bit what the member's solo batch records --, k_mid_ensemble through extrema_record_wide /
// probe_record_block on its workspace planes.

static int ensemble_extrema_release(gpf_ensemble* e) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->members[0]->stream));       // a recording launch may still be queued
    if (e->ext.rec) HIP_TRY(hipFree(e->ext.rec));
    e->ext.rec = nullptr;
    if (e->ext.dev) HIP_TRY(hipFree(e->ext.dev));
    e->ext.dev = nullptr;
    e->ext = gpf_ensemble::Extrema();
    return GPF_OK;
}

extern "C" int gpf_ensemble_extrema_set(gpf_ensemble* e, int64_t every) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_set: null argument");
    if (every < 1) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_set: every >= 1 required (gpf_ensemble_extrema_clear disarms), got " + std::to_string(every));
    const int m = (int)e->members.size();
    for (int i = 0; i < m; ++i) GPF_TRY(extrema_refusal(e->members[i], "gpf_ensemble_extrema_set: member " + std::to_string(i)));
    HIP_TRY(hipSetDevice(e->device));
    gpf_ensemble::Extrema x;
    x.every = every;
    x.cap = LOG_CAPACITY / every + 1;               // series_count(base, ran, every) <= ran / every + 1
    x.host.resize(m); x.cells.resize(m); x.steps.resize(m);
    const size_t per = (size_t)x.cap * EXTREMA_NQ;
    hipError_t err = hipMalloc(&x.rec, (size_t)m * per * (sizeof(double) + 2 * sizeof(int)));
    if (err == hipSuccess) err = hipMalloc(&x.dev, (size_t)m * sizeof(ExtremaArgs));
    std::vector<ExtremaArgs> args(m);
    for (int i = 0; i < m && err == hipSuccess; ++i) {
        args[i].val = x.val(i); args[i].cell = x.cell((size_t)m, i);
        args[i].row_val = nullptr; args[i].row_iy = nullptr;        // k_extrema_partial's: no launch of it here
        args[i].every = every; args[i].cap = x.cap;
    }
    if (err == hipSuccess) err = hipMemcpy(x.dev, args.data(), (size_t)m * sizeof(ExtremaArgs), hipMemcpyHostToDevice);
    if (err != hipSuccess) {                        // the ensemble stays as it was
        if (x.rec) (void)hipFree(x.rec);
        if (x.dev) (void)hipFree(x.dev);
        return fail(GPF_ERR_HIP, std::string("gpf_ensemble_extrema_set: ") + hipGetErrorString(err));
    }
    const int rc = ensemble_extrema_release(e);
    if (rc != GPF_OK) {
        (void)hipFree(x.rec); (void)hipFree(x.dev);
        return rc;
    }
    e->ext = std::move(x);
    return GPF_OK;
}

extern "C" int gpf_ensemble_extrema_clear(gpf_ensemble* e) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_clear: null argument");
    return ensemble_extrema_release(e);
}

extern "C" int gpf_ensemble_extrema_read(gpf_ensemble* e, int member, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out,
                                         int64_t* n_records) {
    if (!e || !n_records) return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_read: null argument (e and n_records are required)");
    if (member < 0 || member >= (int)e->members.size())
        return fail(GPF_ERR_INVALID, "gpf_ensemble_extrema_read: member " + std::to_string(member) + " outside 0 .. " + std::to_string(e->members.size() - 1));
    if (!e->ext.every) return fail(GPF_ERR_STATE, "gpf_ensemble_extrema_read: no extrema are armed (gpf_ensemble_extrema_set)");
    const int64_t have = (int64_t)e->ext.steps[member].size(), take = std::max<int64_t>(0, std::min(have, capacity_records));
    *n_records = have;
    if (values && take > 0) std::memcpy(values, e->ext.host[member].data(), (size_t)take * EXTREMA_NQ * sizeof(double));
    if (cells && take > 0) std::memcpy(cells, e->ext.cells[member].data(), (size_t)take * 2 * EXTREMA_NQ * sizeof(int32_t));
    for (int64_t k = 0; steps_out && k < take; ++k) steps_out[k] = e->ext.steps[member][(size_t)k];
    return GPF_OK;
}

static int ensemble_probes_release(gpf_ensemble* e) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->members[0]->stream));       // a recording launch may still be queued
    if (e->probes.out) HIP_TRY(hipFree(e->probes.out));
    e->probes.out = nullptr;
    if (e->probes.dev) HIP_TRY(hipFree(e->probes.dev));
    e->probes.dev = nullptr;
    e->probes = gpf_ensemble::Probes();
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
    gpf_ensemble::Probes p;
    p.n.resize(m); p.off.resize(m); p.host.resize(m); p.first.assign(m, 0);
    p.nv = with_pressure ? 4 : 3;
    std::vector<size_t> first_cell(m);              // where member i's cells start in `cells`, in cells
    size_t ncells = 0, total = 0;
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
        p.n[i] = n;
        p.off[i] = total;
        ncells = per_member ? ncells + (size_t)n : (size_t)n;
        total += (size_t)h->log_cap * (size_t)n * (size_t)p.nv;     // a record per step of the longest call
    }
    const size_t need = total * sizeof(double), budget = ensemble_probes_budget();
    if (need > budget)
        return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_set: the records of one call need " + std::to_string(need) + " bytes of device memory (" +
                                     std::to_string(LOG_CAPACITY) + " steps x probes x values x 8 per member), more than the budget of " +
                                     std::to_string(budget) + " bytes (GPF_ENSEMBLE_PROBES_MB, in MiB; default 256)");
    HIP_TRY(hipSetDevice(e->device));
    // ProbeArgs[m], then the cells: one small allocation, one copy
    std::vector<char> image((size_t)m * sizeof(ProbeArgs) + ncells * 2 * sizeof(int));
    hipError_t err = hipMalloc(&p.out, need);
    if (err == hipSuccess) err = hipMalloc(&p.dev, image.size());
    if (err == hipSuccess) {
        const int* dev_cells = (const int*)((char*)p.dev + (size_t)m * sizeof(ProbeArgs));
        ProbeArgs* args = (ProbeArgs*)image.data();
        for (int i = 0; i < m; ++i) {
            args[i].cells = dev_cells + 2 * first_cell[i];
            args[i].out = p.out + p.off[i];
            args[i].nprobe = p.n[i]; args[i].nv = p.nv;
            args[i].base = 0; args[i].cap = e->members[i]->log_cap;     // (the one-workgroup kernels take both from their own arguments)
        }
        std::memcpy(image.data() + (size_t)m * sizeof(ProbeArgs), cells, ncells * 2 * sizeof(int));
        err = hipMemcpy(p.dev, image.data(), image.size(), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) {                        // the ensemble stays as it was
        if (p.out) (void)hipFree(p.out);
        if (p.dev) (void)hipFree(p.dev);
        return fail(GPF_ERR_HIP, std::string("gpf_ensemble_probes_set: ") + hipGetErrorString(err));
    }
    const int rc = ensemble_probes_release(e);
    if (rc != GPF_OK) {
        (void)hipFree(p.out); (void)hipFree(p.dev);
        return rc;
    }
    e->probes = std::move(p);
    return GPF_OK;
}

extern "C" int gpf_ensemble_probes_clear(gpf_ensemble* e) {
    if (!e) return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_clear: null argument");
    return ensemble_probes_release(e);
}

extern "C" int gpf_ensemble_probes_read(gpf_ensemble* e, int member, double* out, int64_t capacity_records, int64_t* first_step, int64_t* n_records) {
    if (!e || !n_records) return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_read: null argument (e and n_records are required)");
    if (member < 0 || member >= (int)e->members.size())
        return fail(GPF_ERR_INVALID, "gpf_ensemble_probes_read: member " + std::to_string(member) + " outside 0 .. " + std::to_string(e->members.size() - 1));
    if (!e->probes.armed()) return fail(GPF_ERR_STATE, "gpf_ensemble_probes_read: no probes are set (gpf_ensemble_probes_set)");
    const size_t per = (size_t)e->probes.n[member] * e->probes.nv;
    const int64_t have = (int64_t)(e->probes.host[member].size() / per), take = std::max<int64_t>(0, std::min(have, capacity_records));
    *n_records = have;
    if (first_step) *first_step = e->probes.first[member];
    if (out && take > 0) std::memcpy(out, e->probes.host[member].data(), (size_t)take * per * sizeof(double));
    return GPF_OK;
}
