// Included by api.hip: what a large handle decides by measurement before its first step -- waves per SIMD, cache hints, and which
// buffers its state lives in (plan_step2, plan_placement, plan_trial).

constexpr int K2_LONG_MARCH_ROWS = 100;    // rows per wave from which plan_step2 runs one wave per SIMD instead of two

// One wave marches over one row chunk of one 126-column strip; the chunks are sized so that all waves are resident at
// once (a single round, no tail) when the problem is big enough: two waves per SIMD, or one.
static int plan_apply(gpf_handle* h, int nchunks, int nt, int keep = 0) {
    const Layout& L = h->L;
    const int nstrips = std::max(h->geom2[0].nstrips, h->geom2[1].nstrips);
    nchunks = std::max(1, std::min(nchunks, std::max(1, L.Nx / 4)));        // small grids: >= 4 rows per chunk
    h->nchunks2 = nchunks;
    h->nt_policy2 = nt;
    h->keep_rows2 = nt >= 1 ? std::max(0, std::min(7, keep)) : 0;
    const int nwaves = nstrips * nchunks;
    h->nblocks2 = (((nwaves + 3) / 4) + 7) / 8 * 8;
    if (nwaves > h->npartials2_cap) {
        if (h->partials) HIP_TRY(hipFree(h->partials));
        h->partials = nullptr;
        HIP_TRY(hipMalloc(&h->partials, (size_t)nwaves * sizeof(Partial)));
        HIP_TRY(hipMemset(h->partials, 0, (size_t)nwaves * sizeof(Partial)));
        h->npartials2_cap = nwaves;
    }
    if (h->nblocks2 > h->nblock_partials_cap) {
        const int cap = std::max(1024, h->nblocks2);
        if (h->block_partials) HIP_TRY(hipFree(h->block_partials));
        h->block_partials = nullptr;
        HIP_TRY(hipMalloc(&h->block_partials, (size_t)cap * sizeof(Partial)));
        h->nblock_partials_cap = cap;
    }
    return GPF_OK;
}

static void fill_step2_args(gpf_handle* h, Step2Args& a2, int D, int honor_stop, long long log_base, double* slab_out, bool p2p);

// Mean duration (us) of the fused step with the plan in force, on the handle's own field: the launches read the current state and
// write the OTHER buffer (dead until the next step overwrites it) and commit into a copy of the run state, which is reset before
// every launch -- nothing the solver will read changes.  `both`: every other launch runs the other way round, reading what the
// launch before has written and overwriting the current state (a step reads q[0] and writes q[1], the next one q[1] and q[0], and
// the two can differ by 10 %: it is the buffer WRITTEN that counts); the state is restored from h->plan_master afterwards.
static int plan_trial(gpf_handle* h, int D, float* us, int reps = 6, bool both = false) {
    static const int parity_value[2] = {0, 1};
    if (!h->st_trial) HIP_TRY(hipMalloc(&h->st_trial, sizeof(StepState)));
    prev_state_lost(h, PREV_LOST_PLAN);     // the launches below overwrite the other buffer
    both = both && h->plan_master != nullptr;
    int par = 0;
    if (both) GPF_TRY(current_parity(h, &par));
    Step2Args a2;
    fill_step2_args(h, a2, D, 0, 0, nullptr, false);
    a2.st = h->st_trial; a2.log = nullptr;
    const step2_kernel_t k2 = step2_kernel(h->cfg.eos, h->Ls != nullptr, h->cfg.piezo != 0, D, topo_mode_of(h));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    float total = 0.f;
    for (int r = -1; r < reps; ++r) {       // r = -1: warm-up, not timed
        HIP_TRY(hipMemcpyAsync(h->st_trial, h->st, sizeof(StepState), hipMemcpyDeviceToDevice, h->stream));
        if (both && ((r + 1) & 1))
            HIP_TRY(hipMemcpyAsync(&h->st_trial->parity, &parity_value[par ^ 1], sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipEventRecord(e0, h->stream));
        hipLaunchKernelGGL(k2, dim3(h->nblocks2), dim3(256), 0, h->stream, a2, h->P);
        HIP_TRY(hipEventRecord(e1, h->stream));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) total += ms;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (both) GPF_TRY(field_copy(h->stream, h->q[par], h->plan_master, h->field_bytes));
    HIP_TRY(hipGetLastError());
    *us = total / reps * 1e3f;
    return GPF_OK;
}

// WHERE the fields lie in device memory.  The same kernel on the same device runs at two speeds -- e.g. 167 or 183 us at 4096^2,
// 234 or 275 us with the gap planes -- depending on which physical pages the allocator happened to hand out for the buffers it
// reads and writes: twelve identical handles of one process, with identical virtual layouts, split 1 : 11 in one run and 5 : 7 in
// another, each handle keeping its speed for as long as it lives (tools/ab_inprocess.py, profiles/r03_placement/).  Offsets between
// the buffers, one allocation instead of three and the plane stride were scanned without finding the rule, and physically
// contiguous memory is the slowest of all, so large grids do what the plan does: they TRY.  A few spare buffers join the handle's own
// in a pool.  Most of what distinguishes the buffers shows when they are WRITTEN (profiles/r03_placement/pair_matrices.txt: one
// column of the read x written matrix stands out, not one row), so the step is first timed writing each buffer of the pool in
// turn; then, for the best four, for every ordered (read, written) pair -- a step reads one state buffer and writes the other, the
// next one the other way round, so a pair's figure is the sum of both directions.  The best pair becomes the handle's memory, then
// (kernels that read the gap planes) the best home among a few of the remaining buffers for those; the rest is freed.  With S spares:
// S + 2 + 12 trials of 7 launches and S + 1 buffers of transient memory (whole triples, as first tried: S trials for 3 S buffers).
// GPF_PLACEMENT_TRIES sets S (default: 24, and twelve more for as long as the last twelve still paid, up to 60 -- on one box 10 / 30 / 60
// spares ended at 155.1, 152.6 / 151.1, 151.4 / 150.9 us per step in separate processes; 0: keep the handle's own buffers);
// GPF_PLACEMENT_PRINT=1 prints the figures.
// the best write-scan figure any handle of this process has seen for a kernel and a grid (us; 0: none yet); `mine` > 0 records one
static float placement_best_seen(const gpf_handle* h, int D, float mine) {
    static std::mutex lock;
    static std::map<std::tuple<int, int, int, int, int, int, int>, float> seen;
    const auto key = std::make_tuple(h->L.Nx, h->L.Ny, h->cfg.eos, topo_mode_of(h), D, h->Ls ? 1 : 0, h->cfg.piezo != 0 ? 1 : 0);
    std::lock_guard<std::mutex> g(lock);
    float& v = seen[key];
    if (mine > 0.f && (v == 0.f || mine < v)) v = mine;
    return v;
}

static int plan_placement(gpf_handle* h, int D, std::string& note) {
    const char* env_tries = std::getenv("GPF_PLACEMENT_TRIES");
    const int fixed = env_tries ? std::atoi(env_tries) : -1;            // -1: two batches of 12, then on while a batch still pays
    if (fixed == 0 || !h->plan_master) return GPF_OK;
    const bool print = std::getenv("GPF_PLACEMENT_PRINT") && std::atoi(std::getenv("GPF_PLACEMENT_PRINT")) != 0;
    int par = 0;
    GPF_TRY(current_parity(h, &par));
    const bool planes = topo_mode_of(h) == 0;               // the kernel reads h->topo (otherwise the gap travels as a line)
    double* const master = h->plan_master;                  // the current state, never a candidate
    std::vector<double*> pool = {h->q[par], h->q[par ^ 1]};
    std::vector<char> holds_state = {1, 0};
    std::vector<float> w = {0.f, 0.f};
    // read pool[i], write pool[j]; `both`: and the other way round in every other launch (plan_trial restores the state in pool[i])
    auto trial = [&](int i, int j, float* us, bool both) -> int {
        if (!holds_state[i]) {
            GPF_TRY(field_copy(h->stream, pool[i], master, h->field_bytes));
            holds_state[i] = 1;
        }
        holds_state[j] = 0;
        h->q[par] = pool[i]; h->q[par ^ 1] = pool[j];
        return plan_trial(h, D, us, 6, both);
    };
    // phase 1: every buffer as the one WRITTEN (the state read from the handle's own buffer; that one is written reading its twin) --
    // most of what distinguishes the buffers shows there (profiles/r03_placement/pair_matrices.txt).  The spares come in batches of
    // twelve, all held to the end (freed memory comes straight back): two batches, then another one for as long as the last one
    // lowered the best figure by more than 1 % (at most five; GPF_PLACEMENT_TRIES=n: n spares, no more, no less).
    float best_w = 0.f;
    for (int round = 0; round < (fixed > 0 ? 1 : 5); ++round) {
        int want = fixed > 0 ? fixed : 12;
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        while (want > 0 && (size_t)want * h->field_bytes + (2ull << 30) > free_b) --want;
        const size_t first = pool.size();
        for (int k = 0; k < want; ++k) {
            double* b = nullptr;
            if (field_malloc((void**)&b, h->field_bytes) != hipSuccess) { (void)hipGetLastError(); break; }
            GPF_TRY(field_zero(h->stream, b, h->field_bytes));
            pool.push_back(b); holds_state.push_back(0); w.push_back(0.f);
        }
        if (pool.size() == first) break;
        float batch_best = 0.f;
        for (size_t k = first; k < pool.size(); ++k) {
            GPF_TRY(trial(0, (int)k, &w[k], false));
            if (batch_best == 0.f || w[k] < batch_best) batch_best = w[k];
        }
        const bool paid = best_w == 0.f || batch_best < 0.99f * best_w;
        if (best_w == 0.f || batch_best < best_w) best_w = batch_best;
        // (the buffers an earlier handle of this process rejected come back from the allocator first: a handle that has seen nothing
        // as good as its predecessors with the same kernel and grid goes on past them)
        const float known = placement_best_seen(h, D, 0.f);
        if (round >= 1 && !paid && !(known > 0.f && best_w > 1.03f * known)) break;
    }
    (void)placement_best_seen(h, D, best_w);
    const int n = (int)pool.size();
    if (n == 2) return GPF_OK;
    GPF_TRY(trial(0, 1, &w[1], false));                     // the handle's own two: each written reading the other
    GPF_TRY(trial(1, 0, &w[0], false));
    std::vector<int> order(n);
    for (int k = 0; k < n; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return w[x] < w[y]; });
    // phase 2: the pairs of the best few and the handle's own pair, both directions of the step in each trial
    const int m = std::min(n, 4);
    float own_pair = 0.f;
    GPF_TRY(trial(0, 1, &own_pair, true));
    int bi = 0, bj = 1;
    float best = own_pair, worst = own_pair;
    std::string pairs;
    for (int i = 0; i < m; ++i)
        for (int j = i + 1; j < m; ++j) {
            const int x = std::min(order[i], order[j]), y = std::max(order[i], order[j]);
            if (x == 0 && y == 1) continue;
            float t = 0.f;
            GPF_TRY(trial(x, y, &t, true));
            if (print) { char b2[40]; std::snprintf(b2, sizeof b2, " (%d,%d) %.1f", x, y, t); pairs += b2; }
            if (t < best) { best = t; bi = x; bj = y; }
            worst = std::max(worst, t);
        }
    if (print) {
        std::fprintf(stderr, "[gpf] placement: us per step writing each buffer (0, 1: the handle's own):");
        for (int k = 0; k < n; ++k) std::fprintf(stderr, " %.1f", w[k]);
        std::fprintf(stderr, "\n[gpf] placement: pairs, both directions: (0,1) %.1f%s\n", own_pair, pairs.c_str());
    }
    char buf[200];
    std::snprintf(buf, sizeof buf, " placement: %d buffers, written %.0f .. %.0f us, pair kept %.0f, the handle's own %.0f", n,
                  *std::min_element(w.begin(), w.end()), *std::max_element(w.begin(), w.end()), best, own_pair);
    note = buf;
    std::vector<double*> rest;
    for (int k = 0; k < n; ++k) if (k != bi && k != bj) rest.push_back(pool[k]);
    float us = 0.f;
    if (planes) {
        // the gap planes: their present home or one of the buffers left over
        double* const own = h->topo;
        double* best_home = own;
        float best_t = 0.f;
        std::string seen;
        for (size_t k = 0; k <= std::min<size_t>(rest.size(), 3); ++k) {
            double* cand = k == 0 ? own : rest[k - 1];
            if (cand != own) GPF_TRY(field_copy(h->stream, cand, own, h->field_bytes));
            h->topo = cand;
            float t = 0.f;
            GPF_TRY(trial(bi, bj, &t, true));
            std::snprintf(buf, sizeof buf, " %.0f", t);
            seen += buf;
            if (k == 0 || t < best_t) { best_t = t; best_home = cand; }
        }
        note += "; gap planes:" + seen;
        if (best_home != own) {
            rest.erase(std::find(rest.begin(), rest.end(), best_home));
            rest.push_back(own);
        }
        h->topo = best_home;
    }
    GPF_TRY(trial(bi, bj, &us, true));                      // leaves the state in pool[bi] = q[par]
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (double* b : rest) field_free(b);
    h->q[par] = pool[bi]; h->q[par ^ 1] = pool[bj];
    return GPF_OK;
}

// Which plan: waves per SIMD (row chunks per strip) and the cache policy of the stores.  Neither has a winner that holds across
// kernels and boxes (paired in-process runs at 4096^2, tools/ab_inprocess.py: the x-only-gap kernel is 2-3 % faster with two
// waves per SIMD and indifferent to the store policy, the 2-D-gap kernel 6 % faster with one wave per SIMD AND non-temporal
// stores, 4 % with two waves and plain ones; round 2's runs on other boxes favoured one wave per SIMD for both), so grids of a
// million cells and more TIME the candidates once, on their own data (plan_trial: ~8 ms per handle), and keep the fastest.
// Smaller grids and GPF_PLAN_TUNE=0 take the rule of thumb; GPF_CHUNKS / GPF_NT_STORES pin a choice (A/B runs).
// The keep-set: with non-temporal stores, rows with (ix & 7) < k are stored plain, so that they stay in the Infinity Cache and the
// next step reads them on the die (step2_kernel.hip).  Only the kept lines compete for the cache between a row's store and its next
// load, so k / 8 of a state may be nearly as large as the cache.  At 4096^2 (x-only gap, in-process pairs on one box) k = 2 / 3 / 4 /
// 5 took 0.95 / 0.93 / 0.92 / 0.93 of the time of k = 0 (profiles/r04_keep/).  Where the plan is timed, k in {0, 3, 4} is timed on
// the chosen chunks and hint, launches back to back (plan_trial's `both`: each launch reads what the one before wrote); the rule of
// thumb takes 4.  GPF_KEEP_ROWS=k pins it.
static const char* const NT_NAME[3] = {"plain loads and stores", "non-temporal stores", "non-temporal loads and stores"};
constexpr int K2_KEEP_ROWS_DEFAULT = 4;
static const int K2_KEEP_CANDIDATES[2] = {3, 4};
static std::string keep_note(const gpf_handle* h) {
    if (h->nt_policy2 < 1) return "";
    char buf[64];
    std::snprintf(buf, sizeof buf, ", keep %d/8 rows on-die", h->keep_rows2);
    return buf;
}
// where an x-only-gap kernel takes its row coefficients from: the handle's table (TOPO 4), or its own arithmetic (GPF_ROWCOEF_TABLE=0)
static const char* coef_note(const gpf_handle* h) {
    const int topo = topo_mode_of(h);
    return topo == 4 ? ", row coefficients from the table" : topo == 3 ? ", row coefficients evaluated in the kernel" : "";
}
static int plan_step2(gpf_handle* h, int D) {
    if (h->plan2_valid) return GPF_OK;
    const Layout& L = h->L;
    h->geom2[0] = strip2_geom(L, 1);
    h->geom2[1] = strip2_geom(L, -1);
    const int nstrips = std::max(h->geom2[0].nstrips, h->geom2[1].nstrips);
    int per_cu = 0, ncu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)step2_kernel(h->cfg.eos, h->Ls != nullptr, h->cfg.piezo != 0, 1, topo_mode_of(h)), 256, 0));
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device));
    const int all_resident = std::max(1, std::max(1, per_cu * ncu) * 4 / nstrips);      // every wave resident in one round (two per SIMD)
    const int one_per_simd = (ncu * 4) / nstrips;
    // Non-temporal stores can only pay where a step streams more than the 256-MiB Infinity Cache holds (q read + q written + the
    // topography planes if they are read); below that the previous step's output is still on the die when the next step loads it.
    const double streamed = (double)L.plane * 8.0 * (6 + (topo_mode_of(h) == 0 ? 3 : 0) + (h->Ls ? 1 : 0));
    const bool nt_possible = streamed > 192.0 * 1024 * 1024;
    const char* env_chunks = std::getenv("GPF_CHUNKS");
    const char* env_nt = std::getenv("GPF_NT") ? std::getenv("GPF_NT") : std::getenv("GPF_NT_STORES");      // 0, 1 (stores), 2 (stores and loads)
    const char* env_tune = std::getenv("GPF_PLAN_TUNE");
    // rule of thumb: one wave per SIMD for long marches (>= 100 rows per wave), non-temporal stores where they can pay
    int nchunks = all_resident;
    if (one_per_simd >= 1 && L.Nx / one_per_simd >= K2_LONG_MARCH_ROWS) nchunks = one_per_simd;
    int nt = nt_possible ? 2 : 0;
    if (env_chunks && std::atoi(env_chunks) > 0) nchunks = std::atoi(env_chunks);
    if (env_nt) nt = std::max(0, std::min(2, std::atoi(env_nt)));
    const char* env_keep = std::getenv("GPF_KEEP_ROWS");
    int keep = nt_possible ? K2_KEEP_ROWS_DEFAULT : 0;
    if (env_keep) keep = std::max(0, std::min(7, std::atoi(env_keep)));
    // (a slab tunes like any other handle: the trial launches commit into the scratch state and send nothing)
    const bool tune = !(env_tune && std::atoi(env_tune) == 0) && !h->split_edges && h->pre_run_done && (long long)L.Nx * L.Ny >= (1ll << 20) &&
                      one_per_simd >= 1 && L.Nx / one_per_simd >= 16 && !(env_chunks && env_nt);
    if (!tune) {
        GPF_TRY(plan_apply(h, nchunks, nt, keep));
        std::snprintf(h->plan2_note, sizeof h->plan2_note, "%d chunks per strip, %s%s%s (rule of thumb%s)", h->nchunks2,
                      NT_NAME[h->nt_policy2], coef_note(h), keep_note(h).c_str(), (env_chunks || env_nt || env_keep) ? ", pinned by the environment" : "");
        h->plan2_valid = true;
        return GPF_OK;
    }
    std::string placement_note;
    GPF_TRY(plan_apply(h, nchunks, nt));
    {   // a copy of the state: trials that run the step both ways overwrite it (plan_trial)
        int par = 0;
        GPF_TRY(current_parity(h, &par));
        if (field_malloc((void**)&h->plan_master, h->field_bytes) == hipSuccess)
            GPF_TRY(field_copy(h->stream, h->plan_master, h->q[par], h->field_bytes));
        else { (void)hipGetLastError(); h->plan_master = nullptr; }
    }
    {   // The trials come after an idle stretch (the host has just built the problem) and the device takes ~10 ms of load to reach its
        // running clocks: the first candidates of a scan read 5-10 % slow (profiles/r03_placement/README.md).  Load it first.
        float unused = 0.f;
        const double step_s = 1.1e-11 * (double)L.Nx * L.Ny + 1e-5;    // roughly what a launch takes
        GPF_TRY(plan_trial(h, D, &unused, (int)std::min(200.0, std::max(8.0, 0.012 / step_s))));
    }
    float best = 0.f;
    int best_chunks = nchunks;
    int best_nt = nt;
    int best_keep = 0;
    std::string seen, keep_seen;
    auto pick_plan = [&]() -> int {
        best = 0.f;
        seen.clear();
        for (int c : {one_per_simd, all_resident}) {
            if (env_chunks && std::atoi(env_chunks) > 0) c = std::atoi(env_chunks);
            for (int pol = 0; pol < (nt_possible && !env_nt ? 3 : 1); ++pol) {
                const int cand_nt = env_nt ? nt : pol;
                GPF_TRY(plan_apply(h, c, cand_nt));
                float us = 0.f;
                GPF_TRY(plan_trial(h, D, &us, 6, true));
                char buf[48];
                std::snprintf(buf, sizeof buf, " %d/%s %.0f", h->nchunks2, cand_nt == 2 ? "nt" : cand_nt == 1 ? "nts" : "plain", us);
                seen += buf;
                if (best == 0.f || us < best) { best = us; best_chunks = c; best_nt = cand_nt; }
            }
            if ((env_chunks && std::atoi(env_chunks) > 0) || one_per_simd == all_resident) break;
        }
        // the keep-set on the plan just chosen (k = 0 is the figure above)
        best_keep = 0;
        keep_seen.clear();
        if (best_nt >= 1) {
            if (env_keep) best_keep = keep;
            else if (nt_possible) {
                char buf[48];
                std::snprintf(buf, sizeof buf, " 0 %.0f", best);
                keep_seen = buf;
                float best_k = best;
                for (int k : K2_KEEP_CANDIDATES) {
                    GPF_TRY(plan_apply(h, best_chunks, best_nt, k));
                    float us = 0.f;
                    GPF_TRY(plan_trial(h, D, &us, 6, true));
                    std::snprintf(buf, sizeof buf, ", %d %.0f", k, us);
                    keep_seen += buf;
                    if (us < best_k) { best_k = us; best_keep = k; }
                }
            }
        }
        return plan_apply(h, best_chunks, best_nt, best_keep);
    };
    // the plan on the memory the handle has, the memory under that plan (which pages are good depends on how many streams run),
    // the plan once more on the memory kept
    const bool verify = std::getenv("GPF_PLACEMENT_PRINT") && std::atoi(std::getenv("GPF_PLACEMENT_PRINT")) >= 2;
    auto stamp = [&](const char* when) {
        if (!verify) return;
        int par = 0;
        if (current_parity(h, &par) != GPF_OK) return;
        std::fprintf(stderr, "[gpf] %-28s q[par] %p %016llx   master %p %016llx\n", when, (void*)h->q[par], field_checksum(h->stream, h->q[par], h->field_bytes),
                     (void*)h->plan_master, h->plan_master ? field_checksum(h->stream, h->plan_master, h->field_bytes) : 0ull);
    };
    stamp("before the first plan");
    GPF_TRY(pick_plan());
    stamp("after the first plan");
    const std::string first_seen = seen;
    GPF_TRY(plan_placement(h, D, placement_note));
    stamp("after the placement");
    if (!placement_note.empty()) GPF_TRY(pick_plan());
    stamp("after the second plan");
    HIP_TRY(hipStreamSynchronize(h->stream));
    field_free(h->plan_master);
    h->plan_master = nullptr;
    GPF_TRY(plan_apply(h, best_chunks, best_nt, best_keep));
    const std::string kept = keep_note(h) + (keep_seen.empty() ? (env_keep && h->nt_policy2 >= 1 ? " (pinned by the environment)" : "")
                                                               : " (timed, us: k" + keep_seen + ")");
    std::snprintf(h->plan2_note, sizeof h->plan2_note, "%d chunks per strip, %s%s%s (timed, us:%s;%s%s%s)", h->nchunks2,
                  NT_NAME[h->nt_policy2], coef_note(h), kept.c_str(), seen.c_str(), placement_note.c_str(),
                  placement_note.empty() ? "" : "; before the placement:", placement_note.empty() ? "" : first_seen.c_str());
    DBG("plan_step2: %s", h->plan2_note);
    h->plan2_valid = true;
    return GPF_OK;
}

extern "C" const char* gpf_plan_note(gpf_handle* h) { return h ? h->plan2_note : ""; }
