// Part of api.hip (included there, not compiled on its own): point probes -- per-step records of a few cells, written on the
// device behind every committed step and handed out once per call.  Kernels: probe_kernels.hip.

static ProbeArgs probe_args(const gpf_handle* h, long long base) {
    ProbeArgs r;
    r.cells = h->probes.cells; r.out = h->probes.buf;
    r.nprobe = h->probes.n; r.nv = h->probes.nv; r.base = base; r.cap = h->log_cap;
    return r;
}

// A stepping call begins: its records replace those of the call before; the device buffer (log_cap x nprobe x nvalues
// doubles, at most 32 MiB) is allocated on first use.
static int probes_begin(gpf_handle* h) {
    if (!h->probes.n) return GPF_OK;
    h->probes.host.clear();
    h->probes.first_step = h->host_step + 1;
    // `dev` is set last, once everything it describes is in place: a call that fails part-way is made up for by the next
    if (!h->probes.dev) {
        if (!h->probes.buf) HIP_TRY(hipMalloc(&h->probes.buf, (size_t)h->log_cap * h->probes.n * h->probes.nv * sizeof(double)));
        ProbeArgs* dev = nullptr;
        HIP_TRY(hipMalloc(&dev, sizeof(ProbeArgs)));
        const ProbeArgs r = probe_args(h, 0);
        const hipError_t e = hipMemcpy(dev, &r, sizeof(r), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return fail(GPF_ERR_HIP, std::string("probes_begin: hipMemcpy: ") + hipGetErrorString(e));
        }
        h->probes.dev = dev;
    }
    return GPF_OK;
}

// Behind the launches of one step on the handle's stream: record it if it took the step count to `expect`
static int probes_launch(gpf_handle* h, long long expect, long long base) {
    if (!h->probes.n) return GPF_OK;
    const ProbeArgs r = probe_args(h, base);
    const int nt = r.nprobe * r.nv;
    EOS_DISPATCH(h->cfg.eos, {
        hipLaunchKernelGGL((k_probe_record<EOS_>), dim3((nt + 255) / 256), dim3(256), 0, h->stream, (const double*)h->q[0],
                           (const double*)h->q[1], (const StepState*)h->st, h->L, h->P, r, expect);
    });
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// After the batch's state has been read (the stream is idle): the records of its `ran` committed steps -> host
static int probes_collect(gpf_handle* h, long long, long long ran) {
    if (!h->probes.n || ran <= 0) return GPF_OK;
    const size_t add = (size_t)ran * h->probes.n * h->probes.nv, at = h->probes.host.size();
    h->probes.host.resize(at + add);
    HIP_TRY(hipMemcpy(h->probes.host.data() + at, h->probes.buf, add * sizeof(double), hipMemcpyDeviceToHost));
    return GPF_OK;
}

static SeriesBuffers probes_owned(gpf_handle* h) { return {(void**)&h->probes.cells, (void**)&h->probes.buf, (void**)&h->probes.dev}; }

static int probes_release(gpf_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));       // a recording launch may still be queued
    GPF_TRY(series_free(probes_owned(h)));
    h->probes.n = 0; h->probes.nv = 0;
    h->probes.host.clear(); h->probes.first_step = 0;
    return GPF_OK;
}

// The cases the records do not cover (gpf_probes_set's and, per member, gpf_ensemble_probes_set's), and the one a record with p
// does not
static int probes_refusal(const gpf_handle* h, const std::string& who) {
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": this handle is a slab; probes are not available on slabs");
    if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open; close it first");
    return GPF_OK;
}

static int probes_pressure_refusal(const gpf_handle* h, const std::string& who) {
    if (h->gp[0].set) return fail(GPF_ERR_INVALID, who + ": no EOS pressure to record, this handle's pressure comes from a surrogate");
    return GPF_OK;
}

extern "C" int gpf_probes_set(gpf_handle* h, int n, const int32_t* ix, const int32_t* iy, int with_pressure) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    GPF_TRY(probes_refusal(h, "gpf_probes_set"));
    if (n < 1 || !ix || !iy) return fail(GPF_ERR_INVALID, "gpf_probes_set: n >= 1 cells required (gpf_probes_clear removes them)");
    if (n > PROBE_MAX)
        return fail(GPF_ERR_INVALID, "gpf_probes_set: probe " + std::to_string(PROBE_MAX) + " is one too many (" + std::to_string(n) +
                                     " given, at most " + std::to_string(PROBE_MAX) + " per handle)");
    std::vector<int> cells((size_t)2 * n);
    for (int p = 0; p < n; ++p) {
        if (ix[p] < 0 || ix[p] > h->L.Nx + 1 || iy[p] < 0 || iy[p] > h->L.Ny + 1)
            return fail(GPF_ERR_INVALID, "gpf_probes_set: probe " + std::to_string(p) + " at cell (" + std::to_string(ix[p]) + ", " +
                                         std::to_string(iy[p]) + ") lies outside 0.." + std::to_string(h->L.Nx + 1) + " x 0.." +
                                         std::to_string(h->L.Ny + 1));
        cells[2 * p] = ix[p]; cells[2 * p + 1] = iy[p];
    }
    if (with_pressure) GPF_TRY(probes_pressure_refusal(h, "gpf_probes_set: probe 0"));
    GPF_TRY(series_disarm(h, SERIES[S_PROBES]));
    HIP_TRY(hipMalloc(&h->probes.cells, cells.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(h->probes.cells, cells.data(), cells.size() * sizeof(int), hipMemcpyHostToDevice));
    h->probes.n = n; h->probes.nv = with_pressure ? 4 : 3;
    return GPF_OK;
}

extern "C" int gpf_probes_clear(gpf_handle* h) { return series_clear(h, SERIES[S_PROBES]); }

extern "C" int gpf_probes_read(gpf_handle* h, double* out, int64_t capacity_steps, int64_t* first_step, int64_t* n_steps) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->probes.n) return fail(GPF_ERR_STATE, "gpf_probes_read: no probes are set (gpf_probes_set)");
    const size_t per = (size_t)h->probes.n * h->probes.nv;
    const int64_t have = (int64_t)(h->probes.host.size() / per);
    if (first_step) *first_step = h->probes.first_step;
    if (n_steps) *n_steps = have;
    if (out && capacity_steps > 0)
        std::memcpy(out, h->probes.host.data(), (size_t)std::min<int64_t>(have, capacity_steps) * per * sizeof(double));
    return GPF_OK;
}

// Diagnostic (tools/probe_time.py): n steps as gpf_step enqueues them, with `mode` 0 nothing, 1 k_probe_record (probes must
// be set), 2 an empty kernel behind every step; *ms = first launch to last on the handle's stream.  Small grids take
// k_small_steps, where mode 2 has no meaning and is refused.
extern "C" int gpf_probes_time(gpf_handle* h, int64_t n, int mode, double* ms) {
    GPF_TRY(series_time_checks(h, SERIES[S_PROBES], n, mode, 2, ms, "probes (gpf_probes_set)", [](const gpf_handle* h, const std::string& who) {
        if (h->E.halo[0] || h->E.halo[1] || h->cfg.thinning != GPF_THINNING_NONE) return fail(GPF_ERR_STATE, who + ": fused, unsliced handles only");
        return (int)GPF_OK;
    }));
    if (small_grid_eligible(h) && mode == 2) return fail(GPF_ERR_INVALID, "gpf_probes_time: the small-grid kernel has no launch per step to stand in for");
    GPF_TRY(enter(h));
    // mode 0 and 2 must not record: the probes are put aside for the call
    SeriesAside aside(h, mode == 1 ? &h->probes.n : nullptr);
    GPF_TRY(probes_begin(h));
    return series_time(h, "gpf_probes_time", aside,
                       [&](long long base) {
                           return series_time_steps(h, n, base, [&](long long expect) {
                               if (mode == 2) hipLaunchKernelGGL(k_probe_empty, dim3(1), dim3(64), 0, h->stream);
                               return probes_launch(h, expect, base);
                           });
                       },
                       [&](long long base, long long ran) { return probes_collect(h, base, ran); }, ms);
}
