// Part of api.hip (included there, not compiled on its own): x-slab decomposition: all-gather transport.
// ---------------------------------------------------------------------------------------------
// slab decomposition
// ---------------------------------------------------------------------------------------------
// rows in the message: first and last owned row (3 components each); with shear thinning also the density of the second
// and the second-to-last row (the two-row halo of grad p); then the 8-double record
static size_t halo_rows(const gpf_handle* h) { return h->cfg.thinning != GPF_THINNING_NONE ? 8 : 6; }
static size_t halo_len(gpf_handle* h) { return halo_rows(h) * h->L.pitch + 8; }

static int ensure_halo(gpf_handle* h) {
    if (h->halo) return GPF_OK;
    HIP_TRY(hipMalloc(&h->halo, halo_len(h) * sizeof(double)));
    HIP_TRY(hipMemsetAsync(h->halo, 0, halo_len(h) * sizeof(double), h->stream));
    return GPF_OK;
}

extern "C" int gpf_slab_message(gpf_handle* h, void** message, size_t* count) {
    if (!h || !message || !count) return fail(GPF_ERR_INVALID, "gpf_slab_message: null argument");
    GPF_TRY(enter(h, true));
    GPF_TRY(ensure_halo(h));
    *message = h->halo;
    *count = halo_len(h);
    return GPF_OK;
}

static HaloArgs halo_args(gpf_handle* h, int honor_stop, const double* gathered, int rank_lo, int rank_hi) {
    HaloArgs a;
    a.qa = h->q[0]; a.qb = h->q[1];
    a.msg = h->halo; a.gathered = gathered; a.rank_lo = rank_lo; a.rank_hi = rank_hi;
    a.st = h->st; a.L = h->L; a.E = h->E; a.honor_stop = honor_stop;
    a.work_parity = -1;
    a.beyond = nullptr;
    a.msg_rows = (int)halo_rows(h);
    return a;
}

extern "C" int gpf_step_local(gpf_handle* h, int honor_stop) {
    if (!h) return fail(GPF_ERR_INVALID, "gpf_step_local: null handle");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_step_local: call gpf_pre_run first");
    GPF_TRY(enter(h));
    if (h->cfg.thinning != GPF_THINNING_NONE)
        return fail(GPF_ERR_STATE, "gpf_step_local: shear thinning needs grad p; use the stage-wise slab calls (gpf_stage_message / gpf_stage_absorb)");
    GPF_TRY(ensure_halo(h));
    double* rec = h->halo + (size_t)6 * h->L.pitch;
    GPF_TRY(enqueue_step(h, honor_stop, h->host_step, rec));      // leaves rows and record in the message
    return GPF_OK;
}

extern "C" int gpf_step_commit(gpf_handle* h, int honor_stop, const void* gathered, int nranks, int rank_lo, int rank_hi) {
    if (!h || !gathered || nranks < 1) return fail(GPF_ERR_INVALID, "gpf_step_commit: bad argument");
    if (rank_lo >= nranks || rank_hi >= nranks) return fail(GPF_ERR_INVALID, "gpf_step_commit: neighbour rank out of range");
    if (!h->halo) return fail(GPF_ERR_STATE, "gpf_step_commit without gpf_step_local");
    GPF_TRY(enter(h));
    // one launch: scatter the neighbours' rows, reduce the records in rank order, commit (the split step also prepares
    // the next step's stage-1 ghost data here, so that the next gpf_step_local starts with the stencil)
    const Layout& L = h->L;
    GhostArgs g;
    GPF_TRY(ghost_args(h, honor_stop, g));
    const bool fused = step2_fused(h);
    WaitArgs w;
    w.qa = h->q[0]; w.qb = h->q[1]; w.st = h->st; w.log = h->log; w.log_base = h->host_step; w.log_cap = h->log_cap;
    w.L = L; w.E = h->E; w.honor_stop = honor_stop; w.arrive = h->arrive + 1; w.timeout_ticks = h->p2p_timeout_ticks; w.p2p = p2p_args(h, false);
    w.gathered = (const double*)gathered; w.msg_len = (long long)halo_len(h); w.nranks = nranks; w.rank_lo = rank_lo; w.rank_hi = rank_hi;
    w.stage1 = fused ? 0 : 1;
    const dim3 ggrid(fused ? SLAB_COMMIT_BLOCKS : std::min((L.Nx + L.Ny + 63) / 64, 512));
    EOS_DISPATCH(h->cfg.eos, {
        if (fused) hipLaunchKernelGGL((k_begin_slab<EOS_, false, false, false, false>), ggrid, dim3(256), 0, h->stream, g, w, h->P);
        else if (topo_xonly(h)) hipLaunchKernelGGL((k_begin_slab<EOS_, false, false, true, false>), ggrid, dim3(256), 0, h->stream, g, w, h->P);
        else LS_PIEZO_DISPATCH(h->Ls != nullptr, h->cfg.piezo != 0, hipLaunchKernelGGL((k_begin_slab<EOS_, LS_, PZ_, false, false>), ggrid, dim3(256), 0, h->stream, g, w, h->P));
    });
    HIP_TRY(hipGetLastError());
    h->g1_ready = !fused;
    return GPF_OK;
}
