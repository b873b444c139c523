// Part of api.hip (included there, not compiled on its own): x-slab decomposition: stage-wise step (surrogate closures across slabs).
// ---------------------------------------------------------------------------------------------
// stage-wise step of a slab (GP closures / shear thinning across several GPUs): the rows a neighbour needs
// travel after EACH stage, the scalars once per step
// ---------------------------------------------------------------------------------------------
// Shear thinning on a slab: the density one row beyond each outer row (side 0: beyond row 0, side 1: beyond row Nx+1) of
// the CURRENT state, Ny+2 values; from then on the rows travel with the stage messages.
extern "C" int gpf_upload_beyond(gpf_handle* h, int side, const double* rho_row, size_t count) {
    if (!h || !rho_row || side < 0 || side > 1) return fail(GPF_ERR_INVALID, "gpf_upload_beyond: bad argument");
    const Layout& L = h->L;
    if (count != (size_t)(L.Ny + 2)) return fail(GPF_ERR_INVALID, "gpf_upload_beyond: count must be Ny+2");
    GPF_TRY(enter(h));
    if (!h->beyond) {
        HIP_TRY(hipMalloc(&h->beyond, (size_t)4 * L.pitch * sizeof(double)));
        HIP_TRY(hipMemset(h->beyond, 0, (size_t)4 * L.pitch * sizeof(double)));
    }
    std::vector<double> row((size_t)L.pitch, 0.0);
    for (int iy = 0; iy < L.Ny + 2; ++iy) row[(size_t)L.off + iy] = rho_row[iy];
    HIP_TRY(hipMemcpy(h->beyond + (size_t)side * L.pitch, row.data(), row.size() * sizeof(double), hipMemcpyHostToDevice));
    return GPF_OK;
}

static bool slab_thinning(const gpf_handle* h) { return h->cfg.thinning != GPF_THINNING_NONE && h->beyond != nullptr; }

extern "C" int gpf_stage_message(gpf_handle* h) {
    if (!h || !h->step_open) return fail(GPF_ERR_STATE, "gpf_stage_message: no open step");
    GPF_TRY(enter(h));
    GPF_TRY(ensure_halo(h));
    HaloArgs a = halo_args(h, 0, nullptr, -1, -1);
    a.work_parity = h->open_parity ^ 1;
    if (slab_thinning(h)) a.beyond = h->beyond + 2 * h->L.pitch;       // flag for the packer: two more rows travel
    hipLaunchKernelGGL(k_halo_pack, dim3((h->L.pitch + 255) / 256), dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

extern "C" int gpf_stage_absorb(gpf_handle* h, const void* gathered, int nranks, int rank_lo, int rank_hi) {
    if (!h || !gathered || nranks < 1) return fail(GPF_ERR_INVALID, "gpf_stage_absorb: bad argument");
    if (!h->step_open) return fail(GPF_ERR_STATE, "gpf_stage_absorb: no open step");
    if (rank_lo >= nranks || rank_hi >= nranks) return fail(GPF_ERR_INVALID, "gpf_stage_absorb: neighbour rank out of range");
    GPF_TRY(enter(h));
    HaloArgs a = halo_args(h, 0, (const double*)gathered, rank_lo, rank_hi);
    a.work_parity = h->open_parity ^ 1;
    if (slab_thinning(h)) a.beyond = h->beyond + 2 * h->L.pitch;       // the working field's beyond rows
    hipLaunchKernelGGL(k_halo_unpack, dim3((h->L.pitch + 255) / 256), dim3(256), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// average + validity + ghost rules + this slab's share of the scalars -> record in the message
extern "C" int gpf_close_step_local(gpf_handle* h) {
    if (!h || !h->step_open) return fail(GPF_ERR_STATE, "gpf_close_step_local: no open step");
    GPF_TRY(enter(h));
    GPF_TRY(ensure_halo(h));
    const Layout& L = h->L;
    double* q = h->q[h->open_parity ^ 1];
    const double* q0 = h->q[h->open_parity];
    const long long n = (long long)(L.Nx + 2) * (L.Ny + 2);
    h->gp_state_mean_fresh = false;
    hipLaunchKernelGGL(k_average, dim3(blocks_for(n)), dim3(256), 0, h->stream, q, q0, L);
    if (slab_thinning(h))       // the rows beyond the halo follow the field: new state = (working + old) / 2
        hipLaunchKernelGGL(k_beyond_average, dim3((2 * L.pitch + 255) / 256), dim3(256), 0, h->stream, h->beyond, h->beyond + 2 * L.pitch, 2 * L.pitch);
    ScalarPartial* pre = h->spart + h->nspart;
    ScalarPartial* post = h->spart + h->nspart + 1;
    GPF_TRY(launch_scalars(h, q, pre, false));
    hipLaunchKernelGGL(k_bc_x, dim3((L.Ny + 2 + 255) / 256), dim3(256), 0, h->stream, q, L, h->E);
    hipLaunchKernelGGL(k_bc_y, dim3((L.Nx + 2 + 255) / 256), dim3(256), 0, h->stream, q, L, h->E);
    GPF_TRY(launch_scalars(h, q, post));
    hipLaunchKernelGGL(k_record_unfused, dim3(1), dim3(1), 0, h->stream, pre, post, h->halo + (halo_len(h) - 8));
    if (h->els.on && h->els.relative && h->E.halo[0] != 1)      // the slab holding global row 0: p_ref rides in its record
        hipLaunchKernelGGL(k_els_record_pref, dim3(1), dim3(1), 0, h->stream, (const double*)h->fields, L, h->halo + (halo_len(h) - 8));
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

extern "C" int gpf_close_step_commit(gpf_handle* h, const void* gathered, int nranks, gpf_scalars_t* out) {
    if (!h || !gathered || nranks < 1) return fail(GPF_ERR_INVALID, "gpf_close_step_commit: bad argument");
    if (!h->step_open) return fail(GPF_ERR_STATE, "gpf_close_step_commit: no open step");
    GPF_TRY(enter(h));
    hipLaunchKernelGGL(k_commit_gathered, dim3(1), dim3(1), 0, h->stream, h->st, (const double*)gathered,
                       (long long)halo_len(h), (long long)(halo_len(h) - 8), nranks, (LogEntry*)nullptr, 0ll, 0ll, 0);
    HIP_TRY(hipGetLastError());
    h->step_open = false;
    StepState s;
    GPF_TRY(read_state(h, s));
    // the sound-speed pass of gpf_close_step_local ran on the whole local field, outer rows included (they hold the
    // neighbours' rows of the new state since the corrector's exchange): its mean serves the next step's first closures
    if (h->gp_state_mean_fresh && !s.invalid && s.step == h->host_step + 1) {
        h->gp_state_mean_valid = true;
        h->gp_state_mean_step = s.step;
    }
    h->gp_state_mean_fresh = false;
    h->host_step = s.step; h->next_step = s.step;
    if (out) fill_scalars(s, nullptr, 0.0, out);
    return GPF_OK;
}
