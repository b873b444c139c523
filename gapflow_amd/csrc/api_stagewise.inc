// Part of api.hip (included there, not compiled on its own): the stage-wise step in pieces.
// ---------------------------------------------------------------------------------------------
// the unfused step in pieces, for closures that need the host between stages (GP + active learning)
// ---------------------------------------------------------------------------------------------
extern "C" int gpf_open_step(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "null handle");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_open_step: call gpf_pre_run first");
    if (h->step_open) return fail(GPF_ERR_STATE, "gpf_open_step: a step is already open");
    GPF_TRY(enter(h, true));
    const Layout& L = h->L;
    GPF_TRY(ensure_fields(h));
    if (!h->work) HIP_TRY(hipMalloc(&h->work, (size_t)9 * L.plane * sizeof(double)));
    StepState s;
    GPF_TRY(read_state(h, s));
    if (s.invalid) return fail(GPF_ERR_STATE, "gpf_open_step: the state is invalid (rolled back); nothing to advance");
    h->open_parity = s.parity;
    hipLaunchKernelGGL(k_copy3, dim3(blocks_for(3 * L.plane)), dim3(256), 0, h->stream, h->q[s.parity], h->q[s.parity ^ 1], 3 * L.plane);
    if (h->beyond)      // thinning slab: the working field starts with the state's rows beyond the halo
        hipLaunchKernelGGL(k_copy3, dim3(blocks_for(2 * L.pitch)), dim3(256), 0, h->stream, h->beyond, h->beyond + 2 * L.pitch, 2ll * L.pitch);
    HIP_TRY(hipGetLastError());
    h->step_open = true;
    prev_state_lost(h, PREV_LOST_STAGEWISE);        // the other buffer becomes the working field
    h->open_first_closures = true;
    h->g1_ready = false;
    h->host_step = s.step; h->next_step = s.step;
    return GPF_OK;
}

extern "C" int gpf_stage_closures(gpf_handle* h) {
    if (!h || !h->step_open) return fail(GPF_ERR_STATE, "gpf_stage_closures: no open step");
    GPF_TRY(enter(h, true));
    // the working field still equals the state the step opened on: the sound-speed pass that closed the previous step has
    // left the pressure surrogate's mean of it
    const bool first = h->open_first_closures;
    h->open_first_closures = false;
    const bool cached = first && h->gp_reuse_state_mean && h->gp[0].set && h->gp_state_mean_valid && h->gp_state_mean_step == h->host_step;
    return launch_fields(h, h->q[h->open_parity ^ 1], cached);
}

extern "C" int gpf_stage_advance(gpf_handle* h, int stage) {
    if (!h || !h->step_open) return fail(GPF_ERR_STATE, "gpf_stage_advance: no open step");
    if (stage != 0 && stage != 1) return fail(GPF_ERR_INVALID, "gpf_stage_advance: stage must be 0 (predictor) or 1 (corrector)");
    GPF_TRY(enter(h));
    const Layout& L = h->L;
    double* q = h->q[h->open_parity ^ 1];
    const long long n = (long long)(L.Nx + 2) * (L.Ny + 2);
    const int nb = blocks_for(n);
    double *fx = h->work, *fy = h->work + 3 * L.plane, *src = h->work + 6 * L.plane;
    FieldPtrs F = field_ptrs(h);
    const int mc = h->cfg.mc_order;
    const int sw = mc == 0 ? ((h->host_step % 2 == 0) ? 1 : -1) : mc;
    const int first = ((sw + 1) / 2) ? 1 : -1;
    const int dir = stage == 0 ? first : -first;
    hipLaunchKernelGGL(k_fluxdiff, dim3(nb), dim3(256), 0, h->stream, q, F.p, F.tau, dir, fx, fy, L);
    hipLaunchKernelGGL(k_source, dim3(nb), dim3(256), 0, h->stream, q, h->topo, F.tau, F.lower, F.upper, src, L);
    hipLaunchKernelGGL(k_axpy, dim3(nb), dim3(256), 0, h->stream, q, fx, fy, src, (const double*)&h->st->dt, h->cfg.dx, h->cfg.dy, L);
    hipLaunchKernelGGL(k_bc_x, dim3((L.Ny + 2 + 255) / 256), dim3(256), 0, h->stream, q, L, h->E);
    hipLaunchKernelGGL(k_bc_y, dim3((L.Nx + 2 + 255) / 256), dim3(256), 0, h->stream, q, L, h->E);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

extern "C" int gpf_close_step(gpf_handle* h, gpf_scalars_t* out) {
    if (!h || !h->step_open) return fail(GPF_ERR_STATE, "gpf_close_step: no open step");
    GPF_TRY(enter(h, true));
    const Layout& L = h->L;
    double* q = h->q[h->open_parity ^ 1];
    const double* q0 = h->q[h->open_parity];
    const long long n = (long long)(L.Nx + 2) * (L.Ny + 2);
    h->gp_state_mean_valid = false; h->gp_state_mean_fresh = false;
    hipLaunchKernelGGL(k_average, dim3(blocks_for(n)), dim3(256), 0, h->stream, q, q0, L);
    ScalarPartial* pre = h->spart + h->nspart;
    ScalarPartial* post = h->spart + h->nspart + 1;
    GPF_TRY(launch_scalars(h, q, pre, false));          // validity of the averaged field only (problem.py:565)
    hipLaunchKernelGGL(k_bc_x, dim3((L.Ny + 2 + 255) / 256), dim3(256), 0, h->stream, q, L, h->E);
    hipLaunchKernelGGL(k_bc_y, dim3((L.Nx + 2 + 255) / 256), dim3(256), 0, h->stream, q, L, h->E);
    GPF_TRY(launch_scalars(h, q, post));                // scalars after the ghost update (problem.py:576-578)
    hipLaunchKernelGGL(k_commit_unfused, dim3(1), dim3(1), 0, h->stream, h->st, pre, post);
    HIP_TRY(hipGetLastError());
    h->step_open = false;
    for (int k : SERIES_STAGEWISE) GPF_TRY(series_close_launch(h, SERIES[k]));      // the closed step's records, if it commits
    StepState s;
    GPF_TRY(read_state(h, s));
    for (int k : SERIES_STAGEWISE) GPF_TRY(series_close_collect(h, SERIES[k], s.step - h->host_step));
    // the committed state is the field the sound-speed pass ran on (a rolled-back step keeps the old state instead)
    if (h->gp_state_mean_fresh && !s.invalid && s.step == h->host_step + 1) {
        h->gp_state_mean_valid = true;
        h->gp_state_mean_step = s.step;
    }
    h->gp_state_mean_fresh = false;
    h->fields_step = (!s.invalid && s.step == h->host_step + 1) ? s.step : -1;      // the corrector stage's closures
    h->host_step = s.step; h->next_step = s.step;
    if (out) fill_scalars(s, nullptr, 0.0, out);
    return GPF_OK;
}
