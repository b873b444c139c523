// Part of api.hip (included there, not compiled on its own): elastic deformation of the gap.
// ---------------------------------------------------------------------------------------------
// elastic deformation of the gap (topography.py:257-280, 327-437)
// ---------------------------------------------------------------------------------------------
extern "C" int gpf_elastic_setup(gpf_handle* h, int px, int py, const double* greens_ri, size_t count, double alpha,
                                 double force_scale, int relative) {
    if (!h || !greens_ri) return fail(GPF_ERR_INVALID, "gpf_elastic_setup: null argument");
    const Layout& L = h->L;
    if (px < L.Nx + 2 || py < L.Ny + 2) return fail(GPF_ERR_INVALID, "gpf_elastic_setup: the transform grid must hold the field incl. ghost cells");
    const size_t nspec = (size_t)px * (py / 2 + 1);
    if (count != 2 * nspec) return fail(GPF_ERR_INVALID, "gpf_elastic_setup: count must be 2 * px * (py/2 + 1) (real, imaginary)");
    if (!h->has_topo) return fail(GPF_ERR_STATE, "gpf_elastic_setup: upload the undeformed topography first");
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, "gpf_elastic_setup: not available for slabs (the half-space couples the whole domain)");
    FftLib& F = fftlib();
    if (!F.ok) return fail(GPF_ERR_SOLVER, F.err);
    GPF_TRY(enter(h));
    auto& e = h->el;
    if (e.on) return fail(GPF_ERR_STATE, "gpf_elastic_setup: already set up");
    HIP_TRY(hipMalloc((void**)&e.greens, nspec * sizeof(double2)));
    HIP_TRY(hipMalloc((void**)&e.spec, nspec * sizeof(double2)));
    HIP_TRY(hipMalloc((void**)&e.dense, (size_t)px * py * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&e.u_prev, (size_t)3 * L.plane * sizeof(double)));
    e.h0 = e.u_prev + L.plane; e.deformation = e.u_prev + 2 * L.plane;
    HIP_TRY(hipMemset(e.u_prev, 0, (size_t)3 * L.plane * sizeof(double)));
    HIP_TRY(hipMemcpy(e.greens, greens_ri, nspec * sizeof(double2), hipMemcpyHostToDevice));
    GPF_TRY(field_copy(0, e.h0, h->topo, (size_t)L.plane * sizeof(double)));      // (h->topo may be a scattered field: field_malloc)
    HIP_TRY(hipDeviceSynchronize());
    if (F.plan2d(&e.plan_f, px, py, HIPFFT_D2Z_) != 0 || F.plan2d(&e.plan_b, px, py, HIPFFT_Z2D_) != 0)
        return fail(GPF_ERR_SOLVER, "hipfftPlan2d failed");
    e.px = px; e.py = py; e.alpha = alpha; e.relative = relative ? 1 : 0;
    e.scale = force_scale / ((double)px * (double)py);      // hipFFT's inverse is unnormalised
    e.on = true;
    h->topo_mode = 0;                                       // the gap now changes every step: read the planes
    return GPF_OK;
}

// Topography.update + update_gradients with the pressure of the last closure evaluation (problem.py:566 uses the
// stored field, i.e. stage 2's): h, dh/dx, dh/dy of the handle change in place.
extern "C" int gpf_elastic_update(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "gpf_elastic_update: null handle");
    auto& e = h->el;
    if (!e.on) return fail(GPF_ERR_STATE, "gpf_elastic_update: call gpf_elastic_setup first");
    if (!h->fields) return fail(GPF_ERR_STATE, "gpf_elastic_update: no pressure field yet (gpf_stage_closures / gpf_update_closures)");
    FftLib& F = fftlib();
    GPF_TRY(enter(h));
    const Layout& L = h->L;
    const long long nd = (long long)e.px * e.py, ns = (long long)e.px * (e.py / 2 + 1), nc = (long long)(L.Nx + 2) * (L.Ny + 2);
    F.set_stream(e.plan_f, h->stream); F.set_stream(e.plan_b, h->stream);
    hipLaunchKernelGGL(k_el_pack, dim3(blocks_for(nd)), dim3(256), 0, h->stream, h->fields, L, e.px, e.py, e.relative, e.dense);
    if (F.d2z(e.plan_f, e.dense, e.spec) != 0) return fail(GPF_ERR_SOLVER, "hipfftExecD2Z failed");
    hipLaunchKernelGGL(k_el_multiply, dim3(blocks_for(ns)), dim3(256), 0, h->stream, e.spec, e.greens, ns);
    if (F.z2d(e.plan_b, e.spec, e.dense) != 0) return fail(GPF_ERR_SOLVER, "hipfftExecZ2D failed");
    hipLaunchKernelGGL(k_el_relax, dim3(blocks_for(nc)), dim3(256), 0, h->stream, e.dense, e.py, e.scale, e.alpha, L, e.u_prev);
    hipLaunchKernelGGL(k_el_apply, dim3(blocks_for(nc)), dim3(256), 0, h->stream, e.u_prev, e.h0, e.relative, L, e.deformation, h->topo);
    hipLaunchKernelGGL(k_el_gradient, dim3(blocks_for(nc)), dim3(256), 0, h->stream, h->topo, L, 1.0 / h->cfg.dx, 1.0 / h->cfg.dy,
                       h->topo + L.plane, h->topo + 2 * L.plane);
    HIP_TRY(hipGetLastError());
    h->g1_ready = false;
    for (int k : SERIES_STAGEWISE)              // an armed handle's closed step is recorded with the gap it now holds
        if (SERIES[k].store) GPF_TRY(series_after_elastic_update(h, SERIES[k]));
    return GPF_OK;
}
