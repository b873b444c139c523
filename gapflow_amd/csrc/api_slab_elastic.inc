// Part of api.hip (included there, not compiled on its own): elastic deformation of the gap on x-slabs.
// ---------------------------------------------------------------------------------------------
// The half-space convolution of gpf_elastic_update (topography.py:257-280, 404-437) as a distributed transform, so that no
// rank holds the whole spectrum: 1-D y-transforms of the rows a rank owns, a transpose to ky column slabs, 1-D x-transforms
// and the Green's multiply there, a transpose back to the rows each rank needs, 1-D inverse y-transforms.  The transposes
// and the all-gather of the reference displacement are the caller's collectives (gapflow_amd/slab.py); every call below
// only enqueues on the handle's stream.  The plan (which rows and columns go where) comes from gapflow_amd/elastic.py:
// SlabElasticPlan; plan[] layout:
//   [0] row0 [1] nrows      global transform rows this rank owns (its interior rows, + row 0 on the first rank, + row Nx+1
//                           on the last)
//   [2] k0   [3] nk         its ky column slab of [0, py/2]; nk may be 0
//   [4] nret [5] nmain [6] main_g0   rows it gets back: nmain consecutive global rows from main_g0 (lo-2 .. hi+2 clipped),
//   [7] seam_side [8] seam_g0        then, on a periodic seam edge (side 0 / 1, else -1), three rows from seam_g0
//   [9] nrows_all           sum of every rank's nret
//   [10] g_lo [11] Nx_global [12] rank
//   [13 ...] rows_all       every rank's return rows in rank order (what this rank sends in the second transpose)
// ---------------------------------------------------------------------------------------------
static constexpr int ELS_PLAN_HEAD = 13;

extern "C" int gpf_elastic_slab_setup(gpf_handle* h, int px, int py, int nranks, const int* plan, size_t plan_count,
                                      const double* greens_ri, size_t greens_count, const double* h0_rows, size_t h0_count,
                                      double alpha, double force_scale, int relative) {
    if (!h || !plan || !h0_rows || nranks < 1) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: bad argument");
    const Layout& L = h->L;
    auto& e = h->els;
    if (e.on || h->el.on) return fail(GPF_ERR_STATE, "gpf_elastic_slab_setup: already set up");
    if (!h->has_topo) return fail(GPF_ERR_STATE, "gpf_elastic_slab_setup: upload the undeformed topography first");
    if (plan_count < (size_t)ELS_PLAN_HEAD) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: plan too short");
    const int row0 = plan[0], nrows = plan[1], k0 = plan[2], nk = plan[3], nret = plan[4], nmain = plan[5], main_g0 = plan[6];
    const int seam_side = plan[7], seam_g0 = plan[8], nrows_all = plan[9], g_lo = plan[10], nxg = plan[11], rank = plan[12];
    const int ny = L.Ny + 2, nky = py / 2 + 1;
    if (px < nxg + 2 || py < ny) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: the transform grid must hold the domain incl. ghost cells");
    if (rank < 0 || rank >= nranks) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: rank out of range");
    const KySplit K(nky, nranks);
    if (k0 != K.start(rank) || nk != K.count(rank)) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: ky slab does not follow the even split of [0, py/2]");
    if (g_lo < 0 || g_lo + L.Nx + 1 > nxg + 1) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: slab rows outside the domain");
    if (nrows < 1 || row0 < g_lo || row0 + nrows > g_lo + L.Nx + 2) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: transform rows must be rows of this slab");
    if (main_g0 != std::max(0, g_lo - 1) || main_g0 + nmain - 1 != std::min(nxg + 1, g_lo + L.Nx + 2))
        return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: the return rows must be the slab's rows and one more on each side (clipped)");
    if (seam_side < -1 || seam_side > 1 || (seam_side >= 0 && (h->E.halo[seam_side] != 2 || !h->has_seam[seam_side])))
        return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: seam rows for an edge that is not a periodic seam with seam topography");
    if (seam_side >= 0 && seam_g0 != (seam_side == 0 ? nxg - 1 : 0)) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: seam rows are Nx-1..Nx+1 (side 0) / 0..2 (side 1)");
    if (nret != nmain + (seam_side >= 0 ? 3 : 0)) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: nret != nmain + seam rows");
    if (plan_count != (size_t)ELS_PLAN_HEAD + nrows_all || nrows_all < nret) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: plan length");
    for (int t = 0; t < nrows_all; ++t)
        if (plan[ELS_PLAN_HEAD + t] < 0 || plan[ELS_PLAN_HEAD + t] > nxg + 1) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: return row outside the domain");
    if (greens_count != (size_t)2 * px * nk || (nk > 0 && !greens_ri)) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: count must be 2 * px * nk (this rank's ky slab)");
    if (h0_count != (size_t)nret * ny) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_setup: h0 count must be nret * (Ny+2)");
    FftLib& F = fftlib();
    if (!F.ok) return fail(GPF_ERR_SOLVER, F.err);
    GPF_TRY(enter(h));
    auto alloc = [&](void** p, size_t bytes) -> int {
        HIP_TRY(hipMalloc(p, std::max<size_t>(bytes, 16)));
        HIP_TRY(hipMemset(*p, 0, std::max<size_t>(bytes, 16)));
        return GPF_OK;
    };
    const size_t c16 = sizeof(double2);
    GPF_TRY(alloc((void**)&e.dense, (size_t)nrows * py * sizeof(double)));
    GPF_TRY(alloc((void**)&e.spec, (size_t)nrows * nky * c16));
    GPF_TRY(alloc((void**)&e.send1, (size_t)nrows * nky * c16));
    GPF_TRY(alloc((void**)&e.recv1, (size_t)px * nk * c16));          // rows nxg+2 .. px-1 stay zero (doubled x range)
    GPF_TRY(alloc((void**)&e.xspec, (size_t)px * nk * c16));
    GPF_TRY(alloc((void**)&e.greens, (size_t)px * nk * c16));
    GPF_TRY(alloc((void**)&e.send2, (size_t)nrows_all * nk * c16));
    GPF_TRY(alloc((void**)&e.recv2, (size_t)nret * nky * c16));
    GPF_TRY(alloc((void**)&e.line, (size_t)nret * nky * c16));
    GPF_TRY(alloc((void**)&e.ureal, (size_t)nret * py * sizeof(double)));
    GPF_TRY(alloc((void**)&e.u_prev, ((size_t)2 * nret * ny + L.plane) * sizeof(double)));
    e.h0 = e.u_prev + (size_t)nret * ny; e.deformation = e.u_prev + (size_t)2 * nret * ny;
    GPF_TRY(alloc((void**)&e.ref, (size_t)8 * (nranks + 1) * sizeof(double)));
    GPF_TRY(alloc((void**)&e.rows_all, (size_t)nrows_all * sizeof(int)));
    HIP_TRY(hipMemcpy(e.h0, h0_rows, h0_count * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e.rows_all, plan + ELS_PLAN_HEAD, (size_t)nrows_all * sizeof(int), hipMemcpyHostToDevice));
    if (nk > 0) HIP_TRY(hipMemcpy(e.greens, greens_ri, (size_t)px * nk * c16, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    {
        std::lock_guard<std::mutex> g(fft_plan_mutex());
        int n_y[1] = {py}, e_r[1] = {py}, e_c[1] = {nky}, n_x[1] = {px};
        if (F.plan_many(&e.plan_y, 1, n_y, e_r, 1, py, e_c, 1, nky, HIPFFT_D2Z_, nrows) != 0 ||
            F.plan_many(&e.plan_yb, 1, n_y, e_c, 1, nky, e_r, 1, py, HIPFFT_Z2D_, nret) != 0)
            return fail(GPF_ERR_SOLVER, "hipfftPlanMany (y lines) failed");
        if (nk > 0 && F.plan_many(&e.plan_x, 1, n_x, n_x, nk, 1, n_x, nk, 1, HIPFFT_Z2Z_, nk) != 0)
            return fail(GPF_ERR_SOLVER, "hipfftPlanMany (x columns) failed");
    }
    e.px = px; e.py = py; e.nky = nky; e.nranks = nranks; e.relative = relative ? 1 : 0;
    e.row0 = row0; e.nrows = nrows; e.k0 = k0; e.nk = nk; e.nret = nret; e.nrows_all = nrows_all; e.nmain = nmain; e.main_g0 = main_g0;
    e.seam_side = seam_side; e.seam_g0 = seam_g0; e.nxg = nxg; e.g_lo = g_lo;
    e.ref_row = (relative && g_lo == 0) ? 0 : -1;           // global cell [0, 0] is compact row 0, column 0 of the first slab
    e.alpha = alpha;
    e.scale = force_scale / ((double)px * (double)py);      // hipFFT's inverses are unnormalised
    e.on = true;
    h->topo_mode = 0;                                       // the gap now changes every step: read the planes
    h->plan2_valid = false;
    return GPF_OK;
}

// Device buffers the caller's collectives read and write (counts in doubles): 0 send / 1 receive buffer of the first transpose,
// 2 send / 3 receive buffer of the second, 4 this rank's 8-double reference message, 5 the all-gathered messages (8 per rank).
extern "C" int gpf_elastic_slab_buffer(gpf_handle* h, int which, void** ptr, size_t* count) {
    if (!h || !ptr || !count) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_buffer: null argument");
    const auto& e = h->els;
    if (!e.on) return fail(GPF_ERR_STATE, "gpf_elastic_slab_buffer: call gpf_elastic_slab_setup first");
    switch (which) {
    case 0: *ptr = e.send1; *count = (size_t)2 * e.nrows * e.nky; break;
    case 1: *ptr = e.recv1; *count = (size_t)2 * (e.nxg + 2) * e.nk; break;
    case 2: *ptr = e.send2; *count = (size_t)2 * e.nrows_all * e.nk; break;
    case 3: *ptr = e.recv2; *count = (size_t)2 * e.nret * e.nky; break;
    case 4: *ptr = e.ref; *count = 8; break;
    case 5: *ptr = e.ref + 8; *count = (size_t)8 * e.nranks; break;
    default: return fail(GPF_ERR_INVALID, "gpf_elastic_slab_buffer: which must be 0..5");
    }
    return GPF_OK;
}

// forces of the owned rows (p - p_ref; p_ref from rank 0's record in `gathered`, the message all-gather that
// gpf_close_step_commit consumed) -> batched D2Z -> first transpose's send buffer
extern "C" int gpf_elastic_slab_forward(gpf_handle* h, const void* gathered, int nranks) {
    if (!h) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_forward: null handle");
    auto& e = h->els;
    if (!e.on) return fail(GPF_ERR_STATE, "gpf_elastic_slab_forward: call gpf_elastic_slab_setup first");
    if (!h->fields) return fail(GPF_ERR_STATE, "gpf_elastic_slab_forward: no pressure field yet");
    if (e.relative && (!gathered || nranks != e.nranks || !h->halo)) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_forward: relative mode needs the gathered step messages of all ranks");
    FftLib& F = fftlib();
    GPF_TRY(enter(h));
    const Layout& L = h->L;
    const double* pref = e.relative ? (const double*)gathered + (halo_len(h) - 8) + 7 : nullptr;
    F.set_stream(e.plan_y, h->stream);
    hipLaunchKernelGGL(k_els_pack, dim3(blocks_for((long long)e.nrows * e.py)), dim3(256), 0, h->stream, (const double*)h->fields, L,
                       e.row0 - e.g_lo, e.nrows, e.py, pref, e.dense);
    if (F.d2z(e.plan_y, e.dense, e.spec) != 0) return fail(GPF_ERR_SOLVER, "hipfftExecD2Z failed");
    hipLaunchKernelGGL(k_els_col_pack, dim3(blocks_for((long long)e.nrows * e.nky)), dim3(256), 0, h->stream, e.spec, e.nrows,
                       KySplit(e.nky, e.nranks), e.send1);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// on this rank's ky columns (first transpose received): x-transform, Green's multiply, inverse x-transform, then the rows
// every rank asked for into the second transpose's send buffer
extern "C" int gpf_elastic_slab_convolve(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_convolve: null handle");
    auto& e = h->els;
    if (!e.on) return fail(GPF_ERR_STATE, "gpf_elastic_slab_convolve: call gpf_elastic_slab_setup first");
    if (e.nk == 0) return GPF_OK;                           // no columns here: nothing to send either
    FftLib& F = fftlib();
    GPF_TRY(enter(h));
    const long long ns = (long long)e.px * e.nk;
    F.set_stream(e.plan_x, h->stream);
    if (F.z2z(e.plan_x, e.recv1, e.xspec, HIPFFT_FORWARD_) != 0) return fail(GPF_ERR_SOLVER, "hipfftExecZ2Z (forward) failed");
    hipLaunchKernelGGL(k_el_multiply, dim3(blocks_for(ns)), dim3(256), 0, h->stream, e.xspec, (const double2*)e.greens, ns);
    if (F.z2z(e.plan_x, e.xspec, e.xspec, HIPFFT_BACKWARD_) != 0) return fail(GPF_ERR_SOLVER, "hipfftExecZ2Z (backward) failed");
    hipLaunchKernelGGL(k_els_row_pack, dim3(blocks_for((long long)e.nrows_all * e.nk)), dim3(256), 0, h->stream, (const double2*)e.xspec,
                       e.nk, (const int*)e.rows_all, e.nrows_all, e.send2);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// second transpose received: unpack to [row][ky] lines, batched Z2D, under-relaxation; the slab holding global cell [0, 0]
// also leaves its relaxed displacement in the reference message (buffer 4)
extern "C" int gpf_elastic_slab_finish(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_finish: null handle");
    auto& e = h->els;
    if (!e.on) return fail(GPF_ERR_STATE, "gpf_elastic_slab_finish: call gpf_elastic_slab_setup first");
    FftLib& F = fftlib();
    GPF_TRY(enter(h));
    const int ny = h->L.Ny + 2;
    F.set_stream(e.plan_yb, h->stream);
    hipLaunchKernelGGL(k_els_unpack, dim3(blocks_for((long long)e.nret * e.nky)), dim3(256), 0, h->stream, (const double2*)e.recv2, e.nret,
                       KySplit(e.nky, e.nranks), e.line);
    if (F.z2d(e.plan_yb, e.line, e.ureal) != 0) return fail(GPF_ERR_SOLVER, "hipfftExecZ2D failed");
    hipLaunchKernelGGL(k_els_relax, dim3(blocks_for((long long)e.nret * ny)), dim3(256), 0, h->stream, (const double*)e.ureal, e.nret, ny,
                       e.py, e.scale, e.alpha, e.u_prev, e.ref_row, e.ref);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// deformation = u - u_ref (u_ref: rank 0's reference message in buffer 5, all-gathered by the caller; relative mode only),
// h = h0 + deformation and np.gradient's dh/dx, dh/dy on the slab's rows and on the seam block of a periodic edge
extern "C" int gpf_elastic_slab_apply(gpf_handle* h) {
    if (!h) return fail(GPF_ERR_INVALID, "gpf_elastic_slab_apply: null handle");
    auto& e = h->els;
    if (!e.on) return fail(GPF_ERR_STATE, "gpf_elastic_slab_apply: call gpf_elastic_slab_setup first");
    GPF_TRY(enter(h));
    const Layout& L = h->L;
    const int ny = L.Ny + 2;
    const double* uref = e.relative ? e.ref + 8 : nullptr;          // rank 0's slot 0
    const double idx = 1.0 / h->cfg.dx, idy = 1.0 / h->cfg.dy;
    ElRows R{e.u_prev, e.h0, ny, 0, e.main_g0, e.nxg, 0.0};
    hipLaunchKernelGGL(k_els_apply, dim3(blocks_for((long long)(L.Nx + 2) * ny)), dim3(256), 0, h->stream, R, uref, e.g_lo, L, idx, idy,
                       e.deformation, h->topo);
    if (e.seam_side >= 0) {
        ElRows S{e.u_prev, e.h0, ny, e.nmain, e.seam_g0, e.nxg, 0.0};
        const int g0 = e.seam_side == 0 ? e.nxg : 1, g1 = e.seam_side == 0 ? e.nxg + 1 : 0;
        hipLaunchKernelGGL(k_els_seam, dim3(blocks_for(2ll * ny)), dim3(256), 0, h->stream, S, uref, g0, g1, L, idx, idy,
                           h->seam + (size_t)e.seam_side * 8 * L.pitch);
    }
    HIP_TRY(hipGetLastError());
    h->g1_ready = false;
    return GPF_OK;
}
