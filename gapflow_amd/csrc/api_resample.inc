// Part of api.hip (included there, not compiled on its own): gpf_resample -- a handle's state from another handle's committed
// state on another grid of the same domain (arithmetic: resample.hpp, kernel: resample_kernels.hip).

static bool edge_periodic(const gpf_handle* h, int e) { return h->E.rule[e][0] == BC_P; }

// The cases the operator does not cover, with the error classes gpf_integrals_set gives them; nothing is touched before all pass
static int resample_refusal(const gpf_handle* dst, const gpf_handle* src, const std::string& who) {
    if (!dst || !src) return fail(GPF_ERR_INVALID, who + ": null handle");
    if (dst == src) return fail(GPF_ERR_INVALID, who + ": source and destination are the same handle");
    if (dst->cfg.device != src->cfg.device)
        return fail(GPF_ERR_INVALID, who + ": the source lives on device " + std::to_string(src->cfg.device) + ", the destination on device " +
                                     std::to_string(dst->cfg.device) + " (different devices; one launch reads both)");
    for (const gpf_handle* h : {dst, src}) {
        const std::string which = h == dst ? "destination" : "source";
        if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_STATE, who + ": the " + which + " is a slab; resampling is not available on slabs");
        if (h->step_open) return fail(GPF_ERR_STATE, who + ": a stage-wise step is open on the " + which + "; close it first");
        if (!h->has_q || !h->has_topo) return fail(GPF_ERR_STATE, who + ": the " + which + " has no q or no gap yet; upload q and topography first");
    }
    const double Ls[2] = {src->cfg.Nx * src->cfg.dx, src->cfg.Ny * src->cfg.dy}, Ld[2] = {dst->cfg.Nx * dst->cfg.dx, dst->cfg.Ny * dst->cfg.dy};
    for (int d = 0; d < 2; ++d)
        if (std::fabs(Ls[d] - Ld[d]) > 1e-12 * std::max(std::fabs(Ls[d]), std::fabs(Ld[d]))) {
            char buf[200];
            std::snprintf(buf, sizeof buf, ": the domains differ, L%c = %.17g on the source and %.17g on the destination", d == 0 ? 'x' : 'y', Ls[d], Ld[d]);
            return fail(GPF_ERR_INVALID, who + buf);
        }
    for (int e = 0; e < 4; ++e)
        if (edge_periodic(src, e) != edge_periodic(dst, e))
            return fail(GPF_ERR_INVALID, who + ": the " + (e < 2 ? "x" : "y") + " direction is periodic on the " + (edge_periodic(src, e) ? "source" : "destination") +
                                         " and not on the " + (edge_periodic(src, e) ? "destination" : "source") + " (periodicity mismatch)");
    if (dst->gp[0].set) return fail(GPF_ERR_INVALID, who + ": the destination's pressure comes from a surrogate (not supported)");
    if (ensemble_members_has(dst)) return fail(GPF_ERR_STATE, who + ": the destination is a member of a live ensemble; destroy the ensemble first");
    return GPF_OK;
}

// 16-byte pair stores of k_resample: film_wide_ok's conditions on the planes it writes and the gap plane it reads
// (GPF_FILM_NARROW, read at every call, asks for the 8-byte stores regardless)
static bool resample_wide_ok(const gpf_handle* h) {
    const Layout& L = h->L;
    auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    return ((L.off + 1) & 1) == 0 && (L.pitch & 1) == 0 && (L.plane & 1) == 0 && a16(h->q[0]) && a16(h->q[1]) && a16(h->topo) &&
           std::getenv("GPF_FILM_NARROW") == nullptr;
}

static ResampleArgs resample_args(gpf_handle* dst, const gpf_handle* src, int dst_parity, int src_parity) {
    ResampleArgs a;
    a.sq = src->q[src_parity]; a.sh = src->topo; a.dq = dst->q[dst_parity]; a.dh = dst->topo;
    a.Ls = src->L; a.Ld = dst->L;
    a.rx = dst->cfg.dx / src->cfg.dx; a.ry = dst->cfg.dy / src->cfg.dy;
    a.unit_x = (src->L.Nx == 1 && dst->L.Nx == 1) ? 1 : 0;
    a.unit_y = (src->L.Ny == 1 && dst->L.Ny == 1) ? 1 : 0;
    a.wide = resample_wide_ok(dst) ? 1 : 0;
    return a;
}

// The interior from the source, then the ghost cells by the handle's own edge rules (x edges over all columns, then y edges
// over all rows, as everywhere else)
static int resample_enqueue(gpf_handle* dst, const ResampleArgs& a) {
    const Layout& L = dst->L;
    hipLaunchKernelGGL(k_resample, dim3(L.Nx), dim3(256), 0, dst->stream, a);
    hipLaunchKernelGGL(k_bc_x, dim3((L.Ny + 2 + 255) / 256), dim3(256), 0, dst->stream, a.dq, L, dst->E);
    hipLaunchKernelGGL(k_bc_y, dim3((L.Nx + 2 + 255) / 256), dim3(256), 0, dst->stream, a.dq, L, dst->E);
    HIP_TRY(hipGetLastError());
    return GPF_OK;
}

// The source's run state, once everything queued on its stream has finished
static int resample_source_state(const gpf_handle* src, const std::string& who, StepState& s) {
    HIP_TRY(hipStreamSynchronize(src->stream));
    HIP_TRY(hipMemcpy(&s, src->st, sizeof(s), hipMemcpyDeviceToHost));
    if (s.invalid) return fail(GPF_ERR_STATE, who + ": the source's run state is flagged invalid (its last step was rolled back)");
    return GPF_OK;
}

extern "C" int gpf_resample(gpf_handle* dst, const gpf_handle* src) {
    GPF_TRY(resample_refusal(dst, src, "gpf_resample"));
    HIP_TRY(hipSetDevice(dst->cfg.device));
    StepState ss;
    GPF_TRY(resample_source_state(src, "gpf_resample", ss));
    GPF_TRY(enter(dst));
    int par = 0;
    GPF_TRY(current_parity(dst, &par));
    DBG("gpf_resample: %dx%d -> %dx%d, %s pair stores", src->L.Nx, src->L.Ny, dst->L.Nx, dst->L.Ny, resample_wide_ok(dst) ? "16-byte" : "8-byte");
    GPF_TRY(resample_enqueue(dst, resample_args(dst, src, par, ss.parity)));
    HIP_TRY(hipStreamSynchronize(dst->stream));
    // what gpf_upload of the same field leaves
    dst->has_q = true;
    dst->g1_ready = false;
    prev_state_lost(dst);
    dst->fields_step = -1;
    return stats_restart(dst, dst->host_step);      // another state: armed statistics begin a new window
}

// Diagnostic (tools/resample_time.py): `reps` launches on dst's stream of, `mode` 0, what gpf_resample enqueues, written into the
// buffer that does NOT hold dst's state; 1, k_resample_store_only on the same buffer.  *ms = first launch to last, per launch.
// The state and the run state stay; the other buffer's copy of the previous state does not.
extern "C" int gpf_resample_time(gpf_handle* dst, const gpf_handle* src, int mode, int reps, double* ms) {
    if (!ms) return fail(GPF_ERR_INVALID, "gpf_resample_time: null argument");
    if (mode < 0 || mode > 1 || reps < 1 || reps > 10000) return fail(GPF_ERR_INVALID, "gpf_resample_time: mode in 0..1 and 1 <= reps <= 10000 required");
    GPF_TRY(resample_refusal(dst, src, "gpf_resample_time"));
    HIP_TRY(hipSetDevice(dst->cfg.device));
    StepState ss;
    GPF_TRY(resample_source_state(src, "gpf_resample_time", ss));
    GPF_TRY(enter(dst));
    int par = 0;
    GPF_TRY(current_parity(dst, &par));
    prev_state_lost(dst);
    const ResampleArgs a = resample_args(dst, src, par ^ 1, ss.parity);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    int rc = GPF_OK;
    float t = 0.f;
    if (e == hipSuccess) e = hipEventRecord(e0, dst->stream);
    for (int i = 0; i < reps && rc == GPF_OK && e == hipSuccess; ++i) {
        if (mode == 0) rc = resample_enqueue(dst, a);
        else hipLaunchKernelGGL(k_resample_store_only, dim3(dst->L.Nx), dim3(256), 0, dst->stream, a.dq, dst->L, a.wide, 1.0);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(e1, dst->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    GPF_TRY(rc);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_resample_time: ") + hipGetErrorString(e));
    *ms = (double)t / reps;
    return GPF_OK;
}
