// Part of api.hip (included there, not compiled on its own): x-slab decomposition: peer-to-peer mailbox transport.
// ---------------------------------------------------------------------------------------------
// peer-to-peer slab transport
// ---------------------------------------------------------------------------------------------
extern "C" int gpf_p2p_export(gpf_handle* h, void* ipc_handle, size_t handle_bytes) {
    if (!h || !ipc_handle) return fail(GPF_ERR_INVALID, "gpf_p2p_export: null argument");
    if (handle_bytes != sizeof(hipIpcMemHandle_t)) return fail(GPF_ERR_INVALID, "gpf_p2p_export: the handle buffer must hold 64 bytes");
    if (h->p2p.on) return fail(GPF_ERR_STATE, "gpf_p2p_export: already connected");
    GPF_TRY(enter(h));
    const size_t bytes = p2p_mailbox_bytes(h->L.pitch);
    if (!h->p2p.mine) {
        // fine-grained: peers' stores become visible to a kernel that is already running here
        HIP_TRY(hipExtMallocWithFlags((void**)&h->p2p.mine, bytes, hipDeviceMallocFinegrained));
    }
    HIP_TRY(hipMemset(h->p2p.mine, 0, bytes));
    HIP_TRY(hipDeviceSynchronize());
    hipIpcMemHandle_t hm;
    HIP_TRY(hipIpcGetMemHandle(&hm, h->p2p.mine));
    std::memcpy(ipc_handle, &hm, sizeof(hm));
    return GPF_OK;
}

extern "C" int gpf_p2p_connect(gpf_handle* h, int rank, int nranks, const void* ipc_handles, int rank_lo, int rank_hi) {
    if (!h || !ipc_handles) return fail(GPF_ERR_INVALID, "gpf_p2p_connect: null argument");
    if (nranks < 1 || nranks > P2P_MAX_RANKS) return fail(GPF_ERR_INVALID, "gpf_p2p_connect: 1 <= nranks <= 16");
    if (rank < 0 || rank >= nranks || rank_lo >= nranks || rank_hi >= nranks) return fail(GPF_ERR_INVALID, "gpf_p2p_connect: rank out of range");
    if (!h->p2p.mine) return fail(GPF_ERR_STATE, "gpf_p2p_connect: call gpf_p2p_export first");
    if (h->p2p.on) return fail(GPF_ERR_STATE, "gpf_p2p_connect: already connected");
    GPF_TRY(enter(h));
    const hipIpcMemHandle_t* hs = (const hipIpcMemHandle_t*)ipc_handles;
    for (int r = 0; r < nranks; ++r) {
        if (r == rank) { h->p2p.box[r] = h->p2p.mine; continue; }
        void* p = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&p, hs[r], hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            for (int k = 0; k < r; ++k)
                if (k != rank && h->p2p.box[k]) { hipIpcCloseMemHandle(h->p2p.box[k]); h->p2p.box[k] = nullptr; }
            return fail(GPF_ERR_HIP, std::string("gpf_p2p_connect: hipIpcOpenMemHandle(rank ") + std::to_string(r) + "): " + hipGetErrorString(e));
        }
        h->p2p.box[r] = (char*)p;
    }
    if (!h->p2p.seq) HIP_TRY(hipMalloc((void**)&h->p2p.seq, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(h->p2p.seq, 0, sizeof(unsigned long long)));
    HIP_TRY(hipDeviceSynchronize());
    h->p2p.nranks = nranks; h->p2p.rank = rank; h->p2p.rank_lo = rank_lo; h->p2p.rank_hi = rank_hi;
    h->p2p.on = true;
    return GPF_OK;
}

extern "C" int gpf_p2p_set_timeout(gpf_handle* h, double seconds) {
    if (!h || !(seconds > 0.0)) return fail(GPF_ERR_INVALID, "gpf_p2p_set_timeout: need a handle and a positive time");
    h->p2p_timeout_ticks = (long long)(seconds * 1e8);      // wall_clock64: 100 MHz
    return GPF_OK;
}

// n whole steps, exchanges included, enqueued without touching the host in between
extern "C" int gpf_step_p2p(gpf_handle* h, int64_t n, int honor_stop) {
    if (!h) return fail(GPF_ERR_INVALID, "gpf_step_p2p: null handle");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_step_p2p: call gpf_pre_run first");
    if (!h->p2p.on) return fail(GPF_ERR_STATE, "gpf_step_p2p: call gpf_p2p_export / gpf_p2p_connect first");
    if (n < 0) return fail(GPF_ERR_INVALID, "gpf_step_p2p: n < 0");
    if (h->cfg.thinning != GPF_THINNING_NONE) return fail(GPF_ERR_STATE, "gpf_step_p2p: shear thinning needs grad p; use the stage-wise slab calls");
    GPF_TRY(enter(h));
    GPF_TRY(ensure_halo(h));
    double* rec = h->halo + (size_t)6 * h->L.pitch;
    for (int64_t i = 0; i < n; ++i) GPF_TRY(enqueue_step(h, honor_stop, h->host_step, rec, nullptr, nullptr, true));
    return GPF_OK;
}

extern "C" int gpf_state(gpf_handle* h, gpf_scalars_t* out) {
    if (!h || !out) return fail(GPF_ERR_INVALID, "gpf_state: null argument");
    GPF_TRY(enter(h, true));
    StepState s;
    GPF_TRY(read_state(h, s));
    fill_scalars(s, nullptr, 0.0, out);
    h->host_step = s.step; h->next_step = s.step;
    return GPF_OK;
}

extern "C" int gpf_set_seam_topo(gpf_handle* h, int side, const double* host, size_t count) {
    if (!h || !host || side < 0 || side > 1) return fail(GPF_ERR_INVALID, "gpf_set_seam_topo: bad argument");
    const Layout& L = h->L;
    if (count != (size_t)8 * (L.Ny + 2)) return fail(GPF_ERR_INVALID, "gpf_set_seam_topo: count must be 2*4*(Ny+2)");
    GPF_TRY(enter(h));
    if (!h->seam) {
        HIP_TRY(hipMalloc(&h->seam, (size_t)16 * L.pitch * sizeof(double)));
        HIP_TRY(hipMemset(h->seam, 0, (size_t)16 * L.pitch * sizeof(double)));
    }
    std::vector<double> tmp((size_t)8 * L.pitch, 0.0);
    for (int r = 0; r < 8; ++r)
        for (int iy = 0; iy < L.Ny + 2; ++iy) tmp[(size_t)r * L.pitch + L.off + iy] = host[(size_t)r * (L.Ny + 2) + iy];
    HIP_TRY(hipMemcpy(h->seam + (size_t)side * 8 * L.pitch, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    h->has_seam[side] = true;
    if (h->rowcoef) {
        GPF_TRY(build_rowcoef(h, false, side));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return GPF_OK;
}
