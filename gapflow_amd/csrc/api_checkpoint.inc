// Part of api.hip (included there, not compiled on its own): checkpoint of a handle's run -- everything the next step depends on,
// so that a handle made from the same configuration continues bit for bit (DESIGN.md 3.3d).  Kernels: checkpoint_kernels.hip.
//
// Blob: CkptHeader | StepState | [2][Ny+2] densities beyond the halo (thinning slabs) | planes, each [Nx+2][Ny+2] unpadded:
//   q[parity] (3) | q[1-parity] (3, when it is the state before the last fused step) | h, dh/dx, dh/dy (3) |
//   elastic gap: under-relaxed displacement, undeformed gap, deformation (3) | Ls (1) |
//   the 16 derived planes, when they hold the corrector-stage closures of this state and nothing on the device could form them
//   again (stage-wise steps; a fused step's are formed again from q[1-parity] and dt_last: gpf_update_closures).
static constexpr uint64_t CKPT_MAGIC = 0x3154504b43465047ull;       // "GPFCKPT1"
static constexpr uint32_t CKPT_VERSION = 1;
static constexpr int CKPT_MAX_PLANES = 32;
enum { CKPT_PREV = 1, CKPT_LS = 2, CKPT_ELASTIC = 4, CKPT_DERIVED = 8, CKPT_BEYOND = 16 };

struct CkptHeader {             // 8-byte members first: no implicit padding anywhere
    uint64_t magic;
    uint64_t total_bytes;
    uint64_t digest[CKPT_MAX_PLANES];       // one per plane, in blob order (checkpoint_kernels.hip)
    uint64_t state_digest;                  // of the StepState and the beyond rows, same mix over their 8-byte words
    int64_t fields_step;
    double dx, dy, U, V, eta, zeta, CFL, dt_fixed;
    double eos_par[8], piezo_par[4], thinning_par[4], bc_value[4];
    uint32_t version, header_bytes;
    int32_t Nx, Ny, ncomp_q, ncomp_topo;
    int32_t eos, piezo, thinning, flags;
    int32_t halo[2];
    int32_t mc_order, adaptive;
    int32_t bc_rule[4][3];
    int32_t nplanes, state_bytes;
    uint64_t header_digest;                 // of every byte above
};
static_assert(sizeof(CkptHeader) % 8 == 0, "CkptHeader must be a whole number of 8-byte words");

static uint64_t ckpt_host_digest(const void* p, size_t bytes) {
    uint64_t d = 0, w = 0;
    for (size_t i = 0; i + 8 <= bytes; i += 8) { std::memcpy(&w, (const char*)p + i, 8); d += ckpt_mix(i / 8, w); }
    return d;
}

struct CkptGroup { const char* name; double* base; int nplanes; };

static uint32_t ckpt_flags_of(const gpf_handle* h, const StepState& s) {
    uint32_t f = 0;
    if (h->prev_state_valid) f |= CKPT_PREV;
    if (h->Ls) f |= CKPT_LS;
    if (h->el.on) f |= CKPT_ELASTIC;
    if (h->fields && h->fields_step == s.step && !h->prev_state_valid) f |= CKPT_DERIVED;
    if (h->beyond) f |= CKPT_BEYOND;
    return f;
}

static std::vector<CkptGroup> ckpt_groups(gpf_handle* h, int parity, uint32_t flags) {
    std::vector<CkptGroup> g;
    g.push_back({"q", h->q[parity], 3});
    if (flags & CKPT_PREV) g.push_back({"previous q", h->q[parity ^ 1], 3});
    g.push_back({"gap", h->topo, 3});
    if (flags & CKPT_ELASTIC) g.push_back({"elastic displacement / undeformed gap / deformation", h->el.u_prev, 3});       // (one block: gpf_elastic_setup)
    if (flags & CKPT_LS) g.push_back({"slip length", h->Ls, 1});
    if (flags & CKPT_DERIVED) g.push_back({"derived fields", h->fields, 16});
    return g;
}

static int ckpt_nplanes(const std::vector<CkptGroup>& g) { int n = 0; for (auto& k : g) n += k.nplanes; return n; }

static void ckpt_fill_header(const gpf_handle* h, uint32_t flags, int nplanes, CkptHeader& H) {
    std::memset(&H, 0, sizeof(H));
    const gpf_config& c = h->cfg;
    const size_t W = (size_t)c.Ny + 2, plane_b = ((size_t)c.Nx + 2) * W * 8;
    H.magic = CKPT_MAGIC; H.version = CKPT_VERSION; H.header_bytes = (uint32_t)sizeof(CkptHeader);
    H.Nx = c.Nx; H.Ny = c.Ny; H.ncomp_q = 3; H.ncomp_topo = 3;
    H.eos = c.eos; H.piezo = c.piezo; H.thinning = c.thinning; H.flags = (int32_t)flags;
    H.halo[0] = c.halo_lo; H.halo[1] = c.halo_hi; H.mc_order = c.mc_order; H.adaptive = c.adaptive;
    H.dx = c.dx; H.dy = c.dy; H.U = c.U; H.V = c.V; H.eta = c.eta; H.zeta = c.zeta; H.CFL = c.CFL; H.dt_fixed = c.dt_fixed;
    std::memcpy(H.eos_par, c.eos_par, sizeof(H.eos_par)); std::memcpy(H.piezo_par, c.piezo_par, sizeof(H.piezo_par));
    std::memcpy(H.thinning_par, c.thinning_par, sizeof(H.thinning_par)); std::memcpy(H.bc_value, c.bc_value, sizeof(H.bc_value));
    std::memcpy(H.bc_rule, c.bc_rule, sizeof(H.bc_rule));
    H.nplanes = nplanes;
    H.state_bytes = (int32_t)(sizeof(StepState) + ((flags & CKPT_BEYOND) ? 2 * W * 8 : 0));
    H.total_bytes = sizeof(CkptHeader) + (size_t)H.state_bytes + (size_t)nplanes * plane_b;
    H.fields_step = h->fields_step;
}

// Rows of a chunk and the stage geometry for `np` planes of width W in one half of the scratch (half: doubles).
struct CkptStage { int rows; long long stride; int shift; };
static CkptStage ckpt_stage(int np, int nxg, int W, long long half) {
    CkptStage s;
    s.shift = (W & 1) ? 0 : 1;                  // column 1 of every row on a 16-byte boundary (see checkpoint_kernels.hip)
    long long rows = (half / np - 4) / W;
    rows = std::min<long long>(rows, 2000000000ll / (W / 2 + 1));           // 32-bit item index in the kernels
    s.rows = (int)std::max<long long>(1, std::min<long long>(rows, nxg));
    s.stride = ((long long)s.rows * W + 3) & ~1ll;
    return s;
}

struct CkptScratch {
    double* d = nullptr; unsigned long long* digest = nullptr; long long half = 0;
    ~CkptScratch() { if (d) hipFree(d); if (digest) hipFree(digest); }
};
static int ckpt_scratch(gpf_handle* h, const std::vector<CkptGroup>& groups, CkptScratch& S) {
    const int nxg = h->L.Nx + 2, W = h->L.Ny + 2;
    long long need = 0;
    for (auto& g : groups) need = std::max(need, (long long)g.nplanes * ((long long)nxg * W + 8));
    S.half = std::min(std::max(scratch_half_doubles(), 16ll * (W + 4)), need);
    S.half = (S.half + 31) & ~31ll;
    HIP_TRY(hipMalloc(&S.d, 2 * (size_t)S.half * sizeof(double)));
    HIP_TRY(hipMalloc(&S.digest, CKPT_MAX_PLANES * sizeof(unsigned long long)));
    return GPF_OK;
}

struct CkptChunk { int group, plane0, r0, rows; CkptStage st; };
static std::vector<CkptChunk> ckpt_chunks(const gpf_handle* h, const std::vector<CkptGroup>& groups, long long half) {
    std::vector<CkptChunk> chunks;
    const int nxg = h->L.Nx + 2, W = h->L.Ny + 2;
    int plane0 = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const CkptStage st = ckpt_stage(groups[g].nplanes, nxg, W, half);
        for (int r0 = 0; r0 < nxg; r0 += st.rows) chunks.push_back({(int)g, plane0, r0, std::min(st.rows, nxg - r0), st});
        plane0 += groups[g].nplanes;
    }
    return chunks;
}

static CkptArgs ckpt_args(const gpf_handle* h, const CkptGroup& g, const CkptChunk& k, double* half_base, unsigned long long* digest, bool with_field) {
    CkptArgs a;
    a.field = with_field ? g.base : nullptr; a.plane_stride = h->L.plane;
    a.stage = half_base + k.st.shift; a.stage_stride = k.st.stride;
    a.digest = digest + k.plane0;
    a.pitch = h->L.pitch; a.off = h->L.off; a.W = h->L.Ny + 2;
    a.row0 = k.r0; a.rows = k.rows; a.nplanes = g.nplanes;
    return a;
}
static dim3 ckpt_grid(const CkptChunk& k, int W) {
    const long long n = (long long)k.rows * (W / 2 + 1);
    return dim3((unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 2048)));
}

extern "C" int gpf_checkpoint_size(gpf_handle* h, size_t* bytes) {
    if (!h || !bytes) return fail(GPF_ERR_INVALID, "gpf_checkpoint_size: null argument");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_checkpoint_size: call gpf_pre_run first");
    GPF_TRY(enter(h, true));
    StepState s;
    GPF_TRY(read_state(h, s));
    const uint32_t flags = ckpt_flags_of(h, s);
    CkptHeader H;
    ckpt_fill_header(h, flags, ckpt_nplanes(ckpt_groups(h, s.parity, flags)), H);
    *bytes = (size_t)H.total_bytes;
    return GPF_OK;
}

extern "C" int gpf_checkpoint_save(gpf_handle* h, void* host, size_t capacity, size_t* written) {
    if (!h || !host) return fail(GPF_ERR_INVALID, "gpf_checkpoint_save: null argument");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_checkpoint_save: call gpf_pre_run first");
    if (h->step_open) return fail(GPF_ERR_STATE, "gpf_checkpoint_save: a stage-wise step is open; close it first");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set) return fail(GPF_ERR_INVALID, "gpf_checkpoint_save: surrogate models are not saved");
    if (h->els.on) return fail(GPF_ERR_INVALID, "gpf_checkpoint_save: elastic slabs are not saved");
    GPF_TRY(enter(h, true));
    const Layout& L = h->L;
    const int nxg = L.Nx + 2, W = L.Ny + 2;
    StepState s;
    GPF_TRY(read_state(h, s));
    const uint32_t flags = ckpt_flags_of(h, s);
    const std::vector<CkptGroup> groups = ckpt_groups(h, s.parity, flags);
    CkptHeader H;
    ckpt_fill_header(h, flags, ckpt_nplanes(groups), H);
    if (H.nplanes > CKPT_MAX_PLANES) return fail(GPF_ERR_INVALID, "gpf_checkpoint_save: too many planes");
    if (capacity < H.total_bytes) return fail(GPF_ERR_INVALID, "gpf_checkpoint_save: capacity below gpf_checkpoint_size");
    char* out = (char*)host;
    char* state = out + sizeof(CkptHeader);
    std::memcpy(state, &s, sizeof(s));
    if (flags & CKPT_BEYOND)
        for (int side = 0; side < 2; ++side)
            HIP_TRY(hipMemcpy(state + sizeof(s) + (size_t)side * W * 8, h->beyond + (size_t)side * L.pitch + L.off, (size_t)W * 8, hipMemcpyDeviceToHost));
    H.state_digest = ckpt_host_digest(state, (size_t)H.state_bytes);
    double* planes = (double*)(state + H.state_bytes);
    const size_t plane_d = (size_t)nxg * W;

    CkptScratch S;
    GPF_TRY(ckpt_scratch(h, groups, S));
    HIP_TRY(hipMemsetAsync(S.digest, 0, CKPT_MAX_PLANES * sizeof(unsigned long long), h->stream));
    const std::vector<CkptChunk> chunks = ckpt_chunks(h, groups, S.half);
    auto launch = [&](size_t c) {
        const CkptChunk& k = chunks[c];
        hipLaunchKernelGGL(k_ckpt_pack, ckpt_grid(k, W), dim3(256), 0, h->stream, ckpt_args(h, groups[k.group], k, S.d + (c & 1) * S.half, S.digest, true));
        return hipGetLastError();
    };
    auto copy = [&](size_t c) {
        const CkptChunk& k = chunks[c];
        const double* stage = S.d + (c & 1) * S.half + k.st.shift;
        for (int p = 0; p < groups[k.group].nplanes; ++p) {
            hipError_t r = hipMemcpyAsync(planes + (size_t)(k.plane0 + p) * plane_d + (size_t)k.r0 * W, stage + p * k.st.stride,
                                          (size_t)k.rows * W * 8, hipMemcpyDeviceToHost, h->stream);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    };
    hipError_t e = run_double_buffered(h->stream, chunks.size(), launch, copy);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_checkpoint_save: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpy(H.digest, S.digest, (size_t)H.nplanes * sizeof(uint64_t), hipMemcpyDeviceToHost));
    H.header_digest = ckpt_host_digest(&H, offsetof(CkptHeader, header_digest));
    std::memcpy(out, &H, sizeof(H));
    if (written) *written = (size_t)H.total_bytes;
    return GPF_OK;
}

// the name of plane p of a blob with these groups, for messages
static std::string ckpt_plane_name(const std::vector<CkptGroup>& groups, int p) {
    for (auto& g : groups) {
        if (p < g.nplanes) return std::string(g.name) + (g.nplanes > 1 ? " [" + std::to_string(p) + "]" : "");
        p -= g.nplanes;
    }
    return "?";
}

extern "C" int gpf_checkpoint_load(gpf_handle* h, const void* host, size_t bytes) {
    if (!h || !host) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: null argument");
    if (!h->pre_run_done) return fail(GPF_ERR_STATE, "gpf_checkpoint_load: call gpf_pre_run first");
    if (h->step_open) return fail(GPF_ERR_STATE, "gpf_checkpoint_load: a stage-wise step is open");
    // The mailboxes of a connected peer-to-peer slab carry sequence numbers that all ranks advance together; one rank cannot put
    // its own back without its peers seeing a flag value they have passed.
    if (h->p2p.on) return fail(GPF_ERR_STATE, "gpf_checkpoint_load: not on a handle connected for the peer-to-peer transport (load before gpf_p2p_connect "
                                              "is not supported either: use the all-gather transport to restart)");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set || h->els.on) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: surrogate models and elastic slabs are not restored");
    const char* in = (const char*)host;
    if (bytes < sizeof(CkptHeader)) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: truncated blob (shorter than its header)");
    CkptHeader B;
    std::memcpy(&B, in, sizeof(B));
    if (B.magic != CKPT_MAGIC) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: header: field 'magic' differs (not a checkpoint)");
    if (B.version != CKPT_VERSION) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: header: field 'version' differs (written by format " + std::to_string(B.version) + ")");
    if (B.header_bytes != sizeof(CkptHeader)) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: header: field 'header_bytes' differs");
    if (B.header_digest != ckpt_host_digest(&B, offsetof(CkptHeader, header_digest)))
        return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: header: its digest does not match (damaged header)");
    GPF_TRY(enter(h, true));
    StepState cur;
    GPF_TRY(read_state(h, cur));
    // what this handle's own checkpoint header would say, with the blob's choice of optional planes
    uint32_t mine = (uint32_t)B.flags & (CKPT_PREV | CKPT_DERIVED);
    if (h->Ls) mine |= CKPT_LS;
    if (h->el.on) mine |= CKPT_ELASTIC;
    if (h->beyond) mine |= CKPT_BEYOND;
    CkptHeader H;
    ckpt_fill_header(h, mine, 0, H);
    const char* diff = nullptr;
#define CKPT_CMP(member, name) if (!diff && std::memcmp(&H.member, &B.member, sizeof(H.member)) != 0) diff = name
    CKPT_CMP(Nx, "Nx"); CKPT_CMP(Ny, "Ny"); CKPT_CMP(ncomp_q, "ncomp_q"); CKPT_CMP(ncomp_topo, "ncomp_topo");
    CKPT_CMP(eos, "eos"); CKPT_CMP(eos_par, "eos_par"); CKPT_CMP(piezo, "piezo"); CKPT_CMP(piezo_par, "piezo_par");
    CKPT_CMP(thinning, "thinning"); CKPT_CMP(thinning_par, "thinning_par");
    CKPT_CMP(U, "U"); CKPT_CMP(V, "V"); CKPT_CMP(eta, "eta"); CKPT_CMP(zeta, "zeta"); CKPT_CMP(dx, "dx"); CKPT_CMP(dy, "dy");
    CKPT_CMP(bc_rule, "bc_rule"); CKPT_CMP(bc_value, "bc_value"); CKPT_CMP(halo, "halo");
    CKPT_CMP(mc_order, "mc_order"); CKPT_CMP(adaptive, "adaptive"); CKPT_CMP(CFL, "CFL"); CKPT_CMP(dt_fixed, "dt_fixed");
#undef CKPT_CMP
    if (!diff && ((mine ^ (uint32_t)B.flags) & CKPT_LS)) diff = "slip-length field present";
    if (!diff && ((mine ^ (uint32_t)B.flags) & CKPT_ELASTIC)) diff = "elastic gap present";
    if (!diff && ((mine ^ (uint32_t)B.flags) & CKPT_BEYOND)) diff = "rows beyond the halo present";
    if (diff) return fail(GPF_ERR_INVALID, std::string("gpf_checkpoint_load: header: field '") + diff + "' differs from this handle's configuration");
    const std::vector<CkptGroup> shape = ckpt_groups(h, 0, (uint32_t)B.flags);
    ckpt_fill_header(h, (uint32_t)B.flags, ckpt_nplanes(shape), H);
    if (B.nplanes != H.nplanes || B.state_bytes != H.state_bytes || B.total_bytes != H.total_bytes)
        return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: header: field 'nplanes' / 'total_bytes' differs from what its flags imply");
    if (bytes < B.total_bytes) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: truncated blob (" + std::to_string(bytes) + " of " + std::to_string(B.total_bytes) + " bytes)");
    if (bytes != B.total_bytes) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: header: field 'total_bytes' differs from the length given");
    const char* state = in + sizeof(CkptHeader);
    if (B.state_digest != ckpt_host_digest(state, (size_t)B.state_bytes))
        return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: digest of the run state does not match (damaged blob)");
    StepState s;
    std::memcpy(&s, state, sizeof(s));
    if (s.parity != 0 && s.parity != 1) return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: run state: parity out of range");

    const Layout& L = h->L;
    const int nxg = L.Nx + 2, W = L.Ny + 2;
    const size_t plane_d = (size_t)nxg * W;
    const double* planes = (const double*)(state + B.state_bytes);
    if (B.flags & CKPT_DERIVED) GPF_TRY(ensure_fields(h));
    const std::vector<CkptGroup> groups = ckpt_groups(h, s.parity, (uint32_t)B.flags);
    CkptScratch S;
    GPF_TRY(ckpt_scratch(h, groups, S));
    const std::vector<CkptChunk> chunks = ckpt_chunks(h, groups, S.half);
    uint64_t got[CKPT_MAX_PLANES];
    // pass 0: the blob as it arrived on the device, digested in the staging buffer -- the handle is not touched;
    // pass 1: into the handle's planes, digested from what stands there afterwards
    // Once pass 1 has begun, any failure leaves the planes half-written: the handle then asks for a fresh upload.
    auto spoiled = [&](int rc) { h->has_q = false; h->pre_run_done = false; prev_state_lost(h); h->fields_step = -1; return rc; };
    for (int pass = 0; pass < 2; ++pass) {
        auto run_pass = [&]() -> int {
            HIP_TRY(hipMemsetAsync(S.digest, 0, CKPT_MAX_PLANES * sizeof(unsigned long long), h->stream));
            for (size_t c = 0; c < chunks.size(); ++c) {
                const CkptChunk& k = chunks[c];
                double* stage = S.d + (c & 1) * S.half + k.st.shift;
                for (int p = 0; p < groups[k.group].nplanes; ++p)
                    HIP_TRY(hipMemcpyAsync(stage + p * k.st.stride, planes + (size_t)(k.plane0 + p) * plane_d + (size_t)k.r0 * W, (size_t)k.rows * W * 8,
                                           hipMemcpyHostToDevice, h->stream));
                hipLaunchKernelGGL(k_ckpt_unpack, ckpt_grid(k, W), dim3(256), 0, h->stream,
                                   ckpt_args(h, groups[k.group], k, S.d + (c & 1) * S.half, S.digest, pass == 1));
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipMemcpyAsync(got, S.digest, (size_t)B.nplanes * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            return GPF_OK;
        };
        const int rc = run_pass();
        if (rc != GPF_OK) return pass == 1 ? spoiled(rc) : rc;
        for (int p = 0; p < B.nplanes; ++p) {
            if (got[p] == B.digest[p]) continue;
            if (pass == 0)
                return fail(GPF_ERR_INVALID, "gpf_checkpoint_load: digest of plane '" + ckpt_plane_name(groups, p) + "' does not match what arrived on the device (damaged blob)");
            return spoiled(fail(GPF_ERR_HIP, "gpf_checkpoint_load: digest of plane '" + ckpt_plane_name(groups, p) + "' does not match what was written into the handle; "
                                             "upload q and the gap and call gpf_pre_run again"));
        }
    }
    // the run state; when to stop is this handle's own (a restart may run further than the saved run was allowed to)
    s.tol = cur.tol; s.max_it = cur.max_it;
    bool conv = true;
    for (int i = 0; i < s.rcount && i < 5; ++i) conv = conv && (s.rbuf[i] < s.tol);
    s.converged = conv ? 1 : 0;
    GPF_TRY(write_state(h, s));
    if (B.flags & CKPT_BEYOND) {
        std::vector<double> rows((size_t)4 * L.pitch, 0.0);
        for (int part = 0; part < 2; ++part)
            for (int side = 0; side < 2; ++side)
                std::memcpy(&rows[(size_t)(2 * part + side) * L.pitch + L.off], state + sizeof(s) + (size_t)side * W * 8, (size_t)W * 8);
        HIP_TRY(hipMemcpy(h->beyond, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    // everything the handle derives from the gap, as an upload of the gap does
    int gap0 = (B.flags & CKPT_PREV) ? 6 : 3;
    GPF_TRY(derive_from_topo(h, planes + (size_t)gap0 * plane_d));
    for (int e = 0; e < 2; ++e)
        if (h->rowcoef && h->has_seam[e]) GPF_TRY(build_rowcoef(h, false, e));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->has_q = true; h->has_topo = true;
    h->host_step = s.step; h->next_step = s.step;
    prev_state_after(h, (B.flags & CKPT_PREV) != 0);
    h->g1_ready = false;
    h->gp_state_mean_valid = false;
    h->fields_step = (B.flags & CKPT_DERIVED) ? s.step : -1;
    h->fields_restored = (B.flags & CKPT_DERIVED) != 0;       // otherwise the derived fields are stale: gpf_update_closures forms them again
    return stats_restart(h, s.step);        // accumulators are not part of a checkpoint: armed statistics begin a new window here
}

// Diagnostic: one pass of k_ckpt_pack over the three planes of the current q, chunked through the scratch as gpf_checkpoint_save
// does, without the copies to the host (tools/checkpoint_time.py sets it beside gpf_stream_probe with 3 planes in and out).
extern "C" int gpf_checkpoint_pack_probe(gpf_handle* h, int reps, double* ms_per_pass) {
    if (!h || !ms_per_pass || reps < 1) return fail(GPF_ERR_INVALID, "gpf_checkpoint_pack_probe: bad argument");
    if (!h->has_q) return fail(GPF_ERR_STATE, "gpf_checkpoint_pack_probe: upload q first");
    GPF_TRY(enter(h, true));
    int par = 0;
    GPF_TRY(current_parity(h, &par));
    const int W = h->L.Ny + 2;
    const std::vector<CkptGroup> groups = {{"q", h->q[par], 3}};
    CkptScratch S;
    GPF_TRY(ckpt_scratch(h, groups, S));
    const std::vector<CkptChunk> chunks = ckpt_chunks(h, groups, S.half);
    HIP_TRY(hipMemsetAsync(S.digest, 0, CKPT_MAX_PLANES * sizeof(unsigned long long), h->stream));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    auto pass = [&]() {
        for (size_t c = 0; c < chunks.size(); ++c)
            hipLaunchKernelGGL(k_ckpt_pack, ckpt_grid(chunks[c], W), dim3(256), 0, h->stream, ckpt_args(h, groups[0], chunks[c], S.d + (c & 1) * S.half, S.digest, true));
    };
    pass();
    hipEventRecord(e0, h->stream);
    for (int r = 0; r < reps; ++r) pass();
    hipEventRecord(e1, h->stream);
    hipError_t e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipGetLastError();
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, std::string("gpf_checkpoint_pack_probe: ") + hipGetErrorString(e));
    *ms_per_pass = ms / reps;
    return GPF_OK;
}
