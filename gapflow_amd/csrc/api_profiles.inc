// Part of api.hip (included there, not compiled on its own): through-gap velocity and stress profiles (models/profiles.py),
// as a stateless operator and on a handle's current state.  Kernels: profile_kernels.hip.

static int profile_nplanes(int mask) {
    return ((mask & PROFILE_F_Z) ? 1 : 0) + ((mask & PROFILE_F_U) ? 1 : 0) + ((mask & PROFILE_F_V) ? 1 : 0) + ((mask & PROFILE_F_TAU) ? 6 : 0);
}

static dim3 profile_grid(long long ncell, int nlev) {
    return dim3((unsigned)((ncell + 511) / 512), (unsigned)((nlev + PROFILE_LEVELS_PER_THREAD - 1) / PROFILE_LEVELS_PER_THREAD));
}

static constexpr int PROFILE_MAX_LEVELS = 65535 * PROFILE_LEVELS_PER_THREAD;

// The double-buffered device scratch that large results leave the device through (gpf_gap_profiles, the checkpoint calls):
// doubles per half (GPF_PROFILE_SCRATCH_MB MiB for both, default 256), and the pipeline over the chunks of a request -- the
// kernel of chunk c + 1 is queued into one half ahead of the copy of chunk c in the other, so nothing waits on the host.
static long long scratch_half_doubles() {
    const char* env = std::getenv("GPF_PROFILE_SCRATCH_MB");
    const double mb = env ? std::atof(env) : 256.0;
    return (long long)(std::max(mb, 0.0) * (1 << 20) / 16.0);
}
template <class Launch, class Copy>
static hipError_t run_double_buffered(hipStream_t stream, size_t nchunks, Launch launch, Copy copy) {
    hipError_t e = nchunks ? launch((size_t)0) : hipSuccess;
    for (size_t c = 0; c < nchunks && e == hipSuccess; ++c) {
        if (c + 1 < nchunks && (e = launch(c + 1)) != hipSuccess) break;      // into the other half
        e = copy(c);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    else (void)hipStreamSynchronize(stream);
    return e;
}

// get_velocity_profiles / get_stress_profiles (profiles.py:33-138, 141-1323) for n cells x nz levels
extern "C" int gpf_gap_profiles_op(int64_t n, int nz, const double* z, const double* q, const double* hh, const double* dqx,
                                   const double* dqy, const double* eta, const double* zeta, const double* Ls, int per_cell,
                                   double U, double V, int mode, int field_mask, double* out) {
    if (!z || !q || !eta || !zeta || !Ls || !out) return fail(GPF_ERR_INVALID, "gpf_gap_profiles_op: null argument");
    if (n < 1 || nz < 1 || nz > PROFILE_MAX_LEVELS) return fail(GPF_ERR_INVALID, "gpf_gap_profiles_op: n >= 1 and 1 <= nz <= 262140 required");
    if (mode < PROFILE_BOTH || mode > PROFILE_NONE) return fail(GPF_ERR_INVALID, "gpf_gap_profiles_op: unknown slip mode");
    if (field_mask < 1 || field_mask > 15) return fail(GPF_ERR_INVALID, "gpf_gap_profiles_op: field_mask must select 1..15");
    if (gpf_device_count() == 0) return fail(GPF_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    const size_t N = (size_t)n;
    auto count = [&](int bit, size_t comps) { return comps * (((per_cell >> bit) & 1) ? N : 1); };
    const size_t nin = count(0, 3) + (hh ? count(1, 3) : 0) + (dqx ? count(2, 3) : 0) + (dqy ? count(3, 3) : 0) + count(4, 1) +
                       count(5, 1) + count(6, 1) + count(7, (size_t)nz);
    const int np = profile_nplanes(field_mask);
    const long long pitch = (long long)((N + 1) & ~(size_t)1);
    const size_t nout = (size_t)np * nz * pitch;
    double* d = nullptr;
    HIP_TRY(hipMalloc(&d, (nin + nout + 2) * sizeof(double)));
    ProfileOpSource s;
    ProfileOut o;
    o.out = d;                                  // (first: 256-byte aligned)
    double* w = d + nout;
    hipError_t e = hipSuccess;
    auto put = [&](const double* host, size_t cnt) -> const double* {
        if (!host) return nullptr;
        double* dev = w;
        if (e == hipSuccess) e = hipMemcpy(dev, host, cnt * sizeof(double), hipMemcpyHostToDevice);
        w += cnt;
        return dev;
    };
    s.q = put(q, count(0, 3)); s.hh = put(hh, count(1, 3)); s.dqx = put(dqx, count(2, 3)); s.dqy = put(dqy, count(3, 3));
    s.eta = put(eta, count(4, 1)); s.zeta = put(zeta, count(5, 1)); s.Ls = put(Ls, count(6, 1)); s.z = put(z, count(7, (size_t)nz));
    int rc = GPF_OK;
    if (e != hipSuccess) {
        rc = fail(GPF_ERR_HIP, hipGetErrorString(e));
    } else {
        s.n = n; s.per_cell = per_cell; s.nz = nz; s.mode = mode; s.U = U; s.V = V;
        o.pitch = pitch; o.ncell = n; o.nlev = nz; o.mask = field_mask;
        hipLaunchKernelGGL(k_gap_profiles_op, profile_grid(n, nz), dim3(256), 0, 0, s, o);
        if ((e = hipGetLastError()) != hipSuccess ||
            (e = hipMemcpy2D(out, N * sizeof(double), d, (size_t)pitch * sizeof(double), N * sizeof(double), (size_t)np * nz,
                             hipMemcpyDeviceToHost)) != hipSuccess)
            rc = fail(GPF_ERR_HIP, hipGetErrorString(e));
    }
    hipFree(d);
    return rc;
}

// The handle's current state: ghosted rows [ix0, ix1), z_k = h k / (nz - 1), slip at the upper wall (stress.py:328-345).
// The output goes through a device scratch of GPF_PROFILE_SCRATCH_MB (default 256) in two halves: the kernel of the next
// chunk is queued into one half ahead of the copy of the chunk in the other, so nothing waits on the host between them, and
// a request of any size needs no more device memory than that.  A chunk is a run of rows with all levels or, when one row
// does not fit a half, one row and a run of levels.
extern "C" int gpf_gap_profiles(gpf_handle* h, int nz, int ix0, int ix1, int field_mask, int flags, double* host_out) {
    if (!h || !host_out) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: null argument");
    const Layout& L = h->L;
    if (nz < 2 || nz > PROFILE_MAX_LEVELS) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: 2 <= nz <= 262140 required");
    if (ix0 < 0 || ix1 > L.Nx + 2 || ix0 >= ix1) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: 0 <= ix0 < ix1 <= Nx + 2 required");
    if (field_mask < 1 || field_mask > 15) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: field_mask must select 1..15");
    if ((flags & ~GPF_PROFILE_GRADIENTS) != 0) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: unknown flag");
    if (!h->has_q || !h->has_topo) return fail(GPF_ERR_STATE, "gpf_gap_profiles: upload q and topography first");
    if (h->cfg.thinning != GPF_THINNING_NONE) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: shear thinning needs grad p (not supported)");
    if (h->gp[0].set || h->gp[1].set || h->gp[2].set) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: surrogate closures have no profile");
    if (h->E.halo[0] || h->E.halo[1]) return fail(GPF_ERR_INVALID, "gpf_gap_profiles: not on an x-slab");
    GPF_TRY(enter(h, true));
    int par = 0;
    GPF_TRY(current_parity(h, &par));
    const int np = profile_nplanes(field_mask);
    const int W = L.Ny + 2, nrows = ix1 - ix0;
    long long half = scratch_half_doubles();
    half = std::max(half, (long long)np * (W + 1));                                 // at least one (row, level) unit
    int R, Lv;
    if ((long long)np * nz * ((long long)W + 1) <= half) {
        R = (int)std::min<long long>(nrows, (half / ((long long)np * nz) - 1) / W);
        R = std::max(R, 1);
        Lv = nz;
    } else {
        R = 1;
        Lv = (int)std::min<long long>(nz, half / ((long long)np * (W + 1)));
    }
    const long long pitch = ((long long)R * W + 1) & ~1ll;
    const size_t bufd = (size_t)np * Lv * pitch;
    double* d = nullptr;
    HIP_TRY(hipMalloc(&d, 2 * bufd * sizeof(double)));
    int rc = GPF_OK;
    hipError_t e = hipSuccess;
    struct Chunk { int r0, rows, k0, lev; };
    std::vector<Chunk> chunks;
    for (int r0 = 0; r0 < nrows; r0 += R)
        for (int k0 = 0; k0 < nz; k0 += Lv) chunks.push_back({r0, std::min(R, nrows - r0), k0, std::min(Lv, nz - k0)});
    auto launch = [&](size_t c) {
        const Chunk& k = chunks[c];
        ProfileOut o;
        o.out = d + (c & 1) * bufd;
        o.ncell = (long long)k.rows * W;
        o.pitch = (o.ncell + 1) & ~1ll;
        o.nlev = k.lev; o.mask = field_mask;
        EOS_DISPATCH(h->cfg.eos, {
            ProfileGridSource<EOS_> s;
            s.q = h->q[par]; s.topo = h->topo; s.Ls = h->Ls; s.L = L; s.P = h->P; s.dx = h->cfg.dx; s.dy = h->cfg.dy;
            s.ix0 = ix0 + k.r0; s.width = W; s.nz = nz; s.k0 = k.k0; s.grad = (flags & GPF_PROFILE_GRADIENTS) ? 1 : 0;
            hipLaunchKernelGGL((k_gap_profiles<EOS_>), profile_grid(o.ncell, o.nlev), dim3(256), 0, h->stream, s, o);
        });
        return hipGetLastError();
    };
    auto copy = [&](size_t c) {
        const Chunk& k = chunks[c];
        const size_t ncell = (size_t)k.rows * W, cp = (ncell + 1) & ~(size_t)1;
        for (int f = 0; f < np; ++f) {
            double* dst = host_out + (((size_t)f * nz + k.k0) * nrows + k.r0) * W;
            const double* src = d + (c & 1) * bufd + (size_t)f * k.lev * cp;
            hipError_t r = hipMemcpy2DAsync(dst, (size_t)nrows * W * sizeof(double), src, cp * sizeof(double), ncell * sizeof(double),
                                            (size_t)k.lev, hipMemcpyDeviceToHost, h->stream);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    };
    e = run_double_buffered(h->stream, chunks.size(), launch, copy);
    if (e != hipSuccess) rc = fail(GPF_ERR_HIP, hipGetErrorString(e));
    hipFree(d);
    return rc;
}

// Diagnostic: k_profile_store_only over the grid k_gap_profiles uses for ncell cells x nlev levels x nplanes planes
extern "C" int gpf_profile_store_probe(int device, int64_t ncell, int nlev, int nplanes, int reps, double* ms_per_pass) {
    if (ncell < 1 || nlev < 1 || nlev > PROFILE_MAX_LEVELS || nplanes < 1 || nplanes > 9 || reps < 1 || !ms_per_pass)
        return fail(GPF_ERR_INVALID, "gpf_profile_store_probe: bad argument");
    if (gpf_device_count() == 0) return fail(GPF_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    HIP_TRY(hipSetDevice(device));
    ProfileOut o;
    o.ncell = ncell; o.pitch = (ncell + 1) & ~1ll; o.nlev = nlev; o.mask = 0;
    HIP_TRY(hipMalloc(&o.out, (size_t)nplanes * nlev * o.pitch * sizeof(double)));
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k_profile_store_only, profile_grid(ncell, nlev), dim3(256), 0, 0, o, nplanes);
    hipEventRecord(e0, 0);
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_profile_store_only, profile_grid(ncell, nlev), dim3(256), 0, 0, o, nplanes);
    hipEventRecord(e1, 0);
    hipError_t e = hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(o.out);
    if (e != hipSuccess) return fail(GPF_ERR_HIP, hipGetErrorString(e));
    *ms_per_pass = ms / reps;
    return GPF_OK;
}
