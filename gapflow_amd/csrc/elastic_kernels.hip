// Elastic half-space deformation of the gap (GaPFlow/topography.py:257-280, 404-437): the convolution of the film
// pressure with the half-space Green's function on the device.  The Green's function arrives in Fourier space from the
// host (gapflow_amd/elastic.py); the transforms are hipFFT's (a plain library FFT, loaded with dlopen like rocBLAS), the
// rest are the small kernels below.  Not HBM- or MFMA-critical: two real-to-complex transforms of the (doubled) grid per
// time step next to a stage-wise step of ~15 passes.
#pragma once
#include <dlfcn.h>
#include <mutex>
#include <hip/hip_runtime.h>

namespace gpf {

struct FftLib {
    typedef int (*plan2d_t)(void**, int, int, int);
    typedef int (*exec_d2z_t)(void*, double*, double2*);
    typedef int (*exec_z2d_t)(void*, double2*, double*);
    typedef int (*set_stream_t)(void*, hipStream_t);
    typedef int (*destroy_t)(void*);
    // batched 1-D transforms of the x-slab form (gpf_elastic_slab_*): hipfftPlanMany, hipfftExecZ2Z
    typedef int (*plan_many_t)(void**, int, int*, int*, int, int, int*, int, int, int, int);
    typedef int (*exec_z2z_t)(void*, double2*, double2*, int);
    plan2d_t plan2d = nullptr; exec_d2z_t d2z = nullptr; exec_z2d_t z2d = nullptr; set_stream_t set_stream = nullptr; destroy_t destroy = nullptr;
    plan_many_t plan_many = nullptr; exec_z2z_t z2z = nullptr;
    bool ok = false;
    const char* err = "";
};
enum { HIPFFT_Z2Z_ = 0x69, HIPFFT_D2Z_ = 0x6a, HIPFFT_Z2D_ = 0x6c };     // hipfft.h: hipfftType
enum { HIPFFT_FORWARD_ = -1, HIPFFT_BACKWARD_ = 1 };

inline void fftlib_load(FftLib& F) {
    void* hd = nullptr;
    hd = dlopen("libhipfft.so.0", RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);                         // an image already mapped wins (roclibs())
    if (!hd) if (const char* path = getenv("GPF_HIPFFT_PATH")) hd = dlopen(path, RTLD_NOW | RTLD_GLOBAL);   // the copy PyTorch bundles
    if (!hd) hd = dlopen("libhipfft.so.0", RTLD_NOW | RTLD_GLOBAL);
    if (!hd) hd = dlopen("libhipfft.so", RTLD_NOW | RTLD_GLOBAL);
    if (!hd) hd = dlopen("/opt/rocm/lib/libhipfft.so", RTLD_NOW | RTLD_GLOBAL);
    if (!hd) { F.err = "could not dlopen hipFFT"; return; }
    F.plan2d = (FftLib::plan2d_t)dlsym(hd, "hipfftPlan2d");
    F.d2z = (FftLib::exec_d2z_t)dlsym(hd, "hipfftExecD2Z");
    F.z2d = (FftLib::exec_z2d_t)dlsym(hd, "hipfftExecZ2D");
    F.set_stream = (FftLib::set_stream_t)dlsym(hd, "hipfftSetStream");
    F.destroy = (FftLib::destroy_t)dlsym(hd, "hipfftDestroy");
    F.plan_many = (FftLib::plan_many_t)dlsym(hd, "hipfftPlanMany");
    F.z2z = (FftLib::exec_z2z_t)dlsym(hd, "hipfftExecZ2Z");
    F.ok = F.plan2d && F.d2z && F.z2d && F.set_stream && F.destroy && F.plan_many && F.z2z;
    if (!F.ok) F.err = "hipFFT symbols missing";
}

// Loaded exactly once, whichever thread asks first (the ranks of a ThreadWorld set up their handles concurrently); the
// others wait until the struct is filled.
inline FftLib& fftlib() {
    static FftLib F;
    static std::once_flag once;
    std::call_once(once, [] { fftlib_load(F); });
    return F;
}

// hipFFT plan creation is serialised in this library (the slab form's setup runs on several threads at once)
inline std::mutex& fft_plan_mutex() {
    static std::mutex m;
    return m;
}

// forces = (p - p_ref) on the (Nx+2) x (Ny+2) corner of the transform grid, zero elsewhere (the doubled part)
__global__ void k_el_pack(const double* p, Layout L, int px, int py, int relative, double* dense) {
    const long long n = (long long)px * py;
    const double pref = relative ? p[L.at(0, 0)] : 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int ix = (int)(i / py), iy = (int)(i % py);
        dense[i] = (ix < L.Nx + 2 && iy < L.Ny + 2) ? p[L.at(ix, iy)] - pref : 0.0;
    }
}

__global__ void k_el_multiply(double2* f, const double2* g, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double2 a = f[i], b = g[i];
        f[i] = make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
    }
}

// u_relaxed = (1 - alpha) u_prev + alpha u_computed  (topography.py:419-437), u_computed = scale * inverse transform
__global__ void k_el_relax(const double* dense, int py, double scale, double alpha, Layout L, double* u_prev) {
    const long long w = L.Ny + 2, n = (long long)(L.Nx + 2) * w;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int ix = (int)(i / w), iy = (int)(i % w);
        const long long o = L.at(ix, iy);
        u_prev[o] = (1.0 - alpha) * u_prev[o] + alpha * (scale * dense[(long long)ix * py + iy]);
    }
}

// deformation = u_relaxed (minus its value at [0, 0] unless fully periodic); h = h_undeformed + deformation
__global__ void k_el_apply(const double* u_prev, const double* h0, int relative, Layout L, double* deformation, double* h) {
    const long long w = L.Ny + 2, n = (long long)(L.Nx + 2) * w;
    const double uref = relative ? u_prev[L.at(0, 0)] : 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long o = L.at((int)(i / w), (int)(i % w));
        const double d = u_prev[o] - uref;
        deformation[o] = d;
        h[o] = h0[o] + d;
    }
}

// np.gradient(h, axis) / spacing: central differences, one-sided at the two ends of the array (ghost cells included;
// topography.py:273-280).  A one-cell axis has no gradient in the reference either (np.gradient needs two points): the
// solver never gets there because Nx, Ny >= 1 means at least three points with the ghost cells.
__global__ void k_el_gradient(const double* h, Layout L, double inv_dx, double inv_dy, double* hx, double* hy) {
    const long long w = L.Ny + 2, n = (long long)(L.Nx + 2) * w;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int ix = (int)(i / w), iy = (int)(i % w);
        const int xm = ix > 0 ? ix - 1 : ix, xp = ix < L.Nx + 1 ? ix + 1 : ix;
        const int ym = iy > 0 ? iy - 1 : iy, yp = iy < L.Ny + 1 ? iy + 1 : iy;
        const long long o = L.at(ix, iy);
        hx[o] = (h[L.at(xp, iy)] - h[L.at(xm, iy)]) / (double)(xp - xm) * inv_dx;
        hy[o] = (h[L.at(ix, yp)] - h[L.at(ix, ym)]) / (double)(yp - ym) * inv_dy;
    }
}

// ---------------------------------------------------------------------------------------------
// x-slab form (gpf_elastic_slab_*): the 2-D transform as 1-D y-transforms of the rows a rank owns, a transpose to ky column
// slabs (all-to-all), 1-D x-transforms there, and a transpose back to the rows each rank needs.  The kernels below only
// move data; they are bandwidth kernels on 16-byte double2 elements, coalesced along the contiguous index of both sides
// (a ky column slice of a row is contiguous in both the [row][ky] and the [dest][row][local ky] layouts, so no LDS tile
// is needed).
// ---------------------------------------------------------------------------------------------

// ky column c of [0, nky) -> owning rank: the first `rem` ranks hold base+1 columns, the rest base (gapflow_amd/elastic.py:
// ky_partition); a rank may hold none
struct KySplit {
    int nky, nranks, base, rem;
    __host__ __device__ KySplit(int nky_, int nranks_) : nky(nky_), nranks(nranks_), base(nky_ / nranks_), rem(nky_ % nranks_) {}
    __host__ __device__ __forceinline__ int start(int s) const { return s * base + (s < rem ? s : rem); }
    __host__ __device__ __forceinline__ int count(int s) const { return base + (s < rem ? 1 : 0); }
    __host__ __device__ __forceinline__ int owner(int c) const {
        const int big = rem * (base + 1);
        return c < big ? c / (base + 1) : rem + (c - big) / base;      // base == 0 implies c < big
    }
};

// forces of the transform rows this rank owns, as zero-padded lines of length py: dense[j][iy] = p(row lrow0 + j, iy) - p_ref
// (p_ref: rank 0's pressure at global cell [0, 0], slot 7 of its step record, when relative)
__global__ void k_els_pack(const double* p, Layout L, int lrow0, int nrows, int py, const double* pref_slot, double* dense) {
    const long long n = (long long)nrows * py;
    const double pref = pref_slot ? *pref_slot : 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i / py), iy = (int)(i % py);
        dense[i] = iy < L.Ny + 2 ? p[L.at(lrow0 + j, iy)] - pref : 0.0;
    }
}

// transpose 1, send side: spec[j][c] (nrows x nky) -> send[dest s][j][c - k0(s)]; chunk s starts at nrows * k0(s)
__global__ void k_els_col_pack(const double2* spec, int nrows, KySplit K, double2* send) {
    const long long n = (long long)nrows * K.nky;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i / K.nky), c = (int)(i % K.nky);
        const int s = K.owner(c), k0 = K.start(s);
        send[(long long)nrows * k0 + (long long)j * K.count(s) + (c - k0)] = spec[i];
    }
}

// transpose 2, send side: the x rows every rank asked for, in rank order, each a contiguous run of this rank's nk columns
__global__ void k_els_row_pack(const double2* spec, int nk, const int* rows, int nrows_all, double2* send) {
    const long long n = (long long)nrows_all * nk;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / nk), k = (int)(i % nk);
        send[i] = spec[(long long)rows[t] * nk + k];
    }
}

// transpose 2, receive side: chunk s = [j][c - k0(s)] at nret * k0(s) -> line[j][c] (nret x nky), the input of the batched Z2D
__global__ void k_els_unpack(const double2* recv, int nret, KySplit K, double2* line) {
    const long long n = (long long)nret * K.nky;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i / K.nky), c = (int)(i % K.nky);
        const int s = K.owner(c), k0 = K.start(s);
        line[i] = recv[(long long)nret * k0 + (long long)j * K.count(s) + (c - k0)];
    }
}

// k_el_relax on the compact [nret][Ny+2] rows; the relaxed displacement of row ref_row, column 0 (global cell [0, 0] on
// rank 0) also goes to ref_out for the all-gather that hands it to every rank
__global__ void k_els_relax(const double* dense, int nret, int ny, int py, double scale, double alpha, double* u_prev,
                            int ref_row, double* ref_out) {
    const long long n = (long long)nret * ny;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i / ny), iy = (int)(i % ny);
        const double u = (1.0 - alpha) * u_prev[i] + alpha * (scale * dense[(long long)j * py + iy]);
        u_prev[i] = u;
        if (j == ref_row && iy == 0) ref_out[0] = u;
    }
}

// k_el_apply + k_el_gradient for a run of consecutive global rows held at compact rows [jbase, ...): h = h0 + (u - u_ref) of
// global row g, and np.gradient's stencil clipped to the domain's rows [0, Nx+1]
struct ElRows {
    const double* u_prev; const double* h0;
    int ny, jbase, gbase, Nxg;
    double uref;
    __device__ __forceinline__ double d(int g, int iy) const { const long long o = (long long)(jbase + g - gbase) * ny + iy; return u_prev[o] - uref; }
    __device__ __forceinline__ double h(int g, int iy) const { return h0[(long long)(jbase + g - gbase) * ny + iy] + d(g, iy); }
    __device__ __forceinline__ void eval(int g, int iy, double inv_dx, double inv_dy, double& dd, double& hh, double& hx, double& hy) const {
        const int xm = g > 0 ? g - 1 : g, xp = g < Nxg + 1 ? g + 1 : g;
        const int ym = iy > 0 ? iy - 1 : iy, yp = iy < ny - 1 ? iy + 1 : iy;
        dd = d(g, iy);
        hh = h0[(long long)(jbase + g - gbase) * ny + iy] + dd;
        hx = (h(xp, iy) - h(xm, iy)) / (double)(xp - xm) * inv_dx;
        hy = (h(g, yp) - h(g, ym)) / (double)(yp - ym) * inv_dy;
    }
};

// the slab's own rows 0..Nx+1 (global g_lo + ix): deformation, h, dh/dx, dh/dy planes
__global__ void k_els_apply(ElRows R, const double* uref_slot, int g_lo, Layout L, double inv_dx, double inv_dy,
                            double* deformation, double* topo) {
    if (uref_slot) R.uref = *uref_slot;
    const long long n = (long long)(L.Nx + 2) * R.ny;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int ix = (int)(i / R.ny), iy = (int)(i % R.ny);
        double dd, hh, hx, hy;
        R.eval(g_lo + ix, iy, inv_dx, inv_dy, dd, hh, hx, hy);
        const long long o = L.at(ix, iy);
        deformation[o] = dd;
        topo[o] = hh; topo[L.plane + o] = hx; topo[2 * L.plane + o] = hy;
    }
}

// the seam block of a periodic slab edge ([2 rows][4: h,hx,hy,Ls][pitch], gpf_set_seam_topo): h, dh/dx, dh/dy of its two
// global rows g0, g1 from the three deformed rows held for it (Ls stays)
__global__ void k_els_seam(ElRows R, const double* uref_slot, int g0, int g1, Layout L, double inv_dx, double inv_dy, double* seam) {
    if (uref_slot) R.uref = *uref_slot;
    const long long n = 2ll * R.ny;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / R.ny), iy = (int)(i % R.ny);
        double dd, hh, hx, hy;
        R.eval(r == 0 ? g0 : g1, iy, inv_dx, inv_dy, dd, hh, hx, hy);
        double* b = seam + (long long)r * 4 * L.pitch + L.off + iy;
        b[0] = hh; b[L.pitch] = hx; b[2ll * L.pitch] = hy;
    }
}

// rank 0's pressure at global cell [0, 0] into slot 7 of its step record (the all-gather of gpf_close_step_local carries it)
__global__ void k_els_record_pref(const double* p, Layout L, double* rec) { rec[7] = p[L.at(0, 0)]; }

}  // namespace gpf
