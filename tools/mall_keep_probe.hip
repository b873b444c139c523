// Does the Infinity Cache keep a share of each step's output for the next step?  Two measurements, no arithmetic to speak of.
//   hipcc --offload-arch=gfx950 -O3 tools/mall_keep_probe.hip -o tools/mall_keep_probe && tools/mall_keep_probe
//
// (a) Residency.  Write a buffer of X MB with store policy P, stream Y = 2 x 400 MB past it (1 in / 1 out, non-temporal or plain
//     accesses), then time a re-read of the buffer with non-temporal and with plain loads.  "none" re-reads at once: the on-die
//     rate.  A re-read behind a stream that runs at the "none" rate found the buffer resident; one at the cold rate did not.
// (b) The step's pattern.  Waves march down 126-column windows (128 read: two halo columns) of a 4096^2 fp64 grid with the real
//     row pitch (4128 doubles), 62 chunks per strip, 3 planes in and 3 out, ping-pong, launches back to back so each reads what
//     the previous one wrote.  Rows with (ix & 7) < k are stored with policy P, every other row with `nt`; loads are `nt`, or plain
//     for the kept rows.  Reported: microseconds per launch, kernel boundary included, each configuration timed in every one of
//     several interleaved rounds (median, min, max).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef double d2 __attribute__((ext_vector_type(2)));

// store policies: 0 plain, 1 sc0, 2 sc1, 3 sc0 sc1, 4 nt sc1, 5 nt
static const char* const POL[] = {"plain", "sc0", "sc1", "sc0 sc1", "nt sc1", "nt"};
// s_nop: a store of more than 8 bytes must not be followed at once by a write of its data registers
template <int P>
__device__ __forceinline__ void st16(d2* p, d2 v) {
    if constexpr (P == 0) asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 0" :: "v"(p), "v"(v) : "memory");
    if constexpr (P == 1) asm volatile("global_store_dwordx4 %0, %1, off sc0\n\ts_nop 0" :: "v"(p), "v"(v) : "memory");
    if constexpr (P == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 0" :: "v"(p), "v"(v) : "memory");
    if constexpr (P == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 0" :: "v"(p), "v"(v) : "memory");
    if constexpr (P == 4) asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 0" :: "v"(p), "v"(v) : "memory");
    if constexpr (P == 5) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 0" :: "v"(p), "v"(v) : "memory");
}

// ---------------------------------------------------------------- (a) residency
template <int P>
__global__ __launch_bounds__(256) void k_fill(d2* b, long long n2) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n2; i += (long long)gridDim.x * 256) st16<P>(b + i, d2{(double)i, 1.0});
}
template <bool NT>
__global__ __launch_bounds__(256) void k_copy(const d2* __restrict__ in, d2* __restrict__ out, long long n2) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n2; i += (long long)gridDim.x * 256) {
        const d2 v = NT ? __builtin_nontemporal_load(in + i) : in[i];
        if (NT) __builtin_nontemporal_store(v + 1.0, out + i); else out[i] = v + 1.0;
    }
}
template <bool NT>
__global__ __launch_bounds__(256) void k_read(const d2* __restrict__ b, long long n2, double* sink) {
    d2 s = {0.0, 0.0};
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n2; i += (long long)gridDim.x * 256) s += NT ? __builtin_nontemporal_load(b + i) : b[i];
    if (s.x == -1.25 && s.y == -1.25) sink[0] = s.x;     // never true: keeps the loads without a store per thread
}

static float elapsed(hipEvent_t a, hipEvent_t b) { float ms; CK(hipEventElapsedTime(&ms, a, b)); return ms; }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

template <int P>
static void fill(d2* b, long long n2, int blocks) { hipLaunchKernelGGL(k_fill<P>, dim3(blocks), dim3(256), 0, 0, b, n2); }
static void fill_p(int p, d2* b, long long n2, int blocks) {
    switch (p) { case 0: fill<0>(b, n2, blocks); break; case 1: fill<1>(b, n2, blocks); break; case 2: fill<2>(b, n2, blocks); break;
                 case 3: fill<3>(b, n2, blocks); break; case 4: fill<4>(b, n2, blocks); break; default: fill<5>(b, n2, blocks); }
}

static void residency(int ncu) {
    const long long big2 = 400ll * 1000 * 1000 / 16;                      // 400 MB each way
    d2 *buf, *src, *dst, *flush; double* sink;
    CK(hipMalloc(&buf, 200ll * 1000 * 1000)); CK(hipMalloc(&src, big2 * 16)); CK(hipMalloc(&dst, big2 * 16));
    CK(hipMalloc(&flush, 2 * big2 * 16)); CK(hipMalloc(&sink, 64));
    CK(hipMemset(src, 0, big2 * 16)); CK(hipMemset(dst, 0, big2 * 16)); CK(hipMemset(flush, 0, 2 * big2 * 16));
    const int blocks = ncu * 8;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("(a) residency: write X MB with policy P, stream 400 MB in + 400 MB out past it, re-read X MB.  TB/s of the re-read (median of 7)\n");
    printf("%-8s %-8s | %-22s | %-22s | %-22s\n", "X MB", "P", "no stream: nt / plain", "nt stream: nt / plain", "plain stream: nt / plain");
    for (int xmb : {64, 128, 200}) {
        const long long n2 = (long long)xmb * 1000 * 1000 / 16;
        for (int p = 0; p < 6; ++p) {
            double r[3][2];
            for (int s = 0; s < 3; ++s)
                for (int ld = 0; ld < 2; ++ld) {
                    std::vector<double> t;
                    for (int rep = 0; rep < 7; ++rep) {
                        // start from a cold die: 800 MB of plain copy evicts anything resident
                        hipLaunchKernelGGL(k_copy<false>, dim3(blocks), dim3(256), 0, 0, flush, flush + big2, big2);
                        fill_p(p, buf, n2, blocks);
                        if (s == 1) hipLaunchKernelGGL(k_copy<true>, dim3(blocks), dim3(256), 0, 0, src, dst, big2);
                        if (s == 2) hipLaunchKernelGGL(k_copy<false>, dim3(blocks), dim3(256), 0, 0, src, dst, big2);
                        CK(hipEventRecord(e0, 0));
                        if (ld == 0) hipLaunchKernelGGL(k_read<true>, dim3(blocks), dim3(256), 0, 0, buf, n2, sink);
                        else hipLaunchKernelGGL(k_read<false>, dim3(blocks), dim3(256), 0, 0, buf, n2, sink);
                        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
                        t.push_back(elapsed(e0, e1));
                    }
                    r[s][ld] = n2 * 16.0 / (median(t) * 1e-3) / 1e12;
                }
            printf("%-8d %-8s | %9.2f / %9.2f  | %9.2f / %9.2f  | %9.2f / %9.2f\n", xmb, POL[p], r[0][0], r[0][1], r[1][0], r[1][1], r[2][0], r[2][1]);
            fflush(stdout);
        }
    }
    {   // the cold rate for reference: a re-read behind 800 MB of plain copy of OTHER data, policy of the fill irrelevant
        std::vector<double> t;
        const long long n2 = 128ll * 1000 * 1000 / 16;
        for (int rep = 0; rep < 7; ++rep) {
            fill<0>(buf, n2, blocks);
            hipLaunchKernelGGL(k_copy<false>, dim3(blocks), dim3(256), 0, 0, flush, flush + big2, big2);
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(k_read<true>, dim3(blocks), dim3(256), 0, 0, buf, n2, sink);
            CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
            t.push_back(elapsed(e0, e1));
        }
        printf("cold reference: 128 MB re-read with nt loads behind 800 MB of plain copy: %.2f TB/s\n\n", n2 * 16.0 / (median(t) * 1e-3) / 1e12);
    }
    CK(hipFree(buf)); CK(hipFree(src)); CK(hipFree(dst)); CK(hipFree(flush)); CK(hipFree(sink));
}

// ---------------------------------------------------------------- (b) the march
struct March {
    const double* in; double* out;
    long long plane;        // doubles per plane
    int Nx, Ny, pitch, col0, stride, nstrips, nchunks;
    int keep;               // rows with (ix & 7) < keep are stored with the keep policy
};

// DEPTH rows in flight ahead; KP: store policy of kept rows; KL: kept rows are loaded without the nt hint
template <int KP, bool KL>
__global__ __launch_bounds__(256, 2) void k_march(const March a) {
    constexpr int DEPTH = 2;
    const int nb = gridDim.x;
    const int lb = (int)(blockIdx.x & 7) * (nb >> 3) + (int)(blockIdx.x >> 3);     // contiguous waves per XCD
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int w = lb * 4 + wv;
    const int strip = w % a.nstrips, chunk = w / a.nstrips;
    if (chunk >= a.nchunks) return;
    const int n0 = (int)(((long long)chunk * a.Nx) / a.nchunks), n1 = (int)(((long long)(chunk + 1) * a.Nx) / a.nchunks);
    const int col = a.col0 + strip * a.stride + 2 * lane;
    const bool valid = col + 2 <= a.pitch && 2 * lane < a.stride;
    const unsigned lane_bytes = (unsigned)(col + 2 <= a.pitch ? col : 0) * 8u;
    const int keep = __builtin_amdgcn_readfirstlane(a.keep);
    d2 buf[DEPTH + 1][3];
    auto load = [&](int n, d2* r) {
        const long long rb = (long long)n * a.pitch;
        const bool kept = KL && (n & 7) < keep;
        for (int p = 0; p < 3; ++p) {
            const d2* src = reinterpret_cast<const d2*>(reinterpret_cast<const char*>(a.in + p * a.plane + rb) + lane_bytes);
            r[p] = kept ? *src : __builtin_nontemporal_load(src);
        }
    };
    auto row = [&](int n, d2* cur) {
        const d2 s = (cur[0] + cur[1] + cur[2]) * (1.0 / 3.0);
        const long long rb = (long long)n * a.pitch;
        if (n >= n0 + 1 && n <= n1) {               // halo rows n0 and n1+1 are read, not written
            const bool kept = (n & 7) < keep;
            for (int p = 0; p < 3; ++p) {
                d2* dst = reinterpret_cast<d2*>(reinterpret_cast<char*>(a.out + p * a.plane + rb) + lane_bytes);
                if (valid) { if (kept) st16<KP>(dst, s + (double)p); else st16<5>(dst, s + (double)p); }
            }
        }
        if (n + DEPTH + 1 <= n1 + 1) load(n + DEPTH + 1, cur);
    };
    for (int d = 0; d <= DEPTH; ++d) load(n0 + d, buf[d]);
    for (int n = n0;;) {
        row(n, buf[0]); if (++n > n1 + 1) break;
        row(n, buf[1]); if (++n > n1 + 1) break;
        row(n, buf[2]); if (++n > n1 + 1) break;
    }
}

template <int KP, bool KL>
static double march_us(March a, double* p0, double* p1, int launches, hipEvent_t e0, hipEvent_t e1) {
    const int nwaves = a.nstrips * a.nchunks, nblocks = ((nwaves + 3) / 4 + 7) / 8 * 8;
    auto go = [&](int i) {
        March b = a;
        b.in = i & 1 ? p1 : p0; b.out = i & 1 ? p0 : p1;
        hipLaunchKernelGGL((k_march<KP, KL>), dim3(nblocks), dim3(256), 0, 0, b);
    };
    go(0); go(1);
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < launches; ++i) go(i);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    return elapsed(e0, e1) * 1e3 / launches;
}

struct Cfg { int k, pol; bool kl; };
static double run_cfg(const Cfg& c, March a, double* p0, double* p1, hipEvent_t e0, hipEvent_t e1) {
    a.keep = c.k;
    const int L = 40;
    if (c.kl) {
        switch (c.pol) { case 0: return march_us<0, true>(a, p0, p1, L, e0, e1); case 1: return march_us<1, true>(a, p0, p1, L, e0, e1);
                         case 2: return march_us<2, true>(a, p0, p1, L, e0, e1); case 3: return march_us<3, true>(a, p0, p1, L, e0, e1);
                         case 4: return march_us<4, true>(a, p0, p1, L, e0, e1); default: return march_us<5, true>(a, p0, p1, L, e0, e1); }
    }
    switch (c.pol) { case 0: return march_us<0, false>(a, p0, p1, L, e0, e1); case 1: return march_us<1, false>(a, p0, p1, L, e0, e1);
                     case 2: return march_us<2, false>(a, p0, p1, L, e0, e1); case 3: return march_us<3, false>(a, p0, p1, L, e0, e1);
                     case 4: return march_us<4, false>(a, p0, p1, L, e0, e1); default: return march_us<5, false>(a, p0, p1, L, e0, e1); }
}

static void march() {
    March a;
    a.Nx = 4096; a.Ny = 4096;
    a.pitch = 4128;
    a.plane = (long long)(a.Nx + 2) * a.pitch;
    a.col0 = 14; a.stride = 126;
    a.nstrips = (a.Ny + 2 + a.stride - 1) / a.stride;        // the last window runs past the pitch: those lanes read column 0, write nothing
    a.nchunks = 62;
    double *p0, *p1;
    CK(hipMalloc(&p0, 3 * a.plane * 8 + 4096)); CK(hipMalloc(&p1, 3 * a.plane * 8 + 4096));
    CK(hipMemset(p0, 0, 3 * a.plane * 8)); CK(hipMemset(p1, 0, 3 * a.plane * 8));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<Cfg> cfg;
    cfg.push_back({0, 5, false});
    for (int kl = 0; kl < 2; ++kl)
        for (int pol = 0; pol < 5; ++pol)
            for (int k = 1; k <= 5; ++k) cfg.push_back({k, pol, kl != 0});
    const int rounds = 7;
    std::vector<std::vector<double>> t(cfg.size());
    for (int r = 0; r < rounds; ++r)
        for (size_t i = 0; i < cfg.size(); ++i) {
            t[i].push_back(run_cfg(cfg[i], a, p0, p1, e0, e1));
            if (i + 1 < cfg.size() && cfg[i + 1].k != 0) t[0].push_back(run_cfg(cfg[0], a, p0, p1, e0, e1));   // k = 0 between every pair
        }
    const double base = median(t[0]);
    printf("(b) march 3 in / 3 out, 4096^2, pitch %d, %d strips x %d chunks, back to back, ping-pong; us per launch over %d rounds\n",
           a.pitch, a.nstrips, a.nchunks, rounds);
    printf("    algorithmic bytes per launch %.1f MB; k = 0 (all nt) median %.1f us (min %.1f max %.1f, %zu samples)\n",
           6.0 * 8 * a.Nx * a.Ny / 1e6, base, *std::min_element(t[0].begin(), t[0].end()), *std::max_element(t[0].begin(), t[0].end()), t[0].size());
    printf("%-10s %-10s %3s | %8s %8s %8s | %s\n", "keep pol", "kept load", "k", "median", "min", "max", "vs k=0");
    for (size_t i = 1; i < cfg.size(); ++i) {
        const double m = median(t[i]);
        printf("%-10s %-10s %3d | %8.1f %8.1f %8.1f | %+6.1f %%\n", POL[cfg[i].pol], cfg[i].kl ? "plain" : "nt", cfg[i].k, m,
               *std::min_element(t[i].begin(), t[i].end()), *std::max_element(t[i].begin(), t[i].end()), (m / base - 1.0) * 100.0);
    }
    fflush(stdout);
    CK(hipFree(p0)); CK(hipFree(p1));
}

int main(int argc, char** argv) {
    int ncu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    const bool only_b = argc > 1 && argv[1][0] == 'b';
    if (!only_b) residency(ncu);
    march();
    return 0;
}
