// Running field statistics (entry points in api_stats.inc): for each requested field f of p, rho, jx, jy and each cell of the
// ghosted grid, the mean, the sum of squared deviations m2, the smallest and the largest value over the recorded steps, kept in
// accumulator planes on the device.  p is eos_pressure<EOS> of the committed density -- a probe's p --, the others are the
// committed q[st->parity].
//
// One launch per record, guarded by the device's run state like k_film_partial: `expect` is the step count the launch ahead
// produces IF it commits; a step that did not run or was rolled back leaves st->step below it (or raises st->invalid), and then
// nothing is touched.  `n` is the record's rank since arming, computed on the host (api_stats.inc: stats_rank).  Per cell, with
// every operation rounded on its own (Welford's update):
//     n == 1:  mean = x;  m2 = 0;  min = x;  max = x            -- the accumulators are not read: no memset, no stale data
//     n  > 1:  d = x - mean;  mean = mean + d / n;  m2 = m2 + d * (x - mean);  min = x < min ? x : min;  max = x > max ? x : max
// d / n is an IEEE division by (double)n.  Contraction is off for these statements, and the product d * (x - mean) and the pressure
// pass through __builtin_canonicalize: the library is compiled with -ffp-contract=fast, under which the backend fuses whatever
// a contract pragma says, and the canonicalize between two operations is what it does not fuse across (weighted_kernels.hip).  A
// cell's accumulators are therefore a pure function of the sequence of values recorded for it: a NumPy restatement of the
// recurrences gives the same bits (tests/statistics_cases.py).
//
// A streaming read-modify-write pass.  The work is cut into items: under film_wide_ok's conditions the column pairs
// (1 + 2k, 2 + 2k) of every row, ghost rows included, start on 16 bytes in every plane of the handle's Layout, and an item is
// such a pair -- one 16-byte load or store per lane and plane; ghost column 0, and column Ny + 1 where it is not the second half
// of the last pair (even Ny), are items of one cell with 8-byte accesses.  Otherwise (GPF_FILM_NARROW) every cell is an item of
// its own.  The items of all rows are numbered in one sequence and dealt to the threads of the grid in turn, so every wave but
// the last is full whatever Ny is.  The field mask is tested with uniform branches; the planes of a field that is not
// requested do not exist.  No atomics, no LDS, no private segment: every cell is owned by one thread.
// The accumulators are touched once per record and not again before hundreds of megabytes have gone by: their loads and stores
// carry the non-temporal hint (GPF_STATS_NT=0 at compile time: plain; profiles/statistics/README.md has both).
#pragma once

#ifndef GPF_STATS_NT
#define GPF_STATS_NT 1
#endif

namespace gpf {

constexpr int STATS_NF = 4;             // p rho jx jy: the bits of the field mask
constexpr int STATS_NQ = 4;             // mean m2 min max: the planes of a field, in this order

struct StatsRecord {                    // what the device knows about the window
    long long count, first_step, last_step;
    double t_first, t_last;
};

struct StatsArgs {
    const double *qa, *qb;
    const StepState* st;
    double* acc;            // [requested fields, in the order p rho jx jy][STATS_NQ] planes in the handle's Layout
    StatsRecord* rec;
    Layout L;
    int mask;               // bit f: field f is requested
    int wide;               // 16-byte pair accesses are aligned
};

typedef double stats_d2 __attribute__((ext_vector_type(2)));

template <typename V>
__device__ __forceinline__ V stats_load(const double* p) {
#if GPF_STATS_NT
    return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
#else
    return *reinterpret_cast<const V*>(p);
#endif
}

template <typename V>
__device__ __forceinline__ void stats_store(double* p, V v) {
#if GPF_STATS_NT
    __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
#else
    *reinterpret_cast<V*>(p) = v;
#endif
}

// One value into one cell's accumulators, n > 1
__device__ __forceinline__ void stats_fold(double x, double n, double& mean, double& m2, double& mn, double& mx) {
#pragma clang fp contract(off)
    const double d = x - mean;
    mean = mean + d / n;
    m2 = m2 + __builtin_canonicalize(d * (x - mean));
    mn = x < mn ? x : mn;
    mx = x > mx ? x : mx;
}

__device__ __forceinline__ void stats_fold(stats_d2 x, double n, stats_d2& mean, stats_d2& m2, stats_d2& mn, stats_d2& mx) {
    double a[2][4] = {{mean.x, m2.x, mn.x, mx.x}, {mean.y, m2.y, mn.y, mx.y}};
    stats_fold(x.x, n, a[0][0], a[0][1], a[0][2], a[0][3]);
    stats_fold(x.y, n, a[1][0], a[1][1], a[1][2], a[1][3]);
    mean = stats_d2{a[0][0], a[1][0]}; m2 = stats_d2{a[0][1], a[1][1]}; mn = stats_d2{a[0][2], a[1][2]}; mx = stats_d2{a[0][3], a[1][3]};
}

// One field's four planes at element o (V: one cell, or the pair that starts there)
template <typename V>
__device__ __forceinline__ void stats_item(double* planes, long long plane, long long o, V x, long long n) {
    double* a = planes + o;
    if (n == 1) {
        stats_store<V>(a, x);
        stats_store<V>(a + plane, V(0.0));
        stats_store<V>(a + 2 * plane, x);
        stats_store<V>(a + 3 * plane, x);
        return;
    }
    V mean = stats_load<V>(a), m2 = stats_load<V>(a + plane), mn = stats_load<V>(a + 2 * plane), mx = stats_load<V>(a + 3 * plane);
    stats_fold(x, (double)n, mean, m2, mn, mx);
    stats_store<V>(a, mean);
    stats_store<V>(a + plane, m2);
    stats_store<V>(a + 2 * plane, mn);
    stats_store<V>(a + 3 * plane, mx);
}

template <int EOS>
__device__ __forceinline__ double stats_pressure(double rho, const Phys& P) { return __builtin_canonicalize(eos_pressure<EOS>(rho, P)); }
template <int EOS>
__device__ __forceinline__ stats_d2 stats_pressure(stats_d2 rho, const Phys& P) {
    return stats_d2{stats_pressure<EOS>(rho.x, P), stats_pressure<EOS>(rho.y, P)};
}

// All requested fields of one item
template <int EOS, typename V>
__device__ __forceinline__ void stats_fields(const StatsArgs& a, const Phys& P, const double* q, long long o, long long n) {
    const long long plane = a.L.plane;
    double* planes = a.acc;
    if (a.mask & 3) {
        const V rho = *reinterpret_cast<const V*>(q + o);
        if (a.mask & 1) { stats_item<V>(planes, plane, o, stats_pressure<EOS>(rho, P), n); planes += STATS_NQ * plane; }
        if (a.mask & 2) { stats_item<V>(planes, plane, o, rho, n); planes += STATS_NQ * plane; }
    }
    if (a.mask & 4) { stats_item<V>(planes, plane, o, *reinterpret_cast<const V*>(q + plane + o), n); planes += STATS_NQ * plane; }
    if (a.mask & 8) stats_item<V>(planes, plane, o, *reinterpret_cast<const V*>(q + 2 * plane + o), n);
}

template <int EOS>
__global__ __launch_bounds__(256) void k_stats_update(const StatsArgs a, const Phys P, long long expect, long long n) {
    if (a.st->step != expect || a.st->invalid != 0) return;            // uniform: the step did not run, or was rolled back
    if (n < 1) return;
    const Layout& L = a.L;
    const double* q = a.st->parity ? a.qb : a.qa;
    const int npair = a.wide ? (L.Ny + 1) / 2 : 0;
    const int nitem = a.wide ? npair + 1 + ((L.Ny & 1) ? 0 : 1) : L.Ny + 2;       // items per row
    const long long total = (long long)(L.Nx + 2) * nitem;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int ix = (int)(t / nitem), j = (int)(t - (long long)ix * nitem);
        if (a.wide && j >= 1 && j <= npair) {
            stats_fields<EOS, stats_d2>(a, P, q, L.at(ix, 2 * j - 1), n);
        } else {
            const int iy = a.wide ? (j == 0 ? 0 : L.Ny + 1) : j;
            stats_fields<EOS, double>(a, P, q, L.at(ix, iy), n);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        StatsRecord* r = a.rec;
        if (n == 1) { r->first_step = a.st->step; r->t_first = a.st->simtime; }
        r->count = n; r->last_step = a.st->step; r->t_last = a.st->simtime;
    }
}

// The yardstick of tools/stats_time.py: the bytes of a record of `nf` fields -- `nin` q planes read, 4 nf planes read and
// written -- moved elementwise, 16 bytes per lane and access, with the same hint and the same grid, and no arithmetic.
__global__ __launch_bounds__(256) void k_stats_stream(const double* q, double* acc, long long plane, int nin, int nf) {
    const long long n2 = plane / 2;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n2; t += (long long)gridDim.x * blockDim.x) {
        stats_d2 s = stats_d2{0.0, 0.0};
        for (int p = 0; p < nin; ++p) s += *reinterpret_cast<const stats_d2*>(q + p * plane + 2 * t);
        for (int p = 0; p < STATS_NQ * nf; ++p) {
            double* a = acc + p * plane + 2 * t;
            stats_store<stats_d2>(a, stats_load<stats_d2>(a) + s);
        }
    }
}

}  // namespace gpf
