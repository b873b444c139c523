// Region series (region_kernels.hip, api_regions.inc): what makes a cell a member of a region {field, lo, hi, box}.  This header
// compiles for the host on its own -- it includes nothing of the project -- so that the device kernels, the library's argument
// checks and a stand-alone host program (tests/test_regions_hostcheck.py) evaluate the very same lines.
//
//   value   lo <= f && f < hi, as IEEE comparisons: lo is inclusive, hi exclusive; -0.0 and +0.0 compare equal, so -0.0 belongs to
//           [0.0, hi) and not to [lo, 0.0); -inf / +inf as bounds leave that side open (f = +inf itself is never below hi = +inf);
//           every comparison with a NaN is false, so a NaN value never belongs.
//   box     ix0 <= ix <= ix1 and iy0 <= iy <= iy1, inclusive, in 1-based interior indices (the ghosted index space's 1..Nx, 1..Ny).
#pragma once

#if defined(__HIPCC__)
#define GPF_REGION_HD __host__ __device__ __forceinline__
#else
#define GPF_REGION_HD inline
#endif

namespace gpf {

constexpr int REGION_MAX_K = 8;
constexpr int REGION_NFIELD = 5;        // p rho h jx jy (gpf_region::field)
constexpr int REGION_NI = 5;            // cells ix_min ix_max iy_min iy_max

// One region as the device reads it: the field's index, the bounds, the box
struct Region {
    double lo, hi;
    int field;
    int ix0, ix1, iy0, iy1;
    int pad_;
};

GPF_REGION_HD bool region_value_in(double f, double lo, double hi) { return lo <= f && f < hi; }

GPF_REGION_HD bool region_box_in(int ix, int iy, int ix0, int ix1, int iy0, int iy1) {
    return ix0 <= ix && ix <= ix1 && iy0 <= iy && iy <= iy1;
}

GPF_REGION_HD bool region_member(const Region& r, double f, int ix, int iy) {
    return region_value_in(f, r.lo, r.hi) && region_box_in(ix, iy, r.ix0, r.ix1, r.iy0, r.iy1);
}

// What gpf_regions_set accepts: 0 if the region is well formed on an Nx x Ny interior, else which rule it breaks --
// 1 unknown field, 2 bounds (a NaN, or lo >= hi: nothing could belong), 3 box (outside the interior, or empty)
GPF_REGION_HD int region_check(int field, double lo, double hi, int ix0, int ix1, int iy0, int iy1, int Nx, int Ny) {
    if (field < 0 || field >= REGION_NFIELD) return 1;
    if (!(lo < hi)) return 2;
    if (ix0 < 1 || ix1 > Nx || ix0 > ix1 || iy0 < 1 || iy1 > Ny || iy0 > iy1) return 3;
    return 0;
}

}  // namespace gpf
