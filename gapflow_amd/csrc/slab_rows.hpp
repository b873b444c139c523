// Domain series on x-slabs (slab_series_kernels.hip, api_slab_series.inc): which rank owns a global interior row, and where its
// vector sits in the gathered series message.  This header compiles for the host on its own -- it includes nothing of the
// project -- so that the fold kernels, the library's argument checks and a stand-alone host program
// (tests/test_slab_series_host.py) evaluate the very same lines.
//
// The cut is gapflow_amd/slab.py: partition's: base, rem = divmod(Nx, world); the first `rem` ranks own base + 1 rows, the others
// base, in rank order.  Rows are counted from 0 here (g = global interior row - 1, the local row likewise).
// The message of a rank is padded to the longest slab, [max_nx][W], so that one all-gather of equal parts carries every rank's
// rows: the gathered buffer is [world][max_nx][W], and the local rows >= a rank's own count are never written nor read.
#pragma once

#if defined(__HIPCC__)
#define GPF_SLAB_HD __host__ __device__ __forceinline__
#else
#define GPF_SLAB_HD inline
#endif

namespace gpf {

struct SlabRow { int rank, local; };

// Rows of the longest slab: the padded length of every rank's message
GPF_SLAB_HD int slab_max_nx(int Nx, int world) { return Nx / world + (Nx % world > 0 ? 1 : 0); }

// Rows rank `rank` owns
GPF_SLAB_HD int slab_rank_nx(int Nx, int world, int rank) { return Nx / world + (rank < Nx % world ? 1 : 0); }

// Global rows below rank `rank`'s first: its first global row, counted from 0 (slab.partition's lo - 1)
GPF_SLAB_HD int slab_rank_row0(int Nx, int world, int rank) {
    const int base = Nx / world, rem = Nx % world;
    return rank * base + (rank < rem ? rank : rem);
}

// THE map: global interior row g (0 <= g < Nx, world <= Nx) -> its owner and its row there
GPF_SLAB_HD SlabRow slab_row_of(int g, int Nx, int world) {
    const int base = Nx / world, rem = Nx % world;
    const int split = rem * (base + 1);             // rows of the ranks that own base + 1
    SlabRow r;
    if (g < split) { r.rank = g / (base + 1); r.local = g - r.rank * (base + 1); }
    else { r.rank = rem + (g - split) / base; r.local = (g - split) % base; }
    return r;
}

// Row of the gathered buffer [world][max_nx] that holds global row g
GPF_SLAB_HD long long slab_gathered_row(int g, int Nx, int world) {
    const SlabRow r = slab_row_of(g, Nx, world);
    return (long long)r.rank * slab_max_nx(Nx, world) + r.local;
}

// What gpf_slab_series_set accepts: 0 if a handle of `nx` rows whose first global row is `row0` (from 0) is one rank's slab of
// the cut, else which rule it breaks -- 1 the cut itself (world < 1, or fewer rows than ranks), 2 no rank's slab
GPF_SLAB_HD int slab_check(int row0, int nx, int Nx, int world) {
    if (world < 1 || Nx < world) return 1;
    if (row0 < 0 || nx < 1 || row0 > Nx - nx) return 2;
    const SlabRow r = slab_row_of(row0, Nx, world);
    return r.local == 0 && slab_rank_nx(Nx, world, r.rank) == nx ? 0 : 2;
}

}  // namespace gpf
