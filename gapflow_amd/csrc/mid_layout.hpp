// Workspace tier of the ensembles (mid_kernel.hip, api_ensemble.inc): where a member's planes lie in its workspace in device
// memory.  This header compiles for the host on its own -- it includes nothing of the project -- so that the kernel, the
// library's allocation and a stand-alone host program (tests/test_mid_layout_hostcheck.py) use the very same lines.
//
// A member of nc = (Nx + 2) * (Ny + 2) cells, ghost cells included, has 19 dense planes of nc doubles, cell (ix, iy) of a plane
// at ix * (Ny + 2) + iy:
//     planes  0 ..  8   three state buffers of (rho, jx, jy): the current field, stage 1's result, stage 2's result / the average
//     planes  9 .. 14   fx1 fx2 fy2 s0 s1 s2: the fluxes and sources of the stage under way
//     planes 15 .. 18   h, hx, hy, Ls
// and its workspace is those 19 * nc doubles rounded up to 256 bytes, so that in one allocation for all members every
// workspace starts 256-byte aligned.
#pragma once

#if defined(__HIPCC__)
#define GPF_MID_HD __host__ __device__ __forceinline__
#else
#define GPF_MID_HD inline
#endif

namespace gpf {

constexpr long long MID_GRID_MAX_CELLS = 16384;     // ghost cells included: up to 126 x 126 interior cells
constexpr int MID_DOUBLES_PER_CELL = 19;
constexpr int MID_THREADS = 512;
constexpr int MID_PLANE_Q = 0;                      // first plane of state buffer 0; buffer b starts at plane 3 * b
constexpr int MID_PLANE_F = 9;
constexpr int MID_PLANE_T = 15;
constexpr long long MID_WORKSPACE_ALIGN = 256;      // bytes

GPF_MID_HD long long mid_cells(int Nx, int Ny) { return (long long)(Nx + 2) * (Ny + 2); }

// first double of plane p (0 .. 18) in a workspace of nc-cell planes
GPF_MID_HD long long mid_plane_offset(int p, long long nc) { return (long long)p * nc; }

GPF_MID_HD long long mid_workspace_bytes(long long nc) {
    const long long raw = (long long)MID_DOUBLES_PER_CELL * 8 * nc;
    return (raw + MID_WORKSPACE_ALIGN - 1) / MID_WORKSPACE_ALIGN * MID_WORKSPACE_ALIGN;
}

}  // namespace gpf
