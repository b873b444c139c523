// Checkpoint kernels (entry points in api_checkpoint.inc): planes of a handle <-> the unpadded [plane][ix][iy] host layout,
// with a 64-bit digest of every plane folded in the same pass.
//
// Both kernels are pure streams.  A lane owns two neighbouring cells of one row -- columns (2p - 1, 2p), the pair that starts
// on a 16-byte boundary of the padded row (Layout::off is odd) -- and moves them through all planes of the launch with one
// 16-byte access per plane and side.  The staging buffer is unpadded; the host side shifts its base by one double when Ny + 2 is
// even, so the same pair is 16-byte aligned there as well (with an odd Ny + 2 every other row falls back to two 8-byte accesses).
//
// Digest of a plane: sum over its cells of mix(cell index in the unpadded plane, bit pattern), modulo 2^64.  The mix is a
// bijection of the bit pattern for a fixed index, so any change of one cell changes the sum; the sum does not depend on the order
// of traversal, so the save (by chunks of rows), the load and a later re-save agree.  Lanes fold with wave shuffles, waves through
// LDS, and one vector atomic per block and plane adds to the plane's slot.
#pragma once

namespace gpf {

typedef double ck_d2 __attribute__((ext_vector_type(2)));
static constexpr int CKPT_MAX_LAUNCH_PLANES = 16;

struct CkptArgs {
    double* field;              // first plane of the launch, in the handle's layout
    long long plane_stride;     // doubles between planes of the launch
    double* stage;              // [plane][rows][W], unpadded; plane p of the launch at stage + p * stage_stride
    long long stage_stride;
    unsigned long long* digest; // one slot per plane of the launch
    int pitch, off, W;          // row pitch and offset of column 0 in `field`; W = Ny + 2 columns
    int row0, rows;             // rows [row0, row0 + rows) of the field; the stage holds exactly these
    int nplanes;
};

__host__ __device__ __forceinline__ unsigned long long ckpt_mix(unsigned long long index, unsigned long long bits) {
    unsigned long long x = bits + (index + 1) * 0x9E3779B97F4A7C15ull;        // splitmix64's finaliser: a bijection of x
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ void ckpt_fold(unsigned long long (&acc)[CKPT_MAX_LAUNCH_PLANES], int nplanes, unsigned long long* digest,
                                          unsigned long long (*sm)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < CKPT_MAX_LAUNCH_PLANES; ++p) {        // (unrolled: acc stays in registers)
        if (p < nplanes) {
            unsigned long long v = acc[p];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
            if (lane == 0) sm[p][wave] = v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nplanes) {
        const unsigned long long v = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
        atomicAdd(digest + threadIdx.x, v);
    }
}

// item t of a launch: row r = t / PP of the chunk, pair p = t % PP, columns iy0 = 2p - 1 and iy0 + 1 (PP = W / 2 + 1 pairs cover -1 .. W)
struct CkptItem { long long fo, so; unsigned long long index; bool a, b, pair_f, pair_s; };
__device__ __forceinline__ CkptItem ckpt_item(const CkptArgs& k, unsigned t, unsigned PP) {
    const unsigned r = t / PP, p = t - r * PP;
    const int iy0 = 2 * (int)p - 1;
    CkptItem it;
    it.a = iy0 >= 0; it.b = iy0 + 1 < k.W;
    it.fo = (long long)(k.row0 + (int)r) * k.pitch + k.off + iy0;
    it.so = (long long)r * k.W + iy0;
    it.index = (unsigned long long)(k.row0 + (int)r) * (unsigned long long)k.W + (unsigned long long)(long long)iy0;
    it.pair_f = it.a && it.b;                                                      // (fo is even by construction)
    it.pair_s = it.a && it.b && (((size_t)(k.stage + it.so) & 15) == 0);
    return it;
}

// handle -> stage (save).  stage == nullptr: digest only.
__global__ __launch_bounds__(256) void k_ckpt_pack(const CkptArgs k) {
    __shared__ unsigned long long sm[CKPT_MAX_LAUNCH_PLANES][4];
    unsigned long long acc[CKPT_MAX_LAUNCH_PLANES];
#pragma unroll
    for (int p = 0; p < CKPT_MAX_LAUNCH_PLANES; ++p) acc[p] = 0;
    const unsigned PP = (unsigned)k.W / 2 + 1, n = (unsigned)k.rows * PP;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < n; t += gridDim.x * 256u) {
        const CkptItem it = ckpt_item(k, t, PP);
#pragma unroll
        for (int p = 0; p < CKPT_MAX_LAUNCH_PLANES; ++p) {
            if (p >= k.nplanes) break;
            const double* f = k.field + p * k.plane_stride + it.fo;
            double x = 0.0, y = 0.0;
            if (it.pair_f) { const ck_d2 v = __builtin_nontemporal_load(reinterpret_cast<const ck_d2*>(f)); x = v.x; y = v.y; }
            else { if (it.a) x = f[0]; if (it.b) y = f[1]; }
            if (k.stage) {
                double* s = k.stage + p * k.stage_stride + it.so;
                if (it.pair_s) *reinterpret_cast<ck_d2*>(s) = ck_d2{x, y};
                else { if (it.a) s[0] = x; if (it.b) s[1] = y; }
            }
            if (it.a) acc[p] += ckpt_mix(it.index, (unsigned long long)__double_as_longlong(x));
            if (it.b) acc[p] += ckpt_mix(it.index + 1, (unsigned long long)__double_as_longlong(y));
        }
    }
    ckpt_fold(acc, k.nplanes, k.digest, sm);
}

// stage -> handle (load), then the digest of what now stands in the handle's planes, read back through the layout.
// field == nullptr: digest of the staged data only (the blob is verified before the handle is touched).
__global__ __launch_bounds__(256) void k_ckpt_unpack(const CkptArgs k) {
    __shared__ unsigned long long sm[CKPT_MAX_LAUNCH_PLANES][4];
    unsigned long long acc[CKPT_MAX_LAUNCH_PLANES];
#pragma unroll
    for (int p = 0; p < CKPT_MAX_LAUNCH_PLANES; ++p) acc[p] = 0;
    const unsigned PP = (unsigned)k.W / 2 + 1, n = (unsigned)k.rows * PP;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < n; t += gridDim.x * 256u) {
        const CkptItem it = ckpt_item(k, t, PP);
#pragma unroll
        for (int p = 0; p < CKPT_MAX_LAUNCH_PLANES; ++p) {
            if (p >= k.nplanes) break;
            const double* s = k.stage + p * k.stage_stride + it.so;
            double x = 0.0, y = 0.0;
            if (it.pair_s) { const ck_d2 v = __builtin_nontemporal_load(reinterpret_cast<const ck_d2*>(s)); x = v.x; y = v.y; }
            else { if (it.a) x = s[0]; if (it.b) y = s[1]; }
            if (k.field) {
                double* f = k.field + p * k.plane_stride + it.fo;
                if (it.pair_f) *reinterpret_cast<ck_d2*>(f) = ck_d2{x, y};
                else { if (it.a) f[0] = x; if (it.b) f[1] = y; }
                __threadfence();
                const volatile double* g = f;                   // what the plane holds now, not what was meant to be written
                if (it.a) x = g[0];
                if (it.b) y = g[1];
            }
            if (it.a) acc[p] += ckpt_mix(it.index, (unsigned long long)__double_as_longlong(x));
            if (it.b) acc[p] += ckpt_mix(it.index + 1, (unsigned long long)__double_as_longlong(y));
        }
    }
    ckpt_fold(acc, k.nplanes, k.digest, sm);
}

}  // namespace gpf
