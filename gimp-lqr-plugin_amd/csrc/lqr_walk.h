// lqr_walk.h -- E7's seam pick and the helpers of the one-wave walk: shared by k_vpath1 (k_backtrack.hip, which says what they do and
// why) and the walk role of k_carve_v (k_carve.hip).  The chase itself is vpath1_walk.inc, included by both.
#pragma once
#include "lqr_common.h"

// argmin of row `mrow` (w floats) over a VPATH_THREADS-thread block with liblqr's tie rule: leftmost (lr = 0) / rightmost
// (lr = 1) of equal minima; returns (to every thread) the column, or -1 if no candidate beat liblqr's start value 2^29.
// A thread takes 16 B at a time (4 loads in flight per thread, all issued before the first compare: the row is one
// memory round trip, not fifteen), keeps its own ascending scan, then the block reduces on (value, index) pairs: within
// a wave by DPP-free shuffles, across the four waves through LDS.
__device__ __forceinline__ int row_argmin(const gf32 *mrow, int w, int lr, float *s_val, int *s_idx)
{
    const int tid = threadIdx.x;
    const float INF = __int_as_float(0x7f800000);
    float bv = INF;
    int bi = -1;
    for (int base = 0; base < w; base += 16 * VPATH_THREADS) {
        f32x4 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = base + 4 * (tid + VPATH_THREADS * i);
            // whole vectors only where they are inside the row (the planes have >= 16 floats of padding, but not initialised)
            if (x + 3 < w) v[i] = *(const GLOBAL_AS f32x4 *) (mrow + x);
            else { v[i] = (f32x4) {INF, INF, INF, INF}; for (int j = 0; j < 4; j++) if (x + j < w) v[i][j] = mrow[x + j]; }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x = base + 4 * (tid + VPATH_THREADS * i) + j;
                const float f = v[i][j];
                if (x < w && (f < bv || (f == bv && lr))) { bv = f; bi = x; }
            }
    }
    auto better = [&](float v2, int i2, float v1, int i1) {        // does (v2, i2) replace (v1, i1)?
        if (i2 < 0) return false;
        if (i1 < 0) return true;
        if (v2 < v1) return true;
        if (v2 > v1) return false;
        return lr ? (i2 > i1) : (i2 < i1);
    };
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(bv, o);
        const int i2 = __shfl_xor(bi, o);
        if (better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    }
    if ((tid & 63) == 0) { s_val[tid >> 6] = bv; s_idx[tid >> 6] = bi; }
    __syncthreads();
    bv = s_val[0]; bi = s_idx[0];
#pragma unroll
    for (int k = 1; k < VPATH_THREADS / 64; k++) if (better(s_val[k], s_idx[k], bv, bi)) { bv = s_val[k]; bi = s_idx[k]; }
    // liblqr starts from m = 2^29: a candidate must beat it (or tie it when lr == 1)
    const float lim = 536870912.0f;
    const bool ok = (bi >= 0) && (bv < lim || (bv == lim && lr));
    return ok ? bi : -1;
}

// rows per chunk by delta_x: the path drifts up to ROWS * delta_x columns inside a chunk and must stay within lanes 4 .. 60 of the 64
// spread around its start (<= 28), and the window loaded VP1_AHEAD chunks ahead must still hold those 64 columns
constexpr int vp1_rows(int delta) { return delta == 1 ? 28 : delta == 2 ? 12 : delta == 3 ? 8 : 4; }      // (delta_x 4 .. 7: 4 rows)
#define VP1_AHEAD 3
template <int r>
__device__ __forceinline__ void vp1_step(const int e, int &o, int &path)
{
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(path) : "s"(o), "n"(r));      // lane r <- window offset at row y_top - r
    o += __builtin_amdgcn_readlane(e, o);
}
template <int N, int... Rs>
__device__ __forceinline__ void vp1_chase(const int (&e)[N], int &o, int &path, std::integer_sequence<int, Rs...>)
{
    (vp1_step<Rs>(e[Rs], o, path), ...);
}
