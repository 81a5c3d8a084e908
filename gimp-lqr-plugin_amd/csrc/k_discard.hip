// k_discard.hip -- the discard scan (include_ext/lqr_remove.h): which marked pixels of a carver are still visible,
// how many of them the fullest line holds, and how deep the deepest marked pixel lies.  One pass over bias0 and vs of the base layout,
// 8 bytes per pixel, nothing written but a count per line or column and three words of result.
//   k_discard_line   the lines are the base layout's rows: a workgroup per row
//   k_discard_cross  the lines run ACROSS the base layout's rows (the carver lies the other way; it is not transposed): the reads still
//                    run along the rows, every column keeps a count per tile of rows
//   k_discard_rank   the same lines on a carver that hides pixels: a column of the image is a RANK among a row's visible pixels
//   k_discard_fold   sums the counts either of them left, a lane per column
// A pixel is marked when its bias is below `thr` (= -strength), visible when v == 0 || v >= level -- (unsigned) (v - 1) >= (unsigned)
// (level - 1), as k_sizes.hip states it -- and its depth is v - depth in lqr_vmap_dump's numbering (levels up to `depth` are the pixels
// an enlargement would insert: they are in no dumped map).  The result words are integer sums and maxima, so the atomics that fold
// the workgroups' contributions give the same words in any order; the shim zeroes them in front of the launch.
// Sizes, grids and offsets are lqr_geom.h's (discard_*); static LDS only, no scratch, no waiting on another workgroup.
// (gfx950 / CDNA4, wave64; see lqr_common.h for the file map)
#include "lqr_common.h"
#include "lqr_kernels.h"

// one pixel into a lane's running count of visible marked pixels and its deepest marked level
__device__ __forceinline__ void discard_px(float b, unsigned v, float thr, unsigned level1, unsigned depth, int &count, unsigned &deep)
{
    const bool marked = b < thr;
    count += (marked && v - 1u >= level1) ? 1 : 0;
    const unsigned d = v > depth ? v - depth : 0u;
    deep = (marked && d > deep) ? d : deep;
}

// Four neighbouring columns per lane, DISCARD_CHUNK columns of the row at a time, in 16-byte loads of both planes where the four lie
// inside the row: the chunks start discard_lead columns in front of the row, masked out, so that every lane's four begin on a 16-byte
// boundary of the planes whatever the row (k_compact_sizes' trick; both planes hold 4-byte elements and start on such a boundary).
// The lanes' counts are folded by shuffles within a wave and through four LDS words across the waves.
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_line(const float *bias, const int32_t *vs, int w0, float thr, int level, int depth, int *res)
{
    __shared__ int s_cnt[DISCARD_THREADS / 64];
    __shared__ unsigned s_deep[DISCARD_THREADS / 64];
    const int y = blockIdx.x, tid = threadIdx.x;
    const size_t ri = (size_t) y * w0;
    const float *brow = bias + ri;
    const int32_t *vrow = vs + ri;
    const unsigned level1 = (unsigned) (level - 1), dp = (unsigned) depth;
    int count = 0;
    unsigned deep = 0;
    for (int base = -discard_lead((size_t) y, w0); base < w0; base += DISCARD_CHUNK) {
        const int g = base + 4 * tid;
        if (g >= 0 && g + 3 < w0) {
            const f32x4 bb = *(const f32x4 *) (brow + g);
            const u32x4 vv = *(const u32x4 *) (vrow + g);
            discard_px(bb.x, vv.x, thr, level1, dp, count, deep);
            discard_px(bb.y, vv.y, thr, level1, dp, count, deep);
            discard_px(bb.z, vv.z, thr, level1, dp, count, deep);
            discard_px(bb.w, vv.w, thr, level1, dp, count, deep);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((unsigned) (g + k) < (unsigned) w0) discard_px(brow[g + k], (unsigned) vrow[g + k], thr, level1, dp, count, deep);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        count += __shfl_down(count, o);
        const unsigned d = __shfl_down(deep, o);
        deep = d > deep ? d : deep;
    }
    if ((tid & 63) == 0) { s_cnt[tid >> 6] = count; s_deep[tid >> 6] = deep; }
    __syncthreads();
    if (tid == 0) {
        const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const unsigned d = max(max(s_deep[0], s_deep[1]), max(s_deep[2], s_deep[3]));
        if (c) { atomicAdd(res, c); atomicMax(res + 1, c); }
        if (d) atomicMax(res + 2, (int) d);
    }
}

// A workgroup takes DISCARD_ROWS rows of DISCARD_THREADS neighbouring columns, a column per lane: consecutive lanes read consecutive
// elements of a row (the rows of a tile are independent loads), and a column's count of the tile goes to discard_partial_off(tile, x).
// Grid: discard_col_blocks(w0) x discard_row_tiles(h0).  The deepest level needs no line: a wave's maximum goes straight to the result.
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_cross(const float *bias, const int32_t *vs, int w0, int h0, float thr, int level, int depth,
                                                                 int *partial, int *res)
{
    const int x = blockIdx.x * DISCARD_THREADS + threadIdx.x, tile = blockIdx.y;
    const int y0 = tile * DISCARD_ROWS, y1 = min(y0 + DISCARD_ROWS, h0);
    const unsigned level1 = (unsigned) (level - 1), dp = (unsigned) depth;
    int count = 0;
    unsigned deep = 0;
    if (x < w0) {
#pragma unroll 4
        for (int y = y0; y < y1; y++) {
            const size_t at = (size_t) y * w0 + x;
            discard_px(bias[at], (unsigned) vs[at], thr, level1, dp, count, deep);
        }
        partial[discard_partial_off(tile, x, w0)] = count;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned d = __shfl_down(deep, o);
        deep = d > deep ? d : deep;
    }
    if ((threadIdx.x & 63) == 0 && deep) atomicMax(res + 2, (int) deep);
}

// The lines across the rows of a carver that hides pixels (level > 1): the pixel shown in column x of a line is the x-th VISIBLE pixel of its
// row, so a workgroup ranks a row as k_compact does -- DISCARD_THREADS columns at a time, block_rank_256 -- and a marked visible pixel
// adds one to its image column's count, col[rank] (discard_rank_elems(w) counts, zeroed by the shim; marked pixels are few, and integer
// sums do not depend on their order).  Only a read-out of a carver that lies the other way and is not at level 1 comes here: the
// removal's own scans do not.
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_rank(const float *bias, const int32_t *vs, int w0, int w, float thr, int level, int depth, int *col,
                                                                int *res)
{
    __shared__ int s_wave[DISCARD_THREADS / 64];
    const int y = blockIdx.x, tid = threadIdx.x;
    const float *brow = bias + (size_t) y * w0;
    const int32_t *vrow = vs + (size_t) y * w0;
    const unsigned level1 = (unsigned) (level - 1), dp = (unsigned) depth;
    int carry = 0;
    unsigned deep = 0;
    for (int base = 0; base < w0; base += DISCARD_THREADS) {
        const int x = base + tid;
        const bool in = x < w0;
        const unsigned v = in ? (unsigned) vrow[x] : 0u;
        const bool marked = in && brow[in ? x : 0] < thr, keep = in && v - 1u >= level1;
        int total;
        const int rank = carry + block_rank_256(keep, s_wave, total);
        if (marked && keep && rank < w) atomicAdd(col + rank, 1);
        const unsigned d = v > dp ? v - dp : 0u;
        deep = (marked && d > deep) ? d : deep;
        carry += total;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned d = __shfl_down(deep, o);
        deep = d > deep ? d : deep;
    }
    if ((tid & 63) == 0 && deep) atomicMax(res + 2, (int) deep);
}

// the tiles' counts of every column summed (a lane per column, reads along the rows of `partial`), then the total and the fullest column
__global__ __launch_bounds__(DISCARD_THREADS) void k_discard_fold(const int *partial, int w0, int tiles, int *res)
{
    __shared__ int s_sum[DISCARD_THREADS / 64], s_max[DISCARD_THREADS / 64];
    const int x = blockIdx.x * DISCARD_THREADS + threadIdx.x, tid = threadIdx.x;
    int line = 0;
    if (x < w0)
        for (int t = 0; t < tiles; t++) line += partial[discard_partial_off(t, x, w0)];
    int sum = line, most = line;
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o);
        most = max(most, __shfl_down(most, o));
    }
    if ((tid & 63) == 0) { s_sum[tid >> 6] = sum; s_max[tid >> 6] = most; }
    __syncthreads();
    if (tid == 0) {
        const int c = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (c) { atomicAdd(res, c); atomicMax(res + 1, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]))); }
    }
}
