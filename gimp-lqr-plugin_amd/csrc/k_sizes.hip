// k_sizes.hip -- a carver read at many sizes in one pass over its base layout (include/lqr_sizes.h):
// k_compact_sizes compacts the pixels visible at up to SZ_MAX_JOBS levels from ONE load of each row, k_transpose_sizes turns the
// planes of a carver that lies transposed into image orientation
// (gfx950 / CDNA4, wave64; see lqr_common.h for the file map)
#include "lqr_common.h"
#include "lqr_kernels.h"

// The caller's outputs start at any multiple of the SAMPLE size (a slice of a tensor), not of the pixel size: the widest unit, 1 .. 16
// bytes, that divides both the output's address and the pixel size.  Every pixel of that output then starts on a multiple of it.
__device__ __forceinline__ int sz_unit(const uint8_t *out, int bytes)
{
    const unsigned a = (unsigned) (uintptr_t) out | (unsigned) bytes | 16u;
    return (int) (a & (0u - a));
}
// the lanes in front of this one whose bit is set in a ballot
__device__ __forceinline__ unsigned sz_below(unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((unsigned) (b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) b, 0u)); }
// a pixel of up to 4 bytes, held in a dword, to an address aligned to `unit`
__device__ __forceinline__ void sz_store(uint8_t *dst, uint32_t p, int bytes, int unit)
{
    if (unit == 4) *(uint32_t *) dst = p;
    else if (unit == 2) for (int k = 0; k < bytes; k += 2) *(uint16_t *) (dst + k) = (uint16_t) (p >> (8 * k));
    else for (int k = 0; k < bytes; k++) dst[k] = (uint8_t) (p >> (8 * k));
}
__device__ __forceinline__ uint32_t sz_load(const uint8_t *src, int bytes)
{
    if (bytes == 4) return *(const uint32_t *) src;         // (the base layout and the scratch planes are dword-aligned)
    uint32_t p = 0;
    for (int k = 0; k < bytes; k++) p |= (uint32_t) src[k] << (8 * k);
    return p;
}
// a pixel wider than 4 bytes: BasePx<true>::move where the output is aligned to the pixel's own unit, else in the unit it is aligned to
__device__ __forceinline__ void sz_move(uint8_t *dst, const uint8_t *src, int bytes, int unit)
{
    const unsigned own = ((unsigned) bytes | 16u) & (0u - ((unsigned) bytes | 16u));
    if (unit == (int) own) BasePx<true>::move(dst, src, bytes);
    else if (unit == 8) for (int k = 0; k < bytes; k += 8) *(uint64_t *) (dst + k) = *(const uint64_t *) (src + k);
    else if (unit == 4) for (int k = 0; k < bytes; k += 4) *(uint32_t *) (dst + k) = *(const uint32_t *) (src + k);
    else if (unit == 2) for (int k = 0; k < bytes; k += 2) *(uint16_t *) (dst + k) = *(const uint16_t *) (src + k);
    else for (int k = 0; k < bytes; k++) dst[k] = src[k];
}

// One workgroup per frame row, SZ_CHUNK columns at a time, four columns per lane: their levels are loaded once and stay in registers
// while every job is ranked from them.  A column is kept at a level when v == 0 || v >= level, which is
// (unsigned) (v - 1) >= (unsigned) (level - 1).  Two barriers per chunk however many jobs there are: every wave leaves its totals of ALL
// jobs in LDS (barrier), every lane ranks and stores (barrier), then the carries -- the columns each job kept in earlier chunks -- move
// on; the totals are double-buffered so that the next chunk's may be written while the carries are still being added up.  No array is
// indexed at run time: the kernel uses no scratch.  (rank < width: a map that holds what lqr_vmap_load checks keeps exactly `width`
// columns of a row; whatever the map holds, nothing is written past a row.)
//
// Pixels of up to 4 bytes: a lane takes four NEIGHBOURING columns and holds their pixels too, a dword each, loaded with the levels in
// 16-byte loads where the four lie inside the row.  The chunks are laid so that a lane's four columns start on a 16-byte boundary of
// the plane whatever the row (a row starts at y * w0 elements: the first chunk begins up to three columns in front of it, masked out).
// Rank = carry + the totals of the waves in front + the kept columns of the lanes in front (four ballots, mbcnt) + those of the lane's
// own in front.
static __device__ __forceinline__ void compact_sizes_narrow(const uint8_t *rgb, const int32_t *vs, const SizeJob *s_job, int *s_carry, int n_jobs, int w0, int bytes)
{
    __shared__ int s_tot[2][SZ_MAX_JOBS][4];
    const int y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t ri = (size_t) y * w0;
    const int32_t *vrow = vs + ri;
    int par = 0;
    for (int base = -(int) (ri & 3); base < w0; base += SZ_CHUNK, par ^= 1) {
        const int g = base + 4 * tid;
        const bool full = g >= 0 && g + 3 < w0;
        const bool ok0 = (unsigned) g < (unsigned) w0, ok1 = (unsigned) (g + 1) < (unsigned) w0, ok2 = (unsigned) (g + 2) < (unsigned) w0,
                   ok3 = (unsigned) (g + 3) < (unsigned) w0;
        unsigned v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
        const uint8_t *src = rgb + (ri + g) * bytes;          // (formed for every lane, followed only where ok)
        if (full) {
            const u32x4 vv = *(const u32x4 *) (vrow + g);
            v0 = vv.x; v1 = vv.y; v2 = vv.z; v3 = vv.w;
        } else {
            if (ok0) v0 = (unsigned) vrow[g];
            if (ok1) v1 = (unsigned) vrow[g + 1];
            if (ok2) v2 = (unsigned) vrow[g + 2];
            if (ok3) v3 = (unsigned) vrow[g + 3];
        }
        if (full && bytes == 4) {
            const u32x4 pp = *(const u32x4 *) src;
            p0 = pp.x; p1 = pp.y; p2 = pp.z; p3 = pp.w;
        } else {
            if (ok0) p0 = sz_load(src, bytes);
            if (ok1) p1 = sz_load(src + bytes, bytes);
            if (ok2) p2 = sz_load(src + 2 * bytes, bytes);
            if (ok3) p3 = sz_load(src + 3 * bytes, bytes);
        }
        v0--; v1--; v2--; v3--;
        for (int j = 0; j < n_jobs; j++) {
            const unsigned l = (unsigned) (s_job[j].level - 1);
            const int t = __popcll(__ballot(ok0 && v0 >= l)) + __popcll(__ballot(ok1 && v1 >= l)) + __popcll(__ballot(ok2 && v2 >= l)) +
                          __popcll(__ballot(ok3 && v3 >= l));
            if (lane == 0) s_tot[par][j][wv] = t;
        }
        __syncthreads();
        for (int j = 0; j < n_jobs; j++) {
            const unsigned l = (unsigned) (s_job[j].level - 1);
            const int width = s_job[j].width;
            uint8_t *out = s_job[j].out;
            const int unit = sz_unit(out, bytes);
            const bool k0 = ok0 && v0 >= l, k1 = ok1 && v1 >= l, k2 = ok2 && v2 >= l, k3 = ok3 && v3 >= l;
            const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1), b2 = __ballot(k2), b3 = __ballot(k3);
            int rank = s_carry[j] + (int) (sz_below(b0) + sz_below(b1) + sz_below(b2) + sz_below(b3));
            const int t0 = s_tot[par][j][0], t1 = s_tot[par][j][1], t2 = s_tot[par][j][2];
            rank += (wv > 0 ? t0 : 0) + (wv > 1 ? t1 : 0) + (wv > 2 ? t2 : 0);
            uint8_t *dst = out + ((size_t) y * width + rank) * bytes;
            if (k0 && rank < width) sz_store(dst, p0, bytes, unit);
            if (k0) { rank++; dst += bytes; }
            if (k1 && rank < width) sz_store(dst, p1, bytes, unit);
            if (k1) { rank++; dst += bytes; }
            if (k2 && rank < width) sz_store(dst, p2, bytes, unit);
            if (k2) { rank++; dst += bytes; }
            if (k3 && rank < width) sz_store(dst, p3, bytes, unit);
        }
        __syncthreads();
        if (tid < n_jobs) s_carry[tid] += s_tot[par][tid][0] + s_tot[par][tid][1] + s_tot[par][tid][2] + s_tot[par][tid][3];
    }
}

// Wider pixels (bytes each) are not held: they move from the base layout to every output that keeps them, so what matters is that the
// lanes of a wave write NEIGHBOURING pixels of the output (four neighbouring 32-byte pixels per lane ran at a third of this).  A lane's
// four columns lie 256 apart: slot s of the chunk is 256 consecutive columns, 64 per wave.  Rank = carry + the totals of the slots in
// front + those of the waves in front within the slot + the kept columns of the lanes in front (one ballot): 16 totals per job and chunk.
static __device__ __forceinline__ void compact_sizes_deep(const uint8_t *rgb, const int32_t *vs, const SizeJob *s_job, int *s_carry, int n_jobs, int w0, int bytes)
{
    __shared__ int s_tot[2][SZ_MAX_JOBS][16];
    const int y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t ri = (size_t) y * w0;
    const int32_t *vrow = vs + ri;
    int par = 0;
    for (int base = 0; base < w0; base += SZ_CHUNK, par ^= 1) {
        const int g0 = base + tid, g1 = g0 + 256, g2 = g0 + 512, g3 = g0 + 768;
        const bool ok0 = g0 < w0, ok1 = g1 < w0, ok2 = g2 < w0, ok3 = g3 < w0;
        unsigned v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        if (ok0) v0 = (unsigned) vrow[g0];
        if (ok1) v1 = (unsigned) vrow[g1];
        if (ok2) v2 = (unsigned) vrow[g2];
        if (ok3) v3 = (unsigned) vrow[g3];
        v0--; v1--; v2--; v3--;
        const uint8_t *src = rgb + (ri + g0) * bytes;
        const size_t apart = (size_t) 256 * bytes;
        for (int j = 0; j < n_jobs; j++) {
            const unsigned l = (unsigned) (s_job[j].level - 1);
            const int t0 = __popcll(__ballot(ok0 && v0 >= l)), t1 = __popcll(__ballot(ok1 && v1 >= l)), t2 = __popcll(__ballot(ok2 && v2 >= l)),
                      t3 = __popcll(__ballot(ok3 && v3 >= l));
            if (lane == 0) { s_tot[par][j][wv] = t0; s_tot[par][j][4 + wv] = t1; s_tot[par][j][8 + wv] = t2; s_tot[par][j][12 + wv] = t3; }
        }
        __syncthreads();
        for (int j = 0; j < n_jobs; j++) {
            const unsigned l = (unsigned) (s_job[j].level - 1);
            const int width = s_job[j].width;
            uint8_t *row = s_job[j].out + (size_t) y * width * bytes;
            const int unit = sz_unit(s_job[j].out, bytes);
            const bool k0 = ok0 && v0 >= l, k1 = ok1 && v1 >= l, k2 = ok2 && v2 >= l, k3 = ok3 && v3 >= l;
            const int *t = s_tot[par][j];
#define SZ_FRONT(s) ((wv > 0 ? t[4 * (s)] : 0) + (wv > 1 ? t[4 * (s) + 1] : 0) + (wv > 2 ? t[4 * (s) + 2] : 0))
#define SZ_SLOT(s) (t[4 * (s)] + t[4 * (s) + 1] + t[4 * (s) + 2] + t[4 * (s) + 3])
            int at = s_carry[j];
            const int r0 = at + SZ_FRONT(0) + (int) sz_below(__ballot(k0));
            at += SZ_SLOT(0);
            const int r1 = at + SZ_FRONT(1) + (int) sz_below(__ballot(k1));
            at += SZ_SLOT(1);
            const int r2 = at + SZ_FRONT(2) + (int) sz_below(__ballot(k2));
            at += SZ_SLOT(2);
            const int r3 = at + SZ_FRONT(3) + (int) sz_below(__ballot(k3));
#undef SZ_FRONT
#undef SZ_SLOT
            if (k0 && r0 < width) sz_move(row + (size_t) r0 * bytes, src, bytes, unit);
            if (k1 && r1 < width) sz_move(row + (size_t) r1 * bytes, src + apart, bytes, unit);
            if (k2 && r2 < width) sz_move(row + (size_t) r2 * bytes, src + 2 * apart, bytes, unit);
            if (k3 && r3 < width) sz_move(row + (size_t) r3 * bytes, src + 3 * apart, bytes, unit);
        }
        __syncthreads();
        if (tid < n_jobs) {
            int sum = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) sum += s_tot[par][tid][i];
            s_carry[tid] += sum;
        }
    }
}

template <bool DEEP>
__global__ __launch_bounds__(256) void k_compact_sizes(const uint8_t *rgb, const int32_t *vs, const SizeJob *jobs, int n_jobs, int w0, int bytes)
{
    __shared__ int s_carry[SZ_MAX_JOBS];
    __shared__ SizeJob s_job[SZ_MAX_JOBS];
    if (threadIdx.x < SZ_MAX_JOBS) s_carry[threadIdx.x] = 0;
    if ((int) threadIdx.x < n_jobs) s_job[threadIdx.x] = jobs[threadIdx.x];
    __syncthreads();
    if (DEEP) compact_sizes_deep(rgb, vs, s_job, s_carry, n_jobs, w0, bytes);
    else compact_sizes_narrow(rgb, vs, s_job, s_carry, n_jobs, w0, bytes);
}

// The planes k_compact_sizes left of a carver that lies transposed (job blockIdx.z: `width` x h pixels, frame orientation) into the
// caller's images (h x width): tiles of 32 x 32 pixels through a padded LDS tile, so that the reads run along the rows of the plane
// and the writes along the rows of the image.  The width is the job's: a workgroup whose tile lies beyond it has nothing to do.
// Pixels of up to 4 bytes go through the tile as dwords.  WIDE: wider pixels go in slices of four units of the width the output's
// address allows (a dword where it can be: 16 bytes per pixel and pass), each lane a unit, in the order of the side it touches.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_transpose_sizes(const SizeJob *jobs, int h, int bytes)
{
    __shared__ uint32_t tile[32][WIDE ? 32 * 4 + 1 : 33];
    const SizeJob j = jobs[blockIdx.z];
    const int w = j.width, x0 = blockIdx.x * 32, y0 = blockIdx.y * 32, tid = threadIdx.x;
    if (x0 >= w) return;
    const int unit = sz_unit(j.out, bytes);
    if (!WIDE) {
        const int tx = tid & 31, ty = tid >> 5;
        for (int i = ty; i < 32; i += 8)
            if (x0 + tx < w && y0 + i < h) tile[i][tx] = sz_load(j.src + ((size_t) (y0 + i) * w + x0 + tx) * bytes, bytes);
        __syncthreads();
        for (int i = ty; i < 32; i += 8)
            if (x0 + i < w && y0 + tx < h) sz_store(j.out + ((size_t) (x0 + i) * h + y0 + tx) * bytes, tile[tx][i], bytes, unit);
    } else {
        const int U = unit < 4 ? unit : 4, nu = bytes / U;
        for (int s = 0; s < nu; s += 4) {
            const int nk = nu - s < 4 ? nu - s : 4, per_row = 32 * nk;
            if (s) __syncthreads();
            for (int i = tid; i < 32 * per_row; i += 256) {
                const int r = i / per_row, c = i - r * per_row, px = c / nk, k = c - px * nk;
                if (x0 + px < w && y0 + r < h) {
                    const uint8_t *p = j.src + ((size_t) (y0 + r) * w + x0 + px) * bytes + (size_t) (s + k) * U;
                    tile[r][px * 4 + k] = U == 4 ? *(const uint32_t *) p : U == 2 ? (uint32_t) *(const uint16_t *) p : (uint32_t) *p;
                }
            }
            __syncthreads();
            for (int i = tid; i < 32 * per_row; i += 256) {
                const int px = i / per_row, c = i - px * per_row, r = c / nk, k = c - r * nk;
                if (x0 + px < w && y0 + r < h) {
                    uint8_t *p = j.out + ((size_t) (x0 + px) * h + y0 + r) * bytes + (size_t) (s + k) * U;
                    const uint32_t v = tile[r][px * 4 + k];
                    if (U == 4) *(uint32_t *) p = v; else if (U == 2) *(uint16_t *) p = (uint16_t) v; else *p = (uint8_t) v;
                }
            }
        }
    }
}

// ---- the instantiations the shim launches (lqr_kernels.h declares them)
#define INST_COMPACT_SIZES(D) template __global__ void k_compact_sizes<D>(const uint8_t *, const int32_t *, const SizeJob *, int, int, int);
K_COMPACT_SIZES_FORMS(INST_COMPACT_SIZES)
#define INST_TRANSPOSE_SIZES(W) template __global__ void k_transpose_sizes<W>(const SizeJob *, int, int);
K_TRANSPOSE_SIZES_FORMS(INST_TRANSPOSE_SIZES)
