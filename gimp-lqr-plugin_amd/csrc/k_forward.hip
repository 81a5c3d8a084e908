// k_forward.hip -- forward-energy seam maps (include_ext/lqr_forward.h): a second seam finder beside the tuned seam loop.
// It does not touch a carver's working planes: it reads the base layout of flat carvers once (k_fwd_init) and from then on works on
// planes of its own, H lines of L in the frame of the carving direction, and writes a seam map in image orientation that
// lqr_vmap_load's path validates and loads like any other.
//
// The rule (Rubinstein, Shamir, Avidan 2008; tests/forward_cases.py is the specification, bit for bit).  On the current frame, wc wide:
//     l = I(max(x-1,0), y)   r = I(min(x+1,wc-1), y)   u = I(x, y-1)
//     CU = |r - l|   CL = CU + |u - l|   CR = CU + |u - r|
//     M(x,0) = P(x,0) + CU        M(x,y) = P(x,y) + min(M(x,y-1) + CU, M(x-1,y-1) + CL, M(x+1,y-1) + CR)
// every operation a float operation rounded on its own; ties up, then left, then right; the seam ends at the smallest x with the least
// M(., H-1); its pixels get level k at the positions they had at the start, and leave I, P and the position plane.
//
// Per seam two launches, whatever the number of images:
//   k_fwd_seam    one workgroup per image: the row sweep with the two live rows of M in LDS (one barrier per row), the pick, and the
//                 walk up through the stored choices, FWD_WALK_ROWS rows of the seam's cone staged in LDS at a time
//   k_fwd_remove  one workgroup per line and image: the seam's pixel leaves the line, its level goes to the map
// No spin waits and no hand-overs between workgroups: the workgroup barrier and the order of the launches are the only synchronisation.
#include "lqr_common.h"
#include "lqr_kernels.h"

typedef GLOBAL_AS uint16_t gu16;

// ---------------------------------------------------------------------------
// the one-off pass: I, P and the positions of n images from their base layouts, the maps cleared
// ---------------------------------------------------------------------------
// The base layout is fw0 pixels per row in the carver's frame.  strided = 0: the carving direction runs along those rows (L = fw0);
// 1: across them (the carver lies the other way: pixel x of line y is pixel y of row x).  Every carver comes through deep_value, the
// packed 8-bit ones too: for grey / RGB (+ alpha) it is px_bright's arithmetic, operation for operation.
template <int DEPTH>
__global__ __launch_bounds__(256) void k_fwd_init(const FwdJob *jobs, int L, int H, int fw0, int strided, DeepRead rd, int w_start, int orientation)
{
    const FwdJob j = jobs[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= L) return;
    constexpr int bpc = DEPTH == 0 ? 1 : DEPTH == 1 ? 2 : DEPTH == 2 ? 4 : 8;
    const size_t i = strided ? (size_t) x * fw0 + y : (size_t) y * fw0 + x;
    const size_t o = (size_t) y * L + x;
    ((gf32 *) j.in)[o] = __double2float_rn(deep_value<DEPTH>((const gu8 *) j.rgb0 + i * rd.ch * bpc, rd));
    if (j.p) ((gf32 *) j.p)[o] = __fdiv_rn(((const gf32 *) j.bias0)[i], (float) w_start);
    ((gu16 *) j.pos)[o] = (uint16_t) x;
    ((gi32 *) j.map)[orientation ? (size_t) x * H + y : o] = 0;
}

// ---------------------------------------------------------------------------
// one seam: sweep, pick, walk
// ---------------------------------------------------------------------------
// Thread t holds the pixels t + k * FWD_THREADS of a row: neighbouring threads read neighbouring words of LDS and of the planes.  What
// a row needs from the planes (l, r, the pixel itself -- which is the next row's u -- and P) does not depend on the row above, so the
// loads of row y + 1 are issued before the barrier of row y and land under it (AHEAD; at 16 pixels per thread they would not fit the
// 128 registers of a 16-wave workgroup, and the row loads its own).  Row y reads M from one half of s_m and writes the other.
template <int PXT>
__global__ __launch_bounds__(FWD_THREADS) void k_fwd_seam(const FwdJob *jobs, int wc, int L, int H)
{
    extern __shared__ float s_m[];                          // [2][L]
    __shared__ int8_t s_cone[FWD_WALK_ROWS][2 * FWD_WALK_ROWS];
    __shared__ int s_path[FWD_WALK_ROWS];
    __shared__ float s_rv[FWD_THREADS / 64];
    __shared__ int s_rx[FWD_THREADS / 64];
    __shared__ int s_x;
    constexpr bool AHEAD = PXT <= 8;
    const float INF = __int_as_float(0x7f800000);
    const FwdJob j = jobs[blockIdx.x];
    const gf32 *in = (const gf32 *) j.in, *pl = (const gf32 *) j.p;
    gi8 *choice = (gi8 *) j.choice;
    gi32 *seam = (gi32 *) j.seam;
    const int tid = threadIdx.x;

    float rl[PXT], rr[PXT], rc[PXT], rp[PXT], up[PXT];
#pragma unroll
    for (int k = 0; k < PXT; k++) { rl[k] = rr[k] = rc[k] = rp[k] = up[k] = 0.0f; }
    auto load_row = [&](int y) {
        const gf32 *row = in + (size_t) y * L;
#pragma unroll
        for (int k = 0; k < PXT; k++) {
            const int x = tid + k * FWD_THREADS;
            if (x < wc) {
                rl[k] = row[max(x - 1, 0)];
                rr[k] = row[min(x + 1, wc - 1)];
                rc[k] = row[x];
                if (pl) rp[k] = pl[(size_t) y * L + x];
            }
        }
    };
    // pixel x of row y from its three costs and its P: the recurrence, the choice stored
    auto pixel = [&](int x, int y, const float *mp, float *mc, float cu, float cl, float cr, float pp) {
        float best = cu;
        int d = 0;
        if (y > 0) {
            best = __fadd_rn(mp[x], cu);
            if (x > 0) { const float t = __fadd_rn(mp[x - 1], cl); if (t < best) { best = t; d = -1; } }
            if (x < wc - 1) { const float t = __fadd_rn(mp[x + 1], cr); if (t < best) { best = t; d = 1; } }
        }
        mc[x] = __fadd_rn(pp, best);
        choice[(size_t) y * L + x] = (int8_t) d;
    };
    if (AHEAD) load_row(0);
    for (int y = 0; y < H; y++) {
        const float *mp = s_m + ((y & 1) ^ 1) * L;
        float *mc = s_m + (y & 1) * L;
        if constexpr (AHEAD) {
            float cu[PXT], cl[PXT], cr[PXT], pp[PXT];
#pragma unroll
            for (int k = 0; k < PXT; k++) {
                cu[k] = fabsf(__fsub_rn(rr[k], rl[k]));
                cl[k] = __fadd_rn(cu[k], fabsf(__fsub_rn(up[k], rl[k])));
                cr[k] = __fadd_rn(cu[k], fabsf(__fsub_rn(up[k], rr[k])));
                pp[k] = rp[k];
                up[k] = rc[k];
            }
            if (y + 1 < H) load_row(y + 1);
            __syncthreads();                                // the row above is complete, and nobody reads the half this row writes
#pragma unroll
            for (int k = 0; k < PXT; k++) {
                const int x = tid + k * FWD_THREADS;
                if (x < wc) pixel(x, y, mp, mc, cu[k], cl[k], cr[k], pp[k]);
            }
        } else {
            // pixel by pixel: only the row above's own pixels (up) live from row to row
            const gf32 *row = in + (size_t) y * L;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PXT; k++) {
                const int x = tid + k * FWD_THREADS;
                if (x < wc) {
                    const float l = row[max(x - 1, 0)], r = row[min(x + 1, wc - 1)], c = row[x];
                    const float pp = pl ? pl[(size_t) y * L + x] : 0.0f;
                    const float cu = fabsf(__fsub_rn(r, l));
                    pixel(x, y, mp, mc, cu, __fadd_rn(cu, fabsf(__fsub_rn(up[k], l))), __fadd_rn(cu, fabsf(__fsub_rn(up[k], r))), pp);
                    up[k] = c;
                }
            }
        }
    }
    __syncthreads();

    // the pick: the smallest x with the least M on the last row.  Values that compare with nothing (NaN) are never taken; a row of them
    // ends at column 0
    {
        const float *last = s_m + ((H - 1) & 1) * L;
        float bv = INF;
        int bx = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < PXT; k++) {
            const int x = tid + k * FWD_THREADS;
            if (x < wc) { const float v = last[x]; if (v < bv || (v == bv && x < bx)) { bv = v; bx = x; } }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_down(bv, o);
            const int ox = __shfl_down(bx, o);
            if (ov < bv || (ov == bv && ox < bx)) { bv = ov; bx = ox; }
        }
        if ((tid & 63) == 0) { s_rv[tid >> 6] = bv; s_rx[tid >> 6] = bx; }
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < FWD_THREADS / 64; i++)
                if (s_rv[i] < bv || (s_rv[i] == bv && s_rx[i] < bx)) { bv = s_rv[i]; bx = s_rx[i]; }
            if (bx >= wc) bx = 0;
            s_x = bx;
            seam[H - 1] = bx;
        }
        __syncthreads();
    }

    // the walk.  From column x0 on row y_top the seam can reach columns x0 - r .. x0 + r on row y_top - r: the choices of R rows of that
    // cone are staged by the whole workgroup, thread 0 walks them in LDS, and the columns found go out together
    constexpr int R = FWD_WALK_ROWS, W = 2 * FWD_WALK_ROWS;
    for (int y_top = H - 1; y_top > 0; y_top -= R) {
        const int x0 = s_x;
        const int nrows = min(R, y_top);
        for (int i = tid; i < nrows * W; i += FWD_THREADS) {
            const int r = i / W, ci = i % W;
            const int col = min(max(x0 - R + ci, 0), wc - 1);         // (columns outside the frame: the seam never goes there)
            s_cone[r][ci] = choice[(size_t) (y_top - r) * L + col];
        }
        __syncthreads();
        if (tid == 0) {
            int xx = x0;
            for (int r = 0; r < nrows; r++) {
                xx = min(max(xx + s_cone[r][min(max(xx - x0 + R, 0), W - 1)], 0), wc - 1);
                s_path[r] = xx;                                        // the column on row y_top - 1 - r
            }
            s_x = xx;
        }
        __syncthreads();
        if (tid < nrows) seam[y_top - 1 - tid] = s_path[tid];
    }
}

// ---------------------------------------------------------------------------
// the removal: one line of one image per workgroup
// ---------------------------------------------------------------------------
// The part right of the seam moves one place left, in I, P and the position plane, in rounds of FWD_REMOVE_THREADS * FWD_REMOVE_PX
// pixels: a round reads, waits for the workgroup, and writes -- what it writes the round before has read, what the next round reads
// lies further right.  The level goes to where the seam's pixel stood at the start.
__global__ __launch_bounds__(FWD_REMOVE_THREADS) void k_fwd_remove(const FwdJob *jobs, int wc, int L, int H, int level, int orientation)
{
    const FwdJob j = jobs[blockIdx.y];
    const int y = blockIdx.x, tid = threadIdx.x;
    gf32 *in = (gf32 *) j.in + (size_t) y * L;
    gf32 *pl = j.p ? (gf32 *) j.p + (size_t) y * L : nullptr;
    gu16 *pos = (gu16 *) j.pos + (size_t) y * L;
    const int sx = min(max(((const gi32 *) j.seam)[y], 0), wc - 1);
    const int orig = pos[sx];                                          // (read by every thread before the first round's barrier)
    for (int base = sx; base < wc - 1; base += FWD_REMOVE_THREADS * FWD_REMOVE_PX) {
        float vi[FWD_REMOVE_PX], vp[FWD_REMOVE_PX];
        uint16_t vo[FWD_REMOVE_PX];
#pragma unroll
        for (int k = 0; k < FWD_REMOVE_PX; k++) {
            const int x = base + tid + k * FWD_REMOVE_THREADS;
            vi[k] = 0.0f; vp[k] = 0.0f; vo[k] = 0;
            if (x < wc - 1) {
                vi[k] = in[x + 1];
                if (pl) vp[k] = pl[x + 1];
                vo[k] = pos[x + 1];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FWD_REMOVE_PX; k++) {
            const int x = base + tid + k * FWD_REMOVE_THREADS;
            if (x < wc - 1) {
                in[x] = vi[k];
                if (pl) pl[x] = vp[k];
                pos[x] = vo[k];
            }
        }
    }
    if (tid == 0) ((gi32 *) j.map)[orientation ? (size_t) orig * H + y : (size_t) y * L + orig] = level;
}

#define INSTANTIATE(D) template __global__ void k_fwd_init<D>(const FwdJob *, int, int, int, int, DeepRead, int, int);
K_FWD_INIT_FORMS(INSTANTIATE)
#undef INSTANTIATE
#define INSTANTIATE(P) template __global__ void k_fwd_seam<P>(const FwdJob *, int, int, int);
K_FWD_SEAM_FORMS(INSTANTIATE)
#undef INSTANTIATE
