// k_clipfwd.hip -- forward-energy seams for a clip (include_ext/lqr_clipforward.h): ONE seam map from the forward costs of
// ALL frames.  The I plane of every frame is formed by k_fwd_init (k_forward.hip), the same deep_value path as a single image's build, and
// is never compacted; everything else the finder works on exists once per clip, H lines of L in the frame of the carving direction.
//
// The rule (Rubinstein, Shamir, Avidan 2008; tests/clipforward_cases.py is the specification, bit for bit).  Made once, travelling with
// their pixels:  T = max_{t>=1} |I_t - I_{t-1}|,  Pm = max_t P_t,  Q = Pm + temporal * T.  On the current frames, wc wide, per frame t
//     l = I_t(max(x-1,0), y)   r = I_t(min(x+1,wc-1), y)   u = I_t(x, y-1)
// and over the frames
//     CU = max_t |r - l|   CL = max_t (|r - l| + |u - l|)   CR = max_t (|r - l| + |u - r|)
//     M(x,0) = Q + CU          M(x,y) = Q + min(M(x,y-1) + CU, M(x-1,y-1) + CL, M(x+1,y-1) + CR)
// every operation a float operation rounded on its own; ties up, then left, then right; the seam ends at the smallest x with the least
// M(., H-1); its pixels get level k at the positions they had at the start and leave the costs, Q and the position plane.
//
//   k_clip_fold     once: CU, CL, CR and Q of every pixel from the n frames, CLIPFWD_GROUP frames a launch
// Per seam three launches, whatever the number of frames:
//   k_clip_seam     ONE workgroup: k_fwd_seam's sweep, pick and walk, reading the four costs of a pixel instead of forming them from I
//   k_clip_remove   one workgroup per line: the seam's pixel leaves the costs and the position plane, its level goes to the map
//   k_clip_refresh  one workgroup per line: a seam that left at column s changes l, r or u of the new columns s - 1 and s only; their
//                   three costs are formed again from the n frames, whose pixels are found through the position plane.  (A launch of its
//                   own: it reads the positions of the line above, which that line's removal moves.)
// No spin waits and no hand-overs between workgroups: the workgroup barrier and the order of the launches are the only synchronisation.
// The maxima over frames are taken in registers, by wave shuffles and through LDS: no atomics.
#include "lqr_common.h"
#include "lqr_kernels.h"

typedef GLOBAL_AS uint16_t gu16;
typedef float f32x4 __attribute__((ext_vector_type(4)));        // (a native vector: HIP's float4 class does not copy out of an address space)
typedef GLOBAL_AS f32x4 gf32x4;
static_assert(CLIP_COST_FLOATS == 4, "the costs of a pixel are one 16-byte vector: CU, CL, CR, Q");

// ---------------------------------------------------------------------------
// the fold: the costs of the whole frames, once
// ---------------------------------------------------------------------------
// A thread per pixel; frames first .. first + count - 1 of the clip.  A launch that is not the first continues from the running maxima
// (CU, CL, CR and T in `cost`, Pm in `pm`) and from the I of the frame before its first; the last one mixes Q into T's place.  The bias is
// read from the frames' base layouts as k_fwd_init reads it (fw0 floats per row; strided: the frame lies the other way) -- pm null: no
// frame has one and Pm is 0.  Line 0 has no line above: its CL and CR are 0 and never read.
__global__ __launch_bounds__(CLIPFWD_FOLD_THREADS) void k_clip_fold(const FwdJob *jobs, const float *in_all, int first, int count, int last, int L, int H, int fw0,
                                                                   int strided, int w_start, float temporal, float *cost_all, float *pm_all)
{
    const int x = blockIdx.x * CLIPFWD_FOLD_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= L) return;
    const size_t px = (size_t) L * H, o = (size_t) y * L + x;
    const size_t ol = (size_t) y * L + max(x - 1, 0), orr = (size_t) y * L + min(x + 1, L - 1), ou = y > 0 ? o - L : o;
    const size_t ib = strided ? (size_t) x * fw0 + y : (size_t) y * fw0 + x;
    gf32x4 *cost = (gf32x4 *) cost_all + o;
    gf32 *pm = pm_all ? (gf32 *) pm_all + o : nullptr;
    float cu = 0.0f, cl = 0.0f, cr = 0.0f, tt = 0.0f, pp = 0.0f, prev = 0.0f;
    if (first > 0) {
        const f32x4 c = *cost;
        cu = c.x; cl = c.y; cr = c.z; tt = c.w;
        if (pm) pp = *pm;
        prev = ((const gf32 *) in_all)[clip_frame_off(first - 1, px) + o];
    }
    for (int k = 0; k < count; k++) {
        const int t = first + k;
        const gf32 *in = (const gf32 *) in_all + clip_frame_off(t, px);
        const float l = in[ol], r = in[orr], c = in[o];
        const float a = fabsf(__fsub_rn(r, l));
        cu = fmaxf(cu, a);
        if (y > 0) {
            const float u = in[ou];
            cl = fmaxf(cl, __fadd_rn(a, fabsf(__fsub_rn(u, l))));
            cr = fmaxf(cr, __fadd_rn(a, fabsf(__fsub_rn(u, r))));
        }
        if (t > 0) tt = fmaxf(tt, fabsf(__fsub_rn(c, prev)));
        prev = c;
        if (pm) {
            const float pv = __fdiv_rn(((const gf32 *) jobs[t].bias0)[ib], (float) w_start);
            pp = t > 0 ? fmaxf(pp, pv) : pv;
        }
    }
    if (last) {
        *cost = f32x4{cu, cl, cr, __fadd_rn(pp, __fmul_rn(temporal, tt))};
    } else {
        *cost = f32x4{cu, cl, cr, tt};
        if (pm) *pm = pp;
    }
}

// ---------------------------------------------------------------------------
// one seam: sweep, pick, walk
// ---------------------------------------------------------------------------
// k_fwd_seam's, over given costs.  Thread t holds the pixels t + k * FWD_THREADS of a row.  The costs of a row do not depend on the rows
// above, and one workgroup has nothing else to hide a load's latency behind: the costs of the next AHEAD rows are in flight while a row
// is computed (4 rows at 1 or 2 pixels per thread, 3 at 4, 1 at 8; at 16 they would not fit the 128 registers of a 16-wave workgroup,
// and the row loads its own).  The loads stand outside every branch -- a column or row past the end reads the last one again -- so that
// the compiler waits for the oldest row only.  Row y reads M from one half of s_m and writes the other.
template <int PXT>
__global__ __launch_bounds__(FWD_THREADS) void k_clip_seam(const float *cost_all, int8_t *choice_all, int32_t *seam_all, int wc, int L, int H)
{
    extern __shared__ float s_m[];                          // [2][L]: fwd_lds(L)
    __shared__ int8_t s_cone[FWD_WALK_ROWS][2 * FWD_WALK_ROWS];
    __shared__ int s_path[FWD_WALK_ROWS];
    __shared__ float s_rv[FWD_THREADS / 64];
    __shared__ int s_rx[FWD_THREADS / 64];
    __shared__ int s_x;
    constexpr int AHEAD = PXT <= 2 ? 4 : PXT <= 4 ? 3 : PXT <= 8 ? 1 : 0;      // rows whose costs are in flight
    const float INF = __int_as_float(0x7f800000);
    const gf32x4 *cost = (const gf32x4 *) cost_all;
    gi8 *choice = (gi8 *) choice_all;
    gi32 *seam = (gi32 *) seam_all;
    const int tid = threadIdx.x;

    // pixel x of row y from its costs (c.x up, c.y left, c.z right, c.w Q): the recurrence, the choice stored
    auto pixel = [&](int x, int y, const float *mp, float *mc, const f32x4 c) {
        float best = c.x;
        int d = 0;
        if (y > 0) {
            best = __fadd_rn(mp[x], c.x);
            if (x > 0) { const float t = __fadd_rn(mp[x - 1], c.y); if (t < best) { best = t; d = -1; } }
            if (x < wc - 1) { const float t = __fadd_rn(mp[x + 1], c.z); if (t < best) { best = t; d = 1; } }
        }
        mc[x] = __fadd_rn(c.w, best);
        choice[(size_t) y * L + x] = (int8_t) d;
    };
    if constexpr (AHEAD > 0) {
        // the rows y .. y + AHEAD - 1 are in flight while row y is computed: row y + AHEAD takes row y's registers
        f32x4 nx[AHEAD][PXT];
        auto load_row = [&](int y, f32x4 (&to)[PXT]) {
            const gf32x4 *row = cost + (size_t) y * L;
#pragma unroll
            for (int k = 0; k < PXT; k++) to[k] = row[min(tid + k * FWD_THREADS, wc - 1)];       // (no branch around a load: the waits stay counted)
        };
#pragma unroll
        for (int a = 0; a < AHEAD; a++) load_row(min(a, H - 1), nx[a]);
        for (int y0 = 0; y0 < H; y0 += AHEAD) {
#pragma unroll
            for (int a = 0; a < AHEAD; a++) {
                const int y = y0 + a;
                if (y < H) {                                    // (the same for the whole workgroup)
                    const float *mp = s_m + fwd_row_off((y & 1) ^ 1, L);
                    float *mc = s_m + fwd_row_off(y & 1, L);
                    f32x4 cur[PXT];
#pragma unroll
                    for (int k = 0; k < PXT; k++) cur[k] = nx[a][k];
                    load_row(min(y + AHEAD, H - 1), nx[a]);         // (past the last row: the last row again, never used)
                    __syncthreads();                            // the row above is complete, and nobody reads the half this row writes
#pragma unroll
                    for (int k = 0; k < PXT; k++) {
                        const int x = tid + k * FWD_THREADS;
                        if (x < wc) pixel(x, y, mp, mc, cur[k]);
                    }
                }
            }
        }
    } else {
        for (int y = 0; y < H; y++) {
            const float *mp = s_m + fwd_row_off((y & 1) ^ 1, L);
            float *mc = s_m + fwd_row_off(y & 1, L);
            const gf32x4 *row = cost + (size_t) y * L;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PXT; k++) {
                const int x = tid + k * FWD_THREADS;
                if (x < wc) pixel(x, y, mp, mc, row[x]);
            }
        }
    }
    __syncthreads();

    // the pick: the smallest x with the least M on the last row.  Values that compare with nothing (NaN) are never taken; a row of them
    // ends at column 0
    {
        const float *lastrow = s_m + fwd_row_off((H - 1) & 1, L);
        float bv = INF;
        int bx = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < PXT; k++) {
            const int x = tid + k * FWD_THREADS;
            if (x < wc) { const float v = lastrow[x]; if (v < bv || (v == bv && x < bx)) { bv = v; bx = x; } }
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
// the removal: one line per workgroup
// ---------------------------------------------------------------------------
// k_fwd_remove's rounds over the clip's planes: the part right of the seam moves one place left in the costs (Q with them) and the
// position plane; a round reads, waits for the workgroup, and writes.  The level goes to where the seam's pixel stood at the start.
__global__ __launch_bounds__(FWD_REMOVE_THREADS) void k_clip_remove(float *cost_all, uint16_t *pos_all, const int32_t *seam, int32_t *map, int wc, int L, int H, int level,
                                                                     int orientation)
{
    const int y = blockIdx.x, tid = threadIdx.x;
    gf32x4 *cost = (gf32x4 *) cost_all + (size_t) y * L;
    gu16 *pos = (gu16 *) pos_all + (size_t) y * L;
    const int sx = min(max(((const gi32 *) seam)[y], 0), wc - 1);
    const int orig = pos[sx];                                          // (read by every thread before the first round's barrier)
    for (int base = sx; base < wc - 1; base += FWD_REMOVE_THREADS * FWD_REMOVE_PX) {
        f32x4 vc[FWD_REMOVE_PX];
        uint16_t vo[FWD_REMOVE_PX];
#pragma unroll
        for (int k = 0; k < FWD_REMOVE_PX; k++) {
            const int x = base + tid + k * FWD_REMOVE_THREADS;
            vc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; vo[k] = 0;
            if (x < wc - 1) { vc[k] = cost[x + 1]; vo[k] = pos[x + 1]; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FWD_REMOVE_PX; k++) {
            const int x = base + tid + k * FWD_REMOVE_THREADS;
            if (x < wc - 1) { cost[x] = vc[k]; pos[x] = vo[k]; }
        }
    }
    if (tid == 0) ((gi32 *) map)[orientation ? (size_t) orig * H + y : (size_t) y * L + orig] = level;
}

// ---------------------------------------------------------------------------
// the refresh: the two columns of a line whose neighbours changed, from the n frames
// ---------------------------------------------------------------------------
// After the removal the frames are wn = wc - 1 wide and the seam stood at column s of this line: the new columns s - 1 and s (those of
// them that exist) have a new l, r or u.  The six original positions involved are the same for every frame; thread tid folds the frames
// tid + k * CLIPFWD_REFRESH_THREADS, a wave folds its threads by shuffles, the waves meet in LDS.  Costs are >= 0: a thread without a
// frame, and a column that does not exist, hold 0.  Q stays as it is.
__global__ __launch_bounds__(CLIPFWD_REFRESH_THREADS) void k_clip_refresh(const float *in_all, int n, float *cost_all, const uint16_t *pos_all, const int32_t *seam, int wn,
                                                                         int L, int H)
{
    __shared__ float s_red[CLIPFWD_REFRESH_THREADS / 64 * CLIP_REFRESH_VALUES];
    static_assert(sizeof s_red == clip_refresh_lds_elems(CLIPFWD_REFRESH_THREADS) * sizeof(float), "as lqr_geom.h states it");
    const int y = blockIdx.x, tid = threadIdx.x;
    const size_t px = (size_t) L * H, line = (size_t) y * L;
    const gu16 *pos = (const gu16 *) pos_all + line;
    const int s = min(max(((const gi32 *) seam)[y], 0), wn);           // (a column of the frame before the removal: 0 .. wn)
    float m[CLIP_REFRESH_VALUES];
    size_t il[2], ir[2], iu[2];
    bool valid[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int x = s - 1 + c;
        valid[c] = x >= 0 && x < wn;
        const int xc = min(max(x, 0), wn - 1);
        il[c] = line + pos[max(xc - 1, 0)];
        ir[c] = line + pos[min(xc + 1, wn - 1)];
        iu[c] = y > 0 ? line - L + (pos - L)[xc] : line;
        m[3 * c] = m[3 * c + 1] = m[3 * c + 2] = 0.0f;
    }
    for (int t = tid; t < n; t += CLIPFWD_REFRESH_THREADS) {
        const gf32 *in = (const gf32 *) in_all + clip_frame_off(t, px);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (!valid[c]) continue;
            const float l = in[il[c]], r = in[ir[c]];
            const float a = fabsf(__fsub_rn(r, l));
            m[3 * c] = fmaxf(m[3 * c], a);
            if (y > 0) {
                const float u = in[iu[c]];
                m[3 * c + 1] = fmaxf(m[3 * c + 1], __fadd_rn(a, fabsf(__fsub_rn(u, l))));
                m[3 * c + 2] = fmaxf(m[3 * c + 2], __fadd_rn(a, fabsf(__fsub_rn(u, r))));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < CLIP_REFRESH_VALUES; i++)
        for (int o = 32; o > 0; o >>= 1) m[i] = fmaxf(m[i], __shfl_down(m[i], o));
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < CLIP_REFRESH_VALUES; i++) s_red[clip_refresh_off(tid >> 6) + i] = m[i];
    }
    __syncthreads();
    if (tid < CLIP_REFRESH_VALUES) {
        const int c = tid / 3, x = s - 1 + c;
        if (x >= 0 && x < wn) {
            float v = s_red[tid];
            for (int w = 1; w < CLIPFWD_REFRESH_THREADS / 64; w++) v = fmaxf(v, s_red[clip_refresh_off(w) + tid]);
            ((gf32 *) cost_all)[clip_cost_off(y, x, L) + tid % 3] = v;
        }
    }
}

#define INSTANTIATE(P) template __global__ void k_clip_seam<P>(const float *, int8_t *, int32_t *, int, int, int);
K_CLIP_SEAM_FORMS(INSTANTIATE)
#undef INSTANTIATE
