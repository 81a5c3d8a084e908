// k_static.hip -- static seams for a clip (include_ext/lqr_static.h): the frames of a clip folded into ONE energy plane,
// on which an LQR_EF_NULL carver then finds the seams that every frame is carved by (Rubinstein, Shamir, Avidan 2008, section 3).
//
// The rule (tests/static_cases.py is the specification, bit for bit).  For frame t, in IMAGE orientation,
//     S_t(x, y) = what lqr_carver_get_true_energy(frame t, ., orientation) gives: grad_energy_f on the doubles the energy reads, the
//                 frame of the carving direction deciding which gradient is "x", plus bias / L as the seam loop adds it
//     I_t(x, y) = the float of that double
//     S = max_t S_t      T = max_{t >= 1} |I_t - I_{t-1}|  (float)      E = fl(fl(alpha S) + fl(fl(1 - alpha) T))
//
// k_static_fold: one launch folds a group of up to STATIC_GROUP frames into the running S, T and I_prev planes.  A workgroup owns a
// tile of STATIC_TILE x STATIC_TILE image pixels and walks the group's frames: for each it reads the base-layout pixels of the tile and
// a one-pixel halo ONCE, forms the value the energy reads (px_bright / deep_value, lqr_pixel.h) and keeps it, as a double, in LDS;
// every thread then evaluates its 8 pixels from LDS and keeps the running maxima in registers.  S, T and I_prev are read and written
// once per launch; the last group writes E instead (the mix is its epilogue: there is no launch for it).  A frame that lies the other
// way than the image (a transposed carver) is read along ITS rows and stored across the LDS tile, whose rows are padded to an odd number
// of doubles: no strided gather, and the frame is not transposed.  No scratch, no spin waits, no hand-overs between workgroups.
#include "lqr_common.h"
#include "lqr_kernels.h"

#define ST_SIDE (STATIC_TILE + 2)           // the tile and its halo
#define ST_WAVES (STATIC_THREADS / 64)
#define ST_ROWS (STATIC_TILE / ST_WAVES)           // image rows of the tile per thread: a wave takes rows wv, wv + ST_WAVES, ...
#define ST_LOAD_ROUNDS ((ST_SIDE * ST_SIDE + STATIC_THREADS - 1) / STATIC_THREADS)     // rounds in which the workgroup loads the tile and its halo
#define ST_LOAD_UNROLL 3

// NRG: 0, 1, 2 (norm, sum of absolute values, |x gradient|; brightness or luma by rd.luma) or 6 (LQR_EF_NULL).  DEPTH: LqrColDepth.
// PACKED: 8-bit grey / RGB (+ alpha) pixels, formed by px_bright through the table of v / 255 (DEPTH 0 only).
// frames: the group's first entry; first: its index in the clip (0: there are no running planes yet); e_out non-null: the last group.
template <int NRG, int DEPTH, bool PACKED>
__global__ __launch_bounds__(STATIC_THREADS) void k_static_fold(const StaticFrame *frames, int count, int first, int W, int H, int transposed,
                                                     int orientation, DeepRead rd, float alpha, float *s_plane, float *t_plane,
                                                     float *i_plane, float *e_out)
{
    __shared__ double s_i[ST_SIDE][ST_SIDE + 1];            // rows of 67 doubles: a column-wise store is conflict-free
    __shared__ float s_b[STATIC_TILE][STATIC_TILE + 1];
    __shared__ double s_n255[PACKED ? 256 : 1];
    constexpr int bpc = DEPTH == 0 ? 1 : DEPTH == 1 ? 2 : DEPTH == 2 ? 4 : 8;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int X0 = blockIdx.x * STATIC_TILE, Y0 = blockIdx.y * STATIC_TILE;
    const int fw0 = transposed ? H : W;                     // pixels per row of the base layout
    const int L = orientation ? H : W, lines = orientation ? W : H;
    const int X = X0 + lane;
    if (PACKED) fill_norm255(s_n255, tid, STATIC_THREADS);             // (the barrier at the top of the frame loop covers it)

    // (Every thread evaluates ST_ROWS pixels, those past the image's edge the edge pixel again: the running values are updated without a
    // branch around them, or the compiler copies the three arrays as whole register tuples on every path and spills.)
    const int Xc = min(X, W - 1);
    float s[ST_ROWS], t[ST_ROWS], ip[ST_ROWS];
#pragma unroll
    for (int k = 0; k < ST_ROWS; k++) s[k] = t[k] = ip[k] = 0.0f;
    if (first > 0) {
#pragma unroll
        for (int k = 0; k < ST_ROWS; k++) {
            const size_t o = (size_t) min(Y0 + wv + ST_WAVES * k, H - 1) * W + Xc;
            s[k] = ((const gf32 *) s_plane)[o];
            t[k] = ((const gf32 *) t_plane)[o];
            ip[k] = ((const gf32 *) i_plane)[o];
        }
    }

    for (int f = 0; f < count; f++) {
        const gu8 *rgb0 = (const gu8 *) frames[f].rgb0;
        const gf32 *bias0 = (const gf32 *) frames[f].bias0;
        __syncthreads();                                    // the tile of frame f - 1 has been read (f = 0: the table is filled)
        // Branch-free up to the stores, so that the loads of ST_LOAD_UNROLL elements are in flight together: an element outside the image
        // reads the nearest pixel inside and keeps 0; the rounds past the last element repeat it (the same value to the same place).
#pragma unroll ST_LOAD_UNROLL
        for (int it = 0; it < ST_LOAD_ROUNDS; it++) {
            const int e = min(tid + it * STATIC_THREADS, ST_SIDE * ST_SIDE - 1);
            const int a = e / ST_SIDE, b = e - a * ST_SIDE; // b runs with the lanes: along the base layout's rows
            const int rx = transposed ? a : b, ry = transposed ? b : a;
            const int px = X0 - 1 + rx, py = Y0 - 1 + ry;
            const bool inside = px >= 0 && px < W && py >= 0 && py < H;
            const int cx = min(max(px, 0), W - 1), cy = min(max(py, 0), H - 1);
            const size_t i = transposed ? (size_t) cx * fw0 + cy : (size_t) cy * fw0 + cx;
            double v;
            if (PACKED) v = px_bright(PixPacked::form(rgb0, i, rd.ch), rd.ch, rd.luma != 0, Norm255Lut{s_n255});
            else v = deep_value<DEPTH>(rgb0 + i * rd.ch * bpc, rd);
            const float bv = bias0 ? bias0[i] : 0.0f;
            s_i[ry][rx] = inside ? v : 0.0;
            if (inside && rx >= 1 && rx <= STATIC_TILE && ry >= 1 && ry <= STATIC_TILE) s_b[ry - 1][rx - 1] = bv;
        }
        __syncthreads();
        const bool fresh = first + f == 0;
#pragma unroll
        for (int k = 0; k < ST_ROWS; k++) {
            const int Yc = min(Y0 + wv + ST_WAVES * k, H - 1), r = Yc - Y0, c = Xc - X0;
            // the frame of the carving direction: x along a line of L, y across the lines
            const int x = orientation ? Yc : Xc, y = orientation ? Xc : Yc;
            float en = grad_energy_f<NRG>([&](int xx, int yy) {
                const int ix = orientation ? yy : xx, iy = orientation ? xx : yy;
                return s_i[iy - Y0 + 1][ix - X0 + 1];
            }, x, y, L, lines);
            if (bias0) en = __fadd_rn(en, __fdiv_rn(s_b[r][c], (float) L));
            const float iv = __double2float_rn(s_i[r + 1][c + 1]);
            s[k] = fresh ? en : fmaxf(s[k], en);
            t[k] = fresh ? 0.0f : fmaxf(t[k], fabsf(__fsub_rn(iv, ip[k])));
            ip[k] = iv;
        }
    }

#pragma unroll
    for (int k = 0; k < ST_ROWS; k++) {
        const int Y = Y0 + wv + ST_WAVES * k;
        if (X >= W || Y >= H) continue;
        const size_t o = (size_t) Y * W + X;
        if (e_out) {        // the mix
            ((gf32 *) e_out)[o] = __fadd_rn(__fmul_rn(alpha, s[k]), __fmul_rn(__fsub_rn(1.0f, alpha), t[k]));
        } else {
            ((gf32 *) s_plane)[o] = s[k];
            ((gf32 *) t_plane)[o] = t[k];
            ((gf32 *) i_plane)[o] = ip[k];
        }
    }
}

#define INST(N, D, P) template __global__ void k_static_fold<N, D, P>(const StaticFrame *, int, int, int, int, int, int, DeepRead, float, float *, float *, float *, float *);
K_STATIC_FOLD_FORMS(INST)
#undef INST
