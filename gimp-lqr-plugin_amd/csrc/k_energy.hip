// k_energy.hip -- E1 working planes, E2 masks, E3/E4 energy map, E6 energy update next to the seam, frozen-plane catch-up
// (gfx950 / CDNA4, wave64; see lqr_common.h for the file map and DESIGN.md section 4 for the measurements)
#include "lqr_common.h"
#include "lqr_kernels.h"

// ---------------------------------------------------------------------------
// one-off kernels: working-plane init, full energy map, masks
// ---------------------------------------------------------------------------
// FORM (lqr_pixel.h): PixPacked -- the pixel's bytes in a u32 -- or PixValue<DEPTH> -- the value the energy reads, a double
template <class FORM>
__global__ void k_wk_init(const DevCarver *cs, int w, int h, int stride, typename FORM::Arg a)
{
    const GCarver c = gview_phys(cs[blockIdx.z]);
    GLOBAL_AS typename FORM::T *pix = (GLOBAL_AS typename FORM::T *) c.pix;
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x == 0 && y == 0) { c.flags[FLAG_ORG] = 0; c.flags[FLAG_ORG_PREV] = 0; c.flags[FLAG_SIDE] = 0; }      // planes laid out afresh
    if (x >= stride) return;
    size_t o = (size_t) y * stride + x;
    typename FORM::T p = 0;
    float b = 0.0f, r = 0.0f;
    if (x < w) {
        if constexpr (std::is_same<FORM, PixPacked>::value) {      // PixPacked::form, spelt out: inlined from the call, the 8-bit form of this
            const gu8 *s = c.rgb0 + ((size_t) y * w + x) * a;       // kernel (not of k_wk_init_visible) gets its byte loop scheduled differently
            if (a == 4) p = *(const gu32 *) s;
            else for (int k = 0; k < a; k++) p |= (uint32_t) s[k] << (8 * k);
        } else p = FORM::form(c.rgb0, (size_t) y * w + x, a);
        if (c.bias0) b = c.bias0[(size_t) y * w + x];
        if (c.rig0) r = c.rig0[(size_t) y * w + x];
    }
    pix[o] = p;
    if (c.bias) c.bias[o] = b;
    if (c.rig) c.rig[o] = r;
}

// The same from a carver that is NOT flat (round 6: a session redone after a fault, or working planes lost on a multi-size
// image): the carved frame is the pixels of the base layout that have no level yet (vs == 0), in order -- what k_vs_commit
// ranks.  One block per row, ballot-rank compaction; the tail of the row is zero-filled as k_wk_init does.
template <class FORM>
__global__ __launch_bounds__(256) void k_wk_init_visible(const DevCarver *cs, int w0, int h, int stride, typename FORM::Arg a)
{
    __shared__ int s_wave[4];
    const GCarver c = gview_phys(cs[blockIdx.y]);
    GLOBAL_AS typename FORM::T *pix = (GLOBAL_AS typename FORM::T *) c.pix;
    const int y = blockIdx.x, tid = threadIdx.x;
    if (y == 0 && tid == 0) { c.flags[FLAG_ORG] = 0; c.flags[FLAG_ORG_PREV] = 0; c.flags[FLAG_SIDE] = 0; }
    const size_t ri = (size_t) y * w0, ro = (size_t) y * stride;
    int carry = 0;
    for (int base = 0; base < w0; base += 256) {
        const int col = base + tid;
        const bool keep = (col < w0) && c.vs[ri + col] == 0;
        int total;
        const int rank = carry + block_rank_256(keep, s_wave, total);
        if (keep && rank < stride) {
            pix[ro + rank] = FORM::form(c.rgb0, ri + col, a);
            if (c.bias) c.bias[ro + rank] = c.bias0 ? c.bias0[ri + col] : 0.0f;
            if (c.rig) c.rig[ro + rank] = c.rig0 ? c.rig0[ri + col] : 0.0f;
        }
        carry += total;
    }
    for (int x = carry + tid; x < stride; x += 256) {
        pix[ro + x] = 0;
        if (c.bias) c.bias[ro + x] = 0.0f;
        if (c.rig) c.rig[ro + x] = 0.0f;
    }
}

// E3/E4.  VALUE (lqr_pixel.h, PixRead): the working plane holds the value the energy reads, not packed pixels
template <int NRG, bool VALUE>
__global__ void k_emap_full(const DevCarver *cs, DpK p, int w, int h, int stride)
{
    PixRead<VALUE> rd;
    rd.setup(threadIdx.x, blockDim.x);
    const GCarver c = gview(cs[blockIdx.z]);
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    float e = grad_energy_f<NRG>([&](int xx, int yy) { return rd(c.pix, (size_t) yy * stride + xx, p.ch, NRG >= 3); }, x, y, w, h);
    if (c.bias) e = __fadd_rn(e, __fdiv_rn(c.bias[(size_t) y * stride + x], (float) p.w_start));
    c.en[(size_t) y * stride + x] = e;
}

// E1 + E3/E4 in one pass, for the start of a session on a FLAT carver of packed pixels (lqrhip_wk_init_emap): k_wk_init<PixPacked>
// and k_emap_full<NRG, false> back to back wrote the packed plane and read it straight back (4 bytes per pixel each way), and
// k_emap_full formed the brightness of every pixel once per neighbour that asks for it (2 to 4 times).  Here a thread lays out 4
// columns of row y and computes their energies from the base layout's pixels, which are the packed plane's values: px_bright on
// the same u32 through the same table, grad_energy_f on the same samples -- the energies are k_emap_full's bit for bit.  The
// brightnesses a thread needs (row y: its 4 columns and one either side; rows y - 1, y + 1: its 4 columns, not for the XABS
// energies) are formed once each and held in registers; the sample reader handed to grad_energy_f picks among them by
// compile-time-unrolled selects, not by indexing (no scratch).
// The planes are laid out afresh: the origin is 0, the view the physical one.
template <int NRG>
__global__ __launch_bounds__(256) void k_wk_init_emap(const DevCarver *cs, DpK p, int w, int h, int stride)
{
    PixRead<false> rd;
    rd.setup(threadIdx.x, 256);                     // (a barrier inside: before any thread leaves)
    const GCarver c = gview_phys(cs[blockIdx.z]);
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, ch = p.ch;
    if (x == 0 && y == 0) { c.flags[FLAG_ORG] = 0; c.flags[FLAG_ORG_PREV] = 0; c.flags[FLAG_SIDE] = 0; }
    if (x >= stride) return;
    constexpr bool luma = (NRG >= 3), rows3 = (NRG % 3 != 2) && NRG != 6;
    const size_t o = (size_t) y * stride + x, i0 = (size_t) y * w + x;
    // whole 16-byte vectors where RGBA rows start on 16-byte boundaries in the base layout (width a multiple of 4) and in the working
    // planes (the stride is a multiple of 64): a vector is then wholly inside the row or wholly past it; else column by column
    const bool vst = (stride & 3) == 0 && (((size_t) c.pix | (size_t) c.en) & 15) == 0;        // 16-byte stores of the working planes
    const bool vec = ch == 4 && (w & 3) == 0 && ((size_t) c.rgb0 & 15) == 0;                   // 16-byte loads of the base layout
    auto load4 = [&](int yy, uint32_t *q) {         // pixels x .. x + 3 of row yy (0 past the frame)
        if (vec) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (x < w) v = *(const GLOBAL_AS u32x4 *) (c.rgb0 + ((size_t) yy * w + x) * 4);
            q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = x + k < w ? PixPacked::form(c.rgb0, (size_t) yy * w + x + k, ch) : 0u;
        }
    };
    uint32_t own[4];
    load4(y, own);
    float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vst) *(GLOBAL_AS u32x4 *) (c.pix + o) = u32x4{own[0], own[1], own[2], own[3]};     // (columns past the frame: 0, as k_wk_init leaves them)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x + k >= stride) break;
        if (!vst) c.pix[o + k] = own[k];
        if (c.bias0 && x + k < w) bv[k] = c.bias0[i0 + k];
        if (c.bias) c.bias[o + k] = bv[k];
        if (c.rig) c.rig[o + k] = (c.rig0 && x + k < w) ? c.rig0[i0 + k] : 0.0f;
    }
    if (x >= w) return;                             // the energies: inside the frame only, as k_emap_full
    auto bright = [&](uint32_t q) { return px_bright(q, ch, luma, Norm255Lut{rd.n255}); };
    double bm[6], bu[4] = {0.0, 0.0, 0.0, 0.0}, bd[4] = {0.0, 0.0, 0.0, 0.0};      // row y: columns x - 1 .. x + 4; rows y - 1, y + 1: x .. x + 3
    bm[0] = (NRG != 6 && x > 0) ? bright(PixPacked::form(c.rgb0, i0 - 1, ch)) : 0.0;
    bm[5] = (NRG != 6 && x + 4 < w) ? bright(PixPacked::form(c.rgb0, i0 + 4, ch)) : 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) bm[k + 1] = NRG != 6 ? bright(own[k]) : 0.0;
    if (rows3) {
        uint32_t q[4];
        if (y > 0) {
            load4(y - 1, q);
#pragma unroll
            for (int k = 0; k < 4; k++) bu[k] = bright(q[k]);
        }
        if (y < h - 1) {
            load4(y + 1, q);
#pragma unroll
            for (int k = 0; k < 4; k++) bd[k] = bright(q[k]);
        }
    }
    const bool ven = vst && x + 3 < w;             // the energies of a quad that ends past the frame go one by one: nothing is written past it
    float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x + k >= w) break;
        e[k] = grad_energy_f<NRG>([&](int xx, int yy) {
            const int dx = xx - x, dy = yy - y;
            double r = 0.0;
            if (dy == 0) {
#pragma unroll
                for (int j = 0; j < 6; j++) r = (dx + 1 == j) ? bm[j] : r;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) r = (dx == j) ? (dy < 0 ? bu[j] : bd[j]) : r;
            }
            return r;
        }, x + k, y, w, h);
        if (c.bias) e[k] = __fadd_rn(e[k], __fdiv_rn(bv[k], (float) p.w_start));
        if (!ven) c.en[o + k] = e[k];
    }
    if (ven) *(GLOBAL_AS f32x4 *) (c.en + o) = f32x4{e[0], e[1], e[2], e[3]};
}

// E2: mask value = mean(colour)/255 * alpha/255 (help/en/index.wiki:48)
__global__ void k_mask_add(float *plane, int w0, const uint8_t *mask, int channels, int mw, int x0, int y0, int x1, int y1,
                           int nx, int ny, int transposed, int is_rig, int bias_factor)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= nx || y >= ny) return;
    const uint8_t *px = mask + ((size_t) (y - y0) * mw + (x - x0)) * channels;
    const bool has_alpha = (channels == 2 || channels >= 4);
    const int cc = channels - (has_alpha ? 1 : 0);
    int sum = 0;
    for (int k = 0; k < cc; k++) sum += px[k];
    int xc = transposed ? y + y1 : x + x1;
    int yc = transposed ? x + x1 : y + y1;
    size_t o = (size_t) yc * w0 + xc;
    if (is_rig) {
        double v = __ddiv_rn((double) sum, (double) (255 * cc));
        if (has_alpha) v = __dmul_rn(v, __ddiv_rn((double) px[channels - 1], 255.0));
        plane[o] = __double2float_rn(v);
    } else {
        double b = __ddiv_rn(__dmul_rn((double) bias_factor, (double) sum), (double) (2 * 255 * cc));
        if (has_alpha) b = __dmul_rn(b, __ddiv_rn((double) px[channels - 1], 255.0));
        plane[o] = __fadd_rn(plane[o], __double2float_rn(b));
    }
}

// E6 update_emap: recompute en next to the carved seam (w = new width); runs after the carve.
// The packed-pixel (and bias) planes are frozen in the frame they had at seam `epoch`
// of the session; current coordinates are mapped back by undoing seams k..epoch of the
// row (p += (log[j] <= p)), which costs O(k - epoch) per pixel for ~10 pixels per row and
// saves moving 4 (8 with bias) of the 13 bytes per pixel that a carve would otherwise move.
// Brightness samples staged per row: row y is asked for columns [min - 2, max + 1] of the seam over rows
// y-1..y+1 by its own gradient and [min - 1, max] of the seam over rows y-2..y+2 by its neighbours', and the
// seam moves at most delta_x per row: at most max(4*delta_x + 2, 2*delta_x + 4) columns.  EU_NT is a template
// parameter chosen by the launch from delta_x: 12 (delta_x <= 2), 36 (<= 8), 68 (<= 16 = LQRHIP_MAX_DELTA).
// VALUE: the frozen plane holds the value the energy reads (PixRead: no table of v / 255 then, and the sample is the element).
template <int NRG, int EU_NT, bool VALUE>
__global__ __launch_bounds__(64) void k_emap_update(const DevCarver *cs, DpK p, int w, int h, int stride, int k, int epoch)
{
    const GCarver c = gview(cs[blockIdx.y]);
    PixRead<VALUE> rd;
    rd.setup(threadIdx.x, 64);
    emap_update_block<NRG, EU_NT, VALUE, false>(c, rd, p, w, h, stride, k, epoch, blockIdx.x, threadIdx.x);      // (lqr_pixel.h: shared with k_carve_u)
}

// bring the frozen planes (pix, bias) forward: remove seams [from, to) of the session log from
// every row; w_from = width of the frame the planes are in.  One block per row, in place.  VALUE: 8-byte values instead of packed pixels
template <bool VALUE>
__global__ __launch_bounds__(256) void k_frozen_catchup(const DevCarver *cs, int from, int to, int w_from, int h, int stride)
{
    const GCarver c = gview(cs[blockIdx.y]);
    extern __shared__ int smc[];
    int *xs = smc;                                  // [to - from]
    uint8_t *rem = (uint8_t *) (smc + fc_rem_off(from, to));  // [w_from]
    __shared__ int s_wave[4];
    const int y = blockIdx.x, tid = threadIdx.x, n = to - from;
    for (int i = tid; i < n; i += 256) xs[i] = c.seam_log[(size_t) (from + i) * h + y];
    for (int i = tid; i < w_from; i += 256) rem[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        int pz = xs[i];
        for (int j = i - 1; j >= 0; j--) if (xs[j] <= pz) pz++;
        rem[pz] = 1;
    }
    __syncthreads();
    typedef typename PixRead<VALUE>::T T;
    GLOBAL_AS T *prow = (GLOBAL_AS T *) c.pix + (size_t) y * stride;
    gf32 *brow = c.bias ? c.bias + (size_t) y * stride : (gf32 *) nullptr;
    int carry = 0;
    for (int base = 0; base < w_from; base += 256) {
        const int col = base + tid;
        const bool keep = (col < w_from) && !rem[col];
        const T v = (col < w_from) ? prow[col] : 0;
        const float bv = (brow && col < w_from) ? brow[col] : 0.0f;
        int total;
        const int rank = carry + block_rank_256(keep, s_wave, total);     // barriers inside: all reads of the chunk are done
        if (keep) { prow[rank] = v; if (brow) brow[rank] = bv; }
        carry += total;
    }
}


// ---- the instantiations the shim launches (lqr_kernels.h lists them).  The value forms exist for energies 0, 1, 2 and 6 only:
// the plane already holds brightness or luma, so 3, 4, 5 would be the code of 0, 1, 2 again (plane_nrg in lqr_shim.hip)
#define INST_WK(FORM) template __global__ void k_wk_init<FORM>(const DevCarver *, int, int, int, FORM::Arg); \
    template __global__ void k_wk_init_visible<FORM>(const DevCarver *, int, int, int, FORM::Arg);
INST_WK(PixPacked) INST_WK(PixValue<0>) INST_WK(PixValue<1>) INST_WK(PixValue<2>) INST_WK(PixValue<3>)
#define INST_U(NT, N, V) template __global__ void k_emap_update<N, NT, V>(const DevCarver *, DpK, int, int, int, int, int);
#define INST(N, V) template __global__ void k_emap_full<N, V>(const DevCarver *, DpK, int, int, int); K_EMAP_UPDATE_NT_FORMS(INST_U, N, V)
K_EMAP_FORMS(INST)
#undef INST
#undef INST_U
#define INST_WE(N) template __global__ void k_wk_init_emap<N>(const DevCarver *, DpK, int, int, int);
K_WK_INIT_EMAP_FORMS(INST_WE)
#undef INST_WE
template __global__ void k_frozen_catchup<false>(const DevCarver *, int, int, int, int, int);
template __global__ void k_frozen_catchup<true>(const DevCarver *, int, int, int, int, int);
