// k_carve.hip -- E8 carve: the seam leaves every carved plane, in place; the HBM-bound kernel
// (gfx950 / CDNA4, wave64; see lqr_common.h for the file map and DESIGN.md section 4 for the measurements)
#include "lqr_common.h"
#include "lqr_kernels.h"
#include "lqr_walk.h"

// ---------------------------------------------------------------------------
// E8 carve: remove the seam from every carved plane (en, m, back pointers, rigidity mask), in place, one
// wave per row, 16 B per lane.  The dominant HBM kernel.  Only the SHORTER side of the seam moves
// (DESIGN.md 4.9): k_vpath* compared sum(x) with sum(w - 1 - x) over the seam's rows and published
//   side 0: the part right of the seam moves one to the left, the origin stays;
//   side 1: the part left of it moves one to the right and the image's origin advances by one.
// The side is uniform over an image's rows, so rows stay mutually aligned and every other kernel just sees
// the planes through pointers advanced by the origin.  Seams are delta_x-connected, so a seam's rows differ
// little in x and the per-image choice loses almost nothing against a per-row one; for seams spread over
// the width the mean moved fraction of a row is 1/4 instead of 1/2.
// This kernel works on PHYSICAL positions p = origin + x (rows start 16-byte aligned at p = 0), with aligned
// vector accesses; the element that enters a lane's four from the neighbouring lane comes by DPP.
// The back-pointer plane is re-based on the fly: a stored dx stays valid unless pixel and parent are on
// different sides of the seam (then it changes by one, or becomes LEAST_INVALID if the parent was carved).
// ---------------------------------------------------------------------------

// A group = CG chunks of 256 elements of one plane, as loaded, plus the one element beyond the group that
// its edge lane needs.  All planes of a row are LOADED for a group before any of them is stored: a row wave then has
// three planes' loads in flight at once instead of three load -> store round trips one after the other (non-temporal:
// streaming the rows past L2 is worth 6 % of the kernel).  The element that follows (side 0) / precedes (side 1) a
// lane's four is the neighbouring lane's (DPP); only the edge lane of the group fetches it from memory.
// Chunks per group.  Measured at 64 x 4K (one box, us per launch): planes one after the other at 8 waves per SIMD 510-518;
// all planes of a group loaded first with CG = 1 (77 VGPRs, 6 waves) 495, 2 (100, 4) 486, 3 (120, 4) 509, 4 (142 VGPRs,
// 3 waves per SIMD) 470-485, 6 552; CG = 4 squeezed into 128 VGPRs (11 spilled) 531.  Bytes in flight per wave beat
// occupancy: a row's mean moved part (a quarter of 3840) fits one group of 1024.
#ifndef CG
#define CG 4
#endif
#define CGPX (CG * 256)
struct G32 { u32x4 a[CG]; uint32_t edge; };     // 4-byte planes: en, m, rigidity mask
struct G8 { uint32_t a[CG]; uint32_t edge; };   // the back-pointer bytes, 4 px per dword

// ---- side 0: new[p] = old[p + 1] for p in [pv, pend); pend = physical end (exclusive) of the row after the carve.
// Groups run left to right from `base`, which lies at or below `lo`, the first position of the job: a lane whose four elements
// end below lo takes no part (none does while base is lo rounded down to a vector; with base rounded down to a line, up to 7).
// LINE false: base is lo rounded down to a vector, nothing to test (k_carve, whose instructions tests/test_carve_beside_meta.py pins).
template <bool LINE>
__device__ __forceinline__ void ld_left_u32(const gu32 *row, int base, int lo, int pend, int lane, G32 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = base + u * 256 + lane * 4;
        // x <= pend: the chunk that starts at pend holds the old last element, which the lane before needs
        g.a[u] = ((!LINE || x + 3 >= lo) && x <= pend) ? __builtin_nontemporal_load((const GLOBAL_AS u32x4 *) (row + x)) : (u32x4) {0u, 0u, 0u, 0u};
    }
    g.edge = (lane == 63 && base + CGPX <= pend) ? row[base + CGPX] : 0u;
}
template <bool LINE>
__device__ __forceinline__ void st_left_u32(gu32 *row, int base, int lo, int pv, int pend, int lane, const G32 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = base + u * 256 + lane * 4;
        const uint32_t first_next = (u < CG - 1) ? (uint32_t) __builtin_amdgcn_readlane((int) g.a[u < CG - 1 ? u + 1 : CG - 1].x, 0) : 0u;
        const uint32_t lane63 = (u < CG - 1) ? first_next : g.edge;
        const uint32_t nx = (uint32_t) __builtin_amdgcn_update_dpp((int) lane63, (int) g.a[u].x, DPP_WAVE_SHL1, 0xf, 0xf, false);
        if ((!LINE || x + 3 >= lo) && x < pend) {
            u32x4 o;
            o.x = (x >= pv) ? g.a[u].y : g.a[u].x;
            o.y = (x + 1 >= pv) ? g.a[u].z : g.a[u].y;
            o.z = (x + 2 >= pv) ? g.a[u].w : g.a[u].z;
            o.w = (x + 3 >= pv) ? nx : g.a[u].w;
            __builtin_nontemporal_store(o, (GLOBAL_AS u32x4 *) (row + x));
        }
    }
}

// ---- side 1: new[p] = old[p - 1] for p in (pbeg, pv]; pbeg = the origin before the carve (dead afterwards).
// Groups [gbase, gbase + CGPX) run from the seam towards the origin: a group's stores reach one element past its loads
// on the right, into a group that has been read already.
__device__ __forceinline__ void ld_right_u32(const gu32 *row, int gbase, int pbeg, int pv, int lane, G32 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = gbase + u * 256 + lane * 4;
        // chunks that hold a source (p in [pbeg, pv - 1]) or a destination; x + 3 >= pbeg >= 0 keeps x >= 0
        g.a[u] = (x + 3 >= pbeg && x <= pv) ? __builtin_nontemporal_load((const GLOBAL_AS u32x4 *) (row + x)) : (u32x4) {0u, 0u, 0u, 0u};
    }
    g.edge = (lane == 0 && gbase - 1 >= pbeg) ? row[gbase - 1] : 0u;
}
__device__ __forceinline__ void st_right_u32(gu32 *row, int gbase, int pbeg, int pv, int lane, const G32 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = gbase + u * 256 + lane * 4;
        const uint32_t last_prev = (u > 0) ? (uint32_t) __builtin_amdgcn_readlane((int) g.a[u > 0 ? u - 1 : 0].w, 63) : 0u;
        const uint32_t lane0 = (u > 0) ? last_prev : g.edge;
        const uint32_t pw = (uint32_t) __builtin_amdgcn_update_dpp((int) lane0, (int) g.a[u].w, DPP_WAVE_SHR1, 0xf, 0xf, false);
        if (x <= pv && x + 3 > pbeg) {
            u32x4 o;
            o.x = (x > pbeg && x <= pv) ? pw : g.a[u].x;
            o.y = (x + 1 > pbeg && x + 1 <= pv) ? g.a[u].x : g.a[u].y;
            o.z = (x + 2 > pbeg && x + 2 <= pv) ? g.a[u].y : g.a[u].z;
            o.w = (x + 3 > pbeg && x + 3 <= pv) ? g.a[u].z : g.a[u].w;
            __builtin_nontemporal_store(o, (GLOBAL_AS u32x4 *) (row + x));
        }
    }
}

// ---- the en plane while the energy update runs BESIDE the carve (k_carve_u).  Other workgroups of the same launch write the fresh
// energies of this row to the physical positions [pa, pb] (nrg_interval in the frame after the carve, which starts at org + side;
// pa > pb: nothing).  The carve leaves them alone.  A 16-byte vector that lies wholly outside the interval and is wholly the carve's is
// stored as above (`whole` vectors: x in [x0, x1)).  Of the other vectors the carve stores only the elements that are its own AND outside
// the interval, one dword at a time (en_fix_*: at most 3 per end of the whole vectors, one lane each, loaded before the row's first
// store and stored after its last) and nothing else -- in particular not the "as loaded" elements of the boundary vector, which may
// hold an energy that is stale by now.  The vector LOADS still cover the interval, and what they return from there is the old energy
// or the fresh one; no output outside the interval is made from such an element.  With xmin <= v (nrg_interval starts from the row's
// own seam pixel) and, unless the interval is empty, xmax >= v - 1:
//   side 0: pa = org + xmin <= pv, so an output p >= pv outside the interval has p > pb and takes old[p + 1] >= pb + 2;
//   side 1: pb = org + 1 + xmax >= pv, so an output p = org + 1 + xx outside it has xx < xmin and takes old[org + xx] < pa - 1.
// Positions left of the seam on side 0 and right of it on side 1 are not written at all.
__device__ __forceinline__ void st_left_en(gu32 *row, int base, int x0, int pend, int lane, const G32 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = base + u * 256 + lane * 4;
        const uint32_t first_next = (u < CG - 1) ? (uint32_t) __builtin_amdgcn_readlane((int) g.a[u < CG - 1 ? u + 1 : CG - 1].x, 0) : 0u;
        const uint32_t lane63 = (u < CG - 1) ? first_next : g.edge;
        const uint32_t nx = (uint32_t) __builtin_amdgcn_update_dpp((int) lane63, (int) g.a[u].x, DPP_WAVE_SHL1, 0xf, 0xf, false);
        if (x >= x0 && x < pend) __builtin_nontemporal_store((u32x4) {g.a[u].y, g.a[u].z, g.a[u].w, nx}, (GLOBAL_AS u32x4 *) (row + x));
    }
}
__device__ __forceinline__ void st_right_en(gu32 *row, int gbase, int x0, int x1, int lane, const G32 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = gbase + u * 256 + lane * 4;
        const uint32_t last_prev = (u > 0) ? (uint32_t) __builtin_amdgcn_readlane((int) g.a[u > 0 ? u - 1 : 0].w, 63) : 0u;
        const uint32_t lane0 = (u > 0) ? last_prev : g.edge;
        const uint32_t pw = (uint32_t) __builtin_amdgcn_update_dpp((int) lane0, (int) g.a[u].w, DPP_WAVE_SHR1, 0xf, 0xf, false);
        if (x >= x0 && x < x1) __builtin_nontemporal_store((u32x4) {pw, g.a[u].x, g.a[u].y, g.a[u].z}, (GLOBAL_AS u32x4 *) (row + x));
    }
}
// side 0: the carve's outputs outside the interval are [qa, pend), qa = max(pb + 1, pv); whole vectors from x0 = qa rounded up to a
// vector; lanes 0 .. 2 take q = qa + lane < x0.  Returns the lane's position (-1: none), its value through `val`
__device__ __forceinline__ int en_fix_left(const gu32 *row, int pv, int pend, int pb, int lane, int &x0, uint32_t &val)
{
    const int qa = max(pb + 1, pv);
    x0 = (qa + 3) & ~3;
    const int q = qa + lane;
    const bool mine = q < x0 && q < pend;
    val = mine ? row[q + 1] : 0u;
    return mine ? q : -1;
}
// side 1: the carve's outputs outside the interval are (pbeg, lim], lim = min(pa - 1, pv); whole vectors [x0, x1) = the vectors
// inside; lanes 0 .. 2 take q = pbeg + 1 + lane below x0, lanes 4 .. 6 take q = max(x0, x1) + lane - 4 up to lim
__device__ __forceinline__ int en_fix_right(const gu32 *row, int pbeg, int pv, int pa, int lane, int &x0, int &x1, uint32_t &val)
{
    const int lim = min(pa - 1, pv);
    x0 = (pbeg + 4) & ~3;
    x1 = (lim + 1) & ~3;
    const int q = lane < 4 ? pbeg + 1 + lane : max(x0, x1) + lane - 4;
    const bool mine = q <= lim && (lane < 4 ? (lane < 3 && q < x0) : lane < 7);
    val = mine ? row[q - 1] : 0u;
    return mine ? q : -1;
}

// one back pointer of the carved frame: the pixel that lands on new frame column xx came from old column
// xo = xx + right with back pointer dx (parent at old column xo + dx on row y - 1, whose seam pixel was vprev)
__device__ __forceinline__ int rebase_dx(int dx, int xx, int xo, int vprev, int y)
{
    if (y > 0 && dx != LEAST_INVALID) {
        const int q = xo + dx;
        if (q == vprev) dx = LEAST_INVALID;            // parent was the carved pixel
        else dx = q - (q > vprev ? 1 : 0) - xx;
    }
    return dx;
}

// ---- back pointers, side 0.  New frame column xx sits at physical org + xx and takes old column xx + (xx >= v).
// Pixels left of the seam whose parent may lie right of the seam of the row above (xx >= start = min(v, vprev - delta))
// are re-based too; bytes outside [start, wnew) are written back as loaded.
template <bool LINE>
__device__ __forceinline__ void ld_left_8(const gu32 *row32, int base, int lo, int pend, int lane, G8 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = base + u * 256 + lane * 4;
        g.a[u] = ((!LINE || x + 3 >= lo) && x <= pend) ? __builtin_nontemporal_load(row32 + (x >> 2)) : 0u;
    }
    g.edge = (lane == 63 && base + CGPX <= pend) ? row32[(base + CGPX) >> 2] : 0u;
}
template <bool LINE>
__device__ __forceinline__ void st_left_8(gu32 *row32, int base, int org, int start, int v, int vprev, int y, int wnew, int lane, const G8 &g)
{
    const int pend = org + wnew;
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = base + u * 256 + lane * 4;
        const uint32_t first_next = (u < CG - 1) ? (uint32_t) __builtin_amdgcn_readlane((int) g.a[u < CG - 1 ? u + 1 : CG - 1], 0) : 0u;
        const uint32_t lane63 = (u < CG - 1) ? first_next : g.edge;
        const uint32_t nx = (uint32_t) __builtin_amdgcn_update_dpp((int) lane63, (int) g.a[u], DPP_WAVE_SHL1, 0xf, 0xf, false);
        if ((!LINE || x + 3 >= org + start) && x < pend) {
            const uint64_t both = ((uint64_t) nx << 32) | g.a[u];
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int xx = x + j - org;
                int dx;
                if (xx < start || xx >= wnew) {
                    dx = (int8_t) (g.a[u] >> (8 * j));                  // not part of the job: as loaded
                } else {
                    const bool right = (xx >= v);
                    dx = rebase_dx((int8_t) (both >> (8 * (j + (right ? 1 : 0)))), xx, right ? xx + 1 : xx, vprev, y);
                }
                o |= (uint32_t) (uint8_t) (int8_t) dx << (8 * j);
            }
            __builtin_nontemporal_store(o, row32 + (x >> 2));
        }
    }
}

// ---- back pointers, side 1.  New frame column xx sits at physical org + 1 + xx; pixels left of the seam (xx < v) come
// from physical org + xx (they move), pixels right of it stay where they are and are only re-based while their parent
// may lie left of (or on) the seam of the row above (xx < end_l = max(v, vprev + delta)).  Destination range
// [org + 1, org + 1 + end_l).
__device__ __forceinline__ void ld_right_8(const gu32 *row32, int gbase, int org, int ptop, int lane, G8 &g)
{
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = gbase + u * 256 + lane * 4;
        g.a[u] = (x + 3 >= org && x < ptop) ? __builtin_nontemporal_load(row32 + (x >> 2)) : 0u;      // x + 3 >= org >= 0 keeps x >= 0
    }
    g.edge = (lane == 0 && gbase - 1 >= org) ? row32[(gbase - 4) >> 2] : 0u;
}
__device__ __forceinline__ void st_right_8(gu32 *row32, int gbase, int org, int end_l, int v, int vprev, int y, int lane, const G8 &g)
{
    const int pfirst = org + 1, ptop = org + 1 + end_l;
#pragma unroll
    for (int u = 0; u < CG; u++) {
        const int x = gbase + u * 256 + lane * 4;
        const uint32_t last_prev = (u > 0) ? (uint32_t) __builtin_amdgcn_readlane((int) g.a[u > 0 ? u - 1 : 0], 63) : 0u;
        const uint32_t lane0 = (u > 0) ? last_prev : g.edge;
        const uint32_t pd = (uint32_t) __builtin_amdgcn_update_dpp((int) lane0, (int) g.a[u], DPP_WAVE_SHR1, 0xf, 0xf, false);
        if (x < ptop && x + 3 >= pfirst) {
            const uint64_t both = ((uint64_t) g.a[u] << 8) | (pd >> 24);      // byte k = physical x - 1 + k
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int xx = x + j - pfirst;
                int dx;
                if (xx < 0 || xx >= end_l) {
                    dx = (int8_t) (g.a[u] >> (8 * j));                  // not part of the job: as loaded
                } else {
                    const bool right = (xx >= v);
                    dx = rebase_dx((int8_t) (both >> (8 * (j + (right ? 1 : 0)))), xx, right ? xx + 1 : xx, vprev, y);
                }
                o |= (uint32_t) (uint8_t) (int8_t) dx << (8 * j);
            }
            __builtin_nontemporal_store(o, row32 + (x >> 2));
        }
    }
}

// one row of the carve, by one wave (the body of k_carve's row loop).  c = the
// PHYSICAL view, org / side = what k_vpath* published for this seam, w = the width before the carve.
// BESIDE (k_carve_u, k_carve_v): the energy role of the same launch writes en[pa .. pb] of this row; h and radius are read for that interval only
// SR (lqr_common.h): how seam_x is read -- SeamLive where the walk role of the same launch writes it (k_carve_v)
// line (plan_carve_line, lqr_plan.h): 1 = a row's groups start (side 0) / end (side 1) on a 32-element boundary, so that every
// 1 KB access of a wave to a float plane covers 8 whole 128-byte lines (rows start on line boundaries: the planes' stride is a
// multiple of 64 elements) and neighbouring chunks share none; 0 = on a 4-element boundary, the vector's alignment, as before: 9
// lines in 15 of 16 cases.  Either way the same vectors are loaded and stored, each once; only which wave access takes them differs.
// LINE false: there is no such argument, the vector's alignment at compile time (k_carve: the code it always had).
template <bool BESIDE, bool LINE = true, class SR = SeamPlain>
__device__ __forceinline__ void carve_row(const GCarver &c, int org, int side, int y, int w, int stride, int delta, int move_dp, int line, int lane, int h = 0, int radius = 0, SR sr = SR())
{
    const int wnew = w - 1, amask = LINE && line ? 31 : 3;
    int pa = 0x7fffffff, pb = -1;
    if (BESIDE) {
        int xmin, xmax;
        nrg_interval(c.seam_x, y, h, wnew, radius, xmin, xmax, sr);
        if (xmin <= xmax) { pa = org + side + xmin; pb = org + side + xmax; }
    }
    // (LINE: the seam's columns are uniform, and said so -- every bound of the row's job stays in scalar registers, which pays for the job's lower bound)
    const int v = LINE ? __builtin_amdgcn_readfirstlane(sr(c.seam_x + y)) : sr(c.seam_x + y);
    const size_t ro = (size_t) y * stride;
    const int vprev = y > 0 ? (LINE ? __builtin_amdgcn_readfirstlane(sr(c.seam_x + (y - 1))) : sr(c.seam_x + (y - 1))) : 0;
    gu32 *en = (gu32 *) (c.en + ro), *mm = (gu32 *) (c.m + ro), *l32 = (gu32 *) (c.least + ro);
    gu32 *rg = c.rig ? (gu32 *) (c.rig + ro) : (gu32 *) nullptr;
    // pix and bias are NOT moved: they stay in the frame of `frozen epoch` and the energy
    // update maps current coordinates back through the seam log (k_emap_update)
    if (side == 0) {
        const int pv = org + v, pend = org + wnew;
        int start = (y > 0) ? min(v, vprev - delta) : v;       // where the back pointers' job starts (<= v)
        if (start < 0) start = 0;
        int x0 = 0, fq = -1;
        uint32_t fval = 0;
        if (BESIDE) fq = en_fix_left(en, pv, pend, pb, lane, x0, fval);
        const int lo = org + (move_dp ? start : v);
        for (int base = lo & ~amask; base < pend; base += CGPX) {
            G32 E, M;
            G8 L;
            ld_left_u32<LINE>(en, base, lo, pend, lane, E);
            if (move_dp) { ld_left_u32<LINE>(mm, base, lo, pend, lane, M); ld_left_8<LINE>(l32, base, lo, pend, lane, L); }
            if (BESIDE) st_left_en(en, base, x0, pend, lane, E); else st_left_u32<LINE>(en, base, lo, pv, pend, lane, E);      // (x0 >= pv >= lo)
            if (move_dp) { st_left_u32<LINE>(mm, base, lo, pv, pend, lane, M); st_left_8<LINE>(l32, base, org, start, v, vprev, y, wnew, lane, L); }
        }
        if (BESIDE && fq >= 0) __builtin_nontemporal_store(fval, en + fq);
        if (rg)
            for (int base = pv & ~amask; base < pend; base += CGPX) { G32 R; ld_left_u32<LINE>(rg, base, pv, pend, lane, R); st_left_u32<LINE>(rg, base, pv, pv, pend, lane, R); }
    } else {
        const int pv = org + v;
        const int end_l = (y > 0) ? min(wnew, max(v, vprev + delta)) : min(wnew, v);      // back pointers' job: new columns [0, end_l)
        const int ptop = org + 1 + max(end_l, 0);
        // (the loads and stores of this side carry both bounds of the job already; the edge lane's group always holds a destination)
        const int top_u = (pv | amask) + 1;
        int x0 = 0, x1 = 0, fq = -1;
        uint32_t fval = 0;
        if (BESIDE) fq = en_fix_right(en, org, pv, pa, lane, x0, x1, fval);
        for (int top = move_dp ? max(top_u, (ptop + amask) & ~amask) : top_u; top > org + 1; top -= CGPX) {
            const int gbase = top - CGPX;
            G32 E, M;
            G8 L;
            ld_right_u32(en, gbase, org, pv, lane, E);
            if (move_dp) { ld_right_u32(mm, gbase, org, pv, lane, M); ld_right_8(l32, gbase, org, ptop, lane, L); }
            if (BESIDE) st_right_en(en, gbase, x0, x1, lane, E); else st_right_u32(en, gbase, org, pv, lane, E);
            if (move_dp) { st_right_u32(mm, gbase, org, pv, lane, M); st_right_8(l32, gbase, org, max(end_l, 0), v, vprev, y, lane, L); }
        }
        if (BESIDE && fq >= 0) __builtin_nontemporal_store(fval, en + fq);
        if (rg)
            for (int top = top_u; top > org + 1; top -= CGPX) { G32 R; ld_right_u32(rg, top - CGPX, org, pv, lane, R); st_right_u32(rg, top - CGPX, org, pv, lane, R); }
    }
}

__global__ __launch_bounds__(256) void k_carve(const DevCarver *cs, int w, int h, int stride, int delta, int move_dp)
{
    // blockIdx.x = row block (fastest): consecutive workgroups take consecutive rows of one image (2.5 % faster than
    // image-fastest, which round 1 used so that a concurrent band update could follow all images' top rows)
    const GCarver c = gview_phys(cs[blockIdx.y]);
    const int org = c.flags[FLAG_ORG_PREV], side = c.flags[FLAG_SIDE];      // published by k_vpath* for this seam
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) c.flags[FLAG_OVF_ROW] = h;       // the band kernels lower / overwrite it when they hand rows over to k_dp_sweep<UPDATE>
    for (int y = blockIdx.x * 4 + (threadIdx.x >> 6); y < h; y += gridDim.x * 4) carve_row<false, false>(c, org, side, y, w, stride, delta, move_dp, 0, lane);
}

// ---------------------------------------------------------------------------
// k_carve_e<NRG>: k_carve and k_emap_update<NRG, 12> in ONE launch, for single images and small groups (round 6).  There a seam round is
// a chain of dependent launches of small kernels (a 4K carve is 9 us, the energy update 9 us, each plus its dispatch), and the
// energy of row y needs nothing but row y's own carve: the wave that has moved a row refreshes the energies next to the seam on
// that row.  What k_emap_update does with a thread per row and LDS rows shared between neighbouring threads, a wave does alone:
// lanes 0 .. 35 stage the 12 brightness samples of rows y - 1, y, y + 1 (each mapped back to the frozen pixel plane through the
// seam log, as there), lanes 0 .. 11 then evaluate the gradient energy of the row's changed interval.  Same arithmetic, same
// order of operations: bit-identical energies.  delta_x <= 2 (12 samples per row suffice); larger delta_x and larger groups keep
// the two kernels (the carve's 96 registers and 5 waves per SIMD are what its bandwidth rests on).
// ---------------------------------------------------------------------------
template <int NRG>
__global__ __launch_bounds__(256) void k_carve_e(const DevCarver *cs, DpK p, int w, int h, int stride, int move_dp, int k, int epoch, int line)
{
    constexpr int NT = 12;
    constexpr bool luma = (NRG >= 3);
    const GCarver c = gview_phys(cs[blockIdx.y]);
    const int org = c.flags[FLAG_ORG_PREV], side = c.flags[FLAG_SIDE];      // published by the backtrack for this seam
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ double s_n255[256];
    __shared__ double s_bt[4][3][NT];
    __shared__ float s_bb[4][3][NT];
    __shared__ int s_lo[4][3];
    fill_norm255(s_n255, threadIdx.x, 256);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) c.flags[FLAG_OVF_ROW] = h;
    const int wn = w - 1;                                        // the frame after the carve
    gf32 *en = c.en + org + side;                                // its logical view (the origin after this seam)
    for (int y = blockIdx.x * 4 + wv; y < h; y += gridDim.x * 4) {
        carve_row<false>(c, org, side, y, w, stride, p.delta, move_dp, line, lane);
        if (wn <= 1) continue;
        // ---- the energy of row y next to the seam (k_emap_update, one row)
        const int g = lane / NT, i = lane - g * NT, t = y - 1 + g;          // lanes 0 .. 35: sample i of row t
        const bool samp = lane < 3 * NT && t >= 0 && t < h;
        int lo = 0, r = -1, pos = 0;
        if (samp) {
            int xmin, xmax;
            nrg_interval(c.seam_x, t, h, wn, p.radius, xmin, xmax);
            int l = xmin - 1; r = xmax + 1;
            if (t > 0) { int a, b; nrg_interval(c.seam_x, t - 1, h, wn, p.radius, a, b); if (b >= a) { l = min(l, a); r = max(r, b); } }
            if (t < h - 1) { int a, b; nrg_interval(c.seam_x, t + 1, h, wn, p.radius, a, b); if (b >= a) { l = min(l, a); r = max(r, b); } }
            lo = max(l, 0);
            pos = lo + i;
            const gi32 *lg = c.seam_log + t;
            for (int j = k; j >= epoch; j -= EU_LOGB) {
                int v[EU_LOGB];
#pragma unroll
                for (int u = 0; u < EU_LOGB; u++) v[u] = lg[(size_t) max(j - u, epoch) * h];
#pragma unroll
                for (int u = 0; u < EU_LOGB; u++) { const int vu = (j - u >= epoch) ? v[u] : 0x7fffffff; pos += (vu <= pos) ? 1 : 0; }
            }
            const int wf = wn + (k - epoch) + 1;                 // width of the frozen frame
            const bool ok = (lo + i <= min(r, wn - 1)) && pos < wf;
            const size_t o = (size_t) t * stride + (ok ? pos : 0);
            s_bt[wv][g][i] = ok ? px_bright(c.pix[o], p.ch, luma, Norm255Lut{s_n255}) : 0.0;
            s_bb[wv][g][i] = (ok && c.bias) ? c.bias[o] : 0.0f;
            if (i == 0) s_lo[wv][g] = lo;
        }
        __builtin_amdgcn_wave_barrier();                          // (one wave: its LDS operations execute in order)
        int xmin, xmax;
        nrg_interval(c.seam_x, y, h, wn, p.radius, xmin, xmax);
        const int x = xmin + lane;
        if (x <= xmax) {
            float e = grad_energy_f<NRG>([&](int xx, int yy) { const int gg = yy - y + 1; return s_bt[wv][gg][xx - s_lo[wv][gg]]; }, x, y, wn, h);
            if (c.bias) e = __fadd_rn(e, __fdiv_rn(s_bb[wv][1][x - s_lo[wv][1]], (float) p.w_start));
            // (behind the carve's stores of this row in program order; different cache policies: drain them first)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            en[(size_t) y * stride + x] = e;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------
// k_carve_u<NRG>: k_carve and k_emap_update<NRG, 12, false> in ONE launch, side by side, for the groups too large for k_carve_e.  On
// one stream the energy update used to run alone behind the carve: n * ceil(h / EU_ROWS) one-wave workgroups walking the seam log, the
// chip almost empty.  It is no true dependency of the carve: it reads seam_x, the seam log and the frozen pix / bias planes, none of
// which the carve writes, and it writes en[xmin .. xmax] of every row -- which the carve of this kernel neither writes nor uses
// (st_left_en / st_right_en).  So the two run as separate workgroups of one 1-D grid, each role with its own code:
//   * workgroups [0, n * ceil(h / EU_ROWS)): the energy role, all images.  FIRST in dispatch order: their log walk is the longest
//     dependent chain of the launch and has to start with it, not form its tail.  All four waves fill the table of v / 255, wave 0
//     then runs k_emap_update's body (emap_update_block, lqr_pixel.h: bit-identical energies) and the others leave.  Its en pointer
//     comes from FLAG_ORG, which the backtrack published before this launch; the carve role writes no origin flag.
//   * the rest: the carve role, as k_carve's grid (row blocks fastest within an image), one row per wave.
// The branch is uniform over the workgroup.  delta_x <= 2 (12 samples per row), packed pixels; everything else keeps the two launches.
// ---------------------------------------------------------------------------
template <int NRG>
__global__ __launch_bounds__(256) void k_carve_u(const DevCarver *cs, DpK p, int w, int h, int stride, int move_dp, int k, int epoch, int n, int line)
{
    // (cu_grid / cu_block in lqr_geom.h state this map and the test checks it there; here it stays in the kernel's own text: through the
    // function the instruction stream differs)
    const int eblk = bb_energy_entries(h), ne = n * eblk;
    if ((int) blockIdx.x < ne) {
        const int img = blockIdx.x / eblk, blk = blockIdx.x - img * eblk;
        PixRead<false> rd;
        rd.setup(threadIdx.x, 256);
        if (threadIdx.x >= 64) return;
        const GCarver c = gview(cs[img]);                                    // the frame after this seam
        emap_update_block<NRG, 12, false, true>(c, rd, p, w - 1, h, stride, k, epoch, blk, threadIdx.x);
        return;
    }
    const int rblk = bb_carve_entries(h), cb = blockIdx.x - ne, img = cb / rblk, rb = cb - img * rblk;
    const GCarver c = gview_phys(cs[img]);
    const int org = c.flags[FLAG_ORG_PREV], side = c.flags[FLAG_SIDE];      // published by k_vpath* for this seam
    if (rb == 0 && threadIdx.x == 0) c.flags[FLAG_OVF_ROW] = h;
    const int y = rb * 4 + (threadIdx.x >> 6);
    if (y < h) carve_row<true>(c, org, side, y, w, stride, p.delta, move_dp, line, threadIdx.x & 63, h, p.radius);
}

// ---------------------------------------------------------------------------
// k_carve_v<NRG, DELTA>: k_vpath1, k_carve and k_emap_update<NRG, 12, false> in ONE launch.  On one stream the backtrack ran alone in
// front of the carve: one chasing wave per image for 59 us per 4K seam, the chip otherwise empty.  The carve depends on it only row
// by row (carve_row reads seam_x[y] and seam_x[y - 1], nrg_interval `radius` rows either way) plus one bit, the side -- and the side,
// decided today from the whole path's sum(x), is often fixed long before the walk ends: seams are delta_x-connected, so the rows to
// come lie in a cone (bb_side_bound, lqr_beside.h).  Three roles in one 1-D grid, the branch uniform over the workgroup:
//   * workgroups [0, n): the WALK, one per image, first in dispatch order.  row_argmin on 256 threads; then wave 0 chases (vpath1_walk
//     with BB_WALK_ROWS-row chunks for either delta_x: k_vpath1's 28-row chunks need 171 VGPRs) and leaves every chunk's columns in LDS
//     (s_path, then s_lo = the lowest row found: a wave's LDS operations execute in order); wave 1 PUBLISHES what it finds there, so
//     that no store acknowledgement and no atomic's round trip is on the chase: it writes the rows to seam_x and the session log
//     (write-through), waits for the acknowledgements, evaluates the bound on the sum so far -- once decided it writes the flags
//     exactly as publish_side does -- and pushes the entries whose inputs are final now (bb_first_quad / bb_first_eblk; an image that
//     decides late pushes its backlog at once): one atomic add on the list's tail reserves the slots, write-through stores fill
//     them.  Every image pushes ceil(h / 4) carve and ceil(h / EU_ROWS) energy entries in all.  Neither wave waits for anything
//     outside its workgroup.
//   * the rest, n * (ceil(h / 4) + ceil(h / EU_ROWS)) CONSUMERS: workgroup b polls entry b - n with one lane (agent-scope load,
//     bounded spin, DEVERR_TILE_TIMEOUT as in the other spinning kernels: the session is then redone on the kernels without spins),
//     then is the carve of the entry's four rows (carve_row<true>) or the energy update of its block (emap_update_block), with
//     origin and side from the entry.  Dispatch order is consumption order, so a consumer only ever waits for an entry some walk
//     -- resident since before it -- will push.
// Every read of the CURRENT seam by a consumer (seam_x; log entry k) is an agent-scope load (SeamLive): an XCD's L2 may hold a line
// of it fetched earlier in the launch.  Tags carry the launch (bb_tag): the list is never cleared; of the two tail words a launch
// counts on the one of its tag's parity and image 0's walk clears the other for the next launch.
// Same seams, planes, flags and g_moved_bytes as the separate launches by construction; tests/test_backtrack_beside_gpu.py compares.
// ---------------------------------------------------------------------------
static_assert(BB_EU_ROWS == EU_ROWS, "lqr_beside.h restates EU_ROWS");
typedef GLOBAL_AS unsigned long long gu64;
#ifdef LQR_TIMING
__device__ unsigned long long g_walk_cycles[2];       // image 0's walk role, wall-clock ticks (s_memrealtime, 100 MHz): [0] the chase, [1] until the last entry is pushed
extern "C" int lqrhip_walk_timing(unsigned long long *out) { (void) hipDeviceSynchronize(); return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_walk_cycles), sizeof(unsigned long long) * 2) == hipSuccess ? 0 : -1; }
#endif
__device__ __forceinline__ void st_wt(gi32 *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }      // write-through

template <int NRG, int DELTA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_carve_v(const DevCarver *cs, DpK p, int w, int h, int stride, int lr, int move_dp, int k, int epoch, int n,
                                                 int moved_unit, unsigned tag, unsigned long long *list, unsigned long long *moved_bytes, int *dev_err, int line)
{
    const int eblk = bb_energy_entries(h), rblk = bb_carve_entries(h);
    const unsigned total = (unsigned) n * (unsigned) (eblk + rblk);
    gu64 *entries = (gu64 *) list + BB_LIST_HEAD;
    const int tid = threadIdx.x;
    if ((int) blockIdx.x < n) {
        // ---- the walk role
        __shared__ float s_val[VPATH_THREADS / 64];
        __shared__ int s_idx[VPATH_THREADS / 64];
        __shared__ int s_path[BB_MAX_ROWS];          // the seam's column on every row found so far (h <= BB_MAX_ROWS: lqr_plan.h)
        __shared__ int s_lo;                         // the lowest of them
        __shared__ __attribute__((aligned(16))) int8_t s_win[BB_WALK_ROWS * 256];      // the chase's current chunk (vpath1_walk.inc)
        const int img = blockIdx.x;
        const GCarver c = gview(cs[img]);
        const int org = c.flags[FLAG_ORG];           // read before the publishing wave writes the next one
        if (tid == 0) {
            s_lo = h;
            if (img == 0) __hip_atomic_store((gu64 *) list + ((tag + 1) & 1), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next launch's tail
        }
        const int xmin = row_argmin(c.m + (size_t) (h - 1) * stride, w, lr, s_val, s_idx);       // (a barrier inside: s_lo is set)
        if (tid >= 128) return;
        const int lane = tid & 63;
#ifdef LQR_TIMING
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
#endif
        if (tid < 64) {
            // wave 0: the chase.  Rows go to LDS; the publishing wave takes them from there
            int x = __builtin_amdgcn_readfirstlane(max(xmin, 0));
            __builtin_amdgcn_s_setprio(3);
            constexpr int VP1_ROWS = BB_WALK_ROWS;
#define VP1_RECORD(y_top, nrows, pe, po) \
            if (2 * lane < nrows) LDS_FLAG(s_path[y_top - 2 * lane]) = pe; \
            if (2 * lane + 1 < nrows) LDS_FLAG(s_path[y_top - 2 * lane - 1]) = po; \
            LDS_FLAG(s_lo) = y_top - nrows + 1;
#include "vpath1_walk.inc"
#undef VP1_RECORD
            LDS_FLAG(s_path[0]) = x;
            LDS_FLAG(s_lo) = 0;
#ifdef LQR_TIMING
            if (img == 0 && lane == 0) g_walk_cycles[0] = __builtin_amdgcn_s_memrealtime() - t0;
#endif
            return;
        }
        // wave 1: publish
        gi32 *seam = c.seam_x, *logp = c.seam_log + (size_t) k * h;
        gu64 *tail = (gu64 *) list + (tag & 1);
        int done = h, acc = 0, side = -1, next_q = rblk - 1, next_e = eblk - 1;
        for (unsigned spins = 0; done > 0;) {
            const int lo = __builtin_amdgcn_readfirstlane(LDS_FLAG(s_lo));
            if (lo >= done) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > (1u << 24)) { if (lane == 0) dev_fail(dev_err, DEVERR_TILE_TIMEOUT); return; }      // (the chase waits for nothing but memory)
                continue;
            }
            for (int y = done - 1 - lane; y >= lo; y -= 64) { const int v = LDS_FLAG(s_path[y]); st_wt(seam + y, v); st_wt(logp + y, v); acc += v; }
            const int xlo = __builtin_amdgcn_readfirstlane(LDS_FLAG(s_path[lo]));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the rows have arrived before an entry says so
            done = lo;
            if (side < 0) {
                int S = acc;
                for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
                side = bb_side_bound(S, xlo, lo, DELTA, w, h);        // (lo = 0: the rule itself)
                if (side >= 0 && lane == 0) { c.flags[FLAG_ORG_PREV] = org; c.flags[FLAG_SIDE] = side; c.flags[FLAG_ORG] = org + side; c.flags[FLAG_OVF_ROW] = h; }
            }
            if (side < 0) continue;
            const int e0 = bb_first_eblk(lo, p.radius), q0 = bb_first_quad(lo, p.radius);
            const int ne = max(next_e - e0 + 1, 0), nq = max(next_q - q0 + 1, 0), cnt = ne + nq;
            if (cnt == 0) continue;
            unsigned base = 0;
            if (lane == 0) base = (unsigned) __hip_atomic_fetch_add(tail, (unsigned long long) cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = (unsigned) __builtin_amdgcn_readfirstlane((int) base);
            for (int i = lane; i < cnt; i += 64) {
                const bool en = i < ne;
                const unsigned slot = base + (unsigned) i;
                if (slot < total)        // (always, while every image pushes its count: never a store past the list)
                    __hip_atomic_store(entries + slot, bb_pack(tag, en ? 1 : 0, img, en ? next_e - i : next_q - (i - ne), side, org), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            next_e -= ne; next_q -= nq;
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) {
            const long long all = (long long) h * (w - 1);
            atomicAdd(moved_bytes, (unsigned long long) (side ? (long long) acc : all - acc) * (unsigned long long) moved_unit);
#ifdef LQR_TIMING
            if (img == 0) g_walk_cycles[1] = __builtin_amdgcn_s_memrealtime() - t0;
#endif
        }
        return;
    }
    // ---- a consumer: wait for the entry of this workgroup's place in the dispatch order
    __shared__ unsigned long long s_entry;
    if (tid == 0) {
        gu64 *src = entries + (blockIdx.x - (unsigned) n);
        unsigned long long e = 0;
        for (unsigned sp = 0;;) {
            e = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned) (e >> BB_TAG_SHIFT) == tag) break;
            e = 0;
            if (sp < 16) __builtin_amdgcn_s_sleep(4); else __builtin_amdgcn_s_sleep(32);
            ++sp;
            if ((sp & 255) == 0 && dev_failed(dev_err)) break;
            if (sp > (1u << 18)) { dev_fail(dev_err, DEVERR_TILE_TIMEOUT); break; }
        }
        s_entry = e;
    }
    __syncthreads();
    // (uniform, and said so: image, rows, origin and side stay in scalar registers, as where they come from the block index and the flags)
    const unsigned long long ew = ((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (s_entry >> 32)) << 32) | (unsigned) __builtin_amdgcn_readfirstlane((int) s_entry);
    if (ew == 0) return;                             // timed out: the host finds the code
    const BbEntry e = bb_unpack(ew);
    if (e.image >= n) return;
    if (e.energy) {
        PixRead<false> rd;
        rd.setup(tid, 256);
        if (tid >= 64 || e.index >= eblk) return;
        GCarver c = gview_phys(cs[e.image]);
        c.en += e.org + e.side;                      // the frame after this seam (the only plane the energy role writes; pix / bias are frozen)
        emap_update_block<NRG, 12, false, true>(c, rd, p, w - 1, h, stride, k, epoch, (unsigned) e.index, tid, SeamLive());
        return;
    }
    GCarver c = gview_phys(cs[e.image]);
    // (the descriptor comes by vector loads: the row's plane pointers to scalar registers, or the three roles do not fit 96 VGPRs)
    c.en = uni_ptr(c.en); c.m = uni_ptr(c.m); c.least = uni_ptr(c.least); c.seam_x = uni_ptr(c.seam_x);
    const int y = e.index * 4 + (tid >> 6);
    if (y < h) carve_row<true, true>(c, e.org, e.side, y, w, stride, DELTA, move_dp, line, tid & 63, h, p.radius, SeamLive());
}

// ---- the instantiations the shim launches (lqr_kernels.h lists them)
// (k_carve is not a template)
#define INST(N) template __global__ void k_carve_u<N>(const DevCarver *, DpK, int, int, int, int, int, int, int, int);
K_CARVE_U_FORMS(INST)
#undef INST
#define INST(N, D) template __global__ void k_carve_v<N, D>(const DevCarver *, DpK, int, int, int, int, int, int, int, int, int, unsigned, unsigned long long *, unsigned long long *, int *, int);
K_CARVE_V_FORMS(INST)
#undef INST
#define INST(N) template __global__ void k_carve_e<N>(const DevCarver *, DpK, int, int, int, int, int, int, int);
K_CARVE_E_FORMS(INST)
#undef INST
