// lqr_beside.h -- the backtrack beside the carve (k_carve_v, k_carve.hip): what the walk decides and hands over, as plain C++17.  No HIP,
// no globals, no I/O: constexpr functions of values, so that the same code runs in the kernel and in tests/c/beside_main.cc without a
// GPU.  Three things:
//   * the side bound: the side the carve moves (k_vpath*: side 1 iff 2 * sum(x) < h * (w - 1), sum over the seam's h rows) decided
//     from a PART of the walk.  The walk goes bottom-up; when it stands on row y with column x and the columns of rows y .. h - 1
//     sum to S, the r = y rows still to come are delta_x-connected to x: the k-th of them lies in [x - delta k, x + delta k] and in
//     [0, w - 1].  The sum of what remains therefore lies in [bb_rem_min, bb_rem_max]; where both ends give the same sign the
//     side is known.  With r = 0 the two ends are 0 and the bound IS the rule.
//   * the work list's entries: 8 bytes, tag and payload in one word (the granule idiom of k_dp_tile_p and k_band_levels: a reader
//     that sees the tag has the payload; nothing is cleared between launches).
//   * which entries rows lo .. h - 1 being final allows: the carve of a row-quad reads its rows' seam_x, the row before them and,
//     for nrg_interval, `radius` rows either way; an energy block (emap_update_block) the intervals of its rows, its two halo
//     rows and their neighbours.
#pragma once
#include <stdint.h>

constexpr int BB_WALK_ROWS = 12;            // rows per chunk of the walk role (k_vpath1's delta_x 2 geometry, for delta_x 1 too: 83 VGPRs)
constexpr int BB_MAX_ROWS = 4096;           // rows the walk role's path buffer (LDS, an int per row) holds
constexpr int BB_MAX_IMAGES = 1024;         // the entry's image field
constexpr int BB_EU_ROWS = 62;              // EU_ROWS (lqr_common.h; k_carve.hip asserts that they agree)
constexpr int BB_MIN_ROWS = 3 * BB_WALK_ROWS + 1;      // three chunks of steps

// ---- the side bound
constexpr long long bb_min_ll(long long a, long long b) { return a < b ? a : b; }
// sum over k = 1 .. r of max(0, x - delta k) / of min(w - 1, x + delta k)
constexpr long long bb_rem_min(long long x, long long r, long long delta)
{
    const long long k0 = delta > 0 ? bb_min_ll(r, x / delta) : r;          // rows that still stand right of column 0
    return k0 * x - delta * (k0 * (k0 + 1) / 2);
}
constexpr long long bb_rem_max(long long x, long long r, long long delta, long long w)
{
    const long long k1 = delta > 0 ? bb_min_ll(r, (w - 1 - x) / delta) : r;      // rows that still stand left of column w - 1
    return k1 * x + delta * (k1 * (k1 + 1) / 2) + (r - k1) * (w - 1);
}
// S = sum of the columns of rows y .. h - 1, x = the column on row y, r = y rows to come.  Returns the side (0 / 1) or -1: not yet.
// Frames up to 16384 x 16384: S and the ends stay below 2^29, everything here below 2^31 (in 64 bits all the same)
constexpr int bb_side_bound(long long S, int x, int r, int delta, int w, int h)
{
    const long long all = (long long) h * (w - 1);
    if (2 * (S + bb_rem_max(x, r, delta, w)) < all) return 1;
    if (2 * (S + bb_rem_min(x, r, delta)) >= all) return 0;
    return -1;
}

// ---- entries: tag 26 bits | role 1 | image 10 | index 12 (row-quad, or energy block) | side 1 | origin before the seam 14
constexpr int BB_TAG_SHIFT = 38;
constexpr unsigned BB_EPOCHS = (1u << 26) - 2;              // even: consecutive launches have tags of alternating parity
constexpr unsigned bb_tag(unsigned launches) { return 1u + launches % BB_EPOCHS; }       // never 0: a cleared list holds no entry
struct BbEntry { unsigned tag; int energy, image, index, side, org; };
constexpr uint64_t bb_pack(unsigned tag, int energy, int image, int index, int side, int org)
{
    return ((uint64_t) tag << BB_TAG_SHIFT) | ((uint64_t) (energy & 1) << 37) | ((uint64_t) (image & 1023) << 27) |
           ((uint64_t) (index & 4095) << 15) | ((uint64_t) (side & 1) << 14) | (uint64_t) (org & 16383);
}
constexpr BbEntry bb_unpack(uint64_t e)
{
    return BbEntry{(unsigned) (e >> BB_TAG_SHIFT), (int) ((e >> 37) & 1), (int) ((e >> 27) & 1023), (int) ((e >> 15) & 4095), (int) ((e >> 14) & 1), (int) (e & 16383)};
}

// ---- the list: two tail words (a launch counts on the one of its tag's parity and clears the other for the next), then the entries
constexpr int BB_LIST_HEAD = 2;
constexpr int bb_carve_entries(int h) { return (h + 3) / 4; }
constexpr int bb_energy_entries(int h) { return (h + BB_EU_ROWS - 1) / BB_EU_ROWS; }
constexpr long long bb_entries(int n, int h) { return (long long) n * (bb_carve_entries(h) + bb_energy_entries(h)); }      // = the consumer workgroups
// the lowest row-quad / energy block whose inputs are final once rows lo .. h - 1 are (lo = 0: everything)
constexpr int bb_first_quad(int lo, int radius) { return lo <= 0 ? 0 : (lo + 1 + radius + 3) / 4; }
constexpr int bb_first_eblk(int lo, int radius) { return lo <= 0 ? 0 : (lo + 2 + radius + BB_EU_ROWS - 1) / BB_EU_ROWS; }
