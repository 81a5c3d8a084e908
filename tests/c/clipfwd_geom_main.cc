// The launch geometry of the clip's forward build (csrc/lqr_geom.h, the clip_* functions and the sweep's fwd_lds / fwd_row_off) without a
// GPU; built by tests/test_clipforward_geom.py with -Werror under AddressSanitizer and UndefinedBehaviorSanitizer.  The header is
// included alone.  One argument says what to do:
//   values   every size and offset over the grid of shapes below, one line each: "name args... value".  The test holds the same lines as
//            plain arithmetic of its own and compares.
//   extents  every block of a build and the two LDS blocks are allocated on the heap with exactly the stated number of bytes, and the
//            first and the last element a kernel of k_clipfwd.hip can touch are written, by the kernel's index expression as its source
//            has it (restated here) -- after the header's offset function was checked equal to that expression.  AddressSanitizer is the
//            judge; "ok extents <blocks>" at the end.
#include "lqr_geom.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static const int LS[] = {2, 3, 1023, 1024, 1025, 4097, 16384}, HS[] = {1, 2, 65, 2160}, NS[] = {1, 2, 16, 17, 64};
static const int GROUP = 16, REFRESH_THREADS = 256;     // CLIPFWD_GROUP, CLIPFWD_REFRESH_THREADS (lqr_common.h; the test compares them)

static void values()
{
    printf("CLIP_COST_FLOATS %d\n", CLIP_COST_FLOATS);
    printf("CLIP_REFRESH_VALUES %d\n", CLIP_REFRESH_VALUES);
    printf("clip_refresh_lds_elems %d %zu\n", REFRESH_THREADS, clip_refresh_lds_elems(REFRESH_THREADS));
    for (int n : NS) printf("clip_fold_groups %d %d\n", n, clip_fold_groups(n, GROUP));
    for (int L : LS) {
        printf("fwd_lds %d %zu\n", L, fwd_lds(L));
        printf("fwd_attr %d %d\n", L, (int) lds_needs_attr(fwd_lds(L)));
        for (int H : HS) {
            const size_t px = (size_t) L * H;
            printf("clip_cost_elems %d %d %zu\n", L, H, clip_cost_elems(px));
            printf("clip_cost_off %d %d %zu\n", L, H, clip_cost_off(H - 1, L - 1, L));
            for (int n : NS) {
                printf("clip_intensity_elems %d %d %d %zu\n", L, H, n, clip_intensity_elems(n, px));
                printf("clip_frame_off %d %d %d %zu\n", L, H, n, clip_frame_off(n - 1, px));
            }
        }
    }
}

// a block of exactly `bytes`, first and last byte of the elements at `first` and `last` (element size `sz`) written
static int touch(size_t bytes, size_t sz, size_t first, size_t last)
{
    unsigned char *p = (unsigned char *) malloc(bytes);
    CHECK(p != nullptr, "%zu bytes", bytes);
    memset(p + first * sz, 1, sz);
    memset(p + last * sz, 2, sz);
    const int ok = p[first * sz] != 0 && p[last * sz + sz - 1] == 2;
    free(p);
    return ok;
}

static void extents()
{
    int blocks = 0;
    for (int L : LS)
        for (int H : HS) {
            const size_t px = (size_t) L * H;
            for (int n : NS) {
                if (clip_intensity_elems(n, px) * sizeof(float) > ((size_t) 1 << 31)) continue;       // (what this machine's heap need not give)
                // k_fwd_init writes frame t's I at in + clip_frame_off(t, px) + y * L + x; k_clip_fold and k_clip_refresh read there
                CHECK(clip_frame_off(n - 1, px) + (size_t) (H - 1) * L + (L - 1) == (size_t) n * px - 1, "%d %d %d", L, H, n);
                CHECK(touch(clip_intensity_elems(n, px) * sizeof(float), sizeof(float), 0, clip_frame_off(n - 1, px) + (size_t) (H - 1) * L + (L - 1)), "in");
                blocks++;
            }
            // the costs: k_clip_fold, k_clip_seam and k_clip_remove take pixel o = y * L + x as the 16-byte vector o; k_clip_refresh writes
            // the floats clip_cost_off(y, x, L) + 0 .. 2 of a column x < wn <= L - 1
            CHECK(clip_cost_off(H - 1, L - 1, L) == ((size_t) (H - 1) * L + (L - 1)) * 4, "%d %d", L, H);
            CHECK(touch(clip_cost_elems(px) * sizeof(float), 4 * sizeof(float), 0, (size_t) (H - 1) * L + (L - 1)), "cost as vectors");
            CHECK(touch(clip_cost_elems(px) * sizeof(float), sizeof(float), clip_cost_off(0, 0, L), clip_cost_off(H - 1, L - 2, L) + 2), "cost as floats");
            // Pm, the positions, the choices, the map: px elements each, pixel y * L + x (the map of orientation 1: x * H + y); the seam: H
            CHECK(touch(px * sizeof(float), sizeof(float), 0, px - 1), "pm");
            CHECK(touch(px * sizeof(uint16_t), sizeof(uint16_t), 0, px - 1), "pos");
            CHECK(touch(px * sizeof(int8_t), sizeof(int8_t), 0, px - 1), "choice");
            CHECK(touch(px * sizeof(int32_t), sizeof(int32_t), 0, (size_t) (L - 1) * H + (H - 1)), "map");
            CHECK(touch((size_t) H * sizeof(int32_t), sizeof(int32_t), 0, (size_t) H - 1), "seam");
            blocks += 8;
        }
    for (int L : LS) {
        // k_clip_seam's dynamic LDS: row parity p at fwd_row_off(p, L), columns 0 .. L - 1
        CHECK(fwd_row_off(0, L) == 0 && fwd_row_off(1, L) == L, "%d", L);
        CHECK(touch(fwd_lds(L), sizeof(float), fwd_row_off(0, L), (size_t) fwd_row_off(1, L) + L - 1), "s_m");
        blocks++;
    }
    // k_clip_refresh's s_red: wave v's CLIP_REFRESH_VALUES maxima at clip_refresh_off(v)
    const int waves = REFRESH_THREADS / 64;
    CHECK(clip_refresh_off(waves - 1) + CLIP_REFRESH_VALUES == (int) clip_refresh_lds_elems(REFRESH_THREADS), "%d", waves);
    CHECK(touch(clip_refresh_lds_elems(REFRESH_THREADS) * sizeof(float), sizeof(float), clip_refresh_off(0), (size_t) clip_refresh_off(waves - 1) + CLIP_REFRESH_VALUES - 1), "s_red");
    blocks++;
    printf("ok extents %d\n", blocks);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "values")) values();
    else if (argc == 2 && !strcmp(argv[1], "extents")) extents();
    else { fprintf(stderr, "usage: %s values|extents\n", argv[0]); return 2; }
    return 0;
}
