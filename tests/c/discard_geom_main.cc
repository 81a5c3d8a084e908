// The launch geometry of the discard scan (csrc/lqr_geom.h, the discard_* functions) without a GPU; built by tests/test_remove_geom.py
// with -Werror under AddressSanitizer and UndefinedBehaviorSanitizer.  The header is included alone.  One argument says what to do:
//   values   every size, grid and offset over the grid of shapes below, one line each: "name args... value".  The test holds the same
//            lines as plain arithmetic of its own and compares.
//   extents  the two planes, the result block and the cross scan's counts are allocated on the heap with exactly the stated number of
//            bytes, and every access the three kernels of k_discard.hip make is made here, by the kernels' index expressions as their
//            source has them (restated here), over their whole grids: 16-byte reads where the line scan makes them -- whose addresses
//            must be multiples of 16 bytes --, single elements elsewhere.  Every pixel must be read exactly once by each scan.
//            AddressSanitizer is the judge; "ok extents <shapes>" at the end.
#include "lqr_geom.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static const int WS[] = {1, 2, 3, 5, 40, 255, 256, 257, 1023, 1024, 1025, 2049, 3840}, HS[] = {1, 3, 5, 9, 31, 32, 33, 65, 300};

static void values()
{
    printf("DISCARD_THREADS %d\nDISCARD_CHUNK %d\nDISCARD_ROWS %d\nDISCARD_WORDS %d\n", DISCARD_THREADS, DISCARD_CHUNK, DISCARD_ROWS, DISCARD_WORDS);
    printf("discard_result_elems %zu\n", discard_result_elems());
    printf("discard_result_off %d %d\n", discard_result_off(0), discard_result_off(1));
    for (int w : WS) {
        printf("discard_col_blocks %d %d\n", w, discard_col_blocks(w));
        printf("discard_rank_elems %d %zu\n", w, discard_rank_elems(w));
        for (int h : HS) {
            printf("discard_row_tiles %d %d\n", h, discard_row_tiles(h));
            printf("discard_partial_elems %d %d %zu\n", w, h, discard_partial_elems(w, h));
            printf("discard_partial_off %d %d %zu\n", w, h, discard_partial_off(discard_row_tiles(h) - 1, w - 1, w));
            printf("discard_lead %d %d %d\n", w, h, discard_lead((size_t) h - 1, w));
        }
    }
}

static void extents()
{
    int shapes = 0;
    for (int w0 : WS)
        for (int h0 : HS) {
            const size_t n = (size_t) w0 * h0;
            // (16-byte aligned, as the allocation cache's blocks are)
            float *bias = (float *) aligned_alloc(16, (n * sizeof(float) + 15) & ~(size_t) 15);
            int32_t *vs = (int32_t *) aligned_alloc(16, (n * sizeof(int32_t) + 15) & ~(size_t) 15);
            int *res = (int *) malloc(discard_result_elems() * sizeof(int));
            int *partial = (int *) malloc(discard_partial_elems(w0, h0) * sizeof(int));
            CHECK(bias && vs && res && partial, "%d %d", w0, h0);
            // (the rounding of the two planes above is this program's: reads past n are counted below instead)
            std::vector<int> seen(n, 0);
            for (size_t i = 0; i < n; i++) { bias[i] = -1.0f; vs[i] = 0; }
            memset(res, 0, discard_result_elems() * sizeof(int));
            // k_discard_line: grid h0, DISCARD_THREADS lanes
            long total = 0;
            for (int y = 0; y < h0; y++) {
                const size_t ri = (size_t) y * w0;
                for (int base = -discard_lead((size_t) y, w0); base < w0; base += DISCARD_CHUNK)
                    for (int tid = 0; tid < DISCARD_THREADS; tid++) {
                        const int g = base + 4 * tid;
                        if (g >= 0 && g + 3 < w0) {
                            CHECK(((uintptr_t) (bias + ri + g) & 15) == 0 && ((uintptr_t) (vs + ri + g) & 15) == 0, "%d %d row %d column %d", w0, h0, y, g);
                            CHECK(ri + g + 3 < n, "%d %d", w0, h0);
                            for (int k = 0; k < 4; k++) { total += bias[ri + g + k] < 0 && vs[ri + g + k] == 0; seen[ri + g + k]++; }
                        } else {
                            for (int k = 0; k < 4; k++)
                                if ((unsigned) (g + k) < (unsigned) w0) { total += bias[ri + g + k] < 0 && vs[ri + g + k] == 0; seen[ri + g + k]++; }
                        }
                    }
            }
            CHECK(total == (long) n, "%d %d: the line scan read %ld of %zu", w0, h0, total, n);
            for (size_t i = 0; i < n; i++) CHECK(seen[i] == 1, "%d %d: pixel %zu read %d times by the line scan", w0, h0, i, seen[i]);
            res[discard_result_off(0)] = (int) total;
            // k_discard_cross: grid discard_col_blocks x discard_row_tiles; every element of `partial` is written, once
            const int tiles = discard_row_tiles(h0);
            for (size_t i = 0; i < discard_partial_elems(w0, h0); i++) partial[i] = -1;
            for (int by = 0; by < tiles; by++)
                for (int bx = 0; bx < discard_col_blocks(w0); bx++)
                    for (int tid = 0; tid < DISCARD_THREADS; tid++) {
                        const int x = bx * DISCARD_THREADS + tid, y0 = by * DISCARD_ROWS, y1 = y0 + DISCARD_ROWS < h0 ? y0 + DISCARD_ROWS : h0;
                        if (x >= w0) continue;
                        int count = 0;
                        for (int y = y0; y < y1; y++) { const size_t at = (size_t) y * w0 + x; count += bias[at] < 0 && vs[at] == 0; seen[at]++; }
                        CHECK(partial[discard_partial_off(by, x, w0)] == -1, "%d %d: written twice", w0, h0);
                        partial[discard_partial_off(by, x, w0)] = count;
                    }
            for (size_t i = 0; i < n; i++) CHECK(seen[i] == 2, "%d %d: pixel %zu read %d times by the cross scan", w0, h0, i, seen[i] - 1);
            // k_discard_fold: grid discard_col_blocks
            total = 0;
            for (int bx = 0; bx < discard_col_blocks(w0); bx++)
                for (int tid = 0; tid < DISCARD_THREADS; tid++) {
                    const int x = bx * DISCARD_THREADS + tid;
                    if (x >= w0) continue;
                    int line = 0;
                    for (int t = 0; t < tiles; t++) line += partial[discard_partial_off(t, x, w0)];
                    CHECK(line == h0, "%d %d column %d: %d", w0, h0, x, line);
                    total += line;
                }
            res[discard_result_off(1)] = (int) total;
            res[discard_result_off(1) + DISCARD_WORDS - 1] = 0;              // the last word of the block
            // k_discard_rank: grid h0; every third pixel of a row hidden, w = the visible ones: a visible pixel's rank is its index in col
            {
                const int w = w0 - w0 / 3;
                int *col = (int *) calloc(discard_rank_elems(w), sizeof(int));
                CHECK(col != nullptr, "%d", w);
                for (int y = 0; y < h0; y++) {
                    int carry = 0;
                    for (int base = 0; base < w0; base += DISCARD_THREADS) {
                        int total_here = 0;
                        for (int tid = 0; tid < DISCARD_THREADS; tid++) {
                            const int x = base + tid;
                            const bool in = x < w0, keep = in && x % 3 != 2;
                            const int rank = carry + total_here;
                            if (in) seen[(size_t) y * w0 + x]++;
                            if (keep && rank < w) col[rank]++;
                            total_here += keep;
                        }
                        carry += total_here;
                    }
                    CHECK(carry == w, "%d %d row %d: %d visible", w0, h0, y, carry);
                }
                for (int x = 0; x < w; x++) CHECK(col[x] == h0, "%d %d column %d: %d", w0, h0, x, col[x]);
                free(col);
            }
            CHECK(res[discard_result_off(0)] == res[discard_result_off(1)], "%d %d", w0, h0);
            free(bias); free(vs); free(res); free(partial);
            shapes++;
        }
    printf("ok extents %d\n", shapes);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "values")) values();
    else if (argc == 2 && !strcmp(argv[1], "extents")) extents();
    else { fprintf(stderr, "usage: %s values|extents\n", argv[0]); return 2; }
    return 0;
}
