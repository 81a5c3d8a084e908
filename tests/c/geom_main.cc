// The launch geometry (csrc/lqr_geom.h) without a GPU; built by tests/test_launch_geom.py with -Werror under AddressSanitizer and
// UndefinedBehaviorSanitizer.  The header is included alone.  One argument says what to do:
//   values   every size, part offset, index function, grid and limit over the grid of frames below, one line each: "name args... value".  The test
//            holds the same lines as plain arithmetic of its own and compares.
//   extents  every buffer and dynamic-LDS block is allocated on the heap with exactly the stated number of bytes, and the first and the
//            last element its kernel can touch are written, by the kernel's index expression as the kernel's source has it (restated
//            here) -- after the header's offset function, the one the kernel calls, was checked equal to that expression.  AddressSanitizer is the judge; "ok extents <blocks>" at the end.
//   maps     k_band_levels' and k_carve_u's block maps are one-to-one onto what they enumerate.
//   epochs   the epochs of the two spinning kernels are never 0 and fit their field of the tag.
#include "lqr_geom.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static const int WS[] = {2, 63, 64, 65, 4200, 4201, 16384}, HS[] = {2, 37, 62, 63, 2160, 4096}, NS[] = {1, 7, 8, 9, 64};
static const int PXS[] = {2, 3, 4}, PS[] = {1, 7, 16}, SEAMS[] = {1, 31, 32, 33, 128};
static const int VP_REACH_ = 56;        // lqr_plan.h VP_REACH: a chunk of the parallel backtrack is 56 / delta_x rows
static int vp_rows(int delta) { return VP_REACH_ / delta; }
static int vp_chunks(int h, int rows) { return (h - 1 + rows - 1) / rows; }

static void values()
{
    for (int w : WS) {
        printf("plane_stride %d %d\n", w, plane_stride(w));
        printf("lv_tiles %d %d\n", w, lv_tiles(w));
        printf("lv_near_off %d %zu\n", w, lv_near_off(lv_tiles(w)));
        printf("sweep_lds %d %zu\n", w, sweep_lds(w));
        printf("sweep_attr %d %d\n", w, (int) lds_needs_attr(sweep_lds(w)));
        printf("fwd_lds %d %zu\n", w, fwd_lds(w));
        printf("vmap_t_blocks %d %d\n", w, vmap_t_blocks(w));
        printf("vp_col_blocks %d %d\n", w, vp_col_blocks(w));
        printf("sweep_wpad %d %d\n", w, sweep_wpad(w));
        printf("fwd_row_off %d %d\n", w, fwd_row_off(1, w));
        for (int own : {4, 16, 32, 64, 192, 256}) printf("tiles_of %d %d %d\n", w, own, tiles_of(w, own));
        printf("blocks_of %d %zu\n", w, blocks_of((size_t) w * 4099, 256));
        for (int h : HS) printf("plane_elems %d %d %zu\n", w, h, plane_elems(plane_stride(w), h));
        for (int n : NS) printf("lv_exch_words %d %d %zu\n", w, n, exch_words(lv_near_off(lv_tiles(w)), (size_t) n));
        for (int px : PXS) {
            printf("dpp_tiles %d %d %d\n", w, px, dpp_tiles(w, px));
            printf("dpp_near_off %d %d %zu\n", w, px, dpp_near_off(dpp_tiles(w, px), px));
            printf("dpp_ctr_off %d %d %zu\n", w, px, dpp_ctr_off(dpp_tiles(w, px), px));
            for (int n : NS) printf("exch_image_off_dpp %d %d %d %zu\n", w, px, n, exch_image_off((size_t) n - 1, dpp_near_off(dpp_tiles(w, px), px)));
            for (int n : NS) printf("dpp_exch_words %d %d %d %zu\n", w, px, n, exch_words(dpp_near_off(dpp_tiles(w, px), px), (size_t) n));
        }
        for (int n : NS) printf("exch_image_off_lv %d %d %zu\n", w, n, exch_image_off((size_t) n - 1, lv_near_off(lv_tiles(w))));
        for (int k : SEAMS) {
            printf("fc_rem_off %d %d %d\n", w, k, fc_rem_off(5, 5 + k));
            printf("fc_w_from %d %d %d\n", w, k, fc_w_from(5, 5 + k, w));
            printf("vsc_lvl_off %d %d %d\n", w, k, vsc_lvl_off(k));
            printf("fc_lds %d %d %zu\n", w, k, fc_lds(5, 5 + k, fc_w_from(5, 5 + k, w)));
            printf("vsc_lds %d %d %zu\n", w, k, vsc_lds(k, w));
            printf("vsc_attr %d %d %d\n", w, k, (int) lds_needs_attr(vsc_lds(k, w)));
        }
        for (int h : HS)
            for (int delta = 1; delta <= 10; delta++) {
                const int rows = vp_rows(delta), nc = vp_chunks(h, rows), stride = plane_stride(w);
                printf("vp_map_bytes %d %d %d %zu\n", w, h, delta, vp_map_bytes(nc, stride));
                printf("vp_path_bytes %d %d %d %zu\n", w, h, delta, vp_path_bytes(nc, stride, rows));
                printf("vp_solve_lds %d %d %d %zu\n", w, h, delta, vp_solve_lds(nc));
                // the last chunk, quad, step and column: what k_vp_maps writes last and k_vp_solve reads last
                const int R4 = vp_quads(rows), chunk = nc > 0 ? nc - 1 : 0, x = stride - 1;
                printf("vp_quads %d %d %d %d\n", w, h, delta, R4);
                printf("vp_map_row %d %d %d %zu\n", w, h, delta, vp_map_row(chunk, stride));
                printf("vp_path_chunk %d %d %d %zu\n", w, h, delta, vp_path_chunk(chunk, R4, stride));
                printf("vp_path_quad %d %d %d %zu\n", w, h, delta, vp_path_quad(R4 - 1, stride));
                printf("vp_path_step %d %d %d %zu\n", w, h, delta, vp_path_step(chunk, R4, rows - 1, stride, x));
            }
    }
    for (int px : PXS) printf("layout_dpp %d %d\n", px, exch_layout_dpp(px));
    printf("layout_levels %d\n", EXCH_LAYOUT_LEVELS);
    printf("lv_consts %d %d %d %d\n", LV_FLAG_WORDS, LV_OWN, LV_PMAX, VT_LINES);
    for (int h : HS) {
        printf("band_mw_lds %d %zu\n", h, band_mw_lds(h));
        printf("band_tw_lds %d %zu\n", h, band_tw_lds(h));
        printf("band_tw_touchR_off %d %d\n", h, band_tw_touchR_off(h));
        for (int n : NS) {
            printf("cu_grid %d %d %u\n", n, h, cu_grid((unsigned) n, h));
            printf("cv_grid %d %d %u\n", n, h, cv_grid((unsigned) n, h));
            printf("cv_list_words %d %d %zu\n", n, h, cv_list_words(n, h));
        }
        printf("seam_x_elems %d %zu\n", h, seam_x_elems(h));
        for (int k : SEAMS) printf("seam_log_elems %d %d %zu\n", k, h, seam_log_elems(k, h));
        printf("carve_blocks %d %d\n", h, bb_carve_entries(h));
        printf("energy_blocks %d %d\n", h, bb_energy_entries(h));
    }
    // the two limits the planner asks about, at the heights where they turn
    for (int h : {2, 4096, 8192, 8193, 15360, 15361, 16384}) printf("band_fits %d %d %d\n", h, (int) band_mw_fits(h), (int) band_tw_fits(h));
    for (int n : NS) for (int P : PS) printf("lv_grid %d %d %u\n", n, P, lv_grid((size_t) n, P));
    for (int k : SEAMS) {
        printf("inflate_lds %d %zu\n", k, inflate_lds(k + 6, 7));           // l - max_level + 1 = k levels
        printf("vmap_words %d %zu\n", k, vmap_words(k));
        printf("vmap_check_lds %d %zu\n", k, vmap_check_lds(k));
        printf("vmap_check_t_lds %d %zu\n", k, vmap_check_t_lds(k));
    }
    for (int depth : {14336, 14337, 16383}) printf("vmap_t_attr %d %d\n", depth, (int) vmap_t_needs_attr(vmap_check_t_lds(depth)));
    for (size_t bytes : {(size_t) 65536, (size_t) 65537}) printf("lds_attr %zu %d\n", bytes, (int) lds_needs_attr(bytes));
    // a 30 x 20 mask over a 100 x 50 image: inside, over each edge, outside
    for (int t : {0, 1})
        for (int xo : {-5, 0, 40, 90, 200})
            for (int yo : {-3, 0, 45}) {
                const MaskClip k = mask_clip(100, 50, 30, 20, xo, yo, t);
                printf("mask_clip %d %d %d %d %d %d %d %d %d\n", t, xo, yo, k.x0, k.y0, k.x1, k.y1, k.nx, k.ny);
            }
    // the scenario of ADVICE.md's first item: a vp_path sized for delta_x 7 at 2160 rows, then delta_x 1 on the same frame
    {
        const int stride = plane_stride(3840), h = 2160;
        const size_t have = vp_path_bytes(vp_chunks(h, vp_rows(7)), stride, vp_rows(7)), need = vp_path_bytes(vp_chunks(h, vp_rows(1)), stride, vp_rows(1));
        printf("advice_vp_path %zu %zu %d\n", have, need, (int) (have < need));
    }
}

// a heap block of exactly `bytes` bytes; element i of type T is written
struct Block {
    unsigned char *p;
    size_t bytes;
    explicit Block(size_t n) : p((unsigned char *) malloc(n)), bytes(n) { CHECK(p, "malloc %zu", n); }
    ~Block() { free(p); }
    template <class T> void touch(size_t i) { ((volatile T *) p)[i] = (T) 1; }
    template <class T> void touch_at(size_t byte_off, size_t i) { ((volatile T *) (p + byte_off))[i] = (T) 1; }
};
static long g_blocks = 0;

static void extents()
{
    typedef unsigned long long u64;
    for (int w : WS)
        for (int n : NS) {
            // k_dp_tile_p (k_tiles.hip): near_off = ntiles * EX_TILE + 8, ex_img = exch + image * 2 * near_off; a granule at
            // ex_img + tile * EX_TILE + ((j & 1) * 2 + side) * HALO + column (px 3: ex_img + tile * EX_TILE + (j & 1) * OWN + column), its near
            // copy at + near_off; the counter words at ex_img + ntiles * EX_TILE
            for (int px : PXS) {
                const int HALO = dpp_halo(px), OWN = dpp_own(px), EX_TILE = dpp_ex_tile(px), ntiles = (w + OWN - 1) / OWN;
                const size_t near_off = (size_t) ntiles * EX_TILE + 8;
                Block ex(exch_words(dpp_near_off(ntiles, px), (size_t) n) * sizeof(u64));
                g_blocks++;
                CHECK(dpp_tiles(w, px) == ntiles && dpp_near_off(ntiles, px) == near_off && dpp_ctr_off(ntiles, px) == (size_t) ntiles * EX_TILE, "k_dp_tile_p %d px %d", w, px);
                for (int image : {0, n - 1}) {
                    const size_t ex_img = (size_t) image * 2 * near_off;
                    CHECK(exch_image_off((size_t) image, near_off) == ex_img, "image %d", image);
                    const size_t last_gran = px == 3 ? (size_t) (ntiles - 1) * EX_TILE + (size_t) 1 * OWN + (OWN - 1)
                                                     : (size_t) (ntiles - 1) * EX_TILE + (size_t) (1 * 2 + 1) * HALO + (HALO - 1);
                    ex.touch<u64>(ex_img);
                    ex.touch<u64>(ex_img + last_gran);
                    ex.touch<u64>(ex_img + last_gran + near_off);
                    for (int k = 0; k < 8; k++) { ex.touch<u64>(ex_img + (size_t) ntiles * EX_TILE + k); ex.touch<u64>(ex_img + (size_t) ntiles * EX_TILE + k + near_off); }
                }
            }
            // k_band_levels (k_levels.hip): near_off = 4 * LV_PMAX + 2 * ntiles * OWN; flagw = ex_img [2 parities][LV_PMAX slots][2 tiles],
            // gran = ex_img + 4 * LV_PMAX [2 parities][ntiles][OWN]
            {
                const int OWN = 64, ntiles = (w + OWN - 1) / OWN;
                const size_t near_off = (size_t) 4 * LV_PMAX + (size_t) 2 * ntiles * OWN;
                Block ex(exch_words(lv_near_off(ntiles), (size_t) n) * sizeof(u64));
                g_blocks++;
                CHECK(LV_OWN == OWN && lv_tiles(w) == ntiles && lv_near_off(ntiles) == near_off && LV_FLAG_WORDS == 4 * LV_PMAX, "k_band_levels %d", w);
                for (int image : {0, n - 1}) {
                    const size_t ex_img = (size_t) image * 2 * near_off, gran = ex_img + 4 * LV_PMAX;
                    CHECK(exch_image_off((size_t) image, near_off) == ex_img, "image %d", image);
                    const size_t last_flag = (size_t) 1 * 2 * LV_PMAX + 2 * (LV_PMAX - 1) + 1, last_gran = ((size_t) 1 * ntiles + (ntiles - 1)) * OWN + (OWN - 1);
                    ex.touch<u64>(ex_img); ex.touch<u64>(ex_img + last_flag); ex.touch<u64>(ex_img + last_flag + near_off);
                    ex.touch<u64>(gran); ex.touch<u64>(gran + last_gran); ex.touch<u64>(gran + last_gran + near_off);
                }
            }
        }
    // the parallel backtrack (k_backtrack.hip), the frame as wide as its rows are apart: k_vp_maps writes dword chunk * R4 * stride + x
    // + r4 * stride of vp_path and byte chunk * stride + x of vp_map; k_vp_solve reads byte ((chunk * R4 + (r >> 2)) * stride + xs) * 4 +
    // (r & 3) and 16 bytes of vp_map at (c0 + j) * stride + col with col + 15 < stride; s_xs[nchunks + 1]
    for (int w0 : WS)
        for (int h : HS)
            for (int delta = 1; delta <= 10; delta++) {
                const int stride = plane_stride(w0), w = stride, R = vp_rows(delta), R4 = (R + 3) / 4, nchunks = (h - 1 + R - 1) / R;
                Block map(vp_map_bytes(nchunks, stride)), path(vp_path_bytes(nchunks, stride, R)), xs(vp_solve_lds(nchunks));
                g_blocks += 3;
                map.touch<int8_t>(0); path.touch<uint32_t>(0); xs.touch<int>(0); xs.touch<int>((size_t) nchunks);
                if (nchunks < 1) continue;
                const int chunk = nchunks - 1, x = w - 1, r4 = R4 - 1, r = R - 1;
                CHECK(vp_quads(R) == R4 && vp_map_row(chunk, stride) + x == (size_t) chunk * stride + x, "vp_map %d %d %d", w, h, delta);
                CHECK(vp_path_chunk(chunk, R4, stride) + x + vp_path_quad(r4, stride) == (size_t) chunk * R4 * stride + x + (size_t) r4 * stride, "vp_path dword %d %d %d", w, h, delta);
                CHECK(vp_path_step(chunk, R4, r, stride, x) == (((size_t) chunk * R4 + (r >> 2)) * stride + x) * 4 + (r & 3), "vp_path byte %d %d %d", w, h, delta);
                map.touch<int8_t>((size_t) chunk * stride + x);
                for (int b = 0; b < 16; b++) map.touch<int8_t>((size_t) chunk * stride + (stride - 16) + b);
                path.touch<uint32_t>((size_t) chunk * R4 * stride + x + (size_t) r4 * stride);
                path.touch<int8_t>((((size_t) chunk * R4 + (r >> 2)) * stride + x) * 4 + (r & 3));
            }
    for (int w : WS)
        for (int k : SEAMS) {
            // k_frozen_catchup (k_energy.hip): xs = smc [to - from], rem = (uint8_t *) (smc + (to - from)) [w_from]
            {
                const int from = 5, to = 5 + k, w_from = w + (to - from);
                Block lds(fc_lds(from, to, fc_w_from(from, to, w)));
                g_blocks++;
                CHECK(fc_rem_off(from, to) == to - from && fc_w_from(from, to, w) == w_from, "k_frozen_catchup %d %d", w, k);
                lds.touch<int>(0); lds.touch<int>((size_t) (to - from) - 1);
                lds.touch_at<uint8_t>((size_t) (to - from) * sizeof(int), 0); lds.touch_at<uint8_t>((size_t) (to - from) * sizeof(int), (size_t) w_from - 1);
            }
            // k_vs_commit (k_oneoff.hip): xs = smi [n_seams], lvl = smi + n_seams [wc0]
            {
                Block lds(vsc_lds(k, w));
                g_blocks++;
                CHECK(vsc_lvl_off(k) == k, "k_vs_commit %d", k);
                lds.touch<int>(0); lds.touch<int>((size_t) k - 1); lds.touch<int>((size_t) k); lds.touch<int>((size_t) k + w - 1);
            }
        }
    for (int k : SEAMS) {
        // k_inflate: s_seen[(n_levels + 31) / 32]; k_vmap_check: s_seen[(depth + 31) / 32]; k_vmap_check_t: s_seen[c * words + ((v - 1) >> 5)], c < VT_LINES
        Block inf(inflate_lds(k + 6, 7)), vc(vmap_check_lds(k)), vt(vmap_check_t_lds(k));
        g_blocks += 3;
        const int words = (k + 31) / 32;
        CHECK(vmap_words(k) == (size_t) words && VT_LINES == 32, "k_vmap_check %d", k);
        inf.touch<unsigned>(0); inf.touch<unsigned>((size_t) words - 1);
        vc.touch<unsigned>(0); vc.touch<unsigned>((size_t) ((k - 1) >> 5));
        vt.touch<unsigned>(0); vt.touch<unsigned>((size_t) (32 - 1) * words + ((k - 1) >> 5));
    }
    for (int h : HS) {
        // k_band_update_mw: s_touch[h]; k_band_update_tw: s_touch = s_tw, s_touchR = s_tw + h
        Block mw(band_mw_lds(h)), tw(band_tw_lds(h));
        g_blocks += 2;
        CHECK(band_tw_touchR_off(h) == h, "k_band_update_tw %d", h);
        mw.touch<int>(0); mw.touch<int>((size_t) h - 1);
        tw.touch<int>(0); tw.touch<int>((size_t) h - 1); tw.touch<int>((size_t) h); tw.touch<int>((size_t) h + h - 1);
        // seam_x[y], y < h; the seam log: logp = seam_log + log_index * h, logp[y]
        {
            Block sx(seam_x_elems(h) * sizeof(int));
            g_blocks++;
            sx.touch<int>(0); sx.touch<int>((size_t) h - 1);
            for (int k : SEAMS) {
                Block lg(seam_log_elems(k, h) * sizeof(int));
                g_blocks++;
                lg.touch<int>(0); lg.touch<int>((size_t) (k - 1) * h + (h - 1));
            }
        }
        // k_carve_v's work list: two tail words, then an entry per consumer workgroup
        for (int n : NS) {
            Block wl(cv_list_words(n, h) * sizeof(u64));
            g_blocks++;
            wl.touch<u64>(0); wl.touch<u64>(1);
            wl.touch<u64>((size_t) 2 + (size_t) n * ((h + 3) / 4 + (h + 61) / 62) - 1);
        }
    }
    for (int w : WS) {
        // k_dp_sweep: wpad = (w + 3) & ~3, prev = sm, cur = sm + wpad; k_fwd_seam: s_m + parity * L
        Block sw(sweep_lds(w)), fw(fwd_lds(w));
        g_blocks += 2;
        const int wpad = (w + 3) & ~3;
        CHECK(sweep_wpad(w) == wpad && fwd_row_off(1, w) == 1 * w && fwd_row_off(0, w) == 0, "k_dp_sweep / k_fwd_seam %d", w);
        sw.touch<float>(0); sw.touch<float>((size_t) wpad - 1); sw.touch<float>((size_t) wpad); sw.touch<float>((size_t) wpad + wpad - 1);
        fw.touch<float>(0); fw.touch<float>((size_t) 1 * w + w - 1);
        // a working plane: rows `stride` apart, the row below the frame readable
        for (int h : HS) {
            const int stride = plane_stride(w);
            Block pl(plane_elems(stride, h));
            g_blocks++;
            pl.touch<int8_t>(0); pl.touch<int8_t>((size_t) h * stride + stride - 1);
        }
    }
    printf("ok extents %ld\n", g_blocks);
}

static void maps()
{
    long checked = 0;
    for (int n = 1; n <= 70; n++)
        for (int P = 1; P <= 16; P++) {
            std::vector<int> seen((size_t) n * P, 0);
            const unsigned grid = lv_grid((size_t) n, P);
            for (unsigned b = 0; b < grid + 64; b++) {
                const LvBlock k = lv_block((int) b, P);
                // k_band_levels' own text (tests/test_launch_geom.py holds the kernel's source to it)
                const int b_xcd = (int) b & 7, b_k = (int) b >> 3;
                CHECK(k.slot == b_k % P && k.image == (b_k / P) * 8 + b_xcd, "block %u of (%d, %d): the kernel's text says otherwise", b, n, P);
                CHECK(k.image >= 0 && k.slot >= 0 && k.slot < P, "block %u of (%d, %d)", b, n, P);
                if (b >= grid) { CHECK(k.image >= n, "block %u beyond the grid of (%d, %d) maps to image %d", b, n, P, k.image); continue; }
                if (k.image < n) seen[(size_t) k.image * P + k.slot]++;
            }
            for (size_t i = 0; i < seen.size(); i++) CHECK(seen[i] == 1, "(%d, %d): image %zu slot %zu %d times", n, P, i / P, i % P, seen[i]);
            checked++;
        }
    for (int n : {1, 8, 64})
        for (int h : {2, 4, 5, 62, 63, 2160}) {
            const int eblk = (h + 61) / 62, rblk = (h + 3) / 4;
            std::vector<int> e((size_t) n * eblk, 0), q((size_t) n * rblk, 0);
            const unsigned grid = cu_grid((unsigned) n, h);
            CHECK(grid == (unsigned) (n * eblk + n * rblk) && cu_energy_blocks(n, h) == n * eblk, "(%d, %d): grid %u", n, h, grid);
            for (unsigned b = 0; b < grid; b++) {
                const CuBlock k = cu_block(b, n, h);
                {   // k_carve_u's own text (tests/test_launch_geom.py holds the kernel's source to it)
                    const int ne = n * eblk;
                    if ((int) b < ne) { const int img = b / eblk, blk = b - img * eblk; CHECK(k.energy && k.image == img && k.index == blk, "(%d, %d): energy block %u", n, h, b); }
                    else { const int cb = b - ne, img = cb / rblk, rb = cb - img * rblk; CHECK(!k.energy && k.image == img && k.index == rb, "(%d, %d): carve block %u", n, h, b); }
                }
                CHECK(k.energy == (b < (unsigned) (n * eblk)), "(%d, %d): energy blocks first, block %u", n, h, b);
                CHECK(k.image >= 0 && k.image < n && k.index >= 0 && k.index < (k.energy ? eblk : rblk), "(%d, %d): block %u -> %d %d", n, h, b, k.image, k.index);
                (k.energy ? e : q)[(size_t) k.image * (k.energy ? eblk : rblk) + k.index]++;
            }
            for (int c : e) CHECK(c == 1, "(%d, %d): an energy block %d times", n, h, c);
            for (int c : q) CHECK(c == 1, "(%d, %d): a row-quad %d times", n, h, c);
            checked++;
        }
    printf("ok maps %ld\n", checked);
}

static void epochs()
{
    const long long dpp_mod = (1ll << DPP_EPOCH_BITS) - 2, lv_mod = (1ll << LV_EPOCH_BITS) - 2;
    for (long long mod : {dpp_mod, lv_mod})
        for (long long c : {0ll, 1ll, mod - 1, mod, mod + 1, 2147483647ll}) {
            const int d = dpp_epoch((int) c), l = lv_epoch((int) c);
            CHECK(d > 0 && d < (1 << DPP_EPOCH_BITS), "k_dp_tile_p: launch %lld -> epoch %d", c, d);
            CHECK(l > 0 && l < (1 << LV_EPOCH_BITS), "k_band_levels: launch %lld -> epoch %d", c, l);
            printf("epoch %lld %d %d\n", c, d, l);
        }
    printf("ok epochs %d %d\n", DPP_EPOCH_BITS, LV_EPOCH_BITS);
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "values")) values();
    else if (!strcmp(what, "extents")) extents();
    else if (!strcmp(what, "maps")) maps();
    else if (!strcmp(what, "epochs")) epochs();
    else { fprintf(stderr, "usage: geom_main values | extents | maps | epochs\n"); return 2; }
    return 0;
}
