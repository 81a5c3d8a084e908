"""The geometry of every launch (gimp-lqr-plugin_amd/csrc/lqr_geom.h: sizes of buffers, dynamic-LDS blocks and grids, and the maps
by which a kernel finds its way in them) without a GPU.  tests/c/geom_main.cc includes the header alone and is compiled with -Werror
under AddressSanitizer and UndefinedBehaviorSanitizer, as tests/test_plan.py does with its program.  The values are compared with the
expressions the launch shim held before the header existed, written out below as plain arithmetic; the extents are judged by
AddressSanitizer; the grid maps and the epochs by the program's own checks."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")

WS = (2, 63, 64, 65, 4200, 4201, 16384)
HS = (2, 37, 62, 63, 2160, 4096)
NS = (1, 7, 8, 9, 64)
PXS = (2, 3, 4)
PS = (1, 7, 16)
SEAMS = (1, 31, 32, 33, 128)
DELTAS = range(1, 11)


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_geom_"), "geom_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "c", "geom_main.cc"), "-o", exe], check=True)
    return exe


def run(what):
    r = subprocess.run([program(), what], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().split("\n")


# ---- what the launch shim computed at each site before lqr_geom.h, as plain arithmetic ---------------------------------------------
def dpp_own(px):            # columns a tile of k_dp_tile_p owns: 64 lanes of 2 / 2 / 4 pixels less 16 / 24 / 16 halo lanes on each side
    return {2: 64, 3: 32, 4: 128}[px]


def dpp_ex_tile(px):        # granules a tile publishes: 2 parities x 2 sides x halo columns; px 3: 2 parities x own columns
    return {2: 2 * 2 * 32, 3: 2 * 32, 4: 2 * 2 * 64}[px]


def stride_of(w):           # ensure_working
    return ((w + 16) + 63) & ~63


def vp(h, delta):           # plan_seam_step: rows per chunk, chunks
    rows = 56 // delta
    return rows, (h - 1 + rows - 1) // rows


def expected():
    E = {}

    def put(name, *args_value):
        E[(name,) + tuple(args_value[:-1])] = int(args_value[-1])
    for w in WS:
        put("plane_stride", w, stride_of(w))
        put("lv_tiles", w, (w + 63) // 64)
        put("lv_near_off", w, 4 * 16 + 2 * ((w + 63) // 64) * 64)
        put("sweep_lds", w, 2 * ((w + 3) & ~3) * 4)
        put("sweep_attr", w, 2 * ((w + 3) & ~3) * 4 > 64 * 1024)
        put("fwd_lds", w, 2 * w * 4)
        put("vmap_t_blocks", w, (w + 32 - 1) // 32)
        put("vp_col_blocks", w, (w + 255) // 256)
        put("sweep_wpad", w, (w + 3) & ~3)
        put("fwd_row_off", w, 1 * w)
        for own in (4, 16, 32, 64, 192, 256):
            put("tiles_of", w, own, (w + own - 1) // own)
        put("blocks_of", w, (w * 4099 + 255) // 256)
        for h in HS:
            put("plane_elems", w, h, stride_of(w) * (h + 1) + 1024)
        for n in NS:
            put("lv_exch_words", w, n, 2 * (4 * 16 + 2 * ((w + 63) // 64) * 64) * n)
        for px in PXS:
            ntiles = (w + dpp_own(px) - 1) // dpp_own(px)
            put("dpp_tiles", w, px, ntiles)
            put("dpp_near_off", w, px, ntiles * dpp_ex_tile(px) + 8)
            put("dpp_ctr_off", w, px, ntiles * dpp_ex_tile(px))
            for n in NS:        # the last image's base: blockIdx.y * 2 * near_off
                put("exch_image_off_dpp", w, px, n, (n - 1) * 2 * (ntiles * dpp_ex_tile(px) + 8))
            for n in NS:
                put("dpp_exch_words", w, px, n, 2 * (ntiles * dpp_ex_tile(px) + 8) * n)
        for n in NS:
            put("exch_image_off_lv", w, n, (n - 1) * 2 * (4 * 16 + 2 * ((w + 63) // 64) * 64))
        for k in SEAMS:
            frm, to = 5, 5 + k
            w_from = w + (to - frm)
            put("fc_rem_off", w, k, to - frm)           # rem = smc + (to - from)
            put("fc_w_from", w, k, w_from)
            put("vsc_lvl_off", w, k, k)                 # lvl = smi + n_seams
            put("fc_lds", w, k, (to - frm) * 4 + w_from + 16)
            put("vsc_lds", w, k, (k + w) * 4)
            put("vsc_attr", w, k, (k + w) * 4 > 64 * 1024)
        for h in HS:
            for delta in DELTAS:
                rows, nchunks = vp(h, delta)
                need = (nchunks + 1) * stride_of(w) + 64
                put("vp_map_bytes", w, h, delta, need)
                put("vp_path_bytes", w, h, delta, need * 4 * ((rows + 3) // 4))
                put("vp_solve_lds", w, h, delta, (nchunks + 2) * 4)
                # k_vp_maps / k_vp_solve at the parent, for the last chunk, quad, step and column
                R4, chunk, stride, x, r = (rows + 3) // 4, max(nchunks - 1, 0), stride_of(w), stride_of(w) - 1, rows - 1
                put("vp_quads", w, h, delta, R4)
                put("vp_map_row", w, h, delta, chunk * stride)
                put("vp_path_chunk", w, h, delta, chunk * R4 * stride)
                put("vp_path_quad", w, h, delta, (R4 - 1) * stride)
                put("vp_path_step", w, h, delta, ((chunk * R4 + (r >> 2)) * stride + x) * 4 + (r & 3))
    for px in PXS:
        put("layout_dpp", px, px)
    put("layout_levels", 103)
    for h in HS:
        put("band_mw_lds", h, h * 4)
        put("band_tw_lds", h, 2 * h * 4)
        put("band_tw_touchR_off", h, h)                 # s_touchR = s_tw + h
        for n in NS:
            put("cu_grid", n, h, n * ((h + 62 - 1) // 62) + n * ((h + 3) // 4))
            put("cv_grid", n, h, n + n * ((h + 3) // 4 + (h + 62 - 1) // 62))
            put("cv_list_words", n, h, 2 + n * ((h + 3) // 4 + (h + 62 - 1) // 62))
        put("seam_x_elems", h, h + 8)
        for k in SEAMS:
            put("seam_log_elems", k, h, k * h)
        put("carve_blocks", h, (h + 3) // 4)
        put("energy_blocks", h, (h + 62 - 1) // 62)
    for n in NS:
        for P in PS:
            put("lv_grid", n, P, 8 * ((n + 7) // 8) * P)
    for k in SEAMS:
        put("inflate_lds", k, ((k + 31) // 32 + 1) * 4)
        put("vmap_words", k, (k + 31) // 32)
        put("vmap_check_lds", k, ((k + 31) // 32) * 4)
        put("vmap_check_t_lds", k, 32 * ((k + 31) // 32) * 4)
    for depth in (14336, 14337, 16383):
        put("vmap_t_attr", depth, 32 * ((depth + 31) // 32) * 4 > 56 * 1024)
    for nbytes in (65536, 65537):
        put("lds_attr", nbytes, nbytes > 64 * 1024)
    return E


def test_header_compiles_alone_as_plain_cxx():
    """csrc/lqr_geom.h by itself, no HIP and no other header of the engine in front of it"""
    with tempfile.TemporaryDirectory(prefix="lqr_geom_h_") as tmp:
        src = os.path.join(tmp, "alone.cc")
        with open(src, "w") as f:
            f.write('#include "lqr_geom.h"\nstatic_assert(exch_words(dpp_near_off(1, 2), 1) == 2 * (128 + 8), "one tile of one image");\nint main() { return 0; }\n')
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + CSRC, src], check=True)


def test_every_size_is_what_the_launch_sites_computed():
    got = {}
    band_fits = {}
    advice = None
    masks = 0
    for line in run("values"):
        f = line.split()
        if f[0] == "band_fits":
            band_fits[int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "advice_vp_path":
            advice = tuple(int(x) for x in f[1:])
        elif f[0] == "lv_consts":          # gran = ex_img + 4 * LV_PMAX, OWN = 64, LV_PMAX = 16, VT_LINES 32
            assert [int(x) for x in f[1:]] == [4 * 16, 64, 16, 32], line
        elif f[0] == "mask_clip":
            t, xo, yo = (int(x) for x in f[1:4])
            wt, ht = (50, 100) if t else (100, 50)
            x1, y1 = max(xo, 0), max(yo, 0)
            assert [int(x) for x in f[4:]] == [min(xo, 0), min(yo, 0), x1, y1, min(wt, 30 + xo) - x1, min(ht, 20 + yo) - y1], line
            masks += 1
        else:
            key = (f[0],) + tuple(int(x) for x in f[1:-1])
            assert key not in got, key
            got[key] = int(f[-1])
    want = expected()
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:10]
    wrong = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, wrong[:10]
    assert len(want) > 1500 and masks == 2 * 5 * 3
    # the planner's two conditions (lqr_plan.h before: h * sizeof(int) <= 60 * 1024, 2 * h * sizeof(int) <= 64 * 1024)
    assert band_fits == {h: (int(h * 4 <= 60 * 1024), int(2 * h * 4 <= 64 * 1024)) for h in (2, 4096, 8192, 8193, 15360, 15361, 16384)}
    # ADVICE.md, first item: the pair sized at delta_x 7 (8-row chunks, 2 dwords a column) is too small for delta_x 1 (56 rows, 14 dwords)
    stride = stride_of(3840)
    have, need = (270 + 1) * stride + 64, (39 + 1) * stride + 64
    assert advice == (have * 4 * 2, need * 4 * 14, 1)


def test_every_extent_holds_what_its_kernel_touches():
    last = run("extents")[-1].split()
    # exchange areas 7 x 5 x (3 + 1), backtrack 7 x 6 x 10 x 3, catch-up and commit 7 x 5 x 2, level bits 5 x 3, band kernels, seams, logs and
    # work lists 6 x (2 + 1 + 5 + 5), sweeps and planes 7 x (2 + 6)
    assert last == ["ok", "extents", str(140 + 1260 + 70 + 15 + 78 + 56)], last


def test_grid_maps_are_one_to_one():
    """lv_block and cu_block, and the two kernels that keep the map in their own text: tests/c/geom_main.cc restates that text and checks
    the functions against it block by block; here the kernels' sources are held to the same text"""
    assert run("maps")[-1] == "ok maps %d" % (70 * 16 + 3 * 6)
    levels = open(os.path.join(CSRC, "k_levels.hip")).read()
    assert "const int b_xcd = (int) blockIdx.x & 7, b_k = (int) blockIdx.x >> 3;" in levels
    assert "b_k % P, image = (dbg & 8) ? (int) blockIdx.x / P : (b_k / P) * 8 + b_xcd;" in levels
    carve = open(os.path.join(CSRC, "k_carve.hip")).read()
    assert "const int eblk = bb_energy_entries(h), ne = n * eblk;" in carve
    assert "const int img = blockIdx.x / eblk, blk = blockIdx.x - img * eblk;" in carve
    assert "const int rblk = bb_carve_entries(h), cb = blockIdx.x - ne, img = cb / rblk, rb = cb - img * rblk;" in carve


def test_epochs_fit_their_field_of_the_tag():
    lines = run("epochs")
    assert lines[-1] == "ok epochs 19 22"         # 31 - DPP_BLK_BITS (12); 32 - the 10 bits of level + 1
    rows = [tuple(int(x) for x in ln.split()[1:]) for ln in lines[:-1]]
    assert len(rows) == 12
    for c, d, l in rows:
        assert d == 1 + c % ((1 << (31 - 12)) - 2) and l == 1 + c % ((1 << 22) - 2), (c, d, l)
        assert 0 < d < 1 << 19 and 0 < l < 1 << 22
