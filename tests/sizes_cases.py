"""The cases of the many-sizes read-out (include/lqr_sizes.h) that are judged against the numpy model of a loaded map
(vmap_cases.model, which tests/test_vmap_abi.py pins to the genuine liblqr): seeded permutation maps at the boundaries the kernels of
csrc/k_sizes.hip have, and a vectorised form of the model (the recorded one walks every pixel in Python) that
tests/test_sizes_model.py holds equal to it without a GPU.

A case is stated in the carver's frame: `line` pixels per line of the map's direction, `lines` of them, a map of depth d.  The base
layout is line + d columns wide: that is the width k_compact_sizes walks in chunks of CHUNK columns (four per lane), the first chunk
starting up to three columns early so that loads are 16-byte aligned -- widths around 256 (one wave's share), around CHUNK, rows whose
start is and is not a multiple of four columns.  k_transpose_sizes works in tiles of 32 x 32."""
import numpy as np

import coldepth_cases as CD
import vmap_cases as VC

CHUNK = 1024            # csrc/lqr_common.h SZ_CHUNK
MAX_JOBS = 64           # csrc/lqr_common.h SZ_MAX_JOBS
# bytes per pixel -> (channels, LqrColDepth, lqrx_set_max_channels or None)
PIXELS = {1: (1, 0, None), 2: (2, 0, None), 3: (3, 0, None), 4: (4, 0, None), 5: (5, 0, 8), 8: (4, 1, None), 16: (4, 2, None), 32: (4, 3, None)}


def fast_model(img, m, size):
    """vmap_cases.model, vectorised: the image (h x w x ch) under map m at `size` in the map's direction"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    data, d = np.asarray(m["data"]), int(m["depth"])
    if m["orientation"]:
        return np.ascontiguousarray(np.swapaxes(fast_model(np.swapaxes(img, 0, 1), dict(data=data.T, depth=d, orientation=0), size), 0, 1))
    h, n, ch = img.shape
    k = size - n
    assert -d <= k <= d
    if k <= 0:
        return np.ascontiguousarray(img[(data == 0) | (data > -k)].reshape(h, size, ch))
    dup = (data >= 1) & (data <= k)
    pos = np.arange(n)[None, :] + np.cumsum(dup, axis=1)
    rows = np.broadcast_to(np.arange(h)[:, None], (h, n))
    out = np.empty((h, size, ch), img.dtype)
    out[rows, pos] = img
    left = np.concatenate([img[:, :1], img[:, :-1]], axis=1)
    out[rows[dup], pos[dup] - 1] = VC.average(left, img)[dup]
    return out


def image_of(case):
    ch, depth, _ = PIXELS[case["px"]]
    w, h = (case["line"], case["lines"]) if case["o"] == 0 else (case["lines"], case["line"])
    rng = np.random.default_rng([31, w, h, ch, depth])
    return CD.to_depth(rng, CD.base_image(rng, w, h, ch), depth)


def map_of(case):
    w, h = (case["line"], case["lines"]) if case["o"] == 0 else (case["lines"], case["line"])
    return VC.perm_map(7000 + case["d"], w, h, case["d"], case["o"])


def sizes_of(case):
    """the request: `how` is "one", "full" (every size of [lo, hi], ascending), an int K (K distinct sizes, shuffled) or "repeats" (40
    sizes drawn with repetition)"""
    lo, hi = case["line"] - case["d"], case["line"] + case["d"]
    rng = np.random.default_rng([32, case["line"], case["lines"], case["d"]])
    every = np.arange(lo, hi + 1)
    how = case["how"]
    if how == "one":
        return [int(rng.choice(every))]
    if how == "full":
        return [int(s) for s in every]
    if how == "repeats":
        return [int(s) for s in rng.choice(every[::3], 40)]
    assert isinstance(how, int) and how <= len(every)
    return [int(s) for s in rng.permutation(every)[:how]]


def cases():
    out = []

    def add(w0, lines, d, o, px, how, offsets):
        out.append(dict(name="w0_%d-lines_%d-d%d-o%d-px%d-%s" % (w0, lines, d, o, px, how), line=w0 - d, lines=lines, d=d, o=o, px=px, how=how,
                        offsets=offsets))

    # RGBA, the form with 16-byte loads and dword stores (offset 0) or byte stores (offset one sample): every base width and line
    # count of the list, both directions, every kind of request
    shapes = [(255, 1), (256, 2), (257, 31), (CHUNK - 1, 32), (CHUNK, 33), (CHUNK + 1, 65)]
    hows = ["one", MAX_JOBS, MAX_JOBS + 1, "repeats", "full", MAX_JOBS + 1]
    for i, (w0, lines) in enumerate(shapes):
        for o in (0, 1):
            add(w0, lines, 40, o, 4, hows[(i + o) % len(hows)], (0, 1))
    # the line counts again at the other widths (a row's start is a multiple of four columns or not: the first chunk's early start)
    for w0, lines in ((CHUNK + 1, 1), (CHUNK - 1, 2), (257, 65), (255, 33)):
        add(w0, lines, 33, 0, 4, "full", (1,))
        add(w0, lines, 33, 1, 4, MAX_JOBS + 1, (0,))
    # every pixel size, both directions, the full range, outputs one sample off an aligned address; two chunks of columns for the narrow
    # and the 16-byte pixels
    for px in PIXELS:
        for o in (0, 1):
            add(CHUNK + 1 if px in (3, 16) else 257, 33, 12, o, px, "full", (1,) if px != 16 else (0, 1))
    return out
