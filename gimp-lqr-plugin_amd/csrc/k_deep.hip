// k_deep.hip -- the kernels of carvers that read through the value plane: pixels that are not 8-bit
// (lqr_carver_new_ext: 16I, 32F, 64F), image types beyond grey / RGB with or without alpha (lqr_imagetype.h: CMY, CMYK, CMYKA,
// CUSTOM), more than 4 channels.
// (gfx950 / CDNA4, wave64; see lqr_common.h for the file map)
//
// The seam loop never sees pixels: the DP, the backtrack and the carve work on the float planes whatever the pixel.  Depth and
// image type reach only
//   * the value the energy reads.  An 8-bit grey / RGB (+ alpha) carver keeps its pixels packed in the u32 `pix` plane and turns
//     them into brightness (or luma) on every read; a value-plane carver keeps, in the same plane allocated twice as wide, ONE
//     double per pixel: that value, formed once by k_wk_init_deep with liblqr's normalisation of the depth (v / 255 for 8I,
//     v / 65535 for 16I, (double) v for 32F, v for 64F) and the arithmetic of the image type (deep_value).  k_emap_full_deep,
//     k_emap_update_deep and k_frozen_catchup_deep read and move those doubles where their 8-bit forms unpack a u32.  8 bytes per
//     pixel, whatever the channel count: 32F RGBA is 16, 64F RGBA 32, 32F CMYKA 20.
//   * the one-off passes on the base layout: inflate averages new pixels by the rule of the depth (k_inflate_deep); a transpose
//     of pixels wider than 4 bytes is k_transpose_px, their compaction (flatten, read-out) k_compact_wide / k_compact_jobs_wide;
//     pixels of up to 4 bytes go through the 8-bit kernels, which move them as bytes / one dword.  A pixel is channels x {1, 2, 4, 8}
//     bytes, up to 64 channels: any size from 1 to 512, odd ones included (px_move).
#include "lqr_common.h"
#include "lqr_kernels.h"

typedef GLOBAL_AS double gf64;

// liblqr's lqr_pixel_get_norm: channel k of a pixel as the energy reads it, correctly rounded
template <int DEPTH>
__device__ __forceinline__ double deep_norm(const gu8 *px, int k)
{
    if (DEPTH == 0) return norm255(px[k]);
    if (DEPTH == 1) return __ddiv_rn((double) ((const GLOBAL_AS uint16_t *) px)[k], 65535.0);
    if (DEPTH == 2) return (double) ((const GLOBAL_AS float *) px)[k];
    return ((const gf64 *) px)[k];
}
// liblqr's lqr_carver_read_brightness / _luma for the image type (rd.mode) on the depth's normalised channels, every operation
// rounded individually: px_bright's arithmetic for grey and RGB; CMY(K) turned into RGB first; CUSTOM the mean of the colour
// channels (each lightened by the black channel, the mean inverted if there is one), brightness and luma alike; then times alpha.
// The channels are read from global memory one by one (no private array: none of these kernels may use scratch).
template <int DEPTH>
__device__ __forceinline__ double deep_value(const gu8 *px, const DeepRead &rd)
{
    double b;
    if (rd.mode == RD_GREY) {
        b = deep_norm<DEPTH>(px, 0);
    } else if (rd.mode == RD_CUSTOM) {
        const bool has_black = rd.black >= 0;
        const double kf = __dsub_rn(1.0, has_black ? deep_norm<DEPTH>(px, rd.black) : 0.0);
        double s = 0.0;
        for (int k = 0; k < rd.ch; k++)
            if (k != rd.alpha && k != rd.black) s = __dadd_rn(s, __dsub_rn(1.0, __dmul_rn(__dsub_rn(1.0, deep_norm<DEPTH>(px, k)), kf)));
        s = __ddiv_rn(s, (double) (rd.ch - (rd.alpha >= 0 ? 1 : 0) - (has_black ? 1 : 0)));
        b = has_black ? __dsub_rn(1.0, s) : s;
    } else {
        double r = deep_norm<DEPTH>(px, 0), g = deep_norm<DEPTH>(px, 1), bl = deep_norm<DEPTH>(px, 2);
        if (rd.mode != RD_RGB) {
            r = __dsub_rn(1.0, r); g = __dsub_rn(1.0, g); bl = __dsub_rn(1.0, bl);
            if (rd.mode == RD_CMYK) {
                const double kf = __dsub_rn(1.0, deep_norm<DEPTH>(px, 3));
                r = __dmul_rn(r, kf); g = __dmul_rn(g, kf); bl = __dmul_rn(bl, kf);
            }
        }
        if (rd.luma)
            b = __dadd_rn(__dadd_rn(__dmul_rn(0.2126, r), __dmul_rn(0.7152, g)), __dmul_rn(0.0722, bl));
        else
            b = __ddiv_rn(__dadd_rn(__dadd_rn(r, g), bl), 3.0);
    }
    if (rd.alpha >= 0) b = __dmul_rn(b, deep_norm<DEPTH>(px, rd.alpha));
    return b;
}

// E1 for a flat carver: the value plane (and bias / rigidity planes) from the base layout, as k_wk_init
template <int DEPTH>
__global__ void k_wk_init_deep(const DevCarver *cs, int w, int h, int stride, DeepRead rd)
{
    const GCarver c = gview_phys(cs[blockIdx.z]);
    gf64 *val = (gf64 *) c.pix;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x == 0 && y == 0) { c.flags[FLAG_ORG] = 0; c.flags[FLAG_ORG_PREV] = 0; c.flags[FLAG_SIDE] = 0; }
    if (x >= stride) return;
    const size_t o = (size_t) y * stride + x;
    constexpr int bpc = DEPTH == 0 ? 1 : DEPTH == 1 ? 2 : DEPTH == 2 ? 4 : 8;
    double v = 0.0;
    float b = 0.0f, r = 0.0f;
    if (x < w) {
        v = deep_value<DEPTH>(c.rgb0 + ((size_t) y * w + x) * rd.ch * bpc, rd);
        if (c.bias0) b = c.bias0[(size_t) y * w + x];
        if (c.rig0) r = c.rig0[(size_t) y * w + x];
    }
    val[o] = v;
    if (c.bias) c.bias[o] = b;
    if (c.rig) c.rig[o] = r;
}

// ... and for a carver that is not flat: the pixels without a level, in order (k_wk_init_visible)
template <int DEPTH>
__global__ __launch_bounds__(256) void k_wk_init_visible_deep(const DevCarver *cs, int w0, int h, int stride, DeepRead rd)
{
    __shared__ int s_wave[4];
    const GCarver c = gview_phys(cs[blockIdx.y]);
    gf64 *val = (gf64 *) c.pix;
    constexpr int bpc = DEPTH == 0 ? 1 : DEPTH == 1 ? 2 : DEPTH == 2 ? 4 : 8;
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
            val[ro + rank] = deep_value<DEPTH>(c.rgb0 + (ri + col) * rd.ch * bpc, rd);
            if (c.bias) c.bias[ro + rank] = c.bias0 ? c.bias0[ri + col] : 0.0f;
            if (c.rig) c.rig[ro + rank] = c.rig0 ? c.rig0[ri + col] : 0.0f;
        }
        carry += total;
    }
    for (int x = carry + tid; x < stride; x += 256) {
        val[ro + x] = 0.0;
        if (c.bias) c.bias[ro + x] = 0.0f;
        if (c.rig) c.rig[ro + x] = 0.0f;
    }
}

// E3/E4: k_emap_full on the value plane
template <int NRG>
__global__ void k_emap_full_deep(const DevCarver *cs, DpK p, int w, int h, int stride)
{
    const GCarver c = gview(cs[blockIdx.z]);
    const gf64 *val = (const gf64 *) c.pix;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    float e = grad_energy_f<NRG>([&](int xx, int yy) { return val[(size_t) yy * stride + xx]; }, x, y, w, h);
    if (c.bias) e = __fadd_rn(e, __fdiv_rn(c.bias[(size_t) y * stride + x], (float) p.w_start));
    c.en[(size_t) y * stride + x] = e;
}

// E6: k_emap_update on the value plane (same staging of the samples through the seam log to the frozen frame, same arithmetic)
template <int NRG, int EU_NT>
__global__ __launch_bounds__(64) void k_emap_update_deep(const DevCarver *cs, DpK p, int w, int h, int stride, int k, int epoch)
{
    const GCarver c = gview(cs[blockIdx.y]);
    const gf64 *val = (const gf64 *) c.pix;
    __shared__ double bt[64][EU_NT];
    __shared__ float bb[64][EU_NT];
    __shared__ int slo[64];
    const int tid = threadIdx.x;
    const int y = blockIdx.x * EU_ROWS + tid - 1;
    const bool row_ok = (y >= 0 && y < h);
    int xmin = 0, xmax = -1, lo = 0;
    if (row_ok) {
        nrg_interval(c.seam_x, y, h, w, p.radius, xmin, xmax);
        int l = xmin - 1, r = xmax + 1;
        if (y > 0) { int a, b; nrg_interval(c.seam_x, y - 1, h, w, p.radius, a, b); if (b >= a) { l = min(l, a); r = max(r, b); } }
        if (y < h - 1) { int a, b; nrg_interval(c.seam_x, y + 1, h, w, p.radius, a, b); if (b >= a) { l = min(l, a); r = max(r, b); } }
        lo = max(l, 0);
        int pos[EU_NT];
#pragma unroll
        for (int i = 0; i < EU_NT; i++) pos[i] = lo + i;
        const gi32 *lg = c.seam_log + y;
        for (int j = k; j >= epoch; j -= EU_LOGB) {
            int v[EU_LOGB];
#pragma unroll
            for (int u = 0; u < EU_LOGB; u++) v[u] = lg[(size_t) max(j - u, epoch) * h];
#pragma unroll
            for (int u = 0; u < EU_LOGB; u++) {
                const int vu = (j - u >= epoch) ? v[u] : 0x7fffffff;
#pragma unroll
                for (int i = 0; i < EU_NT; i++) pos[i] += (vu <= pos[i]) ? 1 : 0;
            }
        }
        const int wf = w + (k - epoch) + 1;
#pragma unroll
        for (int i = 0; i < EU_NT; i++) {
            const bool ok = (lo + i <= min(r, w - 1)) && pos[i] < wf;
            const size_t o = (size_t) y * stride + (ok ? pos[i] : 0);
            bt[tid][i] = ok ? val[o] : 0.0;
            bb[tid][i] = (ok && c.bias) ? c.bias[o] : 0.0f;
        }
    }
    slo[tid] = lo;
    __syncthreads();
    if (!row_ok || tid == 0 || tid == 63) return;
    for (int x = xmin; x <= xmax; x++) {
        float e = grad_energy_f<NRG>([&](int xx, int yy) { const int t = tid + (yy - y); return bt[t][xx - slo[t]]; }, x, y, w, h);
        if (c.bias) e = __fadd_rn(e, __fdiv_rn(bb[tid][x - lo], (float) p.w_start));
        c.en[(size_t) y * stride + x] = e;
    }
}

// k_frozen_catchup on the value plane: 8-byte values instead of packed pixels
__global__ __launch_bounds__(256) void k_frozen_catchup_deep(const DevCarver *cs, int from, int to, int w_from, int h, int stride)
{
    const GCarver c = gview(cs[blockIdx.y]);
    extern __shared__ int smc[];
    int *xs = smc;                                  // [to - from]
    uint8_t *rem = (uint8_t *) (smc + (to - from));  // [w_from]
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
    gf64 *vrow = (gf64 *) c.pix + (size_t) y * stride;
    gf32 *brow = c.bias ? c.bias + (size_t) y * stride : (gf32 *) nullptr;
    int carry = 0;
    for (int base = 0; base < w_from; base += 256) {
        const int col = base + tid;
        const bool keep = (col < w_from) && !rem[col];
        const double v = (col < w_from) ? vrow[col] : 0.0;
        const float bv = (brow && col < w_from) ? brow[col] : 0.0f;
        int total;
        const int rank = carry + block_rank_256(keep, s_wave, total);     // barriers inside: all reads of the chunk are done
        if (keep) { vrow[rank] = v; if (brow) brow[rank] = bv; }
        carry += total;
    }
}

// one pixel of `bytes` bytes, in the widest unit that divides it: pixels of a plane start at multiples of their size, so the unit
// is aligned (16-byte accesses for 32F RGBA and 64F grey-alpha / RGBA).  An odd size (8I pixels of 5, 7, 9 .. channels) goes byte
// by byte: its pixels start on odd addresses, and a wider unit would reach past the pixel
__device__ __forceinline__ void px_move(uint8_t *dst, const uint8_t *src, int bytes)
{
    if ((bytes & 15) == 0) for (int k = 0; k < bytes; k += 16) *(u32x4 *) (dst + k) = *(const u32x4 *) (src + k);
    else if ((bytes & 7) == 0) for (int k = 0; k < bytes; k += 8) *(uint64_t *) (dst + k) = *(const uint64_t *) (src + k);
    else if ((bytes & 3) == 0) for (int k = 0; k < bytes; k += 4) *(uint32_t *) (dst + k) = *(const uint32_t *) (src + k);
    else if ((bytes & 1) == 0) for (int k = 0; k < bytes; k += 2) *(uint16_t *) (dst + k) = *(const uint16_t *) (src + k);
    else for (int k = 0; k < bytes; k++) dst[k] = src[k];
}
// a pixel created by enlargement, channel by channel (alpha and black like any other), by liblqr's rule for the depth
// (lqr_carver_inflate): 8I and 16I the integer floor((a + b) / 2); 32F (a + b) * 0.5f in float; 64F (a + b) * 0.5 in double
__device__ __forceinline__ void px_avg_deep(uint8_t *dst, const uint8_t *a, const uint8_t *b, int ch, int depth)
{
    for (int k = 0; k < ch; k++) {
        if (depth == 0) dst[k] = (uint8_t) (((int) a[k] + (int) b[k]) >> 1);
        else if (depth == 1) ((uint16_t *) dst)[k] = (uint16_t) (((int) ((const uint16_t *) a)[k] + (int) ((const uint16_t *) b)[k]) >> 1);
        else if (depth == 2) ((float *) dst)[k] = __fmul_rn(__fadd_rn(((const float *) a)[k], ((const float *) b)[k]), 0.5f);
        else ((double *) dst)[k] = __dmul_rn(__dadd_rn(((const double *) a)[k], ((const double *) b)[k]), 0.5);
    }
}

// E14 for the carvers of a batch that k_inflate does not take: deep ones, 8I ones of more than 4 channels (k_inflate's pass and its fused level self-check; jobs[i].ch = channels)
__global__ __launch_bounds__(256) void k_inflate_deep(const InflateDevX *jobs, int w0, int w1, int l, int max_level, int *dev_err)
{
    __shared__ int s_wave[4];
    extern __shared__ unsigned s_seen[];
    const int n_levels = l - max_level + 1, lvl0 = 2 * max_level - 1;
    for (int i = threadIdx.x; i < (n_levels + 31) / 32; i += 256) s_seen[i] = 0u;
    __syncthreads();
    bool twice = false;
    const InflateDevX jx = jobs[blockIdx.y];
    const InflateDev &j = jx.j;
    const int ch = j.ch, depth = jx.depth, bytes = ch * (depth == 0 ? 1 : depth == 1 ? 2 : depth == 2 ? 4 : 8);
    const int y = blockIdx.x, tid = threadIdx.x;
    const int32_t *vrow = j.vs + (size_t) y * w0;
    const size_t ri = (size_t) y * w0, ro = (size_t) y * w1;
    int carry = 0;
    for (int base = 0; base < w0; base += 256) {
        const int col = base + tid;
        const int v = (col < w0) ? vrow[col] : 0;
        const bool dup = (col < w0) && v != 0 && v <= l + max_level - 1 && v >= 2 * max_level - 1;
        if (dup) twice |= (atomicOr(&s_seen[(v - lvl0) >> 5], 1u << ((v - lvl0) & 31)) >> ((v - lvl0) & 31)) & 1u;
        int total;
        const int rank = carry + block_rank_256(dup, s_wave, total);
        if (col < w0) {
            int z = col + rank;
            const int left = col > 0 ? col - 1 : col;
            if (dup) {
                px_avg_deep(j.nrgb + (ro + z) * bytes, j.rgb + (ri + left) * bytes, j.rgb + (ri + col) * bytes, ch, depth);
                if (j.nbias) j.nbias[ro + z] = __fmul_rn(__fadd_rn(j.bias[ri + left], j.bias[ri + col]), 0.5f);
                if (j.nrig) j.nrig[ro + z] = __fmul_rn(__fadd_rn(j.rig[ri + left], j.rig[ri + col]), 0.5f);
                if (j.nvs) j.nvs[ro + z] = l - v + max_level;
                z++;
            }
            px_move(j.nrgb + (ro + z) * bytes, j.rgb + (ri + col) * bytes, bytes);
            if (j.nbias) j.nbias[ro + z] = j.bias[ri + col];
            if (j.nrig) j.nrig[ro + z] = j.rig[ri + col];
            if (j.nvs) j.nvs[ro + z] = v ? v + l - max_level + 1 : 0;
        }
        carry += total;
    }
    if (dev_err && (twice || (tid == 0 && carry != n_levels))) dev_fail(dev_err, DEVERR_LEVELS);
}

// E11 transpose of pixels wider than 4 bytes (jobs[i].ch = bytes per pixel): one thread per output pixel of a 32 x 32 tile,
// rows of the output written together
__global__ void k_transpose_px(const InflateDev *jobs, int w, int h)
{
    const InflateDev j = jobs[blockIdx.z];
    const int bytes = j.ch;
    const int oy = blockIdx.y * 32 + threadIdx.x;          // output column = old y
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        const int ox = blockIdx.x * 32 + i;                // output row = old x
        if (ox < w && oy < h) {
            const size_t src = (size_t) oy * w + ox, dst = (size_t) ox * h + oy;
            px_move(j.nrgb + dst * bytes, j.rgb + src * bytes, bytes);
            if (j.nbias) j.nbias[dst] = j.bias[src];
            if (j.nrig) j.nrig[dst] = j.rig[src];
        }
    }
}

// E11 / E12 compaction of pixels wider than 4 bytes (flatten and read-out of deep carvers): k_compact / k_compact_jobs with px_move
__global__ __launch_bounds__(256) void k_compact_wide(const uint8_t *rgb, const int32_t *vs, uint8_t *nrgb, int w0, int w, int bytes, int level)
{
    __shared__ int s_wave[4];
    const int y = blockIdx.x, tid = threadIdx.x;
    const int32_t *vrow = vs + (size_t) y * w0;
    const size_t ri = (size_t) y * w0, ro = (size_t) y * w;
    int carry = 0;
    for (int base = 0; base < w0; base += 256) {
        const int col = base + tid;
        const int v = (col < w0) ? vrow[col] : 0;
        const bool keep = (col < w0) && (v == 0 || v >= level);
        int total;
        const int rank = carry + block_rank_256(keep, s_wave, total);
        if (keep && rank < w) px_move(nrgb + (ro + rank) * bytes, rgb + (ri + col) * bytes, bytes);
        carry += total;
    }
}

__global__ __launch_bounds__(256) void k_compact_jobs_wide(const InflateDev *jobs, int w0, int w, int level)
{
    __shared__ int s_wave[4];
    const InflateDev j = jobs[blockIdx.y];
    const int y = blockIdx.x, tid = threadIdx.x, bytes = j.ch;
    const int32_t *vrow = j.vs + (size_t) y * w0;
    const size_t ri = (size_t) y * w0, ro = (size_t) y * w;
    int carry = 0;
    for (int base = 0; base < w0; base += 256) {
        const int col = base + tid;
        const int v = (col < w0) ? vrow[col] : 0;
        const bool keep = (col < w0) && (v == 0 || v >= level);
        int total;
        const int rank = carry + block_rank_256(keep, s_wave, total);
        if (keep && rank < w) {
            px_move(j.nrgb + (ro + rank) * bytes, j.rgb + (ri + col) * bytes, bytes);
            if (j.nbias) j.nbias[ro + rank] = j.bias[ri + col];
            if (j.nrig) j.nrig[ro + rank] = j.rig[ri + col];
        }
        carry += total;
    }
}

// ---- the instantiations the shim launches (lqr_kernels.h declares them)
template __global__ void k_wk_init_deep<0>(const DevCarver *, int, int, int, DeepRead);
template __global__ void k_wk_init_deep<1>(const DevCarver *, int, int, int, DeepRead);
template __global__ void k_wk_init_deep<2>(const DevCarver *, int, int, int, DeepRead);
template __global__ void k_wk_init_deep<3>(const DevCarver *, int, int, int, DeepRead);
template __global__ void k_wk_init_visible_deep<0>(const DevCarver *, int, int, int, DeepRead);
template __global__ void k_wk_init_visible_deep<1>(const DevCarver *, int, int, int, DeepRead);
template __global__ void k_wk_init_visible_deep<2>(const DevCarver *, int, int, int, DeepRead);
template __global__ void k_wk_init_visible_deep<3>(const DevCarver *, int, int, int, DeepRead);
#define INST_EMAP_DEEP(N) template __global__ void k_emap_full_deep<N>(const DevCarver *, DpK, int, int, int); \
    template __global__ void k_emap_update_deep<N, 12>(const DevCarver *, DpK, int, int, int, int, int); \
    template __global__ void k_emap_update_deep<N, 36>(const DevCarver *, DpK, int, int, int, int, int); \
    template __global__ void k_emap_update_deep<N, 68>(const DevCarver *, DpK, int, int, int, int, int);
INST_EMAP_DEEP(0) INST_EMAP_DEEP(1) INST_EMAP_DEEP(2) INST_EMAP_DEEP(3) INST_EMAP_DEEP(4) INST_EMAP_DEEP(5) INST_EMAP_DEEP(6)
