// lqr_pixel.h -- the two forms a pixel takes in the engine, as compile-time policies of the kernels that touch pixels
// (k_energy.hip, k_oneoff.hip).  The seam loop never sees pixels: the DP, the backtrack and the carve work
// on the float planes whatever the pixel.  Depth and image type reach only
//   * the working plane `pix`, the value the energy reads.  PACKED: an 8-bit grey / RGB (+ alpha) carver keeps the pixel's bytes in
//     a u32 and turns them into brightness (or luma) on every read, through a table of v / 255 in LDS.  VALUE: every other carver
//     (16I, 32F, 64F; CMY, CMYK, CMYKA, CUSTOM; more than 4 channels) keeps, in the same plane allocated twice as wide, ONE double
//     per pixel: that value, formed once when the plane is laid out (k_wk_init) with liblqr's normalisation of the depth (v / 255
//     for 8I, v / 65535 for 16I, (double) v for 32F, v for 64F) and the arithmetic of the image type (deep_value).  8 bytes per
//     pixel, whatever the channel count: 32F RGBA is 16, 64F RGBA 32, 32F CMYKA 20.  (PixRead: how a sample is read; PixPacked /
//     PixValue<DEPTH>: how the plane's element is formed from a pixel of the base layout)
//   * the one-off passes on the base layout (BasePx).  8-bit pixels of up to 4 channels move as bytes / one dword and are averaged
//     as such; the DEEP form moves a pixel of any size -- channels x {1, 2, 4, 8} bytes, up to 64 channels: 1 to 512 bytes, odd sizes
//     included (px_move) -- and averages the pixels that inflate creates by the rule of the depth (px_avg_deep).
// Every choice between the forms is made at compile time: each kernel keeps, in either form, the code it would have alone.
#pragma once
#include "lqr_common.h"

typedef GLOBAL_AS double gf64;

// ---------------------------------------------------------------------------
// the working plane: reading a sample
// ---------------------------------------------------------------------------
template <bool VALUE> struct PixRead;
template <> struct PixRead<false> {
    typedef uint32_t T;                 // the plane's element
    const double *n255;
    // the workgroup's table of v / 255 (LDS; a barrier inside: every thread of the workgroup comes here)
    __device__ __forceinline__ void setup(int tid, int nthreads)
    {
        __shared__ double s_n255[256];
        fill_norm255(s_n255, tid, nthreads);
        __syncthreads();
        n255 = s_n255;
    }
    __device__ __forceinline__ double operator()(const gu32 *pix, size_t o, int ch, bool luma) const { return px_bright(pix[o], ch, luma, Norm255Lut{n255}); }
};
template <> struct PixRead<true> {
    typedef double T;
    __device__ __forceinline__ void setup(int, int) {}
    __device__ __forceinline__ double operator()(const gu32 *pix, size_t o, int, bool) const { return ((const gf64 *) pix)[o]; }
};

// E6, one block of EU_ROWS rows by 64 threads: the body of k_emap_update (k_energy.hip, which says what it does) and of the energy
// role of k_carve_u (k_carve.hip), so that the arithmetic exists once.  c = the logical view of the frame AFTER the carve (w wide),
// blk = the row block, tid = 0 .. 63, rd set up by the caller.  ONE_WAVE: the 64 threads are one wave that may be alone in its
// workgroup -- no s_barrier between staging and evaluation then (a wave's LDS operations execute in order)
// SR (lqr_common.h): how the current seam is read -- seam_x and log entry k; older log entries and the frozen planes are read plainly
template <int NRG, int EU_NT, bool VALUE, bool ONE_WAVE, class SR = SeamPlain>
__device__ __forceinline__ void emap_update_block(const GCarver c, const PixRead<VALUE> rd, const DpK p, int w, int h, int stride, int k, int epoch, unsigned blk, int tid, SR sr = SR())
{
    __shared__ double bt[64][EU_NT];
    __shared__ float bb[64][EU_NT];
    __shared__ int slo[64];
    const int y = blk * EU_ROWS + tid - 1;
    const bool row_ok = (y >= 0 && y < h);
    constexpr bool luma = (NRG >= 3);
    int xmin = 0, xmax = -1, lo = 0;
    if (row_ok) {
        nrg_interval(c.seam_x, y, h, w, p.radius, xmin, xmax, sr);
        // samples of this row that rows y-1, y, y+1 will ask for
        int l = xmin - 1, r = xmax + 1;
        if (y > 0) { int a, b; nrg_interval(c.seam_x, y - 1, h, w, p.radius, a, b, sr); if (b >= a) { l = min(l, a); r = max(r, b); } }
        if (y < h - 1) { int a, b; nrg_interval(c.seam_x, y + 1, h, w, p.radius, a, b, sr); if (b >= a) { l = min(l, a); r = max(r, b); } }
        lo = max(l, 0);
        int pos[EU_NT];
#pragma unroll
        for (int i = 0; i < EU_NT; i++) pos[i] = lo + i;
        // undo seams k .. epoch, newest first.  The log entries are loaded eight at a time (unconditionally: indices
        // below `epoch` are clamped and their values replaced by one that moves nothing), so that a row does not wait
        // for one global load per logged seam
        const gi32 *lg = c.seam_log + y;
        for (int j = k; j >= epoch; j -= EU_LOGB) {
            int v[EU_LOGB];
#pragma unroll
            for (int u = 0; u < EU_LOGB; u++) {
                const gi32 *q = lg + (size_t) max(j - u, epoch) * h;
                if (SR::live && u == 0 && j == k) v[u] = sr(q); else v[u] = *q;
            }
#pragma unroll
            for (int u = 0; u < EU_LOGB; u++) {
                const int vu = (j - u >= epoch) ? v[u] : 0x7fffffff;
#pragma unroll
                for (int i = 0; i < EU_NT; i++) pos[i] += (vu <= pos[i]) ? 1 : 0;
            }
        }
        const int wf = w + (k - epoch) + 1;           // width of the frozen frame
#pragma unroll
        for (int i = 0; i < EU_NT; i++) {
            const bool ok = (lo + i <= min(r, w - 1)) && pos[i] < wf;
            const size_t o = (size_t) y * stride + (ok ? pos[i] : 0);
            bt[tid][i] = ok ? rd(c.pix, o, p.ch, luma) : 0.0;
            bb[tid][i] = (ok && c.bias) ? c.bias[o] : 0.0f;
        }
    }
    slo[tid] = lo;
    if (ONE_WAVE) __builtin_amdgcn_wave_barrier(); else __syncthreads();
    if (!row_ok || tid == 0 || tid == 63) return;
    for (int x = xmin; x <= xmax; x++) {
        float e = grad_energy_f<NRG>([&](int xx, int yy) { const int t = tid + (yy - y); return bt[t][xx - slo[t]]; }, x, y, w, h);
        if (c.bias) e = __fadd_rn(e, __fdiv_rn(bb[tid][x - lo], (float) p.w_start));
        c.en[(size_t) y * stride + x] = e;
    }
}

// ---------------------------------------------------------------------------
// the working plane: forming an element from pixel i of the base layout
// ---------------------------------------------------------------------------
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
struct PixPacked {
    typedef uint32_t T;
    typedef int Arg;                    // the launch argument: channels (1 .. 4, a byte each)
    static __device__ __forceinline__ T form(const gu8 *rgb0, size_t i, int ch)
    {
        const gu8 *s = rgb0 + i * ch;
        uint32_t p = 0;
        if (ch == 4) p = *(const gu32 *) s;
        else for (int k = 0; k < ch; k++) p |= (uint32_t) s[k] << (8 * k);
        return p;
    }
};
template <int DEPTH> struct PixValue {  // DEPTH = LqrColDepth (0 = 8I: another image type, or more than 4 channels)
    typedef double T;
    typedef DeepRead Arg;
    static __device__ __forceinline__ T form(const gu8 *rgb0, size_t i, const DeepRead &rd)
    {
        constexpr int bpc = DEPTH == 0 ? 1 : DEPTH == 1 ? 2 : DEPTH == 2 ? 4 : 8;
        return deep_value<DEPTH>(rgb0 + i * rd.ch * bpc, rd);
    }
};

// ---------------------------------------------------------------------------
// the base layout: moving and averaging a pixel
// ---------------------------------------------------------------------------
// one interleaved pixel of `ch` bytes, base layout: RGBA pixels are dword-aligned (rows start at y * w * 4) and move as
// one 32-bit access instead of four byte accesses
__device__ __forceinline__ void px_copy(uint8_t *dst, const uint8_t *src, int ch)
{
    if (ch == 4) *(uint32_t *) dst = *(const uint32_t *) src;
    else for (int k = 0; k < ch; k++) dst[k] = src[k];
}
__device__ __forceinline__ void px_avg(uint8_t *dst, const uint8_t *a, const uint8_t *b, int ch)       // (a + b) / 2 per channel, as integers
{
    if (ch == 4) {
        const uint32_t x = *(const uint32_t *) a, y = *(const uint32_t *) b;
        *(uint32_t *) dst = (x & y) + (((x ^ y) & 0xfefefefeu) >> 1);          // per byte floor((x + y) / 2), no carries across bytes
    } else {
        for (int k = 0; k < ch; k++) dst[k] = (uint8_t) (((int) a[k] + (int) b[k]) / 2);
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
// `bytes` = the job's ch: bytes per pixel; `depth` = the job's LqrColDepth (the 8-bit form has none: a byte per channel)
template <bool DEEP> struct BasePx;
template <> struct BasePx<false> {
    static __device__ __forceinline__ void move(uint8_t *dst, const uint8_t *src, int bytes) { px_copy(dst, src, bytes); }
    static __device__ __forceinline__ void avg(uint8_t *dst, const uint8_t *a, const uint8_t *b, int bytes, int) { px_avg(dst, a, b, bytes); }
};
template <> struct BasePx<true> {
    static __device__ __forceinline__ void move(uint8_t *dst, const uint8_t *src, int bytes) { px_move(dst, src, bytes); }
    static __device__ __forceinline__ void avg(uint8_t *dst, const uint8_t *a, const uint8_t *b, int bytes, int depth) { px_avg_deep(dst, a, b, bytes >> depth, depth); }
};
