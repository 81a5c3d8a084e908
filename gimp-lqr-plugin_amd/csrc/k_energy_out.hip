// k_energy_out.hip -- liblqr's energy read-outs (include/lqr_energy.h): lqr_carver_get_true_energy, lqr_carver_get_energy and
// lqr_carver_get_energy_image on the energy plane `en` that k_emap_full has just built in the carver's frame.  Two kernels:
//   k_energy_range   squash every value, s = 1 / (1 + 1 / e) (e >= 0) or -1 / (1 - 1 / e) (e < 0), and reduce min and max of s to
//                    one pair per workgroup (lanes by wave shuffles, waves through LDS; min and max do not depend on the order, so
//                    the pair is exact; no atomics)
//   k_energy_plane / k_energy_out<TYPE, DEPTH>
//                    every workgroup folds the pairs into e_min / e_max (seeds FLT_MAX and 0, as liblqr's), squashes its own tile
//                    again, normalises it, and stores floats (k_energy_plane) or pixels of the type and depth the caller asked for
//                    (k_energy_out) in IMAGE orientation.  A carver in orientation 1 holds the plane transposed: its tile goes
//                    through LDS (rows of EO_TILE + 1 floats: the column-wise read is conflict-free), so that the read of the
//                    plane and the write of the picture both run along rows.
// Arithmetic.  The float forms are float-only code: every operation rounded to float (PIC = false).  liblqr's picture loop is its
// own code, mixed float / double, pinned as the 53-bit build evaluates it (PIC = true): the squash in double and rounded to float
// ONCE, e_min / e_max over those floats, the normalisation (s - e_min) / (e_max - e_min) and 1 - e in double, 0 where e_max == e_min.
// The true energy is k_energy_plane without squash and normalisation.
#include "lqr_common.h"
#include "lqr_kernels.h"
#include <float.h>

__device__ __forceinline__ float eo_squash(float e)
{
    if (e >= 0.0f) return __fdiv_rn(1.0f, __fadd_rn(1.0f, __fdiv_rn(1.0f, e)));
    return __fdiv_rn(-1.0f, __fsub_rn(1.0f, __fdiv_rn(1.0f, e)));
}

// the picture loop's squash: the same three operations in double, rounded to float once
__device__ __forceinline__ float eo_squash_pic(float ef)
{
    const double e = (double) ef;
    if (ef >= 0.0f) return __double2float_rn(__ddiv_rn(1.0, __dadd_rn(1.0, __ddiv_rn(1.0, e))));
    return __double2float_rn(__ddiv_rn(-1.0, __dsub_rn(1.0, __ddiv_rn(1.0, e))));
}

// min and max over the workgroup's 256 threads; every thread returns with both
__device__ __forceinline__ void eo_block_range(float &mn, float &mx, float (*s_r)[2])
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, d));
        mx = fmaxf(mx, __shfl_xor(mx, d));
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_r[wv][0] = mn; s_r[wv][1] = mx; }
    __syncthreads();
    mn = fminf(fminf(s_r[0][0], s_r[1][0]), fminf(s_r[2][0], s_r[3][0]));
    mx = fmaxf(fmaxf(s_r[0][1], s_r[1][1]), fmaxf(s_r[2][1], s_r[3][1]));
}

// a unit is EO_CHUNK consecutive pixels of one frame row; workgroup g takes units g, g + gridDim.x, ...
template <bool PIC>
__global__ __launch_bounds__(256) void k_energy_range(const DevCarver *cs, int w, int h, int stride, float *partials)
{
    __shared__ float s_r[4][2];
    const GCarver c = gview(cs[0]);
    const int chunks = (w + EO_CHUNK - 1) / EO_CHUNK, units = h * chunks;
    float mn = FLT_MAX, mx = 0.0f;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        const int y = u / chunks, x0 = (u - y * chunks) * EO_CHUNK;
        const gf32 *row = c.en + (size_t) y * stride;
#pragma unroll
        for (int k = 0; k < EO_CHUNK / 256; k++) {
            const int x = x0 + k * 256 + (int) threadIdx.x;
            if (x < w) {
                const float s = PIC ? eo_squash_pic(row[x]) : eo_squash(row[x]);
                mn = fminf(mn, s);
                mx = fmaxf(mx, s);
            }
        }
    }
    eo_block_range(mn, mx, s_r);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = mn; partials[2 * blockIdx.x + 1] = mx; }
}
template __global__ void k_energy_range<false>(const DevCarver *, int, int, int, float *);
template __global__ void k_energy_range<true>(const DevCarver *, int, int, int, float *);

// ---- the pixel: CH values of T, stored with the widest vector the pixel's size (and the buffer's address) allows ----
template <int DEPTH> struct EoDepth;
template <> struct EoDepth<0> { typedef uint8_t T; static __device__ __forceinline__ T of(double v) { return (uint8_t) __dmul_rn(v, 255.0); } };
template <> struct EoDepth<1> { typedef uint16_t T; static __device__ __forceinline__ T of(double v) { return (uint16_t) __dmul_rn(v, 65535.0); } };
template <> struct EoDepth<2> { typedef float T; static __device__ __forceinline__ T of(double v) { return __double2float_rn(v); } };
template <> struct EoDepth<3> { typedef double T; static __device__ __forceinline__ T of(double v) { return v; } };
template <int A> struct EoVec;
template <> struct EoVec<2> { typedef uint16_t V; };
template <> struct EoVec<4> { typedef uint32_t V; };
template <> struct EoVec<8> { typedef uint32_t V __attribute__((ext_vector_type(2))); };
template <> struct EoVec<16> { typedef u32x4 V; };
constexpr int eo_align(int bytes) { return bytes % 16 == 0 ? 16 : bytes % 8 == 0 ? 8 : bytes % 4 == 0 ? 4 : bytes % 2 == 0 ? 2 : 1; }
// channels of LqrImageType RGB, RGBA, GREY, GREYA, CMY, CMYK, CMYKA
constexpr int eo_channels(int type) { return type == 0 ? 3 : type == 1 ? 4 : type == 2 ? 1 : type == 3 ? 2 : type == 4 ? 3 : type == 5 ? 4 : 5; }

template <int TYPE, int DEPTH>
__device__ __forceinline__ void eo_store(uint8_t *out, size_t index, double e, bool vec_ok)
{
    typedef typename EoDepth<DEPTH>::T T;
    constexpr int CH = eo_channels(TYPE), P = CH * (int) sizeof(T), A = eo_align(P);
    constexpr bool has_alpha = TYPE == 1 || TYPE == 3 || TYPE == 6, inverted = TYPE >= 4, black = TYPE >= 5;
    const T ve = EoDepth<DEPTH>::of(inverted ? __dsub_rn(1.0, e) : e);
    T v[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) v[k] = ve;
    if (black) { v[0] = v[1] = v[2] = EoDepth<DEPTH>::of(0.0); }
    if (has_alpha) v[CH - 1] = EoDepth<DEPTH>::of(1.0);
    GLOBAL_AS uint8_t *p = (GLOBAL_AS uint8_t *) out + index * P;
    if constexpr (A > (int) sizeof(T)) {
        if (vec_ok) {
            typedef typename EoVec<A>::V V;
            V chunk[P / A];
            __builtin_memcpy(chunk, v, P);
#pragma unroll
            for (int i = 0; i < P / A; i++) ((GLOBAL_AS V *) p)[i] = chunk[i];
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < CH; k++) ((GLOBAL_AS T *) p)[k] = v[k];
}

// w x h: the carver's frame.  The result is w x h (transposed == 0) or h x w pixels; a workgroup writes EO_TILE x EO_TILE of them,
// a wave one row of the tile at a time: emit(e, index) gets the energy of pixel `index` of the result.
template <class Emit>
__device__ __forceinline__ void eo_tiles(const GCarver &c, int w, int h, int stride, int transposed, float (*t)[EO_TILE + 1], Emit emit)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int W = transposed ? h : w, H = transposed ? w : h;
    const int X0 = blockIdx.x * EO_TILE, Y0 = blockIdx.y * EO_TILE;
    if (transposed) {       // image (X, Y) is frame (Y, X): frame rows X0 .. of the tile, read along frame x = image Y
#pragma unroll 4
        for (int r = wv; r < EO_TILE; r += 4) {
            const int fy = X0 + r, fx = Y0 + lane;
            if (fy < h && fx < w) t[r][lane] = c.en[(size_t) fy * stride + fx];
        }
        __syncthreads();
    }
    const int X = X0 + lane;
#pragma unroll 4
    for (int r = wv; r < EO_TILE; r += 4) {
        const int Y = Y0 + r;
        if (X >= W || Y >= H) continue;
        emit(transposed ? t[lane][r] : c.en[(size_t) Y * stride + X], (size_t) Y * W + X);
    }
}

// e_min / e_max of the whole plane from the pairs k_energy_range left
__device__ __forceinline__ void eo_fold(const float *partials, int n_partials, float (*s_r)[2], float &e_min, float &e_max)
{
    e_min = FLT_MAX; e_max = 0.0f;
    for (int i = threadIdx.x; i < n_partials; i += 256) {
        e_min = fminf(e_min, partials[2 * i]);
        e_max = fmaxf(e_max, partials[2 * i + 1]);
    }
    eo_block_range(e_min, e_max, s_r);
}

// the float forms.  normalised == 0: the values as they are (partials is not read)
__global__ __launch_bounds__(256) void k_energy_plane(const DevCarver *cs, int w, int h, int stride, int transposed, int normalised,
                                                      const float *partials, int n_partials, float *out)
{
    __shared__ float s_r[4][2];
    __shared__ float t[EO_TILE][EO_TILE + 1];
    const GCarver c = gview(cs[0]);
    float e_min = 0.0f, e_max = 0.0f;
    if (normalised) eo_fold(partials, n_partials, s_r, e_min, e_max);
    const bool scale = e_max > e_min;
    const float span = __fsub_rn(e_max, e_min);
    GLOBAL_AS float *o = (GLOBAL_AS float *) out;
    eo_tiles(c, w, h, stride, transposed, t, [&](float e, size_t index) {
        if (normalised) {
            e = eo_squash(e);
            if (scale) e = __fdiv_rn(__fsub_rn(e, e_min), span);
        }
        o[index] = e;
    });
}

// the picture
template <int TYPE, int DEPTH>
__global__ __launch_bounds__(256) void k_energy_out(const DevCarver *cs, int w, int h, int stride, int transposed, const float *partials,
                                                    int n_partials, uint8_t *out)
{
    __shared__ float s_r[4][2];
    __shared__ float t[EO_TILE][EO_TILE + 1];
    const GCarver c = gview(cs[0]);
    float e_min, e_max;
    eo_fold(partials, n_partials, s_r, e_min, e_max);
    const bool scale = e_max > e_min;
    const double lo = (double) e_min, span = __dsub_rn((double) e_max, (double) e_min);
    constexpr int P = eo_channels(TYPE) * (int) sizeof(typename EoDepth<DEPTH>::T);
    const bool vec_ok = ((unsigned long long) out % eo_align(P)) == 0;
    eo_tiles(c, w, h, stride, transposed, t, [&](float e, size_t index) {
        const double v = scale ? __ddiv_rn(__dsub_rn((double) eo_squash_pic(e), lo), span) : 0.0;
        eo_store<TYPE, DEPTH>(out, index, v, vec_ok);
    });
}

#define INST(TYPE, D) template __global__ void k_energy_out<TYPE, D>(const DevCarver *, int, int, int, int, const float *, int, uint8_t *);
K_ENERGY_OUT_FORMS(INST)
#undef INST
