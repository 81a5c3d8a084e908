// lqr_levels.h -- what the two families of the level kernel (k_levels.hip, k_levels2.hip) share beside their body (k_levels_body.inc):
// the timing and jitter sites' macros, and the small device helpers the body calls
#pragma once
#include "lqr_common.h"
#ifdef LQR_TIMING
#define LTT(i) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t__ = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); ltt[i] += t__ - ltprev; ltprev = t__; } while (0)
#else
#define LTT(i) do { } while (0)
#endif

// timing jitter for the soak build (make EXTRA=-DLQR_JITTER; switch 16 of lqrhip_band_levels_debug): pseudo-random sleeps at the protocol's
// hand-over sites, as in k_dp_tile_p; the product build has no site (any edit of this kernel can flip its row schedule)
#ifdef LQR_JITTER
#define LJIT(site) do { if (dbg & 16) { unsigned h__ = (unsigned) (slot * 131 + L * 17 + (site) * 7 + epoch * 2654435761u + q * 40503u + image * 977u); h__ ^= h__ >> 13; h__ *= 0x5bd1e995u; h__ ^= h__ >> 15; \
    for (unsigned i__ = h__ & 15u; i__ > 0; i__--) __builtin_amdgcn_s_sleep(127); } } while (0)
#else
#define LJIT(site) do { } while (0)
#endif
// a value every lane holds (read from LDS), as a scalar
__device__ __forceinline__ unsigned long long uni64(unsigned long long v)
{
    return ((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (v >> 32)) << 32) | (unsigned) __builtin_amdgcn_readfirstlane((int) v);
}
// the OR of v over a tile's own lanes 16 .. 47, as a scalar: a prefix OR inside each row of 16 lanes (DPP row_shr 1, 2, 4, 8; a lane
// without a source reads 0), whose last lanes 31 and 47 then hold their rows' ORs
__device__ __forceinline__ unsigned lv_own_or(unsigned v)
{
    int x = (int) v;
    x |= __builtin_amdgcn_mov_dpp(x, 0x111, 0xf, 0xf, true);
    x |= __builtin_amdgcn_mov_dpp(x, 0x112, 0xf, 0xf, true);
    x |= __builtin_amdgcn_mov_dpp(x, 0x114, 0xf, 0xf, true);
    x |= __builtin_amdgcn_mov_dpp(x, 0x118, 0xf, 0xf, true);
    return (unsigned) (__builtin_amdgcn_readlane(x, 31) | __builtin_amdgcn_readlane(x, 47));
}
struct LvMask {                      // a set of tiles (uniform over the wave); LV_MAX_TILES = 64: one word
    unsigned long long lo;
    __device__ __forceinline__ void set(int t) { lo |= 1ull << t; }
    __device__ __forceinline__ bool has(int t) const { return t >= 0 && t < LV_MAX_TILES && ((lo >> t) & 1ull); }
    __device__ __forceinline__ void set_range(int a, int b) { lo |= ((b - a >= 63) ? ~0ull : ((1ull << (b - a + 1)) - 1ull)) << a; }          // [a, b], 0 <= a <= b < 64
    __device__ __forceinline__ int first() const { return lo ? __builtin_ctzll(lo) : -1; }
    __device__ __forceinline__ int last() const { return lo ? 63 - __builtin_clzll(lo) : -1; }
};
