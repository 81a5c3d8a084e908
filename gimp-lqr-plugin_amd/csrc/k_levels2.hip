// k_levels2.hip -- the level kernel (k_levels.hip) with TWO slots of one image in a 256-thread workgroup
// (gfx950 / CDNA4, wave64; see lqr_common.h for the file map)
#include "lqr_common.h"
#include "lqr_kernels.h"
#include "lqr_levels.h"

// ---------------------------------------------------------------------------
// k_band_levels2: k_band_levels' body (k_levels_body.inc: protocol, words, granules, tags, near copies, bounded spins -- all of it)
// with the slots dealt to workgroups in pairs.  A workgroup of k_band_levels is one slot, two waves; 64 images x 8 slots are 512
// workgroups on 256 compute units, two per unit.  Here a workgroup is four waves: waves 0 and 1 are the turn-taking pair of slot s,
// waves 2 and 3 the pair of slot s + ceil(P / 2) of the same image -- tile t belongs to slot t mod P and a band is ~4 tiles wide, so
// the two are active in the same level only when the band spans more than P / 2 tiles.  64 images x 8 slots are 256 workgroups, one
// per compute unit, four waves on four SIMDs.
// Per slot in LDS: the last level polled and the active sets.  Per workgroup (one image, every slot takes the same decision): s_fail
// and the tables of touched columns.  The four waves meet at the workgroup barrier that ends a level's iteration.  With an odd P the
// last workgroup's second slot does not exist: its waves help to build the tables and leave (a barrier counts the waves that live).
// delta_x 1 without a rigidity mask only.  Grid: lv2_grid (lqr_geom.h), all co-resident.
// Debug switch 32 (this family only): the workgroup's slots are 2 s and 2 s + 1, neighbours that are active together in most levels
// -- the pairing the measurements in profiles/levels_pair/ compare with.
// ---------------------------------------------------------------------------
__device__ unsigned long long g_lv2_stats[8];      // as g_lv_stats (lqrhip_band_levels_stats adds the two up)
#ifdef LQR_TIMING
__device__ unsigned long long g_lv2_time[16][2][10];       // as g_lv_time
extern "C" int lqrhip_band_levels2_timing(unsigned long long *out) { (void) hipDeviceSynchronize(); return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lv2_time), sizeof(unsigned long long) * 320) == hipSuccess ? 0 : -1; }
#endif
__device__ int g_lv2_dbg;              // lqrhip_band_levels_debug's switches, and 32 (see above)

template <bool LR, bool RIG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_band_levels2(DevCarver *cs, DpK p, int w, int h, int stride, unsigned long long *exch, int epoch, int *dev_err, int P, int n_img, int store_rows)
{
    constexpr int DELTA = 1;
    constexpr bool RIGM = false;
#define LV_NT 256
#define LV_SLOT_STATE __shared__ int s_polled2[2]; __shared__ unsigned long long s_A2[2][2];
#define LV_POLLED s_polled2[pr]
#define LV_A s_A2[pr]
#define LV_WAVE const int q = __builtin_amdgcn_readfirstlane((tid >> 6) & 1), pr = __builtin_amdgcn_readfirstlane(tid >> 7);
// (lv2_grid / lv2_block in lqr_geom.h state this map; it stays in the kernel's own text, as k_band_levels')
#define LV_BLOCK const int b_xcd = (int) blockIdx.x & 7, b_k = (int) blockIdx.x >> 3; const int P2 = (P + 1) >> 1, s0 = (dbg & 8) ? (int) blockIdx.x % P2 : b_k % P2, slot = (dbg & 32) ? 2 * s0 + pr : s0 + pr * P2, \
                           image = (dbg & 8) ? (int) blockIdx.x / P2 : (b_k / P2) * 8 + b_xcd;
#define LV_INIT_FLAGS if (tid == 0) s_fail = 0; if ((tid & 127) == 0) LV_POLLED = -1;
#define LV_AFTER_SETUP if (slot >= P) return;
#define LV_LEVEL_END asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#define LV_TRACK 1
#define LV_DBG g_lv2_dbg
#define LV_STATS g_lv2_stats
#define LV_TIME g_lv2_time
#include "k_levels_body.inc"
#include "k_levels_undef.inc"
}

void lqr_levels2_debug(int v) { (void) hipMemcpyToSymbol(HIP_SYMBOL(g_lv2_dbg), &v, sizeof v); }
// adds this family's counters to out[0 .. 8)
int lqr_levels2_stats(unsigned long long *out, int reset)
{
    unsigned long long mine[8];
    if (hipMemcpyFromSymbol(mine, HIP_SYMBOL(g_lv2_stats), sizeof mine) != hipSuccess) return -1;
    for (int i = 0; i < 8; i++) out[i] += mine[i];
    if (reset) { unsigned long long z[8] = {0}; (void) hipMemcpyToSymbol(HIP_SYMBOL(g_lv2_stats), z, sizeof z); }
    return 0;
}

// ---- the instantiations the shim launches (lqr_kernels.h lists them)
#define INST(...) template __global__ void k_band_levels2<__VA_ARGS__>(DevCarver *, DpK, int, int, int, unsigned long long *, int, int *, int, int, int);
K_BAND_LEVELS2_FORMS(INST)
#undef INST
