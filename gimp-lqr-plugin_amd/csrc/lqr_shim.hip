// lqr_shim.hip -- the host side: the lqrhip_* C ABI of include/lqr_hip.h (plain pointers and sizes) on top of the kernels of
// k_*.hip: device selection, the allocation cache (its rules are lqr_pool.h's, over hipMalloc / hipFree), host <-> device transfers
// through a pinned ring (lqr_stage.h, over this file's stream), batches and their streams,
// lqrhip_seam_step's per-seam launch sequence (which form of each stage it runs is lqr_plan.h's choice), read-out, reset from device memory,
// the copy ceiling and the seam-map colour ramp.  Every block of the allocation cache has one owner, a DevBuf or a Scratch of lqr_own.h:
// nothing here gives a block back by hand.  The four kernels that live here (k_poison_random, k_copy16, k_reset_jobs, k_vmap_ramp)
// are debugging / measuring / one-off aids next to their only callers.
#include "lqr_common.h"
#include "lqr_kernels.h"
#include "lqr_own.h"
#include "lqr_pool.h"
#include "lqr_stage.h"
#include <atomic>
#include <memory>
#include <dirent.h>

static thread_local std::string g_err;
static int g_device = -1;

static int *g_dev_err_host = nullptr;      // hipHostMalloc'ed, mapped
static int *g_dev_err = nullptr;           // its device address

#define HIPCK_VOID(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { g_err = std::string(#expr) + ": " + hipGetErrorString(e__); (void) hipGetLastError(); } } while (0)
#define HIPCK(expr)                                                                   \
    do {                                                                              \
        hipError_t e__ = (expr);                                                      \
        if (e__ != hipSuccess) {                                                      \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e__);               \
            (void) hipGetLastError();                                                 \
            return (e__ == hipErrorOutOfMemory) ? LQRHIP_ENOMEM : LQRHIP_EHIP;        \
        }                                                                             \
    } while (0)

// What lqr_plan.h chooses from: the knobs of the lqrhip_set_* hooks, and what the device said -- the co-residency bounds for the spin
// waits of the persistent kernels, set from the occupancy queries in lqrhip_init (dpp_resident_workgroups)
static PlanKnobs g_knobs;
static PlanDevice g_dev;

// ===========================================================================
// host side of the shim
// ===========================================================================
namespace {
struct WorkingPlanes {
    DevBuf<uint32_t> pix;
    DevBuf<float> en, m, m2, bias, rig;
    DevBuf<int8_t> least, least2;
    DevBuf<int32_t> seam_x, seam_log, flags;
    DevBuf<int8_t> vp_map, vp_path;     // parallel backtrack: chunk displacement maps and paths (allocated on first use)
};
}  // namespace
// (hidden: whatever the compiler emits for the struct's members -- its destructor gives the planes back -- stays out of the exports,
// which are those of include/lqr_hip.h)
struct __attribute__((visibility("hidden"))) LqrHipCarver {
    int ch = 0;
    int depth = 0;                   // LqrColDepth: 0 8I, 1 .. 3 16I / 32F / 64F
    int luma = 0;                    // (value plane) the value in `pix` is luma, not brightness
    int mode = RD_RGB, alpha = -1, black = -1;      // how the value is formed (lqrhip_carver_set_read; DeepRead)
    int pix_deep = 0;                // `pix` as allocated holds a double per pixel (reads_value() at the time)
    int w0 = 0, h0 = 0;              // base layout dims
    // base planes
    DevBuf<uint8_t> rgb0;
    DevBuf<int32_t> vs;              // a root's; an attached carver has none and reads its root's (vs_of)
    DevBuf<float> bias0, rig0;
    // working planes
    int active = 0;
    int stride = 0, wk_h = 0;
    WorkingPlanes wk;
    int log_cap = 0, log_h = 0;      // the seam log's shape: seams x rows
    int frozen_epoch = 0;           // pix / bias are in the frame before seam `frozen_epoch` of the session
    // What the session that ended owes the frozen planes (lqrhip_vs_commit): seams [frozen_epoch, owed_to) of its log, still alive, are
    // to be removed from pix / bias, after which the frame is owed_w x owed_h.  Paid by pay_catchup, dropped by drop_catchup; 0: nothing
    int owed_to = 0, owed_w = 0, owed_h = 0;
    LqrHipCarver *root = nullptr;
    std::vector<LqrHipCarver *> aux;
    LqrHipBatch *batch = nullptr;
};

// bytes per pixel of the base layout
static inline size_t px_bytes(const LqrHipCarver *c) { return (size_t) c->ch << (c->depth == 0 ? 0 : c->depth == 1 ? 1 : c->depth == 2 ? 2 : 3); }
// the visibility map a carver reads: its own, or its root's
static inline int32_t *vs_of(const LqrHipCarver *c) { return (c->root ? c->root : c)->vs; }

// E14 / E11: every carver of the batch (roots and their attached carvers) goes through ONE launch (a job table in device
// memory, one grid slice of blocks per job); the new planes replace the old ones after its synchronisation.  Everything
// staged for the pass is owned by a PlaneJobs object until then: dropping it gives all of it back to the pool.
namespace {
struct PlaneJob {
    LqrHipCarver *c;
    DevBuf<uint8_t> nrgb;
    DevBuf<float> nbias, nrig;
};
}  // namespace
struct PlaneJobs {
    std::vector<PlaneJob> jobs;
    std::vector<DevBuf<int32_t>> new_vs;    // one per root (none for a transpose)
    // the job table (ch = bytes per pixel), ordered by the form of the kernel that takes each job (stage()): the first n_narrow go
    // to the pass's 8-bit kernel, the others to its deep form / k_transpose_px (lqr_pixel.h: 16-byte accesses where they fit)
    std::vector<InflateDev> dev;
    DevBuf<InflateDev> d_dev;
    size_t n_narrow = 0;
    // stage the output planes of carver c: n1 pixels each
    int add(LqrHipCarver *c, const int32_t *vs_old, int32_t *nvs, size_t n1)
    {
        jobs.push_back(PlaneJob{c, {}, {}, {}});
        PlaneJob &j = jobs.back();
        int rc = j.nrgb.alloc(n1 * px_bytes(c), "&j.nrgb");
        if (!rc && c->bias0) rc = j.nbias.alloc(n1, "&j.nbias");
        if (!rc && c->rig0) rc = j.nrig.alloc(n1, "&j.nrig");
        if (rc) return rc;
        dev.push_back(InflateDev{c->rgb0, vs_old, c->bias0, c->rig0, j.nrgb, nvs, j.nbias, j.nrig, (int) px_bytes(c), c->depth});
        return 0;
    }
    // the table to the device.  Transpose and flatten (by_width) keep pixels of up to 4 bytes on the 8-bit kernels, which move them
    // as bytes / one dword; inflate averages, so only 8-bit pixels of up to 4 channels stay there
    int stage(hipStream_t s, bool by_width)
    {
        n_narrow = std::stable_partition(dev.begin(), dev.end(), [&](const InflateDev &d) { return d.ch <= 4 && (by_width || d.depth == 0); }) - dev.begin();
        int rc = d_dev.alloc(dev.size(), "&d_dev");
        if (rc) return rc;
        HIPCK(hipMemcpyAsync(d_dev, dev.data(), dev.size() * sizeof(InflateDev), hipMemcpyHostToDevice, s));
        return 0;
    }
    size_t n_wide() const { return dev.size() - n_narrow; }
    const InflateDev *d_wide() const { return d_dev + n_narrow; }
};
// after the pass has completed: the new base planes become the carvers'
static void commit(PlaneJobs &pj)
{
    for (auto &j : pj.jobs) {
        j.c->rgb0 = std::move(j.nrgb);
        if (j.nbias) j.c->bias0 = std::move(j.nbias);
        if (j.nrig) j.c->rig0 = std::move(j.nrig);
    }
}

// Two phases (round 6): lqrhip_inflate / lqrhip_flatten / lqrhip_transpose stage the new planes of the batch, run the pass (the inflate
// pass with its fused self-check) and ADOPT NOTHING; lqrhip_planes_commit adopts what was staged.  The host runs phase one on every
// sub-batch of a group before it commits any: a failed check or a failed allocation in sub-batch k must not find sub-batches 0 .. k - 1
// already living in their new layouts (the roll-back / the error return leaves the whole group where it was).
// lqrhip_session_rollback / lqrhip_batch_abort / lqrhip_batch_destroy discard a staged pass.
struct PendingInflate { PlaneJobs pj; int kind = 0 /* 0 inflate, 1 flatten, 2 transpose */, w1 = 0, h1 = 0; };

struct LqrHipBatch {
    std::vector<LqrHipCarver *> cs;
    DevCarver *d_desc = nullptr;
    size_t desc_cap = 0;                    // descriptors d_desc holds (a parked block may be larger than the batch)
    hipStream_t stream = nullptr;
    DevBuf<unsigned long long> exch;        // k_dp_tile_p: halo granules per image and tile + finished-tile counters
    int exch_ntiles = 0, exch_n = 0, exch_px = 0;      // geometry the exchange area was last laid out for
    int tile_epoch = 0;                     // launches of k_dp_tile_p on this batch (part of the granule tags)
    DevBuf<unsigned long long> wlist;       // k_carve_v: the work list its walk role fills (two tail words, then the entries: lqr_beside.h)
    unsigned wlist_launches = 0;            // launches of k_carve_v on this batch (their tags)
    bool dirty = true;
    int shared_n = 1;                       // ... how many batches of the group there are (lqrhip_batch_set_shared)
    bool shared = false;                    // other batches of the same group run concurrently on their own streams:
                                            // no persistent (spin-waiting, co-residency-dependent) kernels
    bool safe = false;                      // a session is being redone after a fault: kernels without spin waits only
    std::unique_ptr<PendingInflate> pending_inflate;    // the staged planes of lqrhip_inflate / _flatten / _transpose, until lqrhip_planes_commit adopts them
};
static bool g_no_spin = false;             // set by a spin time-out (check_dev_error): the process stays on the non-spinning kernels

struct ProfRec {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    double bytes = 0;
};
static int g_prof = 0;                 // 0 off, 1 every kernel, 2 the roofline kernel (k_carve) only
static std::map<std::string, ProfRec> g_profrec;
static hipStream_t g_stream0 = nullptr;
// the launch census (test hook, lqr_hip.h): which form of each stage was launched, counted on the host at the launch sites
static unsigned long long g_census[LQRHIP_CENSUS_SLOTS];
#define CENSUS(slot) (g_census[(slot)]++)
extern "C" int lqrhip_launch_census(unsigned long long *out, int n, int reset)
{
    if (out && n > 0) memcpy(out, g_census, (size_t) std::min(n, (int) LQRHIP_CENSUS_SLOTS) * sizeof g_census[0]);
    if (reset) memset(g_census, 0, sizeof g_census);
    return LQRHIP_CENSUS_SLOTS;
}

extern "C" const char *lqrhip_last_error(void) { return g_err.c_str(); }

// Workgroups of the spinning kernels (k_dp_tile_p, k_band_levels) the device holds at once.  Their workgroups spin on their
// neighbours, so a grid must be co-resident: each bound is the minimum of the occupancy query over EVERY instantiation of its
// residency class -- the family's one list in lqr_kernels.h, from which the launch picks too, so no kernel can be launched that
// was not asked about -- less one workgroup per CU of margin (the API is known to answer one block per CU too many at some SGPR
// counts: MI355X_MICROARCH.md, residency), times the CU count.  A grid above the bound goes to k_dp_tile (kernel boundaries
// instead of spin waits).
static void dpp_resident_workgroups(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) return;
    enum { PX4, PLAIN, GENERAL, LEVELS, LEVELS2, N_CLASSES };
    int per_cu[N_CLASSES] = {1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20};
    auto q = [&](int cls, auto kern, int threads) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, threads, 0) != hipSuccess) { (void) hipGetLastError(); n = 0; }
        per_cu[cls] = std::min(per_cu[cls], n);
    };
#define QUERY(CLASS, ...) q(CLASS, k_dp_tile_p<__VA_ARGS__>, 64 * DPP_W);
    K_DP_TILE_P_FORMS(QUERY)
#undef QUERY
#define QUERY(...) q(LEVELS, k_band_levels<__VA_ARGS__>, 128);
    K_BAND_LEVELS_FORMS(QUERY)
#undef QUERY
#define QUERY(...) q(LEVELS2, k_band_levels2<__VA_ARGS__>, 256);
    K_BAND_LEVELS2_FORMS(QUERY)
#undef QUERY
    auto bound = [&](int blocks) { return std::max(0, blocks - 1) * prop.multiProcessorCount; };
    g_dev.n_cu = prop.multiProcessorCount;
    // the plain 2-px instantiations stage a whole 32-row block (193 VGPRs): their bound is lower, and a grid that is too large for
    // them but fits the 4-px ones must not be sent to k_dp_tile for it.  The general ones (2 px per lane only) hold more registers still
    g_dev.wgs_px4 = bound(per_cu[PX4]);
    g_dev.wgs_plain = bound(std::min(per_cu[PX4], per_cu[PLAIN]));
    g_dev.wgs_general = bound(per_cu[GENERAL]);
    g_dev.wgs_levels = bound(per_cu[LEVELS]);
    g_dev.wgs_levels2 = bound(per_cu[LEVELS2]);
}

// Large lock-step groups are carved on 4 streams, and those need hardware queues of their own: the HIP runtime's
// GPU_MAX_HW_QUEUES, default 4 per process, read ONCE when the runtime initialises (lqrhip_sub_batches below).  A host
// that has never heard of the variable (the plug-in) would silently get one stream and 10 % less.  So when this library
// is loaded into a process that has not brought the GPU runtime up yet -- no descriptor of /dev/kfd is open -- and the
// variable is not set, it is set to 8 here, before the library's own first HIP call initialises the runtime.  A host that
// set it (to anything) keeps its value; a host whose runtime is already up keeps one stream.
static bool kfd_is_open(void)
{
    DIR *d = opendir("/proc/self/fd");
    if (!d) return true;                      // cannot tell: leave the environment alone
    bool open_ = false;
    while (struct dirent *e = readdir(d)) {
        if (e->d_name[0] == '.') continue;
        char path[64], link[64];
        snprintf(path, sizeof path, "/proc/self/fd/%s", e->d_name);
        const ssize_t n = readlink(path, link, sizeof link - 1);
        if (n <= 0) continue;
        link[n] = 0;
        if (strcmp(link, "/dev/kfd") == 0) { open_ = true; break; }
    }
    closedir(d);
    return open_;
}
__attribute__((constructor)) static void lqrhip_on_load(void)
{
    if (!kfd_is_open()) setenv("GPU_MAX_HW_QUEUES", "8", 0);        // (0: a value that is set stays)
}

extern "C" int lqrhip_init(void)
{
    if (g_device >= 0) return g_device;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_err = "no HIP device visible: the MI355X engine needs a gfx950 GPU (there is no CPU fallback)";
        (void) hipGetLastError();
        return LQRHIP_EHIP;
    }
    int dev = 0;
    const char *lr = getenv("LOCAL_RANK");
    if (lr) dev = atoi(lr) % n;
    HIPCK(hipSetDevice(dev));
    HIPCK(hipStreamCreateWithFlags(&g_stream0, hipStreamNonBlocking));
    HIPCK(hipHostMalloc((void **) &g_dev_err_host, sizeof(int), hipHostMallocMapped));
    *g_dev_err_host = 0;
    HIPCK(hipHostGetDevicePointer((void **) &g_dev_err, g_dev_err_host, 0));
    dpp_resident_workgroups(dev);
    g_device = dev;
    return dev;
}

// A kernel recorded a failure (dev_fail): report it once, as LQRHIP_EFAULT, and clear the word.  The word is one per
// process and whoever synchronises first finds it -- not necessarily the batch whose kernel failed (the host rolls back and
// redoes the session of EVERY sub-batch of the group).  A persistent sweep that gave up half way leaves its batch's exchange
// area (tags, finished-tile counter) and, for an update, the plane pointers in the device descriptors in an unknown state,
// so EVERY live batch is marked for a fresh lay-out of both.
static std::vector<LqrHipBatch *> g_live_batches;
static void invalidate_all_batches(void);
// [0] spin time-outs, [1] failed activity predictions, [2] seam-log self-check failures, [3] level self-check failures,
// [4] sessions rolled back, [5] faults injected (lqrhip_debug_inject), [6] sessions carved on the non-spinning kernels
static unsigned long long g_fault_stats[8];
// After a spin time-out the persistent (co-residency-dependent) kernels are not chosen again in this process: a device that is
// shared or partitioned now will be in a minute, and every further resize would first wait out the time-out (~0.3 s) and then be
// redone.  lqrhip_set_no_spin(0) re-arms them (tests).
extern "C" void lqrhip_set_no_spin(int on) { g_no_spin = on != 0; }
extern "C" int lqrhip_get_no_spin(void) { return g_no_spin ? 1 : 0; }
static int check_dev_error(void)
{
    if (!g_dev_err_host || *g_dev_err_host == 0) return 0;
    const int code = *g_dev_err_host;
    *g_dev_err_host = 0;
    invalidate_all_batches();
    switch (code) {
    case DEVERR_TILE_TIMEOUT:
        g_fault_stats[0]++;
        if (!g_no_spin) fprintf(stderr, "liblqr-hip: a persistent kernel's workgroups were not co-resident in time (GPU shared or partitioned?): "
                                        "this process now uses the non-spinning kernels\n");
        g_no_spin = true;
        g_err = "persistent tiled DP sweep: a neighbour tile never became resident (GPU shared or partitioned?); results of this session are invalid";
        break;
    case DEVERR_BAND_PREDICTION: g_fault_stats[1]++; g_err = "band update: activity prediction failed; results of this session are invalid"; break;
    case DEVERR_SEAMLOG: g_fault_stats[2]++; g_err = "self-check: the session's seam log does not describe delta_x-connected seams inside the frame; results of this session are invalid"; break;
    case DEVERR_LEVELS: g_fault_stats[3]++; g_err = "self-check: a level of the session is missing or occurs twice in a row of the visibility map; results of this session are invalid"; break;
    default: g_err = "device-side failure " + std::to_string(code) + "; results of this session are invalid"; break;
    }
    return LQRHIP_EFAULT;
}
extern "C" int lqrhip_fault_stats(unsigned long long *out8, int reset)
{
    memcpy(out8, g_fault_stats, sizeof g_fault_stats);
    if (reset) memset(g_fault_stats, 0, sizeof g_fault_stats);
    return 0;
}

// Device allocations go through a small size-class cache, the BlockCache of lqr_pool.h (g_cache below): the shim supplies hipMalloc,
// hipFree and the hook that prepares a block handed out, pool_poison.  A block is only returned to the cache after the stream that
// used it has been synchronised.
//
// LQRHIP_POISON=<byte> in the environment (debugging aid, scripts/fuzz_parity.py): every block handed out is first filled
// with that byte and the device synchronised, so that a kernel that reads memory nothing wrote yet fails the same way every
// time instead of depending on what the block held before
// LQRHIP_POISON=r1 / r2 / r3: pseudo-random words that look like what a recycled block holds -- floats in [0, 100),
// integers in [0, 2048), arbitrary bits
__global__ void k_poison_random(unsigned *p, size_t n, int mode, int stride, int c0, int c1, int r0, int r1)
{
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        if (stride > 0) {       // LQRHIP_POISON_WINDOW=stride:c0:c1:r0:r1 -- only that window of a plane, zero elsewhere
            const int col = (int) (i % stride), row = (int) (i / stride);
            if (col < c0 || col >= c1 || row < r0 || row >= r1) { p[i] = 0; continue; }
        }
        unsigned hsh = (unsigned) i * 2654435761u + 0x9e3779b9u;
        hsh ^= hsh >> 15; hsh *= 0x85ebca6bu; hsh ^= hsh >> 13; hsh *= 0xc2b2ae35u; hsh ^= hsh >> 16;
        p[i] = mode == 1 ? __float_as_uint((float) (hsh >> 8) * (100.0f / 16777216.0f)) : mode == 2 ? (hsh >> 21) : hsh;
    }
}
static int g_poison = -2;
static unsigned g_poison32 = 0;
static int pool_poison(void *p, size_t sz, const char *name)     // name: what the allocation is for (LQRHIP_POISON_LOG)
{
    if (g_poison == -2) {
        const char *e = getenv("LQRHIP_POISON");
        g_poison = -1;
        if (e && e[0] == '0' && e[1] == 'x') { g_poison = 256; g_poison32 = (unsigned) strtoul(e, nullptr, 16); }     // a 32-bit word
        else if (e && e[0] == 'r') g_poison = 256 + atoi(e + 1);
        else if (e && *e) g_poison = atoi(e) & 255;
    }
    if (g_poison < 0) return 0;
    {   // LQRHIP_POISON_RANGE=a:b poisons only the allocations numbered a .. b-1 of the process (LQRHIP_POISON_LOG lists them)
        static long seq = 0, lo = 0, hi = -1;
        static int logit = -1;
        if (logit < 0) {
            logit = getenv("LQRHIP_POISON_LOG") != nullptr;
            const char *r = getenv("LQRHIP_POISON_RANGE");
            if (r) sscanf(r, "%ld:%ld", &lo, &hi);
        }
        const long me = seq++;
        if (logit) fprintf(stderr, "alloc %ld %zu %s\n", me, sz, name);
        if (hi >= 0 && (me < lo || me >= hi)) { HIPCK(hipMemset(p, 0, sz)); HIPCK(hipDeviceSynchronize()); return 0; }
    }
    if (g_poison > 256) {
        static int win[5] = {0, 0, 0, 0, 0};
        static bool once = false;
        if (!once) { once = true; const char *wv = getenv("LQRHIP_POISON_WINDOW"); if (wv) sscanf(wv, "%d:%d:%d:%d:%d", win, win + 1, win + 2, win + 3, win + 4); }
        hipLaunchKernelGGL(k_poison_random, dim3(1024), dim3(256), 0, 0, (unsigned *) p, sz / 4, g_poison - 256, win[0], win[1], win[2], win[3], win[4]);
    }
    else if (g_poison == 256) HIPCK(hipMemsetD32((hipDeviceptr_t) p, (int) g_poison32, sz / 4));
    else HIPCK(hipMemset(p, g_poison, sz));
    HIPCK(hipDeviceSynchronize());
    return 0;
}

static int raw_alloc(void **p, size_t bytes, std::string &why)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return 0;
    why = std::string("e: ") + hipGetErrorString(e);
    (void) hipGetLastError();
    return e == hipErrorOutOfMemory ? LQRHIP_ENOMEM : LQRHIP_EHIP;
}
static void raw_free(void *p) { (void) hipFree(p); }
static BlockCache g_cache((size_t) 24 << 30, LQRHIP_ENOMEM, raw_alloc, raw_free, pool_poison);
// fault injection (tests/test_faults_gpu.py): the nth device allocation from now on fails with "out of memory", once (-1: disarmed)
extern "C" void lqrhip_debug_fail_alloc(int nth) { g_cache.fail_in(nth); }
static int lqr_pool_alloc(void **p, size_t bytes, const char *name) { return g_cache.alloc(p, bytes, name, g_err); }
static void lqr_pool_free(void *p) { g_cache.free(p); }
extern "C" unsigned long long lqrhip_debug_pool_live(void) { return g_cache.live(); }

static void lqr_stream_wait(void *stream) { (void) hipStreamSynchronize((hipStream_t) stream); }

// zero device memory and wait: hipMemset on the null stream is asynchronous for device memory and the
// engine's streams are non-blocking, so a null-stream memset is not ordered with the kernels after it
static hipError_t dzero(void *p, size_t bytes)
{
    hipError_t e = hipMemsetAsync(p, 0, bytes, g_stream0);
    return e != hipSuccess ? e : hipStreamSynchronize(g_stream0);
}

// Host <-> device copies of whole images go through a ring of pinned bounce buffers that helper threads fill and empty, the StageRing of
// lqr_stage.h; its device operations are these, on g_stream0.  Both functions return with the transfer complete, also on error.
static const int STAGE_SLOTS = 16;
namespace {
struct Stream0Stage final : StageDevice {
    hipEvent_t ev[STAGE_SLOTS] = {};
    int slot_create(int slot, size_t bytes, void **host) override
    {
        hipError_t e = hipHostMalloc(host, bytes, hipHostMallocDefault);
        if (e == hipSuccess && (e = hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming)) != hipSuccess) (void) hipHostFree(*host);
        if (e == hipSuccess) return 0;
        g_err = std::string("staging buffers: ") + hipGetErrorString(e);
        (void) hipGetLastError();
        return e == hipErrorOutOfMemory ? LQRHIP_ENOMEM : LQRHIP_EHIP;
    }
    void slot_destroy(int slot, void *host) override { (void) hipHostFree(host); (void) hipEventDestroy(ev[slot]); }
    int copy_up(void *dst, const void *src, size_t n) override { HIPCK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, g_stream0)); return 0; }
    int copy_down(void *dst, const void *src, size_t n) override { HIPCK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, g_stream0)); return 0; }
    int record(int slot) override { HIPCK(hipEventRecord(ev[slot], g_stream0)); return 0; }
    int wait(int slot) override { HIPCK(hipEventSynchronize(ev[slot])); return 0; }
    bool landed(int slot) override { return hipEventQuery(ev[slot]) == hipSuccess; }
    int wait_stream(bool quiet) override
    {
        hipError_t e = hipStreamSynchronize(g_stream0);
        if (e == hipSuccess) return 0;
        if (!quiet) g_err = std::string("upload: ") + hipGetErrorString(e);
        return LQRHIP_EHIP;
    }
};
}  // namespace
// created at the first transfer; it lives to the end of the process
static StageRing &stage_ring(void)
{
    static Stream0Stage dev;
    static StageRing *ring = [] {
        const unsigned hw = std::thread::hardware_concurrency();
        return new StageRing(dev, STAGE_SLOTS, (size_t) 4 << 20, hw >= 16 ? 8 : hw >= 4 ? (int) hw / 2 : 1);
    }();
    return *ring;
}
static int h2d_staged(void *dst, const void *src, size_t bytes) { return stage_ring().upload(dst, src, bytes); }
static int d2h_staged(void *dst, const void *src, size_t bytes) { return stage_ring().download(dst, src, bytes); }

// A carver reads through the value plane (`pix` holds one double per pixel, the value the energy reads; lqr_pixel.h) unless it is
// 8-bit grey / RGB with or without alpha in liblqr's default layout: those keep their pixels packed in `pix` and every kernel they had.
// (The rule is restated by tests/imgtype_cases.py reads_value; same_config in host/lqr_carver.c groups only carvers whose type
// and roles are equal, so that a group is on one side of it.  Keep the three in step.)
static inline bool reads_value(const LqrHipCarver *c)
{
    if (c->depth != 0 || c->ch > 4 || (c->mode != RD_GREY && c->mode != RD_RGB)) return true;
    return c->black >= 0 || c->alpha != (c->ch == 2 ? 1 : c->ch == 4 ? 3 : -1);
}
static inline DeepRead deep_read(const LqrHipCarver *c) { return DeepRead{c->ch, c->mode, c->alpha, c->black, c->luma}; }
// The kernels that touch the working plane exist in both forms (template parameter VALUE): f gets the carver's as a compile-time constant
template <class F> static inline void with_form(const LqrHipCarver *c, F f)
{
    if (reads_value(c)) f(std::true_type{}); else f(std::false_type{});
}
// The energy a kernel is instantiated for.  On the value plane the luma energies (3, 4, 5) ARE the brightness energies (0, 1, 2): the
// plane already holds brightness or luma (DeepRead.luma decided it when the plane was laid out) and grad_energy_f only looks at
// NRG % 3, so the six would compile to three pairs of identical kernels.  The value forms are instantiated for 0, 1, 2 and 6 only.
constexpr int plane_nrg(bool value, int nrg) { return value && nrg >= 3 && nrg <= 5 ? nrg - 3 : nrg; }
static inline int nrg_index(int nrg_func) { return nrg_func >= 0 && nrg_func <= 5 ? nrg_func : 6; }      // LqrEnergyFuncBuiltinType; anything else is 6
// Launching a template kernel: the run-time values are matched against the family's list in lqr_kernels.h, by a chain of
// `#define CASE(...) if (<values equal the entry>) <launch that entry>; else` ending in no_form -- values no entry has cannot come
// out of the choices above the launch sites, but they must not launch nothing silently.
static int no_form(const char *family) { g_err = std::string(family) + ": no instantiation for the parameters asked for"; return LQRHIP_EARG; }
// ... for a list of ints: f(std::integral_constant<int, v>{}) and true if the list has v
#define LISTED_CASE_(N) if (v__ == N) { f__(std::integral_constant<int, N>{}); return true; }
#define with_listed(LIST, v, f) [&](int v__, auto f__) { LIST(LISTED_CASE_) return false; }(v, f)
// liblqr's default image type for a channel count, as a read mode
static void default_read(LqrHipCarver *c)
{
    c->mode = c->ch <= 2 ? RD_GREY : c->ch <= 4 ? RD_RGB : c->ch == 5 ? RD_CMYK : RD_CUSTOM;
    c->alpha = c->ch == 2 ? 1 : c->ch == 4 ? 3 : c->ch == 5 ? 4 : -1;
    c->black = c->ch == 5 ? 3 : -1;
}

static int batch_sync_of(LqrHipCarver *c)
{
    LqrHipCarver *r = c->root ? c->root : c;
    if (r->batch) HIPCK(hipStreamSynchronize(r->batch->stream));
    return 0;
}

// the base layout: w x h pixels of `channels` values of `depth` (LqrColDepth: 1 / 2 / 4 / 8 bytes each)
extern "C" LqrHipCarver *lqrhip_carver_create_ext(const void *rgb, int w, int h, int channels, int depth)
{
    if (depth < 0 || depth > 3 || channels < 1 || channels > LQRHIP_MAX_CHANNELS) { g_err = "unsupported colour depth / channels"; return nullptr; }
    if (lqrhip_init() < 0) return nullptr;
    LqrHipCarver *c = new LqrHipCarver();
    c->ch = channels; c->depth = depth; c->w0 = w; c->h0 = h;
    default_read(c);
    const size_t n = (size_t) w * h, bytes = n * px_bytes(c);
    if (c->rgb0.alloc(bytes, "&c->rgb0") || c->vs.alloc(n, "&c->vs")) { lqrhip_carver_destroy(c); return nullptr; }
    // the visibility map is cleared on the same stream, under the upload: one synchronisation for both
    if (hipMemsetAsync(c->vs, 0, n * sizeof(int32_t), g_stream0) != hipSuccess || h2d_staged(c->rgb0, rgb, bytes) != 0) {
        g_err = "upload failed";
        lqrhip_carver_destroy(c);
        return nullptr;
    }
    return c;
}

extern "C" LqrHipCarver *lqrhip_carver_create(const unsigned char *rgb, int w, int h, int channels)
{
    return lqrhip_carver_create_ext(rgb, w, h, channels, 0);
}

extern "C" int lqrhip_carver_set_read_luma(LqrHipCarver *c, int luma)
{
    const int changed = reads_value(c) && (luma != 0) != (c->luma != 0);
    c->luma = luma != 0;
    return changed;
}

extern "C" int lqrhip_carver_set_read(LqrHipCarver *c, int image_type, int alpha, int black)
{
    // LqrImageType: RGB, RGBA, GREY, GREYA, CMY, CMYK, CMYKA, CUSTOM
    static const int mode_of[8] = {RD_RGB, RD_RGB, RD_GREY, RD_GREY, RD_CMY, RD_CMYK, RD_CMYK, RD_CUSTOM};
    if (image_type < 0 || image_type > 7 || alpha >= c->ch || black >= c->ch) return LQRHIP_EARG;
    const bool was = reads_value(c);
    const int mode = mode_of[image_type], a = alpha < 0 ? -1 : alpha, k = black < 0 ? -1 : black;
    const bool differs = mode != c->mode || a != c->alpha || k != c->black;
    c->mode = mode; c->alpha = a; c->black = k;
    return (differs && (was || reads_value(c))) ? 1 : 0;
}

// the frozen planes are about to be laid out afresh, or are garbage: what the last session owed them is owed no more, and the log
// restarts at 0
static inline void drop_catchup(LqrHipCarver *c)
{
    c->owed_to = 0; c->owed_w = 0; c->owed_h = 0;
    c->frozen_epoch = 0;
}

static void free_working(LqrHipCarver *c)
{
    c->wk = WorkingPlanes();
    c->log_cap = 0; c->log_h = 0;
    drop_catchup(c);
}

extern "C" void lqrhip_carver_destroy(LqrHipCarver *c)
{
    if (!c) return;
    // its planes may still be in use by kernels on the owning batch's stream or by the shim's own stream (resets, mask
    // uploads, read-outs): wait for those two, not for the device (tearing a batch down was 64 device synchronisations)
    {
        LqrHipCarver *r = c->root ? c->root : c;
        if (r->batch && r->batch->stream) (void) hipStreamSynchronize(r->batch->stream);
        if (c->batch && c->batch != r->batch && c->batch->stream) (void) hipStreamSynchronize(c->batch->stream);
        if (g_stream0) (void) hipStreamSynchronize(g_stream0);
        (void) hipGetLastError();
    }
    delete c;
}

extern "C" int lqrhip_carver_attach(LqrHipCarver *root, LqrHipCarver *aux)
{
    if (root->w0 != aux->w0 || root->h0 != aux->h0) return LQRHIP_EARG;
    aux->vs.reset();
    aux->root = root;
    root->aux.push_back(aux);
    if (root->batch) root->batch->dirty = true;
    return 0;
}

// (re)allocate the working planes for a w x h carved frame
static int ensure_working(LqrHipCarver *c, int w, int h)
{
    int stride = plane_stride(w);
    bool need_bias = c->bias0 != nullptr, need_rig = c->rig0 != nullptr;
    const int deep = reads_value(c) ? 1 : 0;
    WorkingPlanes &k = c->wk;
    if (k.pix && c->stride == stride && c->wk_h == h && (!!k.bias == need_bias) && (!!k.rig == need_rig) && c->pix_deep == deep) return 0;
    free_working(c);
    c->stride = 0; c->wk_h = 0;
    size_t n = plane_elems(stride, h);
    const size_t npix = deep ? 2 * n : n;              // a value plane holds a double per pixel
    int rc;
    if ((rc = k.pix.alloc(npix, "&c->pix")) || (rc = k.en.alloc(n, "&c->en")) || (rc = k.m.alloc(n, "&c->m")) || (rc = k.least.alloc(n, "&c->least")) ||
        (rc = k.seam_x.alloc(seam_x_elems(h), "&c->seam_x")) || (rc = k.flags.alloc((size_t) FLAG_WORDS, "&c->flags")) ||
        (need_bias && (rc = k.bias.alloc(n, "&c->bias"))) || (need_rig && (rc = k.rig.alloc(n, "&c->rig")))) {
        free_working(c);            // never leave a half-allocated set behind: a retry must not pass the early-out above
        return rc;
    }
    // all on the shim's stream, one synchronisation
    hipError_t e = hipMemsetAsync(k.least, 0, n, g_stream0);
    if (e == hipSuccess) e = hipMemsetAsync(k.m, 0, n * sizeof(float), g_stream0);
    if (e == hipSuccess) e = hipMemsetAsync(k.en, 0, n * sizeof(float), g_stream0);
    if (e == hipSuccess) e = hipMemsetAsync(k.pix, 0, npix * sizeof(uint32_t), g_stream0);
    if (e == hipSuccess) e = hipMemsetAsync(k.flags, 0, (size_t) FLAG_WORDS * sizeof(int32_t), g_stream0);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream0);
    if (e != hipSuccess) { free_working(c); HIPCK(e); }
    c->stride = stride; c->wk_h = h; c->pix_deep = deep;
    if (c->batch) c->batch->dirty = true;
    return 0;
}

static int ensure_log(LqrHipCarver *c, int n_seams, int h)
{
    if (c->wk.seam_log && c->log_cap >= n_seams && c->log_h == h) return 0;
    int rc = c->wk.seam_log.alloc(seam_log_elems(n_seams, h), "&c->seam_log");      // (a log of another shape is replaced, also by a smaller one)
    if (rc) return rc;
    c->log_cap = n_seams; c->log_h = h;
    if (c->batch) c->batch->dirty = true;
    return 0;
}

extern "C" int lqrhip_carver_activate(LqrHipCarver *c)
{
    c->active = 1;
    // E1 lqr_carver_init allocates the DP maps: do the same here, so that the first resize does
    // not pay for hipMalloc (re-done lazily by lqrhip_wk_init if the geometry changes)
    return ensure_working(c, c->w0, c->h0);
}

// ---- masks: the 8-bit ones of lqr.h and the computed ones of include/lqr_masks.h (kernels in k_energy.hip, k_masks.hip) ----------------
extern "C" int lqrhip_mask_plane_ensure(LqrHipCarver *c, int is_rigmask)
{
    DevBuf<float> &plane = is_rigmask ? c->rig0 : c->bias0;
    if (plane) return 0;
    int rc = batch_sync_of(c);
    if (rc) return rc;
    const size_t n = (size_t) c->w0 * c->h0;
    if ((rc = plane.alloc(n, "plane"))) return rc;
    hipError_t e = dzero(plane, n * sizeof(float));
    if (e != hipSuccess) { plane.reset(); HIPCK(e); }
    if (c->batch) c->batch->dirty = true;
    return 0;
}

extern "C" int lqrhip_mask_add(LqrHipCarver *c, const unsigned char *mask, int channels, int width, int height, int x_off,
                               int y_off, int transposed, int is_rigmask, int bias_factor)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    if ((rc = lqrhip_mask_plane_ensure(c, is_rigmask))) return rc;
    float *plane = is_rigmask ? c->rig0 : c->bias0;
    const MaskClip k = mask_clip(c->w0, c->h0, width, height, x_off, y_off, transposed);
    if (k.nx <= 0 || k.ny <= 0) return 0;
    const size_t mbytes = (size_t) width * height * channels;
    Scratch tmp(g_stream0);
    uint8_t *dmask = tmp.get<uint8_t>(mbytes, "&dmask", rc);
    if (rc || (rc = h2d_staged(dmask, mask, mbytes))) return rc;
    dim3 grid(tiles_of(k.nx, 256), k.ny);
    hipLaunchKernelGGL(k_mask_add, grid, dim3(256), 0, g_stream0, plane, c->w0, dmask, channels, width, k.x0, k.y0, k.x1, k.y1, k.nx, k.ny,
                       transposed, is_rigmask, bias_factor);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(g_stream0));
    tmp.done();
    return 0;
}

extern "C" int lqrhip_mask_add_f(LqrHipCarver *c, const void *mask, int depth, int on_device, int width, int height, int x_off, int y_off,
                                 int transposed, int is_rigmask, int bias_factor)
{
    if ((depth != 2 && depth != 3) || !mask || width < 1 || height < 1) { g_err = "mask: float or double values, at least 1 x 1"; return LQRHIP_EARG; }
    int rc = batch_sync_of(c);
    if (rc) return rc;
    if ((rc = lqrhip_mask_plane_ensure(c, is_rigmask))) return rc;
    float *plane = is_rigmask ? c->rig0 : c->bias0;
    const MaskClip k = mask_clip(c->w0, c->h0, width, height, x_off, y_off, transposed);
    if (k.nx <= 0 || k.ny <= 0) return 0;
    const size_t mbytes = (size_t) width * height * (depth == 2 ? sizeof(float) : sizeof(double));
    Scratch tmp(g_stream0);
    const void *src = mask;
    if (!on_device) {
        uint8_t *staged = tmp.get<uint8_t>(mbytes, "&staged", rc);
        if (rc || (rc = h2d_staged(staged, mask, mbytes))) return rc;
        src = staged;
    }
    dim3 grid(tiles_of(k.nx, 256), k.ny);
    if (depth == 2)
        hipLaunchKernelGGL(k_mask_add_f<float>, grid, dim3(256), 0, g_stream0, plane, c->w0, (const float *) src, width, k.x0, k.y0, k.x1, k.y1, k.nx, k.ny,
                           transposed, is_rigmask, bias_factor);
    else
        hipLaunchKernelGGL(k_mask_add_f<double>, grid, dim3(256), 0, g_stream0, plane, c->w0, (const double *) src, width, k.x0, k.y0, k.x1, k.y1, k.nx, k.ny,
                           transposed, is_rigmask, bias_factor);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(g_stream0));        // the caller may reuse its buffer
    tmp.done();
    return 0;
}

static unsigned long long g_mask_flushes = 0;
extern "C" unsigned long long lqrhip_debug_mask_flushes(void) { return g_mask_flushes; }

extern "C" int lqrhip_mask_scatter(LqrHipCarver *c, int is_rigmask, const int *index, const double *value, const size_t *start, int buckets)
{
    if (buckets < 1 || start[buckets] == 0) return 0;
    int rc = batch_sync_of(c);
    if (rc) return rc;
    if ((rc = lqrhip_mask_plane_ensure(c, is_rigmask))) return rc;
    float *plane = is_rigmask ? c->rig0 : c->bias0;
    const size_t n = start[buckets];
    Scratch tmp(g_stream0);
    int *dindex = tmp.get<int>(n, "&dindex", rc);
    if (rc) return rc;
    double *dvalue = tmp.get<double>(n, "&dvalue", rc);
    if (rc || (rc = h2d_staged(dindex, index, n * sizeof(int))) || (rc = h2d_staged(dvalue, value, n * sizeof(double)))) return rc;
    // bucket after bucket on one stream: a pixel that is hit k times receives its values in call order
    for (int b = 0; b < buckets; b++) {
        const size_t nb = start[b + 1] - start[b];
        if (!nb) continue;
        hipLaunchKernelGGL(k_mask_scatter, dim3((unsigned) blocks_of(nb, 256)), dim3(256), 0, g_stream0, plane, dindex + start[b], dvalue + start[b],
                           nb, is_rigmask);
        HIPCK(hipGetLastError());
        g_mask_flushes++;
    }
    HIPCK(hipStreamSynchronize(g_stream0));
    tmp.done();
    return 0;
}

extern "C" int lqrhip_mask_clear(LqrHipCarver *c, int is_rigmask)
{
    DevBuf<float> &plane = is_rigmask ? c->rig0 : c->bias0;
    if (!plane) return 0;
    int rc = batch_sync_of(c);
    if (rc) return rc;
    HIPCK(hipStreamSynchronize(g_stream0));
    plane.reset();
    // the working copy goes at the next lqrhip_wk_init (ensure_working lays the planes out for the masks the carver has)
    if (c->batch) c->batch->dirty = true;
    return 0;
}

extern "C" int lqrhip_read_mask_plane(LqrHipCarver *c, int is_rigmask, int transposed, float *out)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    const size_t n = (size_t) c->w0 * c->h0;
    const float *plane = is_rigmask ? c->rig0 : c->bias0;
    if (!plane) { memset(out, 0, n * sizeof(float)); return 0; }
    if (!transposed) return d2h_staged(out, plane, n * sizeof(float));
    Scratch tmp(g_stream0);
    float *t = tmp.get<float>(n, "&t", rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_plane_transpose, dim3(tiles_of(c->w0, 16), tiles_of(c->h0, 16)), dim3(256), 0, g_stream0, plane, t, c->w0, c->h0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_err = std::string("k_plane_transpose: ") + hipGetErrorString(e); return LQRHIP_EHIP; }
    if ((rc = d2h_staged(out, t, n * sizeof(float)))) return rc;
    (void) hipStreamSynchronize(g_stream0);
    tmp.done();
    return 0;
}

// ---- batch -----------------------------------------------------------------
// A lock-step group can be split over several HIP streams (sub-batches) that advance seam by seam side by side: a seam
// round is a latency-bound chain (backtrack, energy update, band update: ~0.7 ms at 4K whatever the batch size, on a
// few CUs) followed by the bandwidth-bound carve, so one sub-batch's chain runs under another's carve.  Measured at
// 64 x 4K with 4 streams: +12 % throughput (424k vs 377k Mseams*px/s), but every kernel then shares the chip -- a carve
// launch of 16 images takes 0.20 ms next to the others' kernels (2.6 TB/s algorithmic) instead of 0.13 ms alone -- and
// it needs a hardware queue per stream: with the HIP runtime's default of 4 queues per process (GPU_MAX_HW_QUEUES) the
// streams share queues and the same split is 30 % SLOWER.  lqrhip_set_sub_batches (bench.py --sub-batches) pins the
// number of streams; the default is automatic (plan_streams).  NOTES/rounds-1-5.md 4.11.
extern "C" void lqrhip_set_sub_batches(int n) { g_knobs.sub_batches = n > 0 ? n : 0; }
extern "C" int lqrhip_sub_batches(int n)
{
    const char *q = getenv("GPU_MAX_HW_QUEUES");        // (at every call: a host may still set it until the GPU runtime comes up)
    g_dev.hw_queues = q ? atoi(q) : 0;
    return plan_streams(g_knobs, g_dev, n);
}

extern "C" void lqrhip_batch_set_shared(LqrHipBatch *b, int shared) { b->shared = shared != 0; b->shared_n = shared > 1 ? shared : 1; }
extern "C" void lqrhip_batch_set_safe(LqrHipBatch *b, int safe) { b->safe = safe != 0; if (safe) g_fault_stats[6]++; }

// A group is opened and closed around every resize (host/lqr_carver.c group_open / group_close), and creating a stream, a raw hipMalloc,
// destroying the stream and a raw hipFree -- which waits for the device -- per sub-batch were part of every call.  A destroyed batch parks
// its stream (idle: it has been synchronised) and its descriptor block here instead, and the next batch takes them: a parked stream is
// reused before a new one is created, so the process holds no more streams than its largest group had.  Descriptor blocks stay outside
// the counted allocator (they are no failure point of the allocation sweeps and lqrhip_debug_pool_live does not see them).
// lqrhip_pool_trim gives both back.
static const size_t MAX_PARKED = 4;                         // the most sub-batch streams a group runs on (plan_streams)
static std::vector<hipStream_t> g_parked_streams;
static unsigned long long g_fixed_stats[3];           // test hook (lqrhip_debug_fixedcost): [0] batch streams taken from the parked ones, [1] carvers reset by k_reset_jobs, [2] by the runtime's copy and fill
static std::multimap<size_t, DevCarver *> g_parked_desc;    // by capacity in descriptors
extern "C" void lqrhip_debug_fixedcost(unsigned long long out4[4], int reset)
{
    out4[0] = g_parked_streams.size();
    for (int i = 0; i < 3; i++) out4[i + 1] = g_fixed_stats[i];
    if (reset) memset(g_fixed_stats, 0, sizeof g_fixed_stats);
}
static void unpark_all(void)
{
    for (hipStream_t s : g_parked_streams) (void) hipStreamDestroy(s);
    g_parked_streams.clear();
    for (auto &kv : g_parked_desc) (void) hipFree(kv.second);
    g_parked_desc.clear();
}

extern "C" LqrHipBatch *lqrhip_batch_create(LqrHipCarver **carvers, int n)
{
    if (lqrhip_init() < 0 || n <= 0) return nullptr;
    LqrHipBatch *b = new LqrHipBatch();
    for (int i = 0; i < n; i++) {
        b->cs.push_back(carvers[i]);
        carvers[i]->batch = b;
    }
    hipError_t e = hipSuccess;
    if (!g_parked_streams.empty()) { b->stream = g_parked_streams.back(); g_parked_streams.pop_back(); g_fixed_stats[0]++; }
    else e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        auto it = g_parked_desc.lower_bound((size_t) n);        // the smallest parked block that holds n
        if (it != g_parked_desc.end()) { b->d_desc = it->second; b->desc_cap = it->first; g_parked_desc.erase(it); }
        else if ((e = hipMalloc((void **) &b->d_desc, sizeof(DevCarver) * n)) == hipSuccess) b->desc_cap = (size_t) n;
    }
    if (e != hipSuccess) {
        g_err = "batch_create failed";
        (void) hipGetLastError();
        if (b->stream) (void) hipStreamDestroy(b->stream);
        for (auto *c : b->cs) if (c->batch == b) c->batch = nullptr;
        delete b;
        return nullptr;
    }
    g_live_batches.push_back(b);
    return b;
}

static void invalidate_all_batches(void)
{
    for (auto *b : g_live_batches) { b->exch_ntiles = 0; b->dirty = true; }
}

// after a failed resize: drain the stream, drop whatever the kernels recorded (it belongs to the failed call, the next
// resize must not report it), lay everything out afresh
extern "C" void lqrhip_batch_abort(LqrHipBatch *b)
{
    if (!b) return;
    (void) hipStreamSynchronize(b->stream);
    (void) hipGetLastError();
    b->pending_inflate.reset();
    if (g_dev_err_host) *g_dev_err_host = 0;
    invalidate_all_batches();
}

extern "C" void lqrhip_batch_destroy(LqrHipBatch *b)
{
    if (!b) return;
    g_live_batches.erase(std::remove(g_live_batches.begin(), g_live_batches.end(), b), g_live_batches.end());
    if (b->stream) (void) hipStreamSynchronize(b->stream);
    for (auto *c : b->cs) if (c->batch == b) c->batch = nullptr;
    if (b->stream) {
        if (g_parked_streams.size() < MAX_PARKED) g_parked_streams.push_back(b->stream);
        else (void) hipStreamDestroy(b->stream);
    }
    if (b->d_desc) {
        if (g_parked_desc.size() < MAX_PARKED) g_parked_desc.emplace(b->desc_cap, b->d_desc);
        else (void) hipFree(b->d_desc);
    }
    delete b;
}

extern "C" int lqrhip_batch_sync(LqrHipBatch *b)
{
    HIPCK(hipStreamSynchronize(b->stream));
    return check_dev_error();
}
extern "C" void *lqrhip_batch_stream(LqrHipBatch *b) { return (void *) b->stream; }

static DevCarver make_desc(const LqrHipCarver *c)
{
    DevCarver d;
    const WorkingPlanes &k = c->wk;
    d.rgb0 = c->rgb0; d.vs = vs_of(c); d.bias0 = c->bias0; d.rig0 = c->rig0;
    d.pix = k.pix; d.en = k.en; d.m = k.m; d.least = k.least; d.m2 = k.m2; d.least2 = k.least2; d.bias = k.bias; d.rig = k.rig;
    d.seam_x = k.seam_x; d.seam_log = k.seam_log; d.flags = k.flags;
    d.vp_map = k.vp_map; d.vp_path = k.vp_path;
    return d;
}

static int batch_upload(LqrHipBatch *b)
{
    if (!b->dirty) return 0;
    std::vector<DevCarver> h;
    for (auto *c : b->cs) h.push_back(make_desc(c));
    HIPCK(hipStreamSynchronize(b->stream));
    HIPCK(hipMemcpy(b->d_desc, h.data(), sizeof(DevCarver) * h.size(), hipMemcpyHostToDevice));
    b->dirty = false;
    return 0;
}

static DpK make_dpk(const LqrHipDpParams *p, int ch)
{
    DpK k;
    k.delta = p->delta_x; k.use_rig = p->use_rigidity;
    memcpy(k.rigmap, p->rigidity_map, sizeof k.rigmap);
    k.nrg = p->nrg_func; k.radius = p->nrg_radius; k.w_start = p->w_start; k.ch = ch;
    return k;
}

struct ProfScope {
    ProfRec *rec = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t s;
    ProfScope(const char *name, hipStream_t stream, double bytes) : s(stream)
    {
        // every timed scope costs ~10 us of queue time (two event packets): mode 2 keeps that to the one
        // kernel whose launch time the bench line needs
        if (!g_prof || (g_prof == 2 && strcmp(name, "carve") != 0)) return;
        rec = &g_profrec[name];
        rec->bytes += bytes;
        (void) hipEventCreate(&e0); (void) hipEventCreate(&e1);
        (void) hipEventRecord(e0, s);
    }
    ~ProfScope()
    {
        if (!rec) return;
        (void) hipEventRecord(e1, s);
        rec->ev.emplace_back(e0, e1);
    }
};

extern "C" void lqrhip_prof_enable(int on) { g_prof = on; }
extern "C" void lqrhip_prof_reset(void)
{
    for (auto &kv : g_profrec) for (auto &e : kv.second.ev) { (void) hipEventDestroy(e.first); (void) hipEventDestroy(e.second); }
    g_profrec.clear();
}
extern "C" int lqrhip_prof_get(const char *kernel, double *ms_total, long long *launches, double *bytes_total)
{
    auto it = g_profrec.find(kernel);
    *ms_total = 0; *launches = 0; *bytes_total = 0;
    if (it == g_profrec.end()) return 0;
    (void) hipDeviceSynchronize();
    for (auto &e : it->second.ev) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) *ms_total += ms;
    }
    *launches = (long long) it->second.ev.size();
    *bytes_total = it->second.bytes;
    return 0;
}

// Time during which at least one launch of `kernel` was running: with sub-batch streams launches overlap each other and
// other kernels, and bytes / (sum of launch times) would count the overlapped time twice.  Event times are taken relative
// to the first recorded event of the kernel (the GPU's clock is common to all streams).
extern "C" int lqrhip_prof_get_union(const char *kernel, double *ms_union)
{
    *ms_union = 0;
    auto it = g_profrec.find(kernel);
    if (it == g_profrec.end() || it->second.ev.empty()) return 0;
    (void) hipDeviceSynchronize();
    const hipEvent_t base = it->second.ev[0].first;
    std::vector<std::pair<float, float>> iv;
    for (auto &e : it->second.ev) {
        float a = 0, b = 0;
        // an event recorded before `base` on another stream gives a negative time: both orders are tried
        if (hipEventElapsedTime(&a, base, e.first) != hipSuccess) { (void) hipGetLastError(); float t = 0; if (hipEventElapsedTime(&t, e.first, base) == hipSuccess) a = -t; else (void) hipGetLastError(); }
        if (hipEventElapsedTime(&b, base, e.second) != hipSuccess) { (void) hipGetLastError(); float t = 0; if (hipEventElapsedTime(&t, e.second, base) == hipSuccess) b = -t; else (void) hipGetLastError(); }
        iv.emplace_back(a, b);
    }
    std::sort(iv.begin(), iv.end());
    float end = -1e30f;
    for (auto &p : iv) {
        if (p.first > end) { *ms_union += p.second - p.first; end = p.second; }
        else if (p.second > end) { *ms_union += p.second - end; end = p.second; }
    }
    return 0;
}

static int pay_catchup(LqrHipBatch *b);
// what comes before the launch that lays the working planes of a batch out: carvers of one shape and pixel kind, their planes
// allocated, the descriptors on the device, no catch-up owed to planes that are about to be overwritten
static int wk_init_prepare(LqrHipBatch *b)
{
    LqrHipCarver *c0 = b->cs[0];
    int w = c0->w0, h = c0->h0, rc;
    for (auto *c : b->cs) {
        if (c->w0 != w || c->h0 != h || c->ch != c0->ch || c->depth != c0->depth || c->luma != c0->luma || c->mode != c0->mode ||
            c->alpha != c0->alpha || c->black != c0->black)
            return LQRHIP_EARG;
        if ((rc = ensure_working(c, w, h))) return rc;
    }
    if ((rc = batch_upload(b))) return rc;
    for (auto *c : b->cs) drop_catchup(c);
    return 0;
}
extern "C" int lqrhip_wk_init(LqrHipBatch *b, int from_visible)
{
    LqrHipCarver *c0 = b->cs[0];
    int w = c0->w0, h = c0->h0, rc;
    if ((rc = wk_init_prepare(b))) return rc;
    const dim3 grid(tiles_of(c0->stride, 256), h, (unsigned) b->cs.size()), grid_v(h, (unsigned) b->cs.size());
#define LAUNCH_WK(FORM, arg) do { if (from_visible) hipLaunchKernelGGL(k_wk_init_visible<FORM>, grid_v, dim3(256), 0, b->stream, b->d_desc, w, h, c0->stride, arg); \
                                  else hipLaunchKernelGGL(k_wk_init<FORM>, grid, dim3(256), 0, b->stream, b->d_desc, w, h, c0->stride, arg); } while (0)
    if (!reads_value(c0)) LAUNCH_WK(PixPacked, c0->ch);
    else if (c0->depth == 0) LAUNCH_WK(PixValue<0>, deep_read(c0));
    else if (c0->depth == 1) LAUNCH_WK(PixValue<1>, deep_read(c0));
    else if (c0->depth == 2) LAUNCH_WK(PixValue<2>, deep_read(c0));
    else LAUNCH_WK(PixValue<3>, deep_read(c0));
#undef LAUNCH_WK
    HIPCK(hipGetLastError());
    return 0;
}

extern "C" int lqrhip_emap_build(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h)
{
    int rc;
    if ((rc = pay_catchup(b))) return rc;           // the energy reads pix / bias in the carved frame
    if ((rc = batch_upload(b))) return rc;
    LqrHipCarver *c0 = b->cs[0];
    dim3 grid(tiles_of(w, 256), h, (unsigned) b->cs.size());
    DpK k = make_dpk(p, c0->ch);
    const bool value = reads_value(c0);
    const int nrg = plane_nrg(value, nrg_index(p->nrg_func));
#define CASE(N, V) if (nrg == N && value == V) hipLaunchKernelGGL((k_emap_full<N, V>), grid, dim3(256), 0, b->stream, b->d_desc, k, w, h, c0->stride); else
    K_EMAP_FORMS(CASE) return no_form("k_emap_full");
#undef CASE
    HIPCK(hipGetLastError());
    return 0;
}

// lqrhip_wk_init(b, 0) and lqrhip_emap_build(b, p, w, h) of a session that starts on flat carvers.  Packed pixels in the frame the
// planes are laid out in: ONE pass (k_wk_init_emap) -- the packed plane is written and not read back, a pixel's brightness is
// formed once (64 x 4K: 1.36 + 2.29 ms -> 1.58 ms, profiles/onestream/README.md).  Value planes, another frame: the two launches.
extern "C" int lqrhip_wk_init_emap(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h)
{
    LqrHipCarver *c0 = b->cs[0];
    int rc;
    if (reads_value(c0) || w != c0->w0 || h != c0->h0) return (rc = lqrhip_wk_init(b, 0)) ? rc : lqrhip_emap_build(b, p, w, h);
    if ((rc = wk_init_prepare(b))) return rc;
    const dim3 grid(tiles_of(tiles_of(c0->stride, 4), 256), h, (unsigned) b->cs.size());
    DpK k = make_dpk(p, c0->ch);
    const int nrg = nrg_index(p->nrg_func);
#define CASE(N) if (nrg == N) hipLaunchKernelGGL(k_wk_init_emap<N>, grid, dim3(256), 0, b->stream, b->d_desc, k, w, h, c0->stride); else
    K_WK_INIT_EMAP_FORMS(CASE) return no_form("k_wk_init_emap");
#undef CASE
    HIPCK(hipGetLastError());
    return 0;
}

// ---- energy read-outs (include/lqr_energy.h; kernels in k_energy_out.hip) -------------------------
extern "C" int lqrhip_energy_out(LqrHipBatch *b, int w, int h, int transposed, int form, int depth, int image_type, void *out, int on_device)
{
    static const int channels_of[7] = {3, 4, 1, 2, 3, 4, 5};        // RGB RGBA GREY GREYA CMY CMYK CMYKA
    if (b->cs.size() != 1 || !out || w < 1 || h < 1 || form < 0 || form > 2) { g_err = "energy read-out: one carver, a buffer, form 0 .. 2"; return LQRHIP_EARG; }
    if (form != 2) { depth = 2; image_type = 2; }                   // a float per pixel
    if (depth < 0 || depth > 3 || image_type < 0 || image_type > 6) { g_err = "energy read-out: depth 0 .. 3, image type 0 .. 6"; return LQRHIP_EARG; }
    int rc;
    if ((rc = batch_upload(b))) return rc;
    LqrHipCarver *c0 = b->cs[0];
    if (!c0->wk.en) return LQRHIP_EARG;
    const size_t bytes = (size_t) w * h * channels_of[image_type] << depth;
    const int chunks = (w + EO_CHUNK - 1) / EO_CHUNK;
    const int n_partials = form ? (int) std::min((long long) EO_MAX_PARTIALS, (long long) h * chunks) : 0;
    Scratch tmp(b->stream);
    float *partials = form ? tmp.get<float>((size_t) 2 * n_partials, "&partials", rc) : nullptr;
    if (rc) return rc;
    uint8_t *staged = on_device ? nullptr : tmp.get<uint8_t>(bytes, "&staged", rc);
    if (rc) return rc;
    uint8_t *dst = on_device ? (uint8_t *) out : staged;
    {
        // ("energy_out" in lqrhip_prof_get: the output stage alone, with the bytes it reads and writes)
        ProfScope prof("energy_out", b->stream, (double) w * h * sizeof(float) * (form ? 2 : 1) + (double) bytes);
        if (form == 1) hipLaunchKernelGGL(k_energy_range<false>, dim3(n_partials), dim3(256), 0, b->stream, b->d_desc, w, h, c0->stride, partials);
        if (form == 2) hipLaunchKernelGGL(k_energy_range<true>, dim3(n_partials), dim3(256), 0, b->stream, b->d_desc, w, h, c0->stride, partials);
        const int W = transposed ? h : w, H = transposed ? w : h;
        const dim3 grid((W + EO_TILE - 1) / EO_TILE, (H + EO_TILE - 1) / EO_TILE);
#define CASE(T, D) if (image_type == T && depth == D) hipLaunchKernelGGL((k_energy_out<T, D>), grid, dim3(256), 0, b->stream, b->d_desc, w, h, c0->stride, transposed, partials, n_partials, dst); else
        if (form != 2)
            hipLaunchKernelGGL(k_energy_plane, grid, dim3(256), 0, b->stream, b->d_desc, w, h, c0->stride, transposed, form, partials, n_partials, (float *) dst);
        else K_ENERGY_OUT_FORMS(CASE) return no_form("k_energy_out");
#undef CASE
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) { g_err = std::string("energy read-out: ") + hipGetErrorString(e); (void) hipGetLastError(); return LQRHIP_EHIP; }
    if ((rc = check_dev_error())) return rc;
    if (!on_device && (rc = d2h_staged(out, staged, bytes))) return rc;
    tmp.done();
    return 0;
}

// E5 as H/32 dependent launches of one wave per 192-column tile (any batch size)
static int launch_dp_tiled(LqrHipBatch *b, const DpK &k, int w, int h, int lr)
{
    LqrHipCarver *c0 = b->cs[0];
    const dim3 grid(tiles_of(w, DPT_OWN), (unsigned) b->cs.size());
    for (int y0 = 0; y0 < h; y0 += DPT_ROWS) {
        CENSUS(LQRHIP_CENSUS_DP_TILE);
#define CASE(LRV, RIGV) if ((lr != 0) == LRV && (k.use_rig != 0) == RIGV) hipLaunchKernelGGL((k_dp_tile<LRV, RIGV>), grid, dim3(64), 0, b->stream, b->d_desc, k, w, h, c0->stride, y0); else
        K_LR_RIG_FORMS(CASE) return no_form("k_dp_tile");
#undef CASE
    }
    HIPCK(hipGetLastError());
    return 0;
}

// ---- the choice of kernel forms: lqr_plan.h decides, from these ------------------------------------------------------------------
// The test hooks' argument mappings (include/lqr_hip.h); what each knob does is said at its field of PlanKnobs
extern "C" void lqrhip_set_vpath_mode(int mode, int par_max) { g_knobs.vpath_mode = mode; if (par_max > 0) g_knobs.vpath_par_max = par_max; }
extern "C" void lqrhip_set_sweep_threads(int n) { g_knobs.sweep_threads = n == 256 ? 256 : DP_THREADS; }
extern "C" void lqrhip_set_carve_fused(int max_images) { g_knobs.carve_fused = max_images == 1 ? 4 : max_images < 0 ? 0 : max_images; }
extern "C" void lqrhip_set_carve_beside(int mode) { g_knobs.carve_beside = mode < 0 ? -1 : mode ? 1 : 0; }
static unsigned long long g_carve_beside_launches;          // k_carve_u launches (they are counted under LQRHIP_CENSUS_CARVE as well)
extern "C" unsigned long long lqrhip_carve_beside_launches(int reset)
{
    const unsigned long long v = g_carve_beside_launches;
    if (reset) g_carve_beside_launches = 0;
    return v;
}
extern "C" void lqrhip_set_backtrack_beside(int mode) { g_knobs.backtrack_beside = mode < 0 ? -1 : mode ? 1 : 0; }
static unsigned long long g_backtrack_beside_launches;      // k_carve_v launches (counted under LQRHIP_CENSUS_VPATH1, _CARVE and as carve-beside launches as well)
extern "C" unsigned long long lqrhip_backtrack_beside_launches(int reset)
{
    const unsigned long long v = g_backtrack_beside_launches;
    if (reset) g_backtrack_beside_launches = 0;
    return v;
}
extern "C" void lqrhip_set_update_mode(int mode) { g_knobs.update_mode = mode; }
extern "C" void lqrhip_set_dp_persistent_px(int px) { g_knobs.dpp_px = (px == 2 || px == 3 || px == 4) ? px : 0; }
// (0 sends every full DP to k_dp_tile and every incremental update to a band kernel)
extern "C" void lqrhip_set_dp_persistent_limit(int workgroups) { g_knobs.dpp_limit = workgroups; }
extern "C" void lqrhip_set_band_levels(int slots) { g_knobs.band_levels = slots; }
extern "C" void lqrhip_set_levels_wg_slots(int slots) { g_knobs.levels_wg_slots = slots == 1 || slots == 2 ? slots : -1; }
extern "C" void lqrhip_set_carve_line(int mode) { g_knobs.carve_line = mode == 0 || mode == 1 ? mode : -1; }
extern "C" void lqrhip_set_levels_store(int mode) { g_knobs.levels_store = mode == 0 || mode == 1 ? mode : -1; lqr_levels_report_rows(g_knobs.levels_store >= 0); }
static unsigned long long g_levels_pair_launches = 0;
extern "C" unsigned long long lqrhip_levels_pair_launches(int reset) { const unsigned long long n = g_levels_pair_launches; if (reset) g_levels_pair_launches = 0; return n; }
static PlanBatch plan_batch(const LqrHipBatch *b)
{
    PlanBatch pb;
    pb.images = (int) b->cs.size(); pb.shared = b->shared; pb.shared_n = b->shared_n; pb.spin = !(b->safe || g_no_spin);
    pb.wk_h = b->cs[0]->wk_h; pb.value = reads_value(b->cs[0]);
    for (auto *c : b->cs) pb.rigmask |= c->wk.rig != nullptr;
    return pb;
}
extern "C" int lqrhip_general_batch_limit_delta(int w, int delta)
{
    return lqrhip_init() < 0 || w < 1 ? 0 : plan_general_batch_limit(g_knobs, g_dev, w, delta);         // 0: no bound known
}
extern "C" int lqrhip_general_batch_limit(int w) { return lqrhip_general_batch_limit_delta(w, 2); }

// Grow a pair of buffers that every carver of the batch owns one of: ready(c) says that carver c has its pair, make(c) allocates it.  The stream
// is drained once, before the first pair is made (what is in use goes back to the pool); if any was made, the descriptors are uploaded again
template <class Ready, class Make> static int grow_pairs(LqrHipBatch *b, Ready ready, Make make)
{
    int rc;
    bool grew = false;
    for (auto *c : b->cs) {
        if (ready(c)) continue;
        if (!grew) { HIPCK(hipStreamSynchronize(b->stream)); grew = true; }
        if ((rc = make(c))) return rc;
    }
    if (!grew) return 0;
    b->dirty = true;
    return batch_upload(b);
}

// Grow and (re)lay a batch's exchange area for a spinning kernel: `near_off` words and their near copies for `ntiles` tiles of each of
// `n` images, in the layout `layout` (lqr_geom.h: exch_layout_dpp, EXCH_LAYOUT_LEVELS).  Tags and finished-tile
// counters start at 0; afterwards nothing is ever cleared: tags carry the launch epoch, the last tile re-arms the counter
static int exch_ensure(LqrHipBatch *b, size_t near_off, int ntiles, int n, int layout)
{
    int rc;
    bool grew = false;
    const size_t need_elems = exch_words(near_off, (size_t) n);
    if (b->exch.size() < need_elems) HIPCK(hipStreamSynchronize(b->stream));     // (the area in use goes back to the pool)
    if ((rc = b->exch.ensure(need_elems, "&b->exch", &grew))) return rc;
    if (grew) b->exch_ntiles = 0;
    if (b->exch_ntiles != ntiles || b->exch_n != n || b->exch_px != layout) {
        HIPCK(hipMemsetAsync(b->exch, 0, need_elems * sizeof(unsigned long long), b->stream));
        b->exch_ntiles = ntiles; b->exch_n = n; b->exch_px = layout;
    }
    return 0;
}

// The <LR, RIG, DELTA, RIGM> of the spinning DP kernels (k_dp_tile_p, k_band_levels) for a batch's run-time values.
// delta_x 5 .. 10 (round 6): the rigidity form only -- without rigidity the host's table is all zeros, and x + 0.0f is x for every
// candidate (no cumulative minimum is -0.0f: energies are sums of non-negative gradients and finite biases).
// A mask matters with rigidity only (PlanBatch::rigm), so a mask at delta_x 1 is <true, true, 1, true> and nothing else.
struct DpForm { bool lr, rig; int delta; bool rigm; };
static inline DpForm dp_form(const DpK &k, int lr, bool rigm) { return DpForm{lr != 0, k.use_rig != 0 || k.delta >= 5, k.delta, rigm}; }

// E5 (UPDATE = false) or the full-width form of E9 (UPDATE = true) as one persistent launch in the plan's geometry
// (first, count): a range of the batch's images (E5 only: a general batch too large for one persistent grid is swept group after group)
template <bool UPDATE>
static int launch_dp_persistent(LqrHipBatch *b, const DpK &k, const DpPlan &dp, bool rigm, int w, int h, int lr, int first, int count)
{
    LqrHipCarver *c0 = b->cs[0];
    const size_t n = (size_t) count;
    const int px = dp.px;
    if (!px || (UPDATE && n != b->cs.size())) return LQRHIP_EARG;
    const int ntiles = dpp_tiles(w, px);
    int rc;
    if ((rc = exch_ensure(b, dpp_near_off(ntiles, px), ntiles, (int) n, exch_layout_dpp(px)))) return rc;
    // the second planes, allocated on first use -- per carver: a batch may mix carvers that already went through a tiled update on their
    // own with fresh ones
    auto make_second = [&](LqrHipCarver *c) -> int {
        const size_t pe = plane_elems(c->stride, c->wk_h);
        // m2 and least2 are made here and dropped in free_working, both times as a pair; the carver gets the zeroed pair or
        // nothing, so that a plane that was never zeroed cannot pass for an old one
        DevBuf<float> m2;
        DevBuf<int8_t> least2;
        int err;
        if ((err = m2.alloc(pe, "&c->m2")) || (err = least2.alloc(pe, "&c->least2"))) return err;
        // like the first planes (ensure_working): nothing in them depends on what the block held before
        hipError_t e = hipMemsetAsync(m2, 0, pe * sizeof(float), b->stream);
        if (e == hipSuccess) e = hipMemsetAsync(least2, 0, pe, b->stream);
        if (e != hipSuccess) { lqr_stream_wait(b->stream); HIPCK(e); }
        c->wk.m2 = std::move(m2); c->wk.least2 = std::move(least2);
        return 0;
    };
    if (UPDATE && (rc = grow_pairs(b, [](LqrHipCarver *c) { return c->wk.m2 && c->wk.least2; }, make_second))) return rc;
    const int epoch = dpp_epoch(b->tile_epoch++);
    const dim3 grid(ntiles, (unsigned) n);
    CENSUS(dp.general ? LQRHIP_CENSUS_TILE_P_GENERAL : px == 3 ? LQRHIP_CENSUS_TILE_P_G3 : px == 2 ? LQRHIP_CENSUS_TILE_P_G2 : LQRHIP_CENSUS_TILE_P_G4);
    // px code 3 is 2 px per lane with the 24-halo-lane geometry; the general forms exist for 2 px per lane only (plan_persistent_px)
    const DpForm f = dp_form(k, lr, rigm);
    const int px_lane = px == 4 ? 4 : 2, hln = px == 3 ? 24 : 16;
    const bool found = [&] {
#define CASE(CLASS, PX, LR, RIG, UPD, DELTA, RIGM, HLN)                                                                         \
        if constexpr (UPD == UPDATE)                                                                                            \
            if (px_lane == PX && f.lr == LR && f.rig == RIG && f.delta == DELTA && f.rigm == RIGM && hln == HLN) {              \
                hipLaunchKernelGGL((k_dp_tile_p<PX, LR, RIG, UPD, DELTA, RIGM, HLN>), grid, dim3(64 * DPP_W), 0, b->stream, b->d_desc + first, k, w, h, c0->stride, b->exch.get(), epoch, g_dev_err); \
                return true;                                                                                                    \
            }
        K_DP_TILE_P_FORMS(CASE)
#undef CASE
        return false;
    }();
    if (!found) return no_form("k_dp_tile_p");
    HIPCK(hipGetLastError());
    if (UPDATE)       // the kernel's last tile swapped the pointers in the device descriptors: mirror it
        for (auto *c : b->cs) { std::swap(c->wk.m, c->wk.m2); std::swap(c->wk.least, c->wk.least2); }
    return 0;
}

// One DP launch sequence as planned (plan_full_dp, plan_seam_step): E5 (UPDATE = false) or what E9 runs over the full width
template <bool UPDATE>
static int launch_dp(LqrHipBatch *b, const DpK &k, const DpPlan &dp, bool rigm, int w, int h, int lr)
{
    LqrHipCarver *c0 = b->cs[0];
    if (dp.form == LQRHIP_CENSUS_DP_TILE) return launch_dp_tiled(b, k, w, h, lr);
    if (dp.form != LQRHIP_CENSUS_SWEEP_FULL && dp.form != LQRHIP_CENSUS_SWEEP_UPDATE) {
        const int total = (int) b->cs.size();
        int rc;
        for (int first = 0; first < total; first += std::max(dp.per, 1))
            if ((rc = launch_dp_persistent<UPDATE>(b, k, dp, rigm, w, h, lr, first, std::min(dp.per, total - first)))) return rc;
        return 0;
    }
    dim3 grid((unsigned) b->cs.size());
    auto launch = [&](auto kern, int P, int T) -> int {
        if (lds_needs_attr(dp.lds)) {
            HIPCK(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) dp.lds));
            CENSUS(LQRHIP_CENSUS_LDS_ATTR_SWEEP);
        }
        CENSUS(LQRHIP_CENSUS_SWEEP + 2 * (P == 1 ? 0 : P == 2 ? 1 : P == 4 ? 2 : P == 8 ? 3 : 4) + (T == DP_THREADS ? 1 : 0));
        CENSUS(UPDATE ? LQRHIP_CENSUS_SWEEP_UPDATE : LQRHIP_CENSUS_SWEEP_FULL);
        hipLaunchKernelGGL(kern, grid, dim3(T), dp.lds, b->stream, b->d_desc, k, w, h, c0->stride, lr);
        HIPCK(hipGetLastError());
        return 0;
    };
    // only the update has the 256-thread forms
#define CASE(P) if (dp.px == P) { if constexpr (UPDATE) { if (dp.threads == 256) return launch(k_dp_sweep<P, true, 256>, P, 256); } return launch(k_dp_sweep<P, UPDATE, DP_THREADS>, P, DP_THREADS); }
    K_DP_SWEEP_PXT_FORMS(CASE)
#undef CASE
    g_err = "image wider than 16384 px is not supported";
    return LQRHIP_EARG;
}

extern "C" int lqrhip_mmap_build(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h, int leftright)
{
    int rc;
    if ((rc = batch_upload(b))) return rc;
    if (p->delta_x > LQRHIP_MAX_DELTA) return LQRHIP_EARG;
    ProfScope ps("dp_sweep", b->stream, 9.0 * w * h * b->cs.size());
    const PlanBatch pb = plan_batch(b);
    const bool use_rig = p->use_rigidity != 0;
    return launch_dp<false>(b, make_dpk(p, b->cs[0]->ch), plan_full_dp(g_knobs, g_dev, pb, w, p->delta_x, use_rig), pb.rigm(use_rig), w, h, leftright);
}

// remove seams [frozen_epoch, to) from the frozen planes of carvers [first, first + count) of the batch, which are at the same epoch;
// the frame is w_at_to wide after seam to - 1
static int frozen_catchup(LqrHipBatch *b, size_t first, size_t count, int to, int w_at_to, int h)
{
    LqrHipCarver *c0 = b->cs[first];
    const int from = c0->frozen_epoch;
    if (to <= from) return 0;
    const int w_from = fc_w_from(from, to, w_at_to);
    with_form(c0, [&](auto value) {
        hipLaunchKernelGGL(k_frozen_catchup<value>, dim3(h, (unsigned) count), dim3(256), fc_lds(from, to, w_from), b->stream, b->d_desc + first, from, to, w_from, h, c0->stride);
    });
    HIPCK(hipGetLastError());
    for (size_t i = first; i < first + count; i++) b->cs[i]->frozen_epoch = to;
    return 0;
}

// The catch-up a session's end owes (lqrhip_vs_commit) is paid here, by the same launch on the batch's stream, before anything reads
// pix / bias in the carved frame (lqrhip_emap_build) and before the session's log is replaced (lqrhip_seam_log_reserve).  Whatever lays
// the planes out afresh instead (a reload, a flatten, a transpose, lqrhip_wk_init) drops the debt: there the pass was 1.1 ms per
// 16 images of 4K for nothing.
static int pay_catchup(LqrHipBatch *b)
{
    LqrHipCarver *c0 = b->cs[0];
    bool any = false, alike = true;
    for (auto *c : b->cs) {
        any |= c->owed_to > 0;
        alike &= c->owed_to == c0->owed_to && c->owed_w == c0->owed_w && c->owed_h == c0->owed_h && c->frozen_epoch == c0->frozen_epoch && c->stride == c0->stride;
    }
    if (!any) return 0;
    int rc;
    if ((rc = batch_upload(b))) return rc;
    // carvers that ended their last sessions in different batches (alone: a lag of 32; in a group: of 128) owe different ranges, and
    // the kernel takes one range per launch: then one launch per owing carver, each through its own descriptor of the table
    const size_t per = alike ? b->cs.size() : 1;
    for (size_t i = 0; i < b->cs.size(); i += per)
        if ((rc = frozen_catchup(b, i, per, b->cs[i]->owed_to, b->cs[i]->owed_w, b->cs[i]->owed_h))) return rc;
    for (auto *c : b->cs) drop_catchup(c);              // paid: the planes are in the carved frame, the log restarts at 0
    return 0;
}

static int launch_band_levels(LqrHipBatch *b, const DpK &k, int w, int h, int lr, int P, int wg_slots, int store_rows, bool rigm)
{
    LqrHipCarver *c0 = b->cs[0];
    const size_t n = b->cs.size();
    const int ntiles = lv_tiles(w);
    if (int rc = exch_ensure(b, lv_near_off(ntiles), ntiles, (int) n, EXCH_LAYOUT_LEVELS)) return rc;
    const int epoch = lv_epoch(b->tile_epoch++);
    const dim3 grid(lv_grid(n, P));
    CENSUS(LQRHIP_CENSUS_BAND_LEVELS);
    const DpForm f = dp_form(k, lr, rigm);
    if (wg_slots == 2) {            // two slots per workgroup (plan_levels_wg_slots: delta_x 1, no mask)
        const dim3 grid2(lv2_grid(n, P));
#define CASE(LR, RIG) if (f.lr == LR && f.rig == RIG && f.delta == 1 && !f.rigm) \
        hipLaunchKernelGGL((k_band_levels2<LR, RIG>), grid2, dim3(256), 0, b->stream, b->d_desc, k, w, h, c0->stride, b->exch.get(), epoch, g_dev_err, P, (int) n, store_rows); else
        K_BAND_LEVELS2_FORMS(CASE) return no_form("k_band_levels2");
#undef CASE
        HIPCK(hipGetLastError());
        g_levels_pair_launches++;
        return 0;
    }
#define CASE(LR, RIG, DELTA, RIGM) if (f.lr == LR && f.rig == RIG && f.delta == DELTA && f.rigm == RIGM) \
        hipLaunchKernelGGL((k_band_levels<LR, RIG, DELTA, RIGM>), grid, dim3(128), 0, b->stream, b->d_desc, k, w, h, c0->stride, b->exch.get(), epoch, g_dev_err, P, (int) n, store_rows); else
    K_BAND_LEVELS_FORMS(CASE) return no_form("k_band_levels");
#undef CASE
    HIPCK(hipGetLastError());
    return 0;
}
static void inject_after_step(LqrHipBatch *b, int h, int log_index);
static void inject_after_commit(LqrHipBatch *b, int w0, int h0, int first_level);
// ---- one seam step, stage by stage: each launcher runs one case of the step's plan (lqr_plan.h) over the step's values; sizes are lqr_geom.h's
struct StepVals {
    DpK k;
    int w, h, stride, log_index;    // the frame on entry; the seam's row of the log
    int lr_pick, lr_next;           // the side a tie goes to: in this seam's pick, in the DP for the next
    int move_dp;                    // the carve moves m and the back pointers too: an update follows, not a full DP
    int moved_unit;                 // bytes the carve moves per pixel of the side it moves (seam_step_impl)
    int epoch;                      // the frozen planes are in the frame before this seam of the log (catchup_within_lag moves it on)
    bool value, rigm;               // PlanBatch::value, PlanBatch::rigm(use_rigidity)
    unsigned n;                     // carvers
};
// the frozen planes lag too far: compact them up to this seam (needs the seam log only)
static int catchup_within_lag(LqrHipBatch *b, const StepPlan &s, StepVals &v)
{
    const int rc = s.catchup ? frozen_catchup(b, 0, b->cs.size(), v.log_index + 1, v.w - 1, v.h) : 0;
    v.epoch = b->cs[0]->frozen_epoch;
    return rc;
}
// the backtrack: the parallel pair, or the one-wave walk (beside the carve: the walk is a role of the carve's launch)
static int launch_backtrack(LqrHipBatch *b, const StepPlan &s, const StepVals &v)
{
    const int w = v.w, h = v.h, stride = v.stride, n = (int) v.n;
    if (s.backtrack == LQRHIP_CENSUS_VP_PARALLEL) {
        // the maps and paths, per carver, for this step's chunks (vp_path's size depends on delta_x: each answers for its own)
        const size_t need = vp_map_bytes(s.vp_chunks, stride), need_path = vp_path_bytes(s.vp_chunks, stride, s.vp_rows);
        if (int rc = grow_pairs(b, [&](LqrHipCarver *c) { return c->wk.vp_map.size() >= need && c->wk.vp_path.size() >= need_path; }, [&](LqrHipCarver *c) {
                c->wk.vp_map.reset(); c->wk.vp_path.reset();
                const int rc = c->wk.vp_map.alloc(need, "&c->vp_map");
                return rc ? rc : c->wk.vp_path.alloc(need_path, "&c->vp_path");
            })) return rc;
        ProfScope ps("vpath", b->stream, 0);
        CENSUS(LQRHIP_CENSUS_VP_PARALLEL);
        if (!with_listed(K_VP_FORMS, v.k.delta, [&](auto delta) {
                hipLaunchKernelGGL(k_vp_maps<delta>, dim3(vp_col_blocks(w), s.vp_chunks, n), dim3(256), 0, b->stream, b->d_desc, w, h, stride);
                hipLaunchKernelGGL(k_vp_solve<delta>, dim3(n), dim3(VPATH_THREADS), vp_solve_lds(s.vp_chunks), b->stream, b->d_desc, w, h, stride, v.lr_pick, v.log_index, v.moved_unit);
            })) return no_form("k_vp_maps");
    } else if (!s.backtrack_beside) {
        ProfScope ps("vpath", b->stream, 0);
        CENSUS(s.backtrack);
        // the one-wave walk: unrolled for the listed delta_x, the loop over candidates beyond (and for delta_x 0)
        if (!with_listed(K_VPATH1_FORMS, v.k.delta, [&](auto delta) {
                hipLaunchKernelGGL(k_vpath1<delta>, dim3(n), dim3(VPATH_THREADS), 0, b->stream, b->d_desc, w, h, stride, v.lr_pick, v.log_index, v.moved_unit);
            }))
            hipLaunchKernelGGL(k_vpath, dim3(n), dim3(VPATH_THREADS), 0, b->stream, b->d_desc, w, h, stride, v.lr_pick, v.k.delta, v.log_index, v.moved_unit);
    }
    return 0;
}
// the carve: with the energy update fused in, with the walk and the energy update beside it, with the energy update beside it, or plain.
// Algorithmic bytes of one carve launch: read + write of one 4-byte plane over the half of each row right of the seam
// = 8 B * w*h/2 per image, whichever form
static int launch_carve(LqrHipBatch *b, const StepPlan &s, StepVals &v)
{
    int rc;
    const int w = v.w, h = v.h, stride = v.stride, n = (int) v.n;
    const double bytes = 4.0 * (double) w * h * n;
    if (s.carve == LQRHIP_CENSUS_CARVE_E) {
        if ((rc = catchup_within_lag(b, s, v))) return rc;      // (before the carve)
        ProfScope ps("carve", b->stream, bytes);
        CENSUS(LQRHIP_CENSUS_CARVE_E);
        if (!with_listed(K_CARVE_E_FORMS, nrg_index(v.k.nrg), [&](auto nrg) {
                hipLaunchKernelGGL((k_carve_e<nrg>), dim3(bb_carve_entries(h), n), dim3(256), 0, b->stream, b->d_desc, v.k, w, h, stride, v.move_dp, v.log_index, v.epoch, s.carve_line);
            })) return no_form("k_carve_e");
    } else if (s.backtrack_beside) {
        // k_carve_v: the walks' workgroups first, then one consumer per entry of the work list the walks fill -- the carve's row-quads and
        // the energy update's blocks, in the order they become ready (k_carve.hip).  "vpath" and "emap_update" have no launch on this path.
        // (No catch-up here: the plan keeps the step that compacts the frozen planes on the separate launches)
        const size_t need = cv_list_words(n, h);
        if (b->wlist.size() < need) {
            bool grew = false;
            HIPCK(hipStreamSynchronize(b->stream));     // (the list in use goes back to the pool)
            if ((rc = b->wlist.ensure(need, "&b->wlist", &grew))) return rc;
            HIPCK(hipMemsetAsync(b->wlist, 0, need * sizeof(unsigned long long), b->stream));        // no tag, both tails at 0
        }
        unsigned long long *moved = lqr_moved_bytes_dev();
        if (!moved) { g_err = "k_carve_v: no address for the moved-bytes counter"; return LQRHIP_EHIP; }
        const unsigned tag = bb_tag(b->wlist_launches++);
        ProfScope ps("carve", b->stream, bytes);
        CENSUS(LQRHIP_CENSUS_VPATH1);
        CENSUS(LQRHIP_CENSUS_CARVE);
        g_carve_beside_launches++;
        g_backtrack_beside_launches++;
        bool launched = false;
        with_listed(K_CARVE_U_FORMS, nrg_index(v.k.nrg), [&](auto nrg) {
            launched = with_listed(K_CARVE_V_DELTAS, v.k.delta, [&](auto delta) {
                hipLaunchKernelGGL((k_carve_v<nrg, delta>), dim3(cv_grid(n, h)), dim3(256), 0, b->stream, b->d_desc, v.k, w, h, stride, v.lr_pick, v.move_dp, v.log_index, v.epoch,
                                   (int) n, v.moved_unit, tag, b->wlist.get(), moved, g_dev_err, s.carve_line);
            });
        });
        if (!launched) return no_form("k_carve_v");
    } else if (s.energy_beside) {
        // k_carve_u: the energy update's workgroups first, then the carve's, in one 1-D grid (k_carve.hip); "emap_update" has no launch on this path
        if ((rc = catchup_within_lag(b, s, v))) return rc;      // (before the carve)
        ProfScope ps("carve", b->stream, bytes);
        CENSUS(LQRHIP_CENSUS_CARVE);
        g_carve_beside_launches++;
        if (!with_listed(K_CARVE_U_FORMS, nrg_index(v.k.nrg), [&](auto nrg) {
                hipLaunchKernelGGL((k_carve_u<nrg>), dim3(cu_grid(n, h)), dim3(256), 0, b->stream, b->d_desc, v.k, w, h, stride, v.move_dp, v.log_index, v.epoch, (int) n, s.carve_line);
            })) return no_form("k_carve_u");
    } else {
        ProfScope ps("carve", b->stream, bytes);
        // (a grid of a half, a quarter, an eighth of the rows, the kernel striding over the rest, measured at 64 x 4K in round 5: 508 / 504 / 490 k
        // against 488 - 501 k: inside the run-to-run spread; not adopted)
        CENSUS(LQRHIP_CENSUS_CARVE);
        hipLaunchKernelGGL(k_carve, dim3(bb_carve_entries(h), n), dim3(256), 0, b->stream, b->d_desc, w, h, stride, v.k.delta, v.move_dp);
    }
    return 0;
}
// the energy update, where the carve's launch has not taken it
static int launch_energy(LqrHipBatch *b, const StepPlan &s, StepVals &v)
{
    if (s.carve == LQRHIP_CENSUS_CARVE_E || s.energy_beside) return 0;
    ProfScope ps("emap_update", b->stream, 0);
    if (int rc = catchup_within_lag(b, s, v)) return rc;
    const int h = v.h, stride = v.stride, wnew = v.w - 1, log_index = v.log_index, epoch = v.epoch, n = (int) v.n;
    const DpK &k = v.k;
    const bool value = v.value;
    const int nrg = plane_nrg(value, nrg_index(k.nrg)), nt = s.eu_nt;
#define CASE_NT(NT, N, V) if (nrg == N && value == V && nt == NT) hipLaunchKernelGGL((k_emap_update<N, NT, V>), dim3(bb_energy_entries(h), n), dim3(64), 0, b->stream, b->d_desc, k, wnew, h, stride, log_index, epoch); else
#define CASE(N, V) K_EMAP_UPDATE_NT_FORMS(CASE_NT, N, V)
    K_EMAP_FORMS(CASE) return no_form("k_emap_update");
#undef CASE
#undef CASE_NT
    return 0;
}
// the band stage: the kernel that updates the band the seam changed, and the sweep that takes the rows it hands over
static int launch_band(LqrHipBatch *b, const StepPlan &s, const StepVals &v)
{
    const int h = v.h, stride = v.stride, wnew = v.w - 1, leftright_next = v.lr_next, n = (int) v.n;
    const DpK &k = v.k;
    if (s.band == LQRHIP_CENSUS_BAND_LEVELS) {
        ProfScope ps("band_levels", b->stream, 0);
        if (int rc = launch_band_levels(b, k, wnew, h, leftright_next, s.levels_P, s.levels_wg_slots, s.levels_store, v.rigm)) return rc;
    } else if (s.band == LQRHIP_CENSUS_BAND_TW) {
        ProfScope ps("band_update", b->stream, 0);
        CENSUS(LQRHIP_CENSUS_BAND_TW);
#define CASE(LRV, RIGV) if ((leftright_next != 0) == LRV && (k.use_rig != 0) == RIGV) hipLaunchKernelGGL((k_band_update_tw<4, LRV, RIGV>), dim3(n), dim3(128 * 4), band_tw_lds(h), b->stream, b->d_desc, k, wnew, h, stride, g_dev_err); else
        K_LR_RIG_FORMS(CASE) return no_form("k_band_update_tw");
#undef CASE
        // (round 5: the kernel finishing the rows its window cannot hold itself, without the (almost always empty) k_dp_sweep<UPDATE>
        // launch behind it, was built and measured on one box: 527.5 / 523.5 k against 531 / 528 k -- the launch's 22 us reappear in
        // the kernels around it (k_vpath1 74 -> 92 us, k_carve 149 -> 162), the step is not the sum of a chain's kernels; removed)
    } else if (s.band == LQRHIP_CENSUS_BAND_MW8 || s.band == LQRHIP_CENSUS_BAND_MW16) {
        ProfScope ps("band_update", b->stream, 0);
        const int nw = s.band == LQRHIP_CENSUS_BAND_MW16 ? 16 : 8;
        CENSUS(nw == 16 ? LQRHIP_CENSUS_BAND_MW16 : LQRHIP_CENSUS_BAND_MW8);
#define CASE_NW(NWV, LRV, RIGV) if (nw == NWV && (leftright_next != 0) == LRV && (k.use_rig != 0) == RIGV) hipLaunchKernelGGL((k_band_update_mw<2, NWV, 8, LRV, RIGV>), dim3(n), dim3(64 * NWV), band_mw_lds(h), b->stream, b->d_desc, k, wnew, h, stride); else
#define CASE(LRV, RIGV) CASE_NW(8, LRV, RIGV) CASE_NW(16, LRV, RIGV)
        K_LR_RIG_FORMS(CASE) return no_form("k_band_update_mw");
#undef CASE
#undef CASE_NW
    } else {
        ProfScope ps("band_update", b->stream, 0);
        CENSUS(LQRHIP_CENSUS_BAND_GENERIC);
        hipLaunchKernelGGL(k_band_update, dim3(n), dim3(64), 0, b->stream, b->d_desc, k, wnew, h, stride, leftright_next);
    }
    // rows the band kernel handed over (flags[FLAG_OVF_ROW] .. h): the keep rule over the full width
    ProfScope ps("dp_update", b->stream, 0);
    return launch_dp<true>(b, k, s.dp, v.rigm, wnew, h, leftright_next);
}

// One seam of a lock-step batch: k_vpath* (pick + backtrack, publishes the side to move) -> k_carve ->
// k_emap_update -> one form of update_mmap (or the full DP after a side switch), all on the batch's stream.
static int seam_step_impl(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h, int log_index, int leftright_pick,
                          int full_rebuild, int leftright_next)
{
    int rc;
    LqrHipCarver *c0 = b->cs[0];
    for (auto *c : b->cs)
        if (log_index >= c->log_cap || c->owed_to) return LQRHIP_EARG;     // (a carver that owes a catch-up never meets the new session's log)
    if ((rc = batch_upload(b))) return rc;
    // every choice of this step (lqr_plan.h): the launchers run one case of the plan each
    const PlanBatch pb = plan_batch(b);
    const StepPlan s = plan_seam_step(g_knobs, g_dev, pb, p->delta_x, p->use_rigidity != 0, w, h, full_rebuild != 0, log_index + 1 - c0->frozen_epoch);
    const int wnew = w - 1, move_dp = (wnew > 1 && !full_rebuild) ? 1 : 0;
    // bytes the carve moves per pixel of the side it moves, read + write: en 4 (+ m 4 + back pointer 1 unless a full DP follows,
    // + the rigidity mask 4) -- k_vpath* knows how many pixels that is for the seam it finds and keeps the sum (lqrhip_moved_bytes)
    const int moved_unit = 2 * (4 + (move_dp ? 5 : 0) + (pb.rigmask ? 4 : 0));
    StepVals v{make_dpk(p, c0->ch), w, h, c0->stride, log_index, leftright_pick, leftright_next, move_dp, moved_unit, c0->frozen_epoch,
               pb.value, pb.rigm(p->use_rigidity != 0), (unsigned) b->cs.size()};
    if ((rc = launch_backtrack(b, s, v)) || (rc = launch_carve(b, s, v))) return rc;
    if (s.dp.form < 0) { HIPCK(hipGetLastError()); return 0; }          // liblqr's finish_vsmap case: nothing left to update
    if ((rc = launch_energy(b, s, v))) return rc;
    if (s.full || s.band < 0) {         // the full DP after a side switch, or E9 as the tiled full-width update: that launch alone
        ProfScope ps(s.full ? "dp_sweep" : "dp_update_tiled", b->stream, s.full ? 9.0 * wnew * h * v.n : 0);
        rc = s.full ? launch_dp<false>(b, v.k, s.dp, v.rigm, wnew, h, leftright_next) : launch_dp<true>(b, v.k, s.dp, v.rigm, wnew, h, leftright_next);
    } else rc = launch_band(b, s, v);
    if (rc) return rc;
    HIPCK(hipGetLastError());
    return 0;
}

// LQRHIP_DUMP=<prefix> (debugging aid): after every seam step the first image's seam, flags and DP planes go to
// <prefix>_<call>.bin -- header {w, h, stride, log_index, FLAG_COUNT}, flags, seam_x[h], m[stride * h], least[stride * h]
extern "C" int lqrhip_seam_step(LqrHipBatch *b, const LqrHipDpParams *p, int w, int h, int log_index, int leftright_pick,
                                int full_rebuild, int leftright_next)
{
    const int rc = seam_step_impl(b, p, w, h, log_index, leftright_pick, full_rebuild, leftright_next);
    if (rc == 0) inject_after_step(b, h, log_index);
    static const char *dump = getenv("LQRHIP_DUMP");
    if (rc == 0 && dump) {
        static int call = 0;
        LqrHipCarver *c = b->cs[0];
        HIPCK(hipStreamSynchronize(b->stream));
        const size_t np = (size_t) c->stride * h;
        std::vector<int> hdr = {w, h, c->stride, log_index, FLAG_COUNT}, flags(FLAG_COUNT), seam(h);
        std::vector<float> m(np);
        std::vector<int8_t> least(np);
        HIPCK(hipMemcpy(flags.data(), c->wk.flags, FLAG_COUNT * sizeof(int), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(seam.data(), c->wk.seam_x, (size_t) h * sizeof(int), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(m.data(), c->wk.m, np * sizeof(float), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(least.data(), c->wk.least, np, hipMemcpyDeviceToHost));
        char path[512];
        snprintf(path, sizeof path, "%s_%04d.bin", dump, call++);
        if (FILE *f = fopen(path, "wb")) {
            fwrite(hdr.data(), sizeof(int), hdr.size(), f); fwrite(flags.data(), sizeof(int), flags.size(), f);
            fwrite(seam.data(), sizeof(int), seam.size(), f); fwrite(m.data(), sizeof(float), np, f); fwrite(least.data(), 1, np, f);
            fclose(f);
        }
    }
    return rc;
}

extern "C" int lqrhip_seam_log_reserve(LqrHipBatch *b, int n_seams, int h)
{
    int rc;
    if ((rc = pay_catchup(b))) return rc;           // (reads the log of the session before, which ensure_log may replace)
    for (auto *c : b->cs) if ((rc = ensure_log(c, n_seams, h))) return rc;
    return 0;
}

extern "C" int lqrhip_vs_commit(LqrHipBatch *b, int w0, int h0, int wc0, int n_seams, int first_level, int finish)
{
    int rc;
    if ((rc = batch_upload(b))) return rc;
    size_t lds = vsc_lds(n_seams, wc0);
    if (lds > VSC_LDS_MAX) { g_err = "vs_commit: session too large for LDS"; return LQRHIP_EARG; }
    if (lds_needs_attr(lds)) {
        HIPCK(hipFuncSetAttribute((const void *) k_vs_commit, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        CENSUS(LQRHIP_CENSUS_LDS_ATTR_COMMIT);
    }
    hipLaunchKernelGGL(k_vs_commit, dim3(h0, (unsigned) b->cs.size()), dim3(256), lds, b->stream, b->d_desc, w0, h0, wc0, n_seams,
                       first_level, finish);
    HIPCK(hipGetLastError());
    inject_after_commit(b, w0, h0, first_level);
    // the session is over: the frozen planes are owed the seams from frozen_epoch on, and the log stays alive and counts on until
    // pay_catchup has brought them to the carved frame -- or until they are laid out afresh and the debt is dropped
    for (auto *c : b->cs) {
        if (c->frozen_epoch < n_seams) { c->owed_to = n_seams; c->owed_w = wc0 - n_seams; c->owed_h = h0; }
        else drop_catchup(c);
    }
    return 0;
}

// ---- session self-check, roll-back, fault injection (round 6) ---------------------------------------------------------------
// The seam loop's kernels are latency-bound protocols (spin barriers, data-tagged hand-overs); a defect or a device that
// preempts them must not end in LQR_OK with a wrong map.  Two structural checks run inside every session: k_seam_check on the
// seam log BEFORE the levels are committed, and the level count / uniqueness test fused into k_inflate.  Both cost < 1 % of a
// session (1.7 MB of log per 4K image; the inflate pass reads the levels anyway) and are on by default.
static int g_selfcheck = 1, g_recovery = 1;
extern "C" void lqrhip_set_selfcheck(int on) { g_selfcheck = on != 0; }
extern "C" void lqrhip_set_recovery(int on) { g_recovery = on != 0; }
extern "C" int lqrhip_get_recovery(void) { return g_recovery; }
extern "C" int lqrhip_session_check(LqrHipBatch *b, int h, int wc0, int n_seams, int delta_x)
{
    int rc;
    if (!g_selfcheck || n_seams < 1) return 0;
    if ((rc = batch_upload(b))) return rc;
    hipLaunchKernelGGL(k_seam_check, dim3(tiles_of(h, 256), (unsigned) b->cs.size()), dim3(256), 0, b->stream, b->d_desc, h, wc0, n_seams, delta_x, g_dev_err);
    HIPCK(hipGetLastError());
    return 0;
}
// Undo what a failed session left: drain the stream, drop the error record, clear the session's levels from the base layout
// (a no-op when they were never committed).  The working planes are garbage afterwards: the host re-lays them out from the
// base layout (lqrhip_wk_init(b, 1)) before it redoes the session.
extern "C" int lqrhip_session_rollback(LqrHipBatch *b, int w0, int h0, int first_level, int finish)
{
    (void) hipStreamSynchronize(b->stream);
    b->pending_inflate.reset();
    (void) hipGetLastError();
    if (g_dev_err_host) *g_dev_err_host = 0;
    invalidate_all_batches();
    int rc;
    if ((rc = batch_upload(b))) return rc;
    const size_t n = (size_t) w0 * h0;
    hipLaunchKernelGGL(k_vs_rollback, dim3((unsigned) std::min<size_t>(blocks_of(n, 256), 4096), (unsigned) b->cs.size()), dim3(256), 0, b->stream, b->d_desc, n, first_level, finish ? w0 : 0);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(b->stream));
    for (auto *c : b->cs) drop_catchup(c);
    g_fault_stats[4]++;
    return 0;
}
// Fault injection (tests/test_faults_gpu.py).  kind 1: a spin time-out, 2: a failed activity prediction -- the error word is
// written from the host while the kernels of seam step `at_step` of the next session run, which is exactly what the kernels see
// when one of them gives up (they all leave their spins); 3 / 4: one entry of the seam log out of the frame / disconnected (after
// that step); 5 / 6: one committed level cleared / duplicated (between the commit and the inflate pass).  `times`: how many
// sessions in a row are hit (1: the redo succeeds; 2: it fails too).  0 disarms.
static int g_inject_kind = 0, g_inject_step = 0, g_inject_times = 0;
extern "C" void lqrhip_debug_inject(int kind, int at_step, int times) { g_inject_kind = kind; g_inject_step = at_step; g_inject_times = kind ? std::max(times, 1) : 0; }
static void inject_after_step(LqrHipBatch *b, int h, int log_index)
{
    if (g_inject_times <= 0 || log_index != g_inject_step) return;
    if (g_inject_kind == 1 || g_inject_kind == 2) { *g_dev_err_host = g_inject_kind == 1 ? DEVERR_TILE_TIMEOUT : DEVERR_BAND_PREDICTION; }
    else if (g_inject_kind == 3 || g_inject_kind == 4) hipLaunchKernelGGL(k_inject, dim3(1), dim3(64), 0, b->stream, b->d_desc, g_inject_kind - 3, h, 0, log_index, 0);
    else return;
    g_inject_times--; g_fault_stats[5]++;
}
static void inject_after_commit(LqrHipBatch *b, int w0, int h0, int first_level)
{
    if (g_inject_times <= 0 || (g_inject_kind != 5 && g_inject_kind != 6)) return;
    if (g_inject_step > 0) { g_inject_step--; return; }          // (kinds 5 / 6: at_step = how many commits to let pass first -- the second sub-batch of a group)
    hipLaunchKernelGGL(k_inject, dim3(1), dim3(64), 0, b->stream, b->d_desc, g_inject_kind - 3, h0, w0, 0, first_level);
    g_inject_times--; g_fault_stats[5]++;
}

// A pass being staged (phase one).  The batch owns what is staged from the first block on; a return before kept() is an error return:
// the stream is drained and everything staged goes back to the pool
namespace {
struct Staging {
    LqrHipBatch *b;
    bool keep = false;
    Staging(LqrHipBatch *batch, int kind, int w1, int h1) : b(batch)
    {
        b->pending_inflate.reset(new PendingInflate());         // (in place of a staged pass nobody committed)
        b->pending_inflate->kind = kind; b->pending_inflate->w1 = w1; b->pending_inflate->h1 = h1;
    }
    ~Staging() { if (!keep) { lqr_stream_wait(b->stream); b->pending_inflate.reset(); } }
    PlaneJobs &jobs() const { return b->pending_inflate->pj; }
    int kept() { keep = true; return 0; }
};
}  // namespace
// phase one of the inflate pass; `levels`: the plane every job reads its levels from (lqrhip_vmap_load), null: each root's own
static int inflate_stage(LqrHipBatch *b, int w0, int h0, int l, int max_level, const int32_t *levels)
{
    int rc;
    const int w1 = w0 + l - max_level + 1;
    Staging st(b, 0, w1, h0);
    PlaneJobs &pj = st.jobs();
    for (auto *c : b->cs) {
        pj.new_vs.emplace_back();
        DevBuf<int32_t> &nvs = pj.new_vs.back();
        if ((rc = nvs.alloc((size_t) w1 * h0, "&nvs"))) return rc;
        const int32_t *vs = levels ? levels : c->vs.get();
        for (auto *a : c->aux)
            if ((rc = pj.add(a, vs, nullptr, (size_t) w1 * h0))) return rc;
        if ((rc = pj.add(c, vs, nvs, (size_t) w1 * h0))) return rc;
    }
    if ((rc = pj.stage(b->stream, false))) return rc;
    const size_t lds = inflate_lds(l, max_level);       // one bit per level of the session (the fused self-check)
    if (pj.n_narrow)
        hipLaunchKernelGGL(k_inflate<false>, dim3(h0, (unsigned) pj.n_narrow), dim3(256), lds, b->stream, pj.d_dev.get(), w0, w1, l, max_level, g_selfcheck ? g_dev_err : (int *) nullptr);
    if (pj.n_wide())
        hipLaunchKernelGGL(k_inflate<true>, dim3(h0, (unsigned) pj.n_wide()), dim3(256), lds, b->stream, pj.d_wide(), w0, w1, l, max_level, g_selfcheck ? g_dev_err : (int *) nullptr);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(b->stream));
    if ((rc = check_dev_error())) return rc;            // a failed level check: nothing is adopted, the host rolls the session back
    return st.kept();
}
extern "C" int lqrhip_inflate(LqrHipBatch *b, int w0, int h0, int l, int max_level) { return inflate_stage(b, w0, h0, l, max_level, nullptr); }

// ---- lqr_vmap_load (include/lqr_vmap.h): a caller's seam map becomes the visibility map of flat carvers ------------------------------
// The map is brought to the device once (a host map through the pinned ring; a device map is read where it lies), checked by ONE pass
// of k_vmap_check / k_vmap_check_t -- which for an orientation-1 map also writes the plane in the carver's frame -- and only then do
// batches stage their inflate pass on it: every job of every batch reads its levels from that ONE plane (InflateDev.vs), nothing is
// copied per carver.  A map that fails the check is LQRHIP_EMAP: the error word is cleared here, no batch is invalidated, nothing is
// counted in lqrhip_fault_stats and nothing sticks (the non-spinning mode, the recovery).
struct __attribute__((visibility("hidden"))) LqrHipVMap {
    DevBuf<int32_t> own;            // the checked plane where it is the shim's (a host map; an orientation-1 map, transposed)
    const int32_t *plane = nullptr; // lines x len in the carver's frame: `own`, or the caller's device memory (orientation 0)
    int len = 0, lines = 0, depth = 0;
};
extern "C" int lqrhip_vmap_stage(const int *map, int on_device, int width, int height, int depth, int orientation, LqrHipVMap **out)
{
    *out = nullptr;
    if (lqrhip_init() < 0) return LQRHIP_EHIP;
    const int len = orientation ? height : width, lines = orientation ? width : height;
    if (!map || width < 1 || height < 1 || (orientation != 0 && orientation != 1) || depth < 1 || depth >= len || depth >= LQRHIP_MAX_FRAME_WIDTH) {
        g_err = "vmap: depth, size or orientation out of range";
        return LQRHIP_EARG;
    }
    int rc;
    const size_t n = (size_t) width * height;
    std::unique_ptr<LqrHipVMap> m(new LqrHipVMap());
    m->len = len; m->lines = lines; m->depth = depth;
    Scratch tmp(g_stream0);
    const int32_t *src = (const int32_t *) map;
    if (!on_device) {
        int32_t *d = orientation ? tmp.get<int32_t>(n, "&vmap_raw", rc) : ((rc = m->own.alloc(n, "&vmap")) ? nullptr : m->own.get());
        if (rc) return rc;
        if ((rc = h2d_staged(d, map, n * sizeof(int32_t)))) return rc;
        src = d;
    }
    if (orientation) {
        if ((rc = m->own.alloc(n, "&vmap_t"))) return rc;
        const size_t lds = vmap_check_t_lds(depth);
        if (vmap_t_needs_attr(lds)) HIPCK(hipFuncSetAttribute((const void *) k_vmap_check_t, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        hipLaunchKernelGGL(k_vmap_check_t, dim3(vmap_t_blocks(width)), dim3(256), lds, g_stream0, src, m->own.get(), width, height, depth, g_dev_err);
        m->plane = m->own;
    } else {
        hipLaunchKernelGGL(k_vmap_check, dim3(height), dim3(256), vmap_check_lds(depth), g_stream0, src, width, depth, g_dev_err);
        m->plane = src;
    }
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(g_stream0));
    tmp.done();
    if (g_dev_err_host && *g_dev_err_host == DEVERR_VMAP) {
        *g_dev_err_host = 0;
        g_err = "vmap: a value outside [0, depth], or a level that is missing or occurs twice in a line";
        return LQRHIP_EMAP;
    }
    if ((rc = check_dev_error())) return rc;
    *out = m.release();
    return 0;
}
extern "C" void lqrhip_vmap_release(LqrHipVMap *m) { delete m; }
extern "C" int lqrhip_vmap_load(LqrHipBatch *b, const LqrHipVMap *m)
{
    if (!m || !m->plane) return LQRHIP_EARG;
    for (auto *c : b->cs)
        if (c->w0 != m->len || c->h0 != m->lines) { g_err = "vmap: the carver's frame is not the map's"; return LQRHIP_EARG; }
    return inflate_stage(b, m->len, m->lines, m->depth, 1, m->plane);
}
extern "C" int lqrhip_planes_commit(LqrHipBatch *b)
{
    PendingInflate *pi = b->pending_inflate.get();
    if (!pi) return LQRHIP_EARG;
    PlaneJobs &pj = pi->pj;
    commit(pj);
    for (auto &j : pj.jobs) { j.c->w0 = pi->w1; j.c->h0 = pi->h1; }
    if (pi->kind != 0)                      // flat, or flat and transposed: the working planes are laid out afresh from here
        for (auto *c : b->cs) drop_catchup(c);
    if (pi->kind != 2) {                    // (a transpose keeps the carvers' -- all zero -- visibility maps)
        size_t i = 0;
        for (auto *c : b->cs) c->vs = std::move(pj.new_vs[i++]);
    }
    b->dirty = true;
    b->pending_inflate.reset();             // (what is left of it: the job table)
    return 0;
}
extern "C" int lqrhip_inflate_commit(LqrHipBatch *b) { return lqrhip_planes_commit(b); }

extern "C" int lqrhip_flatten(LqrHipBatch *b, int w0, int h0, int w, int level)
{
    int rc;
    Staging st(b, 1, w, h0);
    PlaneJobs &pj = st.jobs();
    for (auto *c : b->cs) {
        pj.new_vs.emplace_back();
        DevBuf<int32_t> &nvs = pj.new_vs.back();        // the flat carver's visibility map: all zero
        if ((rc = nvs.alloc((size_t) w * h0, "&nvs"))) return rc;
        HIPCK(hipMemsetAsync(nvs, 0, (size_t) w * h0 * sizeof(int32_t), b->stream));
        for (auto *a : c->aux)
            if ((rc = pj.add(a, c->vs, nullptr, (size_t) w * h0))) return rc;
        if ((rc = pj.add(c, c->vs, nullptr, (size_t) w * h0))) return rc;
    }
    if ((rc = pj.stage(b->stream, true))) return rc;
    if (pj.n_narrow)
        hipLaunchKernelGGL(k_compact_jobs<false>, dim3(h0, (unsigned) pj.n_narrow), dim3(256), 0, b->stream, pj.d_dev.get(), w0, w, level);
    if (pj.n_wide())
        hipLaunchKernelGGL(k_compact_jobs<true>, dim3(h0, (unsigned) pj.n_wide()), dim3(256), 0, b->stream, pj.d_wide(), w0, w, level);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(b->stream));
    return st.kept();
}

extern "C" int lqrhip_transpose(LqrHipBatch *b, int w, int h)
{
    int rc;
    Staging st(b, 2, h, w);
    PlaneJobs &pj = st.jobs();
    for (auto *c : b->cs) {
        for (auto *a : c->aux)
            if ((rc = pj.add(a, nullptr, nullptr, (size_t) w * h))) return rc;
        if ((rc = pj.add(c, nullptr, nullptr, (size_t) w * h))) return rc;
        HIPCK(hipMemsetAsync(c->vs, 0, (size_t) w * h * sizeof(int32_t), b->stream));   // flat carver: all zero already
    }
    if ((rc = pj.stage(b->stream, true))) return rc;
    if (pj.n_narrow)
        hipLaunchKernelGGL(k_transpose, dim3(tiles_of(w, 32), tiles_of(h, 32), (unsigned) pj.n_narrow), dim3(32, 8), 0, b->stream, pj.d_dev.get(), w, h);
    if (pj.n_wide())
        hipLaunchKernelGGL(k_transpose_px, dim3(tiles_of(w, 32), tiles_of(h, 32), (unsigned) pj.n_wide()), dim3(32, 8), 0, b->stream, pj.d_wide(), w, h);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(b->stream));
    return st.kept();
}

// ---- read-back ---------------------------------------------------------------
// the pixels of carver c visible at `level`, compacted into device memory (w x h0 pixels); on g_stream0, not synchronised
static void launch_read_visible(const LqrHipCarver *c, int w0, int h0, int w, int level, uint8_t *d)
{
#define LAUNCH_RV(DEEP) hipLaunchKernelGGL(k_compact<DEEP>, dim3(h0), dim3(256), 0, g_stream0, c->rgb0.get(), vs_of(c), (const float *) nullptr, (const float *) nullptr, \
                                           d, (float *) nullptr, (float *) nullptr, (int32_t *) nullptr, w0, w, (int) px_bytes(c), level, 0)
    if (px_bytes(c) > 4) LAUNCH_RV(true); else LAUNCH_RV(false);
#undef LAUNCH_RV
}
extern "C" int lqrhip_read_visible(LqrHipCarver *c, int w0, int h0, int w, int level, unsigned char *out)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    size_t n = (size_t) w * h0 * px_bytes(c);
    Scratch tmp(g_stream0);
    uint8_t *d = tmp.get<uint8_t>(n, "&d", rc);
    if (rc) return rc;
    launch_read_visible(c, w0, h0, w, level, d);
    HIPCK(hipGetLastError());
    if ((rc = d2h_staged(out, d, n))) return rc;
    tmp.done();
    return 0;
}

extern "C" int lqrhip_read_visible_device(LqrHipCarver *c, int w0, int h0, int w, int level, void *device_out)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    launch_read_visible(c, w0, h0, w, level, (uint8_t *) device_out);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(g_stream0));
    return 0;
}

// lqr_sizes.h: many sizes from one pass.  The sizes are served in chunks of at most SZ_MAX_JOBS, one k_compact_sizes launch each.  Only a
// device caller of a carver that is not transposed gets the compaction's stores directly; otherwise a size passes through scratch
// planes -- one in frame orientation in front of k_transpose_sizes, one in front of the copy to the host -- and a chunk ends where
// its planes would pass SZ_SCRATCH_MAX.  The job table of the whole call and one scratch block (the largest chunk's, reused: the
// chunks follow each other on one stream) are taken before the first launch.
static const size_t SZ_SCRATCH_MAX = (size_t) 512 << 20;
extern "C" int lqrhip_read_sizes(LqrHipCarver *c, int w0, int h0, int transposed, const int *levels, int n, void *const *outs, int on_device)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    if (n < 1 || !levels || !outs || w0 < 1 || h0 < 1) return LQRHIP_EARG;
    for (int k = 0; k < n; k++)
        if (levels[k] < 1 || levels[k] > w0 || !outs[k]) return LQRHIP_EARG;
    const size_t bytes = px_bytes(c);
    const int planes = (on_device ? 0 : 1) + (transposed ? 1 : 0);          // scratch planes a size passes through
    auto width_of = [&](int k) { return w0 - levels[k] + 1; };
    auto plane_bytes = [&](int k) { return ((size_t) width_of(k) * h0 * bytes + 255) & ~(size_t) 255; };
    struct Chunk { int first, count; };
    std::vector<Chunk> chunks;
    size_t scratch_bytes = 0;
    for (int k = 0; k < n;) {
        size_t used = 0;
        int m = 0;
        while (k + m < n && m < SZ_MAX_JOBS && (m == 0 || used + planes * plane_bytes(k + m) <= SZ_SCRATCH_MAX)) used += planes * plane_bytes(k + m), m++;
        chunks.push_back(Chunk{k, m});
        scratch_bytes = std::max(scratch_bytes, used);
        k += m;
    }
    std::vector<SizeJob> jobs(2 * (size_t) n);                               // (outlives the Scratch, which waits for the copy that reads it)
    std::vector<const uint8_t *> result(n);                                  // where the host copy finds image k
    Scratch tmp(g_stream0);
    SizeJob *d_jobs = tmp.get<SizeJob>(2 * (size_t) n, "&d_jobs", rc);      // [0, n) the compactions, [n, 2 n) the transpositions
    if (rc) return rc;
    uint8_t *scratch = nullptr;
    if (planes) {
        scratch = tmp.get<uint8_t>(scratch_bytes, "&scratch", rc);
        if (rc) return rc;
    }
    for (const Chunk &ch : chunks) {
        size_t at = 0;
        for (int k = ch.first; k < ch.first + ch.count; k++) {
            uint8_t *frame = (uint8_t *) outs[k], *image = (uint8_t *) outs[k];
            if (planes) { frame = scratch + at; at += plane_bytes(k); }
            if (transposed && !on_device) { image = scratch + at; at += plane_bytes(k); }
            jobs[k] = SizeJob{frame, nullptr, levels[k], width_of(k)};
            jobs[n + k] = SizeJob{image, frame, levels[k], width_of(k)};
            result[k] = transposed ? image : frame;
        }
    }
    HIPCK(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(SizeJob), hipMemcpyHostToDevice, g_stream0));
    for (const Chunk &ch : chunks) {
#define LAUNCH_CS(DEEP) hipLaunchKernelGGL(k_compact_sizes<DEEP>, dim3(h0), dim3(256), 0, g_stream0, (const uint8_t *) c->rgb0.get(), (const int32_t *) vs_of(c), \
                                           (const SizeJob *) (d_jobs + ch.first), ch.count, w0, (int) bytes)
        if (bytes > 4) LAUNCH_CS(true); else LAUNCH_CS(false);
#undef LAUNCH_CS
        CENSUS(LQRHIP_CENSUS_COMPACT_SIZES);
        HIPCK(hipGetLastError());
        if (transposed) {
            int wmax = 0;
            for (int k = ch.first; k < ch.first + ch.count; k++) wmax = std::max(wmax, width_of(k));
            const dim3 grid(tiles_of(wmax, 32), tiles_of(h0, 32), (unsigned) ch.count);
#define LAUNCH_TS(WIDE) hipLaunchKernelGGL(k_transpose_sizes<WIDE>, grid, dim3(256), 0, g_stream0, (const SizeJob *) (d_jobs + n + ch.first), h0, (int) bytes)
            if (bytes > 4) LAUNCH_TS(true); else LAUNCH_TS(false);
#undef LAUNCH_TS
            CENSUS(LQRHIP_CENSUS_TRANSPOSE_SIZES);
            HIPCK(hipGetLastError());
        }
        if (!on_device)
            for (int k = ch.first; k < ch.first + ch.count; k++)
                if ((rc = d2h_staged(outs[k], result[k], (size_t) width_of(k) * h0 * bytes))) return rc;
    }
    HIPCK(hipStreamSynchronize(g_stream0));
    tmp.done();
    return 0;
}

// ---- include_ext/lqr_remove.h: the discard scan (kernels in k_discard.hip) ------------------------------------------------------------------
// One Scratch owns the result block and the cross scan's counts; both are taken before anything is launched.  The result words are
// zeroed on the stream in front of the kernels, which fold into them with integer atomics, and reach the host through the staged read.
static unsigned long long g_discard_launches[4];       // k_discard_line, k_discard_cross, k_discard_rank, k_discard_fold
extern "C" void lqrhip_discard_launches(unsigned long long out4[4], int reset)
{
    if (out4) memcpy(out4, g_discard_launches, sizeof g_discard_launches);
    if (reset) memset(g_discard_launches, 0, sizeof g_discard_launches);
}
extern "C" int lqrhip_discard_scan(LqrHipCarver *c, int w0, int h0, int w, int level, int depth, float strength, int which, int *out)
{
    if (!c || c->root || !out || w0 < 1 || h0 < 1 || w < 1 || w > w0 || level < 1 || depth < 0 || !(which & 3) || !(strength >= 0.0f) || c->w0 != w0 || c->h0 != h0) {
        g_err = "discard scan: a root carver in its own base layout, a level, a strength >= 0 and a scan to run";
        return LQRHIP_EARG;
    }
    int rc = batch_sync_of(c);
    if (rc) return rc;
    const bool line = which & LQRHIP_DISCARD_LINE, cross = which & LQRHIP_DISCARD_CROSS;
    memset(out, 0, discard_result_elems() * sizeof(int));
    if (!c->bias0) return 0;            // no plane: nothing is marked
    Scratch tmp(g_stream0);
    int *res = tmp.get<int>(discard_result_elems(), "&res", rc);
    if (rc) return rc;
    // the lines across the rows: a column of the layout is a column of the image only while nothing is hidden (level 1)
    const bool ranked = cross && level > 1;
    int *partial = nullptr;
    if (cross) {
        partial = tmp.get<int>(ranked ? discard_rank_elems(w) : discard_partial_elems(w0, h0), "&partial", rc);
        if (rc) return rc;
    }
    HIPCK(hipMemsetAsync(res, 0, discard_result_elems() * sizeof(int), g_stream0));
    if (ranked) HIPCK(hipMemsetAsync(partial, 0, discard_rank_elems(w) * sizeof(int), g_stream0));
    const float thr = -strength;
    const double plane_bytes = 8.0 * w0 * h0;         // bias0 and vs, once (lqrhip_prof_get: "discard_line", "discard_cross")
    if (line) {
        ProfScope ps("discard_line", g_stream0, plane_bytes);
        hipLaunchKernelGGL(k_discard_line, dim3(h0), dim3(DISCARD_THREADS), 0, g_stream0, (const float *) c->bias0.get(), (const int32_t *) c->vs.get(), w0, thr, level,
                           depth, res + discard_result_off(0));
        g_discard_launches[0]++;
        HIPCK(hipGetLastError());
    }
    if (ranked) {
        ProfScope ps("discard_cross", g_stream0, plane_bytes);
        hipLaunchKernelGGL(k_discard_rank, dim3(h0), dim3(DISCARD_THREADS), 0, g_stream0, (const float *) c->bias0.get(), (const int32_t *) c->vs.get(), w0, w, thr, level,
                           depth, partial, res + discard_result_off(1));
        g_discard_launches[2]++;
        HIPCK(hipGetLastError());
        hipLaunchKernelGGL(k_discard_fold, dim3(discard_col_blocks(w)), dim3(DISCARD_THREADS), 0, g_stream0, (const int *) partial, w, 1, res + discard_result_off(1));
        g_discard_launches[3]++;
        HIPCK(hipGetLastError());
    } else if (cross) {
        ProfScope ps("discard_cross", g_stream0, plane_bytes + 8.0 * discard_partial_elems(w0, h0));
        hipLaunchKernelGGL(k_discard_cross, dim3(discard_col_blocks(w0), discard_row_tiles(h0)), dim3(DISCARD_THREADS), 0, g_stream0, (const float *) c->bias0.get(),
                           (const int32_t *) c->vs.get(), w0, h0, thr, level, depth, partial, res + discard_result_off(1));
        g_discard_launches[1]++;
        HIPCK(hipGetLastError());
        hipLaunchKernelGGL(k_discard_fold, dim3(discard_col_blocks(w0)), dim3(DISCARD_THREADS), 0, g_stream0, (const int *) partial, w0, discard_row_tiles(h0),
                           res + discard_result_off(1));
        g_discard_launches[3]++;
        HIPCK(hipGetLastError());
    }
    // 16 bytes for one scan, 32 for both
    const int first = line ? 0 : 1, count = line && cross ? 2 : 1;
    if ((rc = d2h_staged(out + discard_result_off(first), res + discard_result_off(first), (size_t) count * DISCARD_WORDS * sizeof(int)))) return rc;
    tmp.done();
    return 0;
}

// ---- include_ext/lqr_forward.h: forward-energy seam maps (kernels in k_forward.hip) ---------------------------------------------------------
// A build owns its planes -- per image I, P (with a bias plane), the positions, the choices, the seam, and the map unless the caller
// gave one -- and the job table, all taken in lqrhip_forward_begin before anything is launched.  It runs on g_stream0; the two events
// are the ends of the last two slices.
struct __attribute__((visibility("hidden"))) LqrHipForward {
    struct Planes {
        DevBuf<float> in, p;
        DevBuf<uint16_t> pos;
        DevBuf<int8_t> choice;
        DevBuf<int32_t> seam, map;
    };
    std::vector<Planes> img;
    std::vector<FwdJob> jobs;               // (read by the copy to d_jobs)
    DevBuf<FwdJob> d_jobs;
    hipEvent_t slice_end[2] = {nullptr, nullptr};
    int slices = 0, next_seam = 0;
    int n = 0, L = 0, H = 0, depth = 0, orientation = 0, pxt = 0;
    size_t lds = 0;
    ~LqrHipForward()
    {
        if (g_stream0) (void) hipStreamSynchronize(g_stream0);      // the planes go back to the pool when the members are destroyed
        for (hipEvent_t e : slice_end)
            if (e) (void) hipEventDestroy(e);
        (void) hipGetLastError();
    }
};
// (atomic, relaxed: a second thread may poll the hook while a build counts, lqr_hip.h)
static std::atomic<unsigned long long> g_forward_launches{0};
extern "C" unsigned long long lqrhip_forward_launches(int reset)
{
    return reset ? g_forward_launches.exchange(0, std::memory_order_relaxed) : g_forward_launches.load(std::memory_order_relaxed);
}
// the job of carver c: its base layout and the planes pl, the map `map`
static FwdJob forward_job(const LqrHipCarver *c, const LqrHipForward::Planes &pl, int32_t *map)
{
    return FwdJob{c->rgb0, c->bias0, pl.in, pl.p, pl.pos, pl.choice, pl.seam, map};
}
// the one-off pass for n jobs of carvers that read like c0
static int forward_launch_init(const LqrHipCarver *c0, const FwdJob *d_jobs, int n, int L, int H, int strided, int luma, int w_start, int orientation,
                               std::atomic<unsigned long long> &launches = g_forward_launches)
{
    DeepRead rd = deep_read(c0);
    rd.luma = luma != 0;
    const dim3 grid(tiles_of(L, 256), H, (unsigned) n);
#define CASE(D) if (c0->depth == D) hipLaunchKernelGGL(k_fwd_init<D>, grid, dim3(256), 0, g_stream0, d_jobs, L, H, c0->w0, strided, rd, w_start, orientation); else
    K_FWD_INIT_FORMS(CASE) return no_form("k_fwd_init");
#undef CASE
    launches.fetch_add(1, std::memory_order_relaxed);
    HIPCK(hipGetLastError());
    return 0;
}
extern "C" int lqrhip_forward_begin(LqrHipCarver *const *cs, int n, int depth, int orientation, int transposed, int luma, int w_start,
                                    void *const *device_maps, LqrHipForward **out)
{
    if (out) *out = nullptr;
    if (!cs || !out || n < 1 || n > LQRHIP_FORWARD_MAX_LINES || (orientation != 0 && orientation != 1) || w_start < 1) { g_err = "forward map: arguments"; return LQRHIP_EARG; }
    const LqrHipCarver *c0 = cs[0];
    for (int i = 0; i < n; i++) {
        const LqrHipCarver *c = cs[i];
        if (!c || c->root || c->w0 != c0->w0 || c->h0 != c0->h0 || c->ch != c0->ch || c->depth != c0->depth || c->mode != c0->mode ||
            c->alpha != c0->alpha || c->black != c0->black || (device_maps && !device_maps[i])) {
            g_err = "forward map: root carvers of one shape and pixel kind, a map for each";
            return LQRHIP_EARG;
        }
    }
    const int strided = (transposed != 0) != (orientation != 0);
    const int L = strided ? c0->h0 : c0->w0, H = strided ? c0->w0 : c0->h0;
    if (depth < 1 || depth >= L || L > FWD_THREADS * FWD_MAX_PXT || L > LQRHIP_MAX_FRAME_WIDTH || H > LQRHIP_FORWARD_MAX_LINES) {
        g_err = "forward map: 0 < depth < line length <= " + std::to_string(LQRHIP_MAX_FRAME_WIDTH) + ", at most " + std::to_string(LQRHIP_FORWARD_MAX_LINES) + " lines";
        return LQRHIP_EARG;
    }
    int rc;
    for (int i = 0; i < n; i++)
        if ((rc = batch_sync_of(cs[i]))) return rc;     // whatever still writes the base layouts
    std::unique_ptr<LqrHipForward> f(new LqrHipForward());
    f->n = n; f->L = L; f->H = H; f->depth = depth; f->orientation = orientation;
    f->pxt = L <= FWD_THREADS ? 1 : L <= 2 * FWD_THREADS ? 2 : L <= 4 * FWD_THREADS ? 4 : L <= 8 * FWD_THREADS ? 8 : 16;
    f->lds = fwd_lds(L);
    const size_t px = (size_t) L * H;
    f->img.resize(n);
    for (int i = 0; i < n; i++) {
        LqrHipForward::Planes &pl = f->img[i];
        if ((rc = pl.in.alloc(px, "&fwd_in")) || (cs[i]->bias0 && (rc = pl.p.alloc(px, "&fwd_p"))) || (rc = pl.pos.alloc(px, "&fwd_pos")) ||
            (rc = pl.choice.alloc(px, "&fwd_choice")) || (rc = pl.seam.alloc((size_t) H, "&fwd_seam")) ||
            (!device_maps && (rc = pl.map.alloc(px, "&fwd_map"))))
            return rc;
        f->jobs.push_back(forward_job(cs[i], pl, device_maps ? (int32_t *) device_maps[i] : pl.map.get()));
    }
    if ((rc = f->d_jobs.alloc((size_t) n, "&fwd_jobs"))) return rc;
    for (hipEvent_t &e : f->slice_end) HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (lds_needs_attr(f->lds)) {
#define CASE(P) if (f->pxt == P) HIPCK(hipFuncSetAttribute((const void *) k_fwd_seam<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) f->lds)); else
        K_FWD_SEAM_FORMS(CASE) return no_form("k_fwd_seam");
#undef CASE
    }
    // -- everything is allocated: the first launch
    HIPCK(hipMemcpyAsync(f->d_jobs, f->jobs.data(), (size_t) n * sizeof(FwdJob), hipMemcpyHostToDevice, g_stream0));
    if ((rc = forward_launch_init(c0, f->d_jobs, n, L, H, strided, luma, w_start, orientation))) return rc;
    *out = f.release();
    return 0;
}
extern "C" int lqrhip_forward_seams(LqrHipForward *f, int first_seam, int n_seams)
{
    if (!f || first_seam != f->next_seam || n_seams < 1 || first_seam + n_seams > f->depth) { g_err = "forward map: seams out of order or range"; return LQRHIP_EARG; }
    for (int s = first_seam; s < first_seam + n_seams; s++) {
        const int wc = f->L - s;
#define CASE(P) if (f->pxt == P) hipLaunchKernelGGL(k_fwd_seam<P>, dim3((unsigned) f->n), dim3(FWD_THREADS), f->lds, g_stream0, (const FwdJob *) f->d_jobs.get(), wc, f->L, f->H); else
        K_FWD_SEAM_FORMS(CASE) return no_form("k_fwd_seam");
#undef CASE
        hipLaunchKernelGGL(k_fwd_remove, dim3((unsigned) f->H, (unsigned) f->n), dim3(FWD_REMOVE_THREADS), 0, g_stream0, (const FwdJob *) f->d_jobs.get(), wc, f->L,
                           f->H, s + 1, f->orientation);
        g_forward_launches.fetch_add(2, std::memory_order_relaxed);
        HIPCK(hipGetLastError());
    }
    f->next_seam = first_seam + n_seams;
    HIPCK(hipEventRecord(f->slice_end[f->slices & 1], g_stream0));
    if (f->slices > 0) HIPCK(hipEventSynchronize(f->slice_end[(f->slices - 1) & 1]));
    f->slices++;
    return 0;
}
extern "C" int lqrhip_forward_finish(LqrHipForward *f)
{
    if (!f || f->next_seam != f->depth) { g_err = "forward map: the build is not complete"; return LQRHIP_EARG; }
    HIPCK(hipStreamSynchronize(g_stream0));
    return check_dev_error();
}
extern "C" const int *lqrhip_forward_map(const LqrHipForward *f, int i)
{
    return (f && i >= 0 && i < f->n) ? (const int *) f->jobs[i].map : nullptr;
}
extern "C" int lqrhip_forward_read_map(LqrHipForward *f, int i, int *out)
{
    if (!f || i < 0 || i >= f->n || !out) return LQRHIP_EARG;
    return d2h_staged(out, f->jobs[i].map, (size_t) f->L * f->H * sizeof(int32_t));
}
extern "C" void lqrhip_forward_release(LqrHipForward *f) { delete f; }
extern "C" int lqrhip_forward_intensity(LqrHipCarver *c, int orientation, int transposed, int luma, float *out)
{
    if (!c || c->root || !out || (orientation != 0 && orientation != 1)) return LQRHIP_EARG;
    int rc = batch_sync_of(c);
    if (rc) return rc;
    const int strided = (transposed != 0) != (orientation != 0);
    const int L = strided ? c->h0 : c->w0, H = strided ? c->w0 : c->h0;
    if (L > LQRHIP_MAX_FRAME_WIDTH || H > LQRHIP_FORWARD_MAX_LINES) return LQRHIP_EARG;
    const size_t px = (size_t) L * H;
    Scratch tmp(g_stream0);
    float *in = tmp.get<float>(px, "&fwd_in", rc);
    uint16_t *pos = rc ? nullptr : tmp.get<uint16_t>(px, "&fwd_pos", rc);
    int32_t *map = rc ? nullptr : tmp.get<int32_t>(px, "&fwd_map", rc);
    FwdJob *d_job = rc ? nullptr : tmp.get<FwdJob>(1, "&fwd_jobs", rc);
    if (rc) return rc;
    const FwdJob job{c->rgb0, nullptr, in, nullptr, pos, nullptr, nullptr, map};
    HIPCK(hipMemcpyAsync(d_job, &job, sizeof job, hipMemcpyHostToDevice, g_stream0));
    HIPCK(hipStreamSynchronize(g_stream0));                         // (`job` is on this frame)
    if ((rc = forward_launch_init(c, d_job, 1, L, H, strided, luma, 1, orientation))) return rc;
    if ((rc = d2h_staged(out, in, px * sizeof(float)))) return rc;
    tmp.done();
    return 0;
}

// ---- include_ext/lqr_static.h: the frames of a clip folded into one energy plane (kernel in k_static.hip) -----------------------------------
// A fold owns, through its Scratch, the table of frame pointers, the running planes S, T and I_prev (clips of more than STATIC_GROUP
// frames only) and the plane E unless the caller gave device memory for it: all taken in lqrhip_static_begin before anything is
// launched.  It runs on g_stream0, reads the carvers' base layouts and changes nothing of theirs.
struct __attribute__((visibility("hidden"))) LqrHipStatic {
    Scratch tmp{g_stream0};
    std::vector<StaticFrame> frames;        // (read by the copy to d_frames)
    StaticFrame *d_frames = nullptr;
    float *s = nullptr, *t = nullptr, *ip = nullptr, *e = nullptr;
    int n = 0, W = 0, H = 0, transposed = 0, orientation = 0, nrg = 0, depth = 0, next = 0;
    bool packed = false;
    float alpha = 0.0f;
    DeepRead rd{};
};
extern "C" int lqrhip_static_begin(LqrHipCarver *const *cs, int n, int orientation, int transposed, int nrg_func, float alpha, void *device_energy,
                                   LqrHipStatic **out)
{
    if (out) *out = nullptr;
    if (!cs || !out || n < 1 || n > LQRHIP_STATIC_MAX_FRAMES || (orientation != 0 && orientation != 1) || !(alpha >= 0.0f && alpha <= 1.0f)) {
        g_err = "static energy: arguments";
        return LQRHIP_EARG;
    }
    const LqrHipCarver *c0 = cs[0];
    for (int i = 0; i < n; i++) {
        const LqrHipCarver *c = cs[i];
        if (!c || c->root || c->w0 != c0->w0 || c->h0 != c0->h0 || c->ch != c0->ch || c->depth != c0->depth || c->mode != c0->mode ||
            c->alpha != c0->alpha || c->black != c0->black) {
            g_err = "static energy: root carvers of one shape and pixel kind";
            return LQRHIP_EARG;
        }
    }
    int rc;
    for (int i = 0; i < n; i++)
        if ((rc = batch_sync_of(cs[i]))) return rc;     // whatever still writes the base layouts
    std::unique_ptr<LqrHipStatic> st(new LqrHipStatic());
    st->n = n; st->transposed = transposed != 0; st->orientation = orientation; st->alpha = alpha;
    st->W = transposed ? c0->h0 : c0->w0; st->H = transposed ? c0->w0 : c0->h0;
    const int nrg = nrg_index(nrg_func);
    st->nrg = plane_nrg(true, nrg);
    st->rd = deep_read(c0);
    st->rd.luma = nrg >= 3 && nrg <= 5;
    st->depth = c0->depth;
    st->packed = !reads_value(c0);
    const size_t px = (size_t) st->W * st->H;
    st->d_frames = st->tmp.get<StaticFrame>((size_t) n, "&static_frames", rc);
    if (rc) return rc;
    if (n > STATIC_GROUP) {
        if (!(st->s = st->tmp.get<float>(px, "&static_s", rc))) return rc;
        if (!(st->t = st->tmp.get<float>(px, "&static_t", rc))) return rc;
        if (!(st->ip = st->tmp.get<float>(px, "&static_i", rc))) return rc;
    }
    st->e = (float *) device_energy;
    if (!st->e && !(st->e = st->tmp.get<float>(px, "&static_e", rc))) return rc;
    for (int i = 0; i < n; i++) st->frames.push_back(StaticFrame{cs[i]->rgb0, cs[i]->bias0});
    // -- everything is allocated
    HIPCK(hipMemcpyAsync(st->d_frames, st->frames.data(), (size_t) n * sizeof(StaticFrame), hipMemcpyHostToDevice, g_stream0));
    *out = st.release();
    return 0;
}
extern "C" int lqrhip_static_groups(const LqrHipStatic *st) { return st ? tiles_of(st->n, STATIC_GROUP) : 0; }
// the next group of frames: one launch
extern "C" int lqrhip_static_fold(LqrHipStatic *st)
{
    if (!st || st->next >= st->n) { g_err = "static energy: no frames left to fold"; return LQRHIP_EARG; }
    const int first = st->next, count = std::min(STATIC_GROUP, st->n - first);
    const bool last = first + count == st->n;
    const dim3 grid(tiles_of(st->W, STATIC_TILE), tiles_of(st->H, STATIC_TILE));
#define CASE(N, D, P) if (st->nrg == N && st->depth == D && st->packed == P) \
        hipLaunchKernelGGL((k_static_fold<N, D, P>), grid, dim3(STATIC_THREADS), 0, g_stream0, (const StaticFrame *) st->d_frames + first, count, first, st->W, st->H, \
                           st->transposed, st->orientation, st->rd, st->alpha, st->s, st->t, st->ip, last ? st->e : (float *) nullptr); else
    K_STATIC_FOLD_FORMS(CASE) return no_form("k_static_fold");
#undef CASE
    CENSUS(LQRHIP_CENSUS_STATIC_FOLD);
    HIPCK(hipGetLastError());
    st->next = first + count;
    return 0;
}
// waits for the fold; host_energy non-null: E, width x height floats, copied there.  0: E is complete
extern "C" int lqrhip_static_finish(LqrHipStatic *st, float *host_energy)
{
    if (!st || st->next != st->n) { g_err = "static energy: the fold is not complete"; return LQRHIP_EARG; }
    HIPCK(hipStreamSynchronize(g_stream0));
    int rc = check_dev_error();
    if (rc) return rc;
    if (host_energy && (rc = d2h_staged(host_energy, st->e, (size_t) st->W * st->H * sizeof(float)))) return rc;
    st->tmp.done();
    return 0;
}
extern "C" const float *lqrhip_static_energy(const LqrHipStatic *st) { return st ? st->e : nullptr; }
extern "C" void lqrhip_static_release(LqrHipStatic *st) { delete st; }

// ---- include_ext/lqr_clipforward.h: one forward-energy seam map from all frames of a clip (kernels in k_clipfwd.hip) -------------------------
// A build owns, through its one Scratch, the I planes of the n frames (one block, frame after frame), the costs, Pm while the fold runs
// (frames with a bias plane only), the positions, the choices, the seam, the map unless the caller gave one, and the job table: all taken
// in lqrhip_clipfwd_begin before anything is launched.  It runs on g_stream0; the two events are the ends of the last two slices.
struct __attribute__((visibility("hidden"))) LqrHipClipFwd {
    Scratch tmp{g_stream0};
    std::vector<FwdJob> jobs;               // (read by the copy to d_jobs)
    FwdJob *d_jobs = nullptr;
    float *in = nullptr, *cost = nullptr, *pm = nullptr;
    uint16_t *pos = nullptr;
    int8_t *choice = nullptr;
    int32_t *seam = nullptr, *map = nullptr;
    hipEvent_t slice_end[2] = {nullptr, nullptr};
    hipEvent_t fold_ends[2] = {nullptr, nullptr};       // around the fold's launches (lqrhip_clipfwd_fold_ms)
    int slices = 0, next_seam = 0;
    int n = 0, L = 0, H = 0, depth = 0, orientation = 0, pxt = 0;
    size_t lds = 0;
    ~LqrHipClipFwd()
    {
        if (g_stream0) (void) hipStreamSynchronize(g_stream0);      // the blocks go back to the pool when tmp is destroyed
        tmp.done();
        for (hipEvent_t e : {slice_end[0], slice_end[1], fold_ends[0], fold_ends[1]})
            if (e) (void) hipEventDestroy(e);
        (void) hipGetLastError();
    }
};
// (atomic, relaxed: a second thread may poll the hook while a build counts, lqr_hip.h)
static std::atomic<unsigned long long> g_clipfwd_launches{0};
extern "C" unsigned long long lqrhip_clipfwd_launches(int reset)
{
    return reset ? g_clipfwd_launches.exchange(0, std::memory_order_relaxed) : g_clipfwd_launches.load(std::memory_order_relaxed);
}
// the device time between the first and the last launch of the last finished build's fold, in ms (bench hook, lqr_hip.h)
static std::atomic<double> g_clipfwd_fold_ms{0.0};
extern "C" double lqrhip_clipfwd_fold_ms(void) { return g_clipfwd_fold_ms.load(std::memory_order_relaxed); }
extern "C" int lqrhip_clipfwd_begin(LqrHipCarver *const *cs, int n, int depth, int orientation, int transposed, int luma, int w_start, float temporal,
                                    void *device_map, LqrHipClipFwd **out)
{
    if (out) *out = nullptr;
    if (!cs || !out || n < 1 || n > LQRHIP_FORWARD_MAX_LINES || (orientation != 0 && orientation != 1) || w_start < 1 ||
        !(temporal >= 0.0f && temporal <= 3.402823466e38f)) {
        g_err = "clip forward map: arguments";
        return LQRHIP_EARG;
    }
    const LqrHipCarver *c0 = cs[0];
    for (int i = 0; i < n; i++) {
        const LqrHipCarver *c = cs[i];
        if (!c || c->root || c->w0 != c0->w0 || c->h0 != c0->h0 || c->ch != c0->ch || c->depth != c0->depth || c->mode != c0->mode ||
            c->alpha != c0->alpha || c->black != c0->black || !c->bias0 != !c0->bias0) {
            g_err = "clip forward map: root carvers of one shape and pixel kind";
            return LQRHIP_EARG;
        }
    }
    const int strided = (transposed != 0) != (orientation != 0);
    const int L = strided ? c0->h0 : c0->w0, H = strided ? c0->w0 : c0->h0;
    if (depth < 1 || depth >= L || L > FWD_THREADS * FWD_MAX_PXT || L > LQRHIP_MAX_FRAME_WIDTH || H > LQRHIP_FORWARD_MAX_LINES) {
        g_err = "clip forward map: 0 < depth < line length <= " + std::to_string(LQRHIP_MAX_FRAME_WIDTH) + ", at most " + std::to_string(LQRHIP_FORWARD_MAX_LINES) + " lines";
        return LQRHIP_EARG;
    }
    int rc;
    for (int i = 0; i < n; i++)
        if ((rc = batch_sync_of(cs[i]))) return rc;     // whatever still writes the base layouts
    std::unique_ptr<LqrHipClipFwd> f(new LqrHipClipFwd());
    f->n = n; f->L = L; f->H = H; f->depth = depth; f->orientation = orientation;
    f->pxt = L <= FWD_THREADS ? 1 : L <= 2 * FWD_THREADS ? 2 : L <= 4 * FWD_THREADS ? 4 : L <= 8 * FWD_THREADS ? 8 : 16;
    f->lds = fwd_lds(L);
    const size_t px = (size_t) L * H;
    if (!(f->in = f->tmp.get<float>(clip_intensity_elems(n, px), "&clip_in", rc))) return rc;
    if (!(f->cost = f->tmp.get<float>(clip_cost_elems(px), "&clip_cost", rc))) return rc;
    if (c0->bias0 && !(f->pm = f->tmp.get<float>(px, "&clip_pm", rc))) return rc;
    if (!(f->pos = f->tmp.get<uint16_t>(px, "&clip_pos", rc))) return rc;
    if (!(f->choice = f->tmp.get<int8_t>(px, "&clip_choice", rc))) return rc;
    if (!(f->seam = f->tmp.get<int32_t>((size_t) H, "&clip_seam", rc))) return rc;
    f->map = (int32_t *) device_map;
    if (!f->map && !(f->map = f->tmp.get<int32_t>(px, "&clip_map", rc))) return rc;
    if (!(f->d_jobs = f->tmp.get<FwdJob>((size_t) n, "&clip_jobs", rc))) return rc;
    // k_fwd_init's jobs: every frame its own I plane; no P plane (the fold divides the bias itself); the positions and the cleared map
    // are the clip's, which every frame's pass writes alike
    for (int i = 0; i < n; i++)
        f->jobs.push_back(FwdJob{cs[i]->rgb0, cs[i]->bias0, f->in + clip_frame_off(i, px), nullptr, f->pos, nullptr, nullptr, f->map});
    for (hipEvent_t &e : f->slice_end) HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (hipEvent_t &e : f->fold_ends) HIPCK(hipEventCreate(&e));
    if (lds_needs_attr(f->lds)) {
#define CASE(P) if (f->pxt == P) HIPCK(hipFuncSetAttribute((const void *) k_clip_seam<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) f->lds)); else
        K_CLIP_SEAM_FORMS(CASE) return no_form("k_clip_seam");
#undef CASE
    }
    // -- everything is allocated: the first launch
    HIPCK(hipMemcpyAsync(f->d_jobs, f->jobs.data(), (size_t) n * sizeof(FwdJob), hipMemcpyHostToDevice, g_stream0));
    if ((rc = forward_launch_init(c0, f->d_jobs, n, L, H, strided, luma, w_start, orientation, g_clipfwd_launches))) return rc;
    const dim3 grid(tiles_of(L, CLIPFWD_FOLD_THREADS), H);
    HIPCK(hipEventRecord(f->fold_ends[0], g_stream0));
    for (int g = 0; g < clip_fold_groups(n, CLIPFWD_GROUP); g++) {
        const int first = g * CLIPFWD_GROUP, count = std::min(CLIPFWD_GROUP, n - first);
        hipLaunchKernelGGL(k_clip_fold, grid, dim3(CLIPFWD_FOLD_THREADS), 0, g_stream0, (const FwdJob *) f->d_jobs, (const float *) f->in, first, count,
                           first + count == n ? 1 : 0, L, H, c0->w0, strided, w_start, temporal, f->cost, f->pm);
        g_clipfwd_launches.fetch_add(1, std::memory_order_relaxed);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipEventRecord(f->fold_ends[1], g_stream0));
    *out = f.release();
    return 0;
}
extern "C" int lqrhip_clipfwd_seams(LqrHipClipFwd *f, int first_seam, int n_seams)
{
    if (!f || first_seam != f->next_seam || n_seams < 1 || first_seam + n_seams > f->depth) { g_err = "clip forward map: seams out of order or range"; return LQRHIP_EARG; }
    for (int s = first_seam; s < first_seam + n_seams; s++) {
        const int wc = f->L - s;
#define CASE(P) if (f->pxt == P) hipLaunchKernelGGL(k_clip_seam<P>, dim3(1), dim3(FWD_THREADS), f->lds, g_stream0, (const float *) f->cost, f->choice, f->seam, wc, f->L, f->H); else
        K_CLIP_SEAM_FORMS(CASE) return no_form("k_clip_seam");
#undef CASE
        hipLaunchKernelGGL(k_clip_remove, dim3((unsigned) f->H), dim3(FWD_REMOVE_THREADS), 0, g_stream0, f->cost, f->pos, (const int32_t *) f->seam, f->map, wc, f->L, f->H,
                           s + 1, f->orientation);
        g_clipfwd_launches.fetch_add(2, std::memory_order_relaxed);
        if (s + 1 < f->depth) {         // (after the last seam nobody reads the costs)
            hipLaunchKernelGGL(k_clip_refresh, dim3((unsigned) f->H), dim3(CLIPFWD_REFRESH_THREADS), 0, g_stream0, (const float *) f->in, f->n, f->cost,
                               (const uint16_t *) f->pos, (const int32_t *) f->seam, wc - 1, f->L, f->H);
            g_clipfwd_launches.fetch_add(1, std::memory_order_relaxed);
        }
        HIPCK(hipGetLastError());
    }
    f->next_seam = first_seam + n_seams;
    HIPCK(hipEventRecord(f->slice_end[f->slices & 1], g_stream0));
    if (f->slices > 0) HIPCK(hipEventSynchronize(f->slice_end[(f->slices - 1) & 1]));
    f->slices++;
    return 0;
}
extern "C" int lqrhip_clipfwd_finish(LqrHipClipFwd *f)
{
    if (!f || f->next_seam != f->depth) { g_err = "clip forward map: the build is not complete"; return LQRHIP_EARG; }
    HIPCK(hipStreamSynchronize(g_stream0));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, f->fold_ends[0], f->fold_ends[1]) == hipSuccess) g_clipfwd_fold_ms.store(ms, std::memory_order_relaxed);
    (void) hipGetLastError();
    return check_dev_error();
}
extern "C" const int *lqrhip_clipfwd_map(const LqrHipClipFwd *f) { return f ? (const int *) f->map : nullptr; }
extern "C" int lqrhip_clipfwd_read_map(LqrHipClipFwd *f, int *out)
{
    if (!f || !out) return LQRHIP_EARG;
    return d2h_staged(out, f->map, (size_t) f->L * f->H * sizeof(int32_t));
}
extern "C" void lqrhip_clipfwd_release(LqrHipClipFwd *f) { delete f; }

extern "C" int lqrhip_mask_line_max(const unsigned char *mask, int channels, int width, int height, int a0, int b0, int n_lines,
                                    int line_len, int direction)
{
    if (lqrhip_init() < 0) return LQRHIP_EHIP;
    if (n_lines <= 0 || line_len <= 0) return 0;
    int rc, result = 0;
    size_t bytes = (size_t) width * height * channels;
    Scratch tmp(g_stream0);
    uint8_t *d = tmp.get<uint8_t>(bytes, "&d", rc);
    if (rc) return rc;
    int *dout = tmp.get<int>(1, "&dout", rc);
    if (rc) return rc;
    HIPCK(hipMemcpyAsync(d, mask, bytes, hipMemcpyHostToDevice, g_stream0));
    HIPCK(hipMemsetAsync(dout, 0, sizeof(int), g_stream0));
    hipLaunchKernelGGL(k_mask_line_max, dim3(n_lines), dim3(256), 0, g_stream0, d, channels, width, a0, b0, line_len, direction, dout);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(&result, dout, sizeof(int), hipMemcpyDeviceToHost, g_stream0));
    HIPCK(hipStreamSynchronize(g_stream0));
    tmp.done();
    return result;
}

extern "C" void lqrhip_pool_trim(void)
{
    (void) hipDeviceSynchronize();
    g_cache.trim();
    unpark_all();
}

extern "C" int lqrhip_device_sync(void)
{
    HIPCK(hipDeviceSynchronize());
    return check_dev_error();
}

extern "C" int lqrhip_read_vmap(LqrHipCarver *c, int w0, int h0, int w, int level, int depth, int *out)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    size_t n = (size_t) w * h0;
    Scratch tmp(g_stream0);
    int32_t *d = tmp.get<int32_t>(n, "&d", rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_compact<false>, dim3(h0), dim3(256), 0, g_stream0, (const uint8_t *) nullptr, vs_of(c), (const float *) nullptr,
                       (const float *) nullptr, (uint8_t *) nullptr, (float *) nullptr, (float *) nullptr, d, w0, w, c->ch, level,
                       depth);
    HIPCK(hipGetLastError());
    if ((rc = d2h_staged(out, d, n * sizeof(int32_t)))) return rc;
    tmp.done();
    return 0;
}

// Test hook: what the backtrack published for the last seam -- the origin every kernel uses, the origin before that seam, the side it moved
extern "C" int lqrhip_read_seam_flags(LqrHipCarver *c, int *org, int *org_prev, int *side)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    if (!c->wk.flags) return LQRHIP_EARG;
    int32_t fl[FLAG_COUNT];
    HIPCK(hipMemcpy(fl, c->wk.flags, sizeof fl, hipMemcpyDeviceToHost));
    *org = fl[FLAG_ORG]; *org_prev = fl[FLAG_ORG_PREV]; *side = fl[FLAG_SIDE];
    return 0;
}
extern "C" int lqrhip_read_working(LqrHipCarver *c, int w, int h, float *en, float *m, int *least_dx)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    if (!c->wk.pix) return LQRHIP_EARG;
    int32_t fl[FLAG_COUNT];
    HIPCK(hipMemcpy(fl, c->wk.flags, sizeof fl, hipMemcpyDeviceToHost));
    const int org = fl[FLAG_ORG];                 // the carved planes start `org` elements into each row
    size_t n = (size_t) c->stride * h;
    std::vector<float> t(n);
    std::vector<int8_t> tl(n);
    if (en) {
        HIPCK(hipMemcpy(t.data(), c->wk.en, n * sizeof(float), hipMemcpyDeviceToHost));
        for (int y = 0; y < h; y++) memcpy(en + (size_t) y * w, t.data() + (size_t) y * c->stride + org, (size_t) w * sizeof(float));
    }
    if (m) {
        HIPCK(hipMemcpy(t.data(), c->wk.m, n * sizeof(float), hipMemcpyDeviceToHost));
        for (int y = 0; y < h; y++) memcpy(m + (size_t) y * w, t.data() + (size_t) y * c->stride + org, (size_t) w * sizeof(float));
    }
    if (least_dx) {
        HIPCK(hipMemcpy(tl.data(), c->wk.least, n, hipMemcpyDeviceToHost));
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) least_dx[(size_t) y * w + x] = y == 0 ? 0 : (int) tl[(size_t) y * c->stride + org + x];
    }
    return 0;
}

// ---- start over from a device-resident image ---------------------------------------------------
__global__ __launch_bounds__(256) void k_copy16(const u32x4 *__restrict__ src, u32x4 *__restrict__ dst, size_t n16);
// the host side of a reset, up to the fresh base planes: what lqrhip_carver_reset and lqrhip_carver_reset_batch do alike per carver
static int reset_planes(LqrHipCarver *c, int w, int h)
{
    int rc = batch_sync_of(c);
    if (rc) return rc;
    const size_t n = (size_t) w * h;
    c->rgb0.reset(); c->vs.reset(); c->bias0.reset(); c->rig0.reset();
    // a carver that had masks carries bias / rig working planes: the fresh carver has none
    if (c->wk.bias || c->wk.rig) { free_working(c); c->stride = 0; c->wk_h = 0; }
    c->w0 = w; c->h0 = h;
    drop_catchup(c);                // (the working planes are laid out afresh from the new image: nothing is owed to them)
    if ((rc = c->rgb0.alloc(n * px_bytes(c), "&c->rgb0")) || (rc = c->vs.alloc(n, "&c->vs"))) return rc;
    return 0;
}
extern "C" int lqrhip_carver_reset(LqrHipCarver *c, const void *device_rgb, int w, int h)
{
    // roots without attached carvers only: an attached carver holds no visibility map of its own (vs_of)
    if (!c || c->root || !c->aux.empty() || w < 1 || h < 1) return LQRHIP_EARG;
    int rc = reset_planes(c, w, h);
    if (rc) return rc;
    const size_t n = (size_t) w * h;
    // (round 6: these copies on four more streams side by side -- one 33 MB device-to-device copy runs at ~0.5 TB/s, 64 of them are 4 ms of a
    // 190-ms step -- made the 64-image step 45 % LONGER: with g_stream0 and the four sub-batch streams that is nine streams on the
    // process's eight hardware queues, and sub-batch streams that share a queue run one after the other.  One stream.)
    {
        // the runtime's device-to-device copy kernel moves a 33 MB image in 66 us (0.5 TB/s; 64 of them: 4.2 ms of a 190-ms step, one after
        // the other); the engine's own streaming copy (k_copy16, the one that measures the HBM ceiling) takes ~10
        const size_t bytes = n * px_bytes(c), n16 = bytes / 16;
        if (n16 && !(((uintptr_t) device_rgb | (uintptr_t) c->rgb0.get()) & 15)) {
            hipLaunchKernelGGL(k_copy16, dim3((unsigned) blocks_of(n16, 256)), dim3(256), 0, g_stream0, (const u32x4 *) device_rgb, (u32x4 *) c->rgb0.get(), n16);
            HIPCK(hipGetLastError());
            if (bytes & 15) HIPCK(hipMemcpyAsync(c->rgb0 + n16 * 16, (const uint8_t *) device_rgb + n16 * 16, bytes & 15, hipMemcpyDeviceToDevice, g_stream0));
        } else {
            HIPCK(hipMemcpyAsync(c->rgb0, device_rgb, bytes, hipMemcpyDeviceToDevice, g_stream0));
        }
    }
    HIPCK(hipMemsetAsync(c->vs, 0, n * sizeof(int32_t), g_stream0));
    if (c->batch) c->batch->dirty = true;
    if (c->active && (rc = ensure_working(c, w, h))) return rc;        // synchronises g_stream0 when it allocates
    return 0;
}

// The same for a whole list, as the batch drivers reload (64 carvers per step): per carver the bookkeeping above, in the same order, and
// then ONE launch per RESET_JOBS carvers that copies their images and clears their visibility maps -- 64 copy kernels and 64 fills one
// after the other on the stream were ~4 ms of a 64 x 4K step for 6.4 GB, 1.6 TB/s.  The jobs travel in the kernel's arguments: nothing
// is allocated for them.  An image that does not start on a 16-byte boundary goes the way lqrhip_carver_reset copies it.
// On a failure the carvers before the failing one are reset completely (lqrhip_carver_reset_batch_count says how many), the failing
// one is as lqrhip_carver_reset leaves it, the ones after it are untouched.
enum { RESET_JOBS = 16 };
struct ResetJob { const uint8_t *src; uint8_t *dst; uint8_t *vs; size_t bytes; };
struct ResetJobs { ResetJob j[RESET_JOBS]; };
__global__ __launch_bounds__(256) void k_reset_jobs(const ResetJobs jobs, const size_t vs_bytes);
static int g_reset_batch_count = 0;
extern "C" int lqrhip_carver_reset_batch_count(void) { return g_reset_batch_count; }
extern "C" int lqrhip_carver_reset_batch(LqrHipCarver **cs, const void *const *device_rgb, int n, int w, int h)
{
    g_reset_batch_count = 0;
    if (!cs || !device_rgb || n < 1 || w < 1 || h < 1) return LQRHIP_EARG;
    for (int i = 0; i < n; i++)         // every argument before any carver is touched
        if (!cs[i] || cs[i]->root || !cs[i]->aux.empty() || !device_rgb[i]) return LQRHIP_EARG;
    const size_t npx = (size_t) w * h, vs_bytes = npx * sizeof(int32_t);
    ResetJobs jobs = {};
    int nj = 0;
    size_t most = vs_bytes;             // the longest plane of the jobs collected
    auto flush = [&]() -> int {
        if (!nj) return 0;
        const unsigned blocks = (unsigned) std::min<size_t>(blocks_of(most / 16, 256) + 1, 4096);
        hipLaunchKernelGGL(k_reset_jobs, dim3(blocks, (unsigned) nj), dim3(256), 0, g_stream0, jobs, vs_bytes);
        nj = 0; most = vs_bytes;
        HIPCK(hipGetLastError());
        return 0;
    };
    for (int i = 0; i < n; i++) {
        LqrHipCarver *c = cs[i];
        g_reset_batch_count = i;
        int rc = reset_planes(c, w, h);
        if (rc) { (void) flush(); return rc; }
        const size_t bytes = npx * px_bytes(c);
        if (!(((uintptr_t) device_rgb[i] | (uintptr_t) c->rgb0.get() | (uintptr_t) c->vs.get()) & 15)) {
            jobs.j[nj++] = ResetJob{(const uint8_t *) device_rgb[i], c->rgb0.get(), (uint8_t *) c->vs.get(), bytes};
            most = std::max(most, bytes);
            g_fixed_stats[1]++;
        } else {
            g_fixed_stats[2]++;
            hipError_t e = hipMemcpyAsync(c->rgb0, device_rgb[i], bytes, hipMemcpyDeviceToDevice, g_stream0);
            if (e == hipSuccess) e = hipMemsetAsync(c->vs, 0, vs_bytes, g_stream0);
            if (e != hipSuccess) { (void) flush(); HIPCK(e); }
        }
        if (c->batch) c->batch->dirty = true;
        if (c->active && (rc = ensure_working(c, w, h))) { (void) flush(); return rc; }       // synchronises g_stream0 when it allocates
        if (nj == RESET_JOBS && (rc = flush())) return rc;
    }
    int rc = flush();
    if (rc) return rc;
    g_reset_batch_count = n;
    return 0;
}

// order everything the shim enqueued on its own stream (resets, mask uploads) before the caller goes on
extern "C" int lqrhip_reset_sync(void)
{
    if (g_stream0) HIPCK(hipStreamSynchronize(g_stream0));
    return 0;
}

extern "C" int lqrhip_mem_info(unsigned long long *free_bytes, unsigned long long *total_bytes, unsigned long long *cached_bytes)
{
    if (lqrhip_init() < 0) return LQRHIP_EHIP;
    size_t f = 0, t = 0;
    HIPCK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    if (cached_bytes) *cached_bytes = g_cache.cached_bytes();
    return 0;
}

// ---- measured HBM ceiling: streaming copy, ONE 16-byte element per thread, non-temporal -- the form that measured
// fastest on this device (6.5 TB/s read + write at 2 GiB; grid-stride loops with 1-8 loads in flight per thread and
// 1k-64k workgroups: 4.4-5.8 TB/s; scripts/dbg/t_copy.hip)
__global__ __launch_bounds__(256) void k_copy16(const u32x4 *__restrict__ src, u32x4 *__restrict__ dst, size_t n16)
{
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i < n16) __builtin_nontemporal_store(__builtin_nontemporal_load((const GLOBAL_AS u32x4 *) src + i), (GLOBAL_AS u32x4 *) dst + i);
}

// The reload of a list of carvers (lqrhip_carver_reset_batch): job blockIdx.y copies its image and clears its visibility map, 16 bytes
// per access, the grid striding over the planes; src, dst and vs are 16-byte aligned.  The bytes past the last multiple of 16 are moved
// one each by the grid's last threads.
__global__ __launch_bounds__(256) void k_reset_jobs(const ResetJobs jobs, const size_t vs_bytes)
{
    const ResetJob j = jobs.j[blockIdx.y];
    const size_t tid = (size_t) blockIdx.x * 256 + threadIdx.x, nthreads = (size_t) gridDim.x * 256;
    const size_t n16 = j.bytes / 16, z16 = vs_bytes / 16;
    for (size_t i = tid; i < n16; i += nthreads)
        __builtin_nontemporal_store(__builtin_nontemporal_load((const GLOBAL_AS u32x4 *) j.src + i), (GLOBAL_AS u32x4 *) j.dst + i);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (size_t i = tid; i < z16; i += nthreads) __builtin_nontemporal_store(zero, (GLOBAL_AS u32x4 *) j.vs + i);
    const size_t back = nthreads - 1 - tid;         // 0 for the last thread of the grid row
    if (back < (j.bytes & 15)) j.dst[n16 * 16 + back] = j.src[n16 * 16 + back];
    if (back < (vs_bytes & 15)) j.vs[z16 * 16 + back] = 0;
}

extern "C" int lqrhip_copy_bandwidth(unsigned long long bytes, int iters, double *gbps)
{
    if (lqrhip_init() < 0) return LQRHIP_EHIP;
    if (iters < 1 || bytes < 4096) return LQRHIP_EARG;
    struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void) hipEventDestroy(e); } } e0, e1;      // (destroyed after the Scratch has waited)
    int rc;
    Scratch tmp(g_stream0);
    uint8_t *a = tmp.get<uint8_t>(bytes, "&a", rc);
    if (rc) return rc;
    uint8_t *b = tmp.get<uint8_t>(bytes, "&b", rc);
    if (rc) return rc;
    float ms = 0;
    const size_t n16 = bytes / 16;
    HIPCK(hipMemsetAsync(a, 1, bytes, g_stream0));
    HIPCK(hipEventCreate(&e0.e)); HIPCK(hipEventCreate(&e1.e));
    const dim3 grid((unsigned) blocks_of(n16, 256));
    hipLaunchKernelGGL(k_copy16, grid, dim3(256), 0, g_stream0, (const u32x4 *) a, (u32x4 *) b, n16);     // warm-up
    HIPCK(hipEventRecord(e0.e, g_stream0));
    for (int i = 0; i < iters; i++) hipLaunchKernelGGL(k_copy16, grid, dim3(256), 0, g_stream0, (const u32x4 *) a, (u32x4 *) b, n16);
    HIPCK(hipEventRecord(e1.e, g_stream0));
    HIPCK(hipStreamSynchronize(g_stream0));
    HIPCK(hipEventElapsedTime(&ms, e0.e, e1.e));
    tmp.done();
    if (gbps) *gbps = 2.0 * (double) (n16 * 16) * iters / (ms * 1e-3) / 1e9;
    return 0;
}

// ---- seam-map colour ramp -----------------------------------------------------
// write_vmap_to_layer's per-pixel arithmetic, src/io_functions.c:249-279, in double with every
// operation individually rounded; (guchar)(255 * x) truncates.  One thread per pixel, streaming.
__global__ __launch_bounds__(256) void k_vmap_ramp(const int32_t *__restrict__ vmap, uint32_t *__restrict__ out, size_t n, int depth,
                                                   double sr, double sg, double sb, double er, double eg, double eb)
{
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int vs = vmap[i];
    uint32_t px = 0;                                                     // vs == 0: all four bytes 0 (:253-259)
    if (vs != 0) {
        const double value = __ddiv_rn((double) (depth + 1 - vs), (double) (depth + 1));        // :263
        const double inv = __dsub_rn(1.0, value);
        const double rd = __dadd_rn(__dmul_rn(value, sr), __dmul_rn(inv, er));                    // :264
        const double gr = __dadd_rn(__dmul_rn(value, sg), __dmul_rn(inv, eg));                    // :265
        const double bl = __dadd_rn(__dmul_rn(value, sb), __dmul_rn(inv, eb));                    // :266
        const double al = __dmul_rn(0.5, __dadd_rn(1.0, value));                                  // :267
        // (guchar) of a double: truncation towards zero, then the low 8 bits (values are in [0, 255])
        const uint32_t r8 = (uint32_t) (int) __dmul_rn(255.0, rd) & 0xffu, g8 = (uint32_t) (int) __dmul_rn(255.0, gr) & 0xffu;
        const uint32_t b8 = (uint32_t) (int) __dmul_rn(255.0, bl) & 0xffu, a8 = (uint32_t) (int) __dmul_rn(255.0, al) & 0xffu;
        px = r8 | (g8 << 8) | (b8 << 16) | (a8 << 24);
    }
    out[i] = px;
}

extern "C" int lqrhip_vmap_to_rgba(const int *vmap, int w, int h, int depth, const double col_start[3], const double col_end[3],
                                   unsigned char *out_rgba)
{
    if (lqrhip_init() < 0) return LQRHIP_EHIP;
    if (!vmap || !out_rgba || w < 1 || h < 1) return LQRHIP_EARG;
    const size_t n = (size_t) w * h;
    int rc;
    Scratch tmp(g_stream0);
    int32_t *dv = tmp.get<int32_t>(n, "&dv", rc);
    if (rc) return rc;
    uint32_t *dout = tmp.get<uint32_t>(n, "&dout", rc);
    if (rc) return rc;
    HIPCK(hipMemcpyAsync(dv, vmap, n * sizeof(int32_t), hipMemcpyHostToDevice, g_stream0));
    hipLaunchKernelGGL(k_vmap_ramp, dim3((unsigned) blocks_of(n, 256)), dim3(256), 0, g_stream0, dv, dout, n, depth, col_start[0], col_start[1],
                       col_start[2], col_end[0], col_end[1], col_end[2]);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out_rgba, dout, n * 4, hipMemcpyDeviceToHost, g_stream0));
    HIPCK(hipStreamSynchronize(g_stream0));
    tmp.done();
    return 0;
}
