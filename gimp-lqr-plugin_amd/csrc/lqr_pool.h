// lqr_pool.h -- the launch shim's allocation cache, as plain C++17.  No HIP, no globals: one class over three functions its owner
// supplies (the raw allocator, the raw free, and a hook that prepares a block before it is handed out), so that the same code runs in
// tests/c/pool_main.cc over malloc / free without a GPU.  The carve path allocates and frees image-sized planes for every inflate /
// flatten / read-out, and the raw pair (hipMalloc, and hipFree, which synchronises the device) would cost more than the kernels
// between them.  Whoever frees a block knows that nothing queued on the device still uses it (lqr_own.h).
// Everything here has internal linkage (the library exports the C ABI of include/lqr_hip.h and nothing else).
#pragma once
#include <stddef.h>
#include <map>
#include <string>

namespace {

class BlockCache {
public:
    // `bytes` of memory: 0 and *p, or the owner's error code with the reason in `why`.  `nomem` (below) is the code the cache retries on
    typedef int (*RawAlloc)(void **p, size_t bytes, std::string &why);
    typedef void (*RawFree)(void *p);
    // make `bytes` at p ready for their user (the shim: LQRHIP_POISON); `name` says what the block is for.  0, or an error code; the
    // hook reports its own reason
    typedef int (*Prepare)(void *p, size_t bytes, const char *name);

    // cap: the most bytes kept cached.  nomem: the raw allocator's code for "out of memory", also what an injected failure returns
    BlockCache(size_t cap, int nomem, RawAlloc raw_alloc, RawFree raw_free, Prepare prepare)
        : cap_(cap), nomem_(nomem), raw_alloc_(raw_alloc), raw_free_(raw_free), prepare_(prepare) {}
    BlockCache(const BlockCache &) = delete;
    BlockCache &operator=(const BlockCache &) = delete;

    static size_t size_class(size_t bytes) { return (bytes + ((size_t) 1 << 20) - 1) & ~(((size_t) 1 << 20) - 1); }      // 1 MiB classes

    // fault injection: the nth allocation from now on fails with `nomem`, once, before anything is taken (-1: disarmed)
    void fail_in(long nth) { fail_in_ = nth; }

    // A block of the class of `bytes`: a cached one of exactly that class, else a raw one.  0 and *p, or an error code with *p null and
    // (unless the hook failed, which says so itself) the reason in `err`
    int alloc(void **p, size_t bytes, const char *name, std::string &err)
    {
        *p = nullptr;
        const size_t sz = size_class(bytes);
        if (fail_in_ >= 0 && fail_in_-- == 0) { err = std::string("injected allocation failure (") + (name ? name : "?") + ")"; return nomem_; }
        auto it = free_.find(sz);
        if (it != free_.end()) {
            *p = it->second;
            free_.erase(it);
            cached_ -= sz;
        } else {
            std::string why;
            int e = raw_alloc_(p, sz, why);
            if (e == nomem_ && !free_.empty()) {       // give the cache back and retry once
                trim();
                e = raw_alloc_(p, sz, why);
            }
            if (e) { *p = nullptr; err = why; return e; }
            size_[*p] = sz;
        }
        const int rc = prepare_(*p, sz, name);
        if (rc) { free(*p); *p = nullptr; }      // a failed allocation hands nothing out
        return rc;
    }
    // ... back to the cache; beyond the cap, or a pointer the cache does not know, to the raw free
    void free(void *p)
    {
        auto it = size_.find(p);
        if (it == size_.end()) { raw_free_(p); return; }
        if (cached_ + it->second > cap_) {
            raw_free_(p);
            size_.erase(it);
            return;
        }
        free_.emplace(it->second, p);
        cached_ += it->second;
    }
    // every cached block goes to the raw free: the out-of-memory retry, and lqrhip_pool_trim
    void trim()
    {
        for (auto &kv : free_) { raw_free_(kv.second); size_.erase(kv.second); }
        free_.clear();
        cached_ = 0;
    }
    size_t live() const { return size_.size() - free_.size(); }      // blocks handed out and not given back
    size_t cached_bytes() const { return cached_; }

private:
    const size_t cap_;
    const int nomem_;
    const RawAlloc raw_alloc_;
    const RawFree raw_free_;
    const Prepare prepare_;
    std::multimap<size_t, void *> free_;        // the cached blocks, by class
    std::map<void *, size_t> size_;             // every block the cache knows, handed out or cached
    size_t cached_ = 0;
    long fail_in_ = -1;
};

}  // namespace
