// lqr_own.h -- who owns a device block: the launch shim's whole ownership rule, as plain C++17.  No HIP, no globals: two small types
// over three functions that the shim (lqr_shim.hip) defines on its allocation cache, so that the same code runs in tests/c/own_main.cc
// over malloc / free without a GPU.  DevBuf<T> is a block that lives as long as its owner (a carver's plane, a batch's exchange area, a
// staged plane of a pass); Scratch holds the blocks of one call.  Nothing outside this file gives a block back to the cache.
// Everything here has internal linkage (the library exports the C ABI of include/lqr_hip.h and nothing else).
#pragma once
#include <stddef.h>
#include <vector>

// `bytes` of device memory; `name` says what for (LQRHIP_POISON_LOG, the text of an injected failure).  0, or LQRHIP_E* with *p null
static int lqr_pool_alloc(void **p, size_t bytes, const char *name);
// ... back to the cache.  Whoever calls this knows that nothing queued on the device still uses the block
static void lqr_pool_free(void *p);
// wait for everything queued on `stream` (a hipStream_t); errors are not reported
static void lqr_stream_wait(void *stream);

namespace {

// One block and the number of elements it was sized for.  Move-only; a move into a buffer that holds a block gives that block back.
template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p_) lqr_pool_free(p_);
        p_ = nullptr; n_ = 0;
    }
    // a fresh block of n elements (0: of one); what the buffer held goes back first.  On failure the buffer is empty
    int alloc(size_t n, const char *name)
    {
        reset();
        void *p = nullptr;
        const int rc = lqr_pool_alloc(&p, (n ? n : 1) * sizeof(T), name);
        if (rc) return rc;
        p_ = (T *) p; n_ = n;
        return 0;
    }
    // ... unless the block it holds is large enough.  *grew says whether a new block was taken
    int ensure(size_t n, const char *name, bool *grew)
    {
        *grew = !p_ || n_ < n;
        return *grew ? alloc(n, name) : 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t size() const { return n_; }          // elements asked for; 0 when empty
};

// The temporaries of one call whose device work runs on `stream`.  Every return path gives them back; one that did not reach done()
// is an error return, on which kernels or copies that use them may still be queued: the destructor waits for the stream first.
// A call that succeeds has synchronised already (that is how it knows) and says so with done(): no wait is added to it.
class Scratch {
    void *stream_;
    std::vector<void *> blocks_;
    bool done_ = false;

public:
    explicit Scratch(void *stream) : stream_(stream) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch()
    {
        if (!done_) lqr_stream_wait(stream_);
        for (void *p : blocks_) lqr_pool_free(p);
    }
    // n elements (0: one); null and rc set on failure
    template <typename T>
    T *get(size_t n, const char *name, int &rc)
    {
        void *p = nullptr;
        if ((rc = lqr_pool_alloc(&p, (n ? n : 1) * sizeof(T), name))) return nullptr;
        blocks_.push_back(p);
        return (T *) p;
    }
    void done() { done_ = true; }
};

}  // namespace
