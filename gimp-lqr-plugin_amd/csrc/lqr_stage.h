// lqr_stage.h -- host <-> device copies of whole images through a ring of pinned bounce buffers, as plain C++17.  No HIP, no globals: one
// class over the few device operations its owner supplies (StageDevice; the shim implements them on its own stream), so that the same
// code runs in tests/c/stage_main.cc over a fake device under ThreadSanitizer and AddressSanitizer without a GPU.
// The plug-in hands over and takes back PAGEABLE memory (a g_malloc'ed buffer at lqr_carver_new, render.c:222; the scan-line buffer at
// read-out, io_functions.c:155-164); hipMemcpy on pageable memory runs at ~1-2 GB/s here (it pins and unpins as it goes).  The copies go
// through the ring instead, and the CPU side of the bounce -- memcpy between the caller's pageable buffer and the ring, page faults of a
// freshly allocated destination included -- is done by a few helper threads in parallel while the DMA engine moves other chunks
// (round 3: one thread, two 8 MB buffers: 8.6 GB/s up, 4.2 GB/s down; a single core's memcpy and its page faults were the limit, not
// PCIe).  The helpers touch host memory only; every device operation stays on the caller's thread.
// upload and download return with the transfer complete, also on error (the helpers and the stream are drained before they return).
// Everything here has internal linkage (the library exports the C ABI of include/lqr_hip.h and nothing else).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace {

// What the ring asks of the device, all on one stream.  Every int is 0 or the owner's error code, which upload / download return as
// it is; the owner keeps the reason
struct StageDevice {
    // slot i: `bytes` of pinned host memory and an event (one never recorded counts as complete).  On failure nothing of it is left
    virtual int slot_create(int slot, size_t bytes, void **host) = 0;
    virtual void slot_destroy(int slot, void *host) = 0;
    virtual int copy_up(void *dev_dst, const void *host_src, size_t n) = 0;         // asynchronous copies, queued on the stream
    virtual int copy_down(void *host_dst, const void *dev_src, size_t n) = 0;
    virtual int record(int slot) = 0;           // the slot's event, on the stream
    virtual int wait(int slot) = 0;             // ... until it is complete
    virtual bool landed(int slot) = 0;          // ... whether it is complete, without waiting
    // wait for everything queued on the stream.  quiet: the caller has an earlier error to report, the reason of this one is not kept
    virtual int wait_stream(bool quiet) = 0;

protected:
    ~StageDevice() = default;
};

class StageRing {
public:
    StageRing(StageDevice &dev, int slots, size_t slot_bytes, int helpers) : dev_(dev), slots_((size_t) slots), bytes_(slot_bytes), helpers_(helpers) {}
    StageRing(const StageRing &) = delete;
    StageRing &operator=(const StageRing &) = delete;
    ~StageRing()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_job_.notify_all();
        for (auto &t : th_) t.join();
        for (size_t i = 0; i < slot_.size(); i++) dev_.slot_destroy((int) i, slot_[i]);
    }

    // host -> device.  Ends with a wait for the stream: whatever was queued on it under the upload has completed too
    int upload(void *dst, const void *src, size_t bytes)
    {
        int rc = create();
        if (rc) return rc;
        const size_t nchunk = chunks(bytes);
        begin(nchunk);
        auto body = [&]() -> int {
            size_t submitted = 0;
            for (size_t i = 0; i < nchunk; i++) {
                // keep the helpers a ring ahead: chunk j goes into slot j % slots once the DMA that last read it is done
                for (; submitted < nchunk && submitted < i + slots_; submitted++) {
                    const size_t slot = submitted % slots_, off = submitted * bytes_;
                    if (int r = dev_.wait((int) slot)) return r;
                    submit(submitted, slot_[slot], (const uint8_t *) src + off, std::min(bytes_, bytes - off));
                }
                const size_t slot = i % slots_, off = i * bytes_;
                wait(i);
                if (int r = dev_.copy_up((uint8_t *) dst + off, slot_[slot], std::min(bytes_, bytes - off))) return r;
                if (int r = dev_.record((int) slot)) return r;
            }
            return 0;
        };
        rc = body();
        drain();            // whatever happened, nobody touches the caller's buffer or the ring after we return
        const int e = dev_.wait_stream(rc != 0);
        return rc ? rc : e;
    }
    // device -> host.  One that succeeds has waited for every slot's event, and adds no wait for the stream
    int download(void *dst, const void *src, size_t bytes)
    {
        int rc = create();
        if (rc) return rc;
        const size_t nchunk = chunks(bytes);
        begin(nchunk);
        size_t copied_out = 0;      // chunks handed to the helpers
        auto hand_over = [&](size_t j) -> int {
            const size_t slot = j % slots_, off = j * bytes_;
            if (int r = dev_.wait((int) slot)) return r;
            submit(j, (uint8_t *) dst + off, slot_[slot], std::min(bytes_, bytes - off));
            return 0;
        };
        auto body = [&]() -> int {
            for (size_t i = 0; i < nchunk; i++) {
                if (i >= slots_) {              // slot reuse: the helper must have emptied it
                    for (; copied_out <= i - slots_; copied_out++) if (int r = hand_over(copied_out)) return r;
                    wait(i - slots_);
                }
                const size_t slot = i % slots_, off = i * bytes_;
                if (int r = dev_.copy_down(slot_[slot], (const uint8_t *) src + off, std::min(bytes_, bytes - off))) return r;
                if (int r = dev_.record((int) slot)) return r;
                // hand over whatever has landed already, without waiting for it
                for (; copied_out < i && dev_.landed((int) (copied_out % slots_)); copied_out++) if (int r = hand_over(copied_out)) return r;
            }
            for (; copied_out < nchunk; copied_out++) if (int r = hand_over(copied_out)) return r;
            return 0;
        };
        rc = body();
        drain();            // the helpers are done with the caller's buffer
        if (rc) (void) dev_.wait_stream(true);
        return rc;
    }
    // no helper has work or is at work (what both directions leave behind)
    bool idle()
    {
        std::lock_guard<std::mutex> lk(mu_);
        return pending_ == 0 && q_.empty();
    }

private:
    struct Job { size_t ticket; void *dst; const void *src; size_t n; };

    size_t chunks(size_t bytes) const { return (bytes + bytes_ - 1) / bytes_; }
    // The slots and the helpers, at the first transfer.  All or nothing: a partial set of slots is released again, so a later call
    // starts over
    int create()
    {
        if (slot_.size() == slots_) return 0;
        for (size_t i = 0; i < slots_; i++) {
            void *host = nullptr;
            const int rc = dev_.slot_create((int) i, bytes_, &host);
            if (rc) {
                for (size_t k = 0; k < slot_.size(); k++) dev_.slot_destroy((int) k, slot_[k]);
                slot_.clear();
                return rc;
            }
            slot_.push_back((uint8_t *) host);
        }
        for (int i = 0; i < helpers_; i++) th_.emplace_back([this] { run(); });
        return 0;
    }
    void run()
    {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_job_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (stop_ && q_.empty()) return;
                j = q_.front(); q_.pop_front();
            }
            memcpy(j.dst, j.src, j.n);
            {
                std::lock_guard<std::mutex> lk(mu_);
                done_[j.ticket] = 1;
                pending_--;
            }
            cv_done_.notify_all();
        }
    }
    void begin(size_t tickets) { std::lock_guard<std::mutex> lk(mu_); done_.assign(tickets, 0); }
    void submit(size_t ticket, void *dst, const void *src, size_t n)
    {
        { std::lock_guard<std::mutex> lk(mu_); q_.push_back(Job{ticket, dst, src, n}); pending_++; }
        cv_job_.notify_one();
    }
    void drain()
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [this] { return pending_ == 0; });
    }
    void wait(size_t ticket)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [&] { return done_[ticket] != 0; });
    }

    StageDevice &dev_;
    const size_t slots_, bytes_;        // the ring: so many pinned buffers of so many bytes
    const int helpers_;
    std::vector<uint8_t *> slot_;       // all of them, or none
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_job_, cv_done_;
    std::deque<Job> q_;
    std::vector<char> done_;            // per ticket (chunk) of the current transfer
    size_t pending_ = 0;                // submitted and not finished
    bool stop_ = false;
};

}  // namespace
