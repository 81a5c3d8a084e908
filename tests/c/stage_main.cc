// The launch shim's pinned transfer ring and its helper threads (gimp-lqr-plugin_amd/csrc/lqr_stage.h) without a GPU, over a fake device:
// "device memory" and the pinned slots are heap blocks of exactly their size, a DMA thread executes the queued copies in order with a
// deterministic pseudo-random yield before each, and an event is complete once the queue has passed it (one never recorded counts as
// complete, as in HIP).  4 slots of 64 bytes and 3 helpers, so that every boundary of the ring is a few hundred bytes away.
// Built twice by tests/test_stage.py with -Werror, under ThreadSanitizer and under AddressSanitizer + UndefinedBehaviorSanitizer;
// prints "stage ok" and exits 0, or says which check failed.  The caller's buffers are heap blocks of exactly the transfer's size and
// are freed on the line after the call returns: a helper that still copies, or a chunk one byte too long, is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "lqr_stage.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

enum { SLOTS = 4, SLOT_BYTES = 64, HELPERS = 3, EFAKE = -9 };

class FakeDevice final : public StageDevice {
public:
    // what the ring asked for, in order: c<slot> d<slot> slot made / released, w<slot> event wait, r<slot> event record, ?<slot> event query,
    // u<slot>:<offset in device memory>+<bytes> / d.. copy up / down, s stream wait, q quiet stream wait; a failed one ends in '!'
    std::string journal;
    const uint8_t *dev_base = nullptr;          // offsets in the journal are relative to it
    long fail_op = -1;                          // the kth operation of a transfer from now on fails, once (slot_create is not counted)
    bool fired = false;                         // ... it did
    char fired_kind = 0;
    int fail_slot = -1;                         // the pinned allocation of this slot fails, once
    int live_slots = 0;

    explicit FakeDevice(int slots = SLOTS) : slots_(slots), dma_([this] { run(); }) {}
    ~FakeDevice()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_work_.notify_all();
        dma_.join();
    }
    bool queue_empty()
    {
        std::lock_guard<std::mutex> lk(mu_);
        return passed_ == issued_ && q_.empty();
    }

    int slot_create(int slot, size_t bytes, void **host) override
    {
        CHECK(slot >= 0 && slot < slots_ && bytes == SLOT_BYTES && !slot_[slot]);
        if (slot == fail_slot) { fail_slot = -1; note('c', slot, true); return EFAKE; }
        slot_[slot] = (uint8_t *) malloc(bytes);
        CHECK(slot_[slot]);
        ev_[slot] = 0;
        live_slots++;
        note('c', slot, false);
        *host = slot_[slot];
        return 0;
    }
    void slot_destroy(int slot, void *host) override
    {
        CHECK(slot >= 0 && slot < slots_ && host && host == slot_[slot]);
        free(slot_[slot]);
        slot_[slot] = nullptr;
        live_slots--;
        note('x', slot, false);
    }
    int copy_up(void *dev_dst, const void *host_src, size_t n) override { return copy('u', dev_dst, host_src, n, host_src, dev_dst); }
    int copy_down(void *host_dst, const void *dev_src, size_t n) override { return copy('d', host_dst, dev_src, n, host_dst, dev_src); }
    int record(int slot) override
    {
        if (fails('r')) { note('r', slot, true); return EFAKE; }
        note('r', slot, false);
        std::lock_guard<std::mutex> lk(mu_);
        ev_[slot] = ++issued_;
        q_.push_back(Op{nullptr, nullptr, 0});
        cv_work_.notify_one();
        return 0;
    }
    int wait(int slot) override
    {
        if (fails('w')) { note('w', slot, true); return EFAKE; }
        note('w', slot, false);
        std::unique_lock<std::mutex> lk(mu_);
        cv_passed_.wait(lk, [&] { return passed_ >= ev_[slot]; });
        return 0;
    }
    bool landed(int slot) override
    {
        if (fails('?')) { note('?', slot, true); return false; }
        note('?', slot, false);
        std::lock_guard<std::mutex> lk(mu_);
        return passed_ >= ev_[slot];
    }
    // one that fails reports it after the stream has stopped, as the runtime reports an asynchronous error at the synchronisation
    int wait_stream(bool quiet) override
    {
        const bool f = fails('s');
        journal += quiet ? " q" : " s";
        if (f) journal += '!';
        std::unique_lock<std::mutex> lk(mu_);
        cv_passed_.wait(lk, [&] { return passed_ == issued_; });
        return f ? EFAKE : 0;
    }

private:
    struct Op { void *dst; const void *src; size_t n; };       // n == 0: an event's place in the queue

    bool fails(char kind)
    {
        if (fail_op < 0 || fail_op-- != 0) return false;
        fired = true; fired_kind = kind;
        return true;
    }
    void note(char kind, int slot, bool failed)
    {
        journal += ' '; journal += kind; journal += std::to_string(slot);
        if (failed) journal += '!';
    }
    int copy(char kind, void *dst, const void *src, size_t n, const void *host, const void *dev)
    {
        int slot = 0;
        while (slot < slots_ && host != slot_[slot]) slot++;
        CHECK(slot < slots_ && n > 0 && n <= SLOT_BYTES);        // a whole slot's start, and no more than a slot
        const bool f = fails(kind);
        note(kind, slot, false);
        journal += ':' + std::to_string((const uint8_t *) dev - dev_base) + '+' + std::to_string(n);
        if (f) { journal += '!'; return EFAKE; }
        std::lock_guard<std::mutex> lk(mu_);
        ++issued_;
        q_.push_back(Op{dst, src, n});
        cv_work_.notify_one();
        return 0;
    }
    void run()
    {
        unsigned lcg = 12345;
        for (;;) {
            Op op;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_work_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                op = q_.front(); q_.pop_front();
            }
            lcg = lcg * 1664525u + 1013904223u;
            for (unsigned y = (lcg >> 24) & 3; y > 0; y--) std::this_thread::yield();
            if (op.n) memcpy(op.dst, op.src, op.n);
            { std::lock_guard<std::mutex> lk(mu_); passed_++; }
            cv_passed_.notify_all();
        }
    }

    const int slots_;
    uint8_t *slot_[SLOTS] = {};
    unsigned long ev_[SLOTS] = {};              // the place in the queue of the slot's last record; 0: never recorded
    std::mutex mu_;
    std::condition_variable cv_work_, cv_passed_;
    std::deque<Op> q_;
    unsigned long issued_ = 0, passed_ = 0;     // operations queued / executed
    bool stop_ = false;
    std::thread dma_;                           // (last: it starts in the constructor)
};

static uint8_t pattern(size_t i, unsigned salt) { return (uint8_t) ((i * 131u + (i >> 8) * 7u + salt) & 0xff); }

// upload `bytes` to fresh device memory; the source is freed on the line after the call.  The device block is the caller's to free
static int up(FakeDevice &dev, StageRing &ring, size_t bytes, unsigned salt, uint8_t **dmem)
{
    uint8_t *src = (uint8_t *) malloc(bytes);
    *dmem = (uint8_t *) malloc(bytes);
    CHECK((src && *dmem) || !bytes);
    for (size_t i = 0; i < bytes; i++) src[i] = pattern(i, salt);
    dev.dev_base = *dmem;
    const int rc = ring.upload(*dmem, src, bytes);
    free(src);
    CHECK(dev.queue_empty() && ring.idle());
    return rc;
}
// ... and back; the destination is compared (on success) and freed right after the call
static int down(FakeDevice &dev, StageRing &ring, size_t bytes, unsigned salt, const uint8_t *dmem)
{
    uint8_t *dst = (uint8_t *) malloc(bytes);
    CHECK(dst || !bytes);
    dev.dev_base = dmem;
    const int rc = ring.download(dst, dmem, bytes);
    size_t bad = 0;
    if (!rc) for (size_t i = 0; i < bytes; i++) bad += dst[i] != pattern(i, salt);
    free(dst);
    CHECK(dev.queue_empty() && ring.idle());
    CHECK(bad == 0);
    return rc;
}
static void round_trip(FakeDevice &dev, StageRing &ring, size_t bytes, unsigned salt)
{
    uint8_t *dmem = nullptr;
    CHECK(up(dev, ring, bytes, salt, &dmem) == 0);
    CHECK(down(dev, ring, bytes, salt, dmem) == 0);
    free(dmem);
}

static void test_round_trips()
{
    FakeDevice dev;
    StageRing ring(dev, SLOTS, SLOT_BYTES, HELPERS);
    CHECK(dev.live_slots == 0);                 // created at the first transfer
    // the ring exactly full +- 1, the first slot reused, two wraps with a short last chunk, a thousand chunks
    static const size_t sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 320, 583, 64003};
    unsigned salt = 1;
    for (size_t bytes : sizes) round_trip(dev, ring, bytes, salt++);
    for (size_t bytes : sizes) round_trip(dev, ring, bytes, salt++);       // ... and again, on events that have all been recorded
    CHECK(dev.live_slots == SLOTS);
    // The narrowest rings, one and two slots with one helper: a slot is refilled right after its chunk was handed over, so that the
    // only thing between the helper that empties it and the copy that fills it again is the ring's own wait
    for (int slots = 1; slots <= 2; slots++) {
        FakeDevice narrow(slots);
        StageRing ring1(narrow, slots, SLOT_BYTES, 1);
        for (size_t bytes : sizes) round_trip(narrow, ring1, bytes, salt++);
        CHECK(narrow.live_slots == slots);
    }
}

// what h2d_staged of the parent commit issues for 1, 3 and 6 chunks on a fresh ring of 4 slots, read off its source: the helpers are kept
// a ring ahead (an event wait per chunk before a helper may fill its slot), each chunk is one copy and one record of its slot's event,
// and the upload ends with a wait for the stream
static void test_upload_journal()
{
    static const struct { size_t bytes; const char *ops; } cases[] = {
        {64, " c0 c1 c2 c3 w0 u0:0+64 r0 s"},
        {191, " c0 c1 c2 c3 w0 w1 w2 u0:0+64 r0 u1:64+64 r1 u2:128+63 r2 s"},
        {330, " c0 c1 c2 c3 w0 w1 w2 w3 u0:0+64 r0 w0 u1:64+64 r1 w1 u2:128+64 r2 u3:192+64 r3 u0:256+64 r0 u1:320+10 r1 s"},
    };
    for (auto &c : cases) {
        FakeDevice dev;
        {
            StageRing ring(dev, SLOTS, SLOT_BYTES, HELPERS);
            uint8_t *dmem = nullptr;
            CHECK(up(dev, ring, c.bytes, 7, &dmem) == 0);
            if (dev.journal != c.ops) { fprintf(stderr, "upload of %zu bytes issued\n%s\nnot\n%s\n", c.bytes, dev.journal.c_str(), c.ops); exit(1); }
            CHECK(down(dev, ring, c.bytes, 7, dmem) == 0);
            free(dmem);
        }
        CHECK(dev.live_slots == 0);
    }
}

// a 6-chunk transfer in each direction with its kth device operation failing, for every k it makes
static void test_error_paths()
{
    const size_t bytes = 330;
    FakeDevice dev;
    StageRing ring(dev, SLOTS, SLOT_BYTES, HELPERS);
    round_trip(dev, ring, bytes, 3);            // the ring exists, every event has been recorded
    long k = 0;
    for (;; k++) {                              // uploads
        uint8_t *dmem = nullptr;
        dev.fired = false; dev.fail_op = k;
        const int rc = up(dev, ring, bytes, 40 + (unsigned) k, &dmem);
        dev.fail_op = -1;
        free(dmem);
        if (!dev.fired) { CHECK(rc == 0); break; }
        CHECK(rc == EFAKE);
        round_trip(dev, ring, bytes, 90 + (unsigned) k);       // the next transfer on the same ring
    }
    CHECK(k == 6 + 6 + 6 + 1);                  // an event wait, a copy and a record per chunk, and the stream wait
    uint8_t *dmem = nullptr;
    CHECK(up(dev, ring, bytes, 5, &dmem) == 0);
    for (k = 0;; k++) {                         // downloads: how many event queries one makes depends on timing
        dev.fired = false; dev.fail_op = k;
        const int rc = down(dev, ring, bytes, 5, dmem);
        dev.fail_op = -1;
        if (!dev.fired) { CHECK(rc == 0); break; }
        CHECK(rc == (dev.fired_kind == '?' ? 0 : EFAKE));      // a query that fails says "not yet": the chunk is waited for later
        uint8_t *d2 = nullptr;
        CHECK(up(dev, ring, bytes, 60 + (unsigned) k, &d2) == 0);
        CHECK(down(dev, ring, bytes, 60 + (unsigned) k, d2) == 0);
        free(d2);
    }
    CHECK(k >= 6 + 6 + 6);                      // a copy, a record and an event wait per chunk at the least
    free(dmem);
}

// the pinned allocation of slot k fails: the call fails, every slot made so far is released, the next call creates the ring
static void test_creation()
{
    for (int k = 0; k < SLOTS; k++) {
        FakeDevice dev;
        {
            StageRing ring(dev, SLOTS, SLOT_BYTES, HELPERS);
            dev.fail_slot = k;
            uint8_t *dmem = nullptr;
            CHECK(up(dev, ring, 100, 1, &dmem) == EFAKE && dev.live_slots == 0);
            std::string want;
            for (int i = 0; i < k; i++) want += " c" + std::to_string(i);
            want += " c" + std::to_string(k) + "!";
            for (int i = 0; i < k; i++) want += " x" + std::to_string(i);
            CHECK(dev.journal == want);         // no device operation but those
            dev.fail_slot = k;
            CHECK(down(dev, ring, 100, 1, dmem) == EFAKE && dev.live_slots == 0);      // a download creates it just as well
            free(dmem);
            round_trip(dev, ring, 583, 2);
            CHECK(dev.live_slots == SLOTS);
        }
        CHECK(dev.live_slots == 0);
    }
}

int main()
{
    test_round_trips();
    test_upload_journal();
    test_error_paths();
    test_creation();
    printf("stage ok\n");
    return 0;
}
