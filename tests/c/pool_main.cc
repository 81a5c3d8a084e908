// The launch shim's allocation cache (gimp-lqr-plugin_amd/csrc/lqr_pool.h) without a GPU: the raw allocator and the raw free are
// malloc / free with a journal and a switch that makes the raw allocator report out of memory, the prepare hook can be told to fail.
// Built by tests/test_pool.py with -Werror under AddressSanitizer and UndefinedBehaviorSanitizer; prints "pool ok" and exits 0, or
// says which check failed.  LeakSanitizer confirms at exit what the live count says: no block is left.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "lqr_pool.h"

enum { ENOMEM_ = -2, EOTHER_ = -3, EHOOK_ = -7 };              // stand-ins for LQRHIP_ENOMEM, LQRHIP_EHIP and a hook's own code
static const size_t MiB = (size_t) 1 << 20;

struct Event { char kind; void *p; size_t bytes; };             // 'a' raw alloc, 'x' raw alloc that failed, 'f' raw free
static std::vector<Event> journal;
static std::vector<void *> raw_live;
static bool raw_broken = false;                                 // the raw allocator fails, and not for lack of memory
static long oom_for = 0;                                        // the next so many raw allocations report out of memory
static int hook_rc = 0;                                         // what the prepare hook returns
static std::string hook_name;                                   // ... and the name it was last given
static size_t hook_bytes = 0;

static int raw_alloc(void **p, size_t bytes, std::string &why)
{
    if (raw_broken) { journal.push_back({'x', nullptr, bytes}); why = "raw: broken"; return EOTHER_; }
    if (oom_for > 0) { oom_for--; journal.push_back({'x', nullptr, bytes}); why = "raw: out of memory"; return ENOMEM_; }
    *p = malloc(64);            // (the cache never touches a block: its class is what it is told)
    if (!*p) abort();
    raw_live.push_back(*p);
    journal.push_back({'a', *p, bytes});
    return 0;
}
static void raw_free(void *p)
{
    size_t i = 0;
    while (i < raw_live.size() && raw_live[i] != p) i++;
    if (i == raw_live.size()) { fprintf(stderr, "raw free of a block that is not live\n"); abort(); }
    raw_live.erase(raw_live.begin() + (long) i);
    journal.push_back({'f', p, 0});
    free(p);
}
static int prepare(void *p, size_t bytes, const char *name)
{
    if (!p) { fprintf(stderr, "prepare of no block\n"); abort(); }
    hook_name = name; hook_bytes = bytes;
    return hook_rc;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
static std::string kinds(size_t from = 0)
{
    std::string s;
    for (size_t i = from; i < journal.size(); i++) s += journal[i].kind;
    return s;
}
// live and cached after every step
#define STATE(cache, n_live, n_cached) CHECK((cache).live() == (size_t) (n_live) && (cache).cached_bytes() == (size_t) (n_cached))

static void test_classes()
{
    journal.clear();
    BlockCache c((size_t) 24 << 30, ENOMEM_, raw_alloc, raw_free, prepare);
    std::string err;
    void *a = nullptr, *b = nullptr, *d = nullptr;
    STATE(c, 0, 0);
    CHECK(BlockCache::size_class(1) == MiB && BlockCache::size_class(MiB) == MiB && BlockCache::size_class(MiB + 1) == 2 * MiB);
    CHECK(c.alloc(&a, 1, "one byte", err) == 0 && a && kinds() == "a" && journal[0].bytes == MiB);
    CHECK(hook_name == "one byte" && hook_bytes == MiB && err.empty());
    STATE(c, 1, 0);
    c.free(a);
    CHECK(kinds() == "a");                                      // cached, not given back
    STATE(c, 0, MiB);
    CHECK(c.alloc(&b, MiB, "one MiB", err) == 0 && b == a && kinds() == "a");          // the same class: no raw call
    STATE(c, 1, 0);
    c.free(b);
    STATE(c, 0, MiB);
    CHECK(c.alloc(&d, MiB + 1, "one MiB and a byte", err) == 0 && d && d != a);         // the next class: not served by that block
    CHECK(kinds() == "aa" && journal[1].bytes == 2 * MiB && hook_bytes == 2 * MiB);
    STATE(c, 1, MiB);
    c.free(d);
    STATE(c, 0, 3 * MiB);
    c.trim();
    CHECK(kinds() == "aaff" && raw_live.empty());
    STATE(c, 0, 0);
}

static void test_oom_retry()
{
    journal.clear();
    BlockCache c((size_t) 24 << 30, ENOMEM_, raw_alloc, raw_free, prepare);
    std::string err;
    void *a = nullptr, *b = nullptr, *p = nullptr, *q = nullptr;
    // an empty cache: exactly one raw call
    oom_for = 1;
    CHECK(c.alloc(&p, 10, "empty", err) == ENOMEM_ && !p && kinds() == "x" && err == "raw: out of memory");
    STATE(c, 0, 0);
    // two cached blocks of other classes, one live one: the first OOM gives the cached ones back, the retry succeeds
    CHECK(c.alloc(&a, 2 * MiB, "a", err) == 0 && c.alloc(&b, 3 * MiB, "b", err) == 0 && c.alloc(&q, 5 * MiB, "q", err) == 0);
    c.free(a); c.free(b);
    STATE(c, 1, 5 * MiB);
    journal.clear(); err.clear();
    oom_for = 1;
    CHECK(c.alloc(&p, 4 * MiB, "retried", err) == 0 && p && kinds() == "xffa" && err.empty());
    CHECK(journal[1].p == a && journal[2].p == b && journal[3].bytes == 4 * MiB && raw_live.size() == 2);
    STATE(c, 2, 0);
    // ... and a second OOM is the answer: one retry only
    c.free(p);
    STATE(c, 1, 4 * MiB);
    journal.clear();
    oom_for = 2;
    void *r = &r;
    CHECK(c.alloc(&r, 7 * MiB, "twice", err) == ENOMEM_ && r == nullptr && kinds() == "xfx" && err == "raw: out of memory");
    STATE(c, 1, 0);
    CHECK(oom_for == 0 && raw_live.size() == 1);
    // the cache is empty now: one raw call again
    journal.clear();
    oom_for = 1;
    CHECK(c.alloc(&r, 7 * MiB, "empty again", err) == ENOMEM_ && !r && kinds() == "x");
    STATE(c, 1, 0);
    c.free(q);
    STATE(c, 0, 5 * MiB);
    c.trim();
    STATE(c, 0, 0);
    CHECK(raw_live.empty());
}

static void test_injected_failure()
{
    for (int n = 0; n < 3; n++) {
        journal.clear();
        BlockCache c((size_t) 24 << 30, ENOMEM_, raw_alloc, raw_free, prepare);
        std::string err;
        void *s0 = nullptr, *s1 = nullptr;
        CHECK(c.alloc(&s0, MiB, "seed", err) == 0 && c.alloc(&s1, MiB, "seed", err) == 0);
        c.free(s0); c.free(s1);                                 // two blocks of class 1 MiB are cached: requests of it are hits, of 2 MiB misses
        STATE(c, 0, 2 * MiB);
        // hit, miss, hit, miss ...: the nth of them fails, whichever it would have been
        static const char *names[4] = {"&first", "&second", "&third", "&fourth"};
        std::vector<void *> got;
        c.fail_in(n);
        for (int i = 0; i < 4; i++) {
            const bool would_hit = i % 2 == 0;
            const size_t before = journal.size(), live = c.live(), cached = c.cached_bytes();
            void *p = &p;
            err.clear();
            const int rc = c.alloc(&p, would_hit ? 1 : 2 * MiB, names[i], err);
            if (i == n) {
                CHECK(rc == ENOMEM_ && p == nullptr);
                CHECK(err == std::string("injected allocation failure (") + names[i] + ")");
                CHECK(journal.size() == before);                // no raw call
                STATE(c, live, cached);                          // nothing taken from the cache
            } else {                                            // before it and after it: as if nothing were armed
                CHECK(rc == 0 && p && err.empty());
                CHECK(journal.size() == before + (would_hit ? 0 : 1));
                STATE(c, live + 1, cached - (would_hit ? MiB : 0));
                got.push_back(p);
            }
        }
        CHECK(got.size() == 3);
        void *p = nullptr;
        CHECK(c.alloc(&p, 1, "once only", err) == 0 && p);      // it fails once
        got.push_back(p);
        c.fail_in(0); c.fail_in(-1);                            // disarmed again
        CHECK(c.alloc(&p, 1, "disarmed", err) == 0 && p);
        got.push_back(p);
        STATE(c, 5, 0);
        for (void *g : got) c.free(g);
        CHECK(c.live() == 0 && c.cached_bytes() > 0);
        c.trim();
        STATE(c, 0, 0);
        CHECK(raw_live.empty());
    }
    {   // no name: the text says so
        BlockCache c(0, ENOMEM_, raw_alloc, raw_free, prepare);
        std::string err;
        void *p = &p;
        c.fail_in(0);
        CHECK(c.alloc(&p, 1, nullptr, err) == ENOMEM_ && !p && err == "injected allocation failure (?)");
        STATE(c, 0, 0);
    }
}

static void test_prepare_fails()
{
    journal.clear();
    BlockCache c((size_t) 24 << 30, ENOMEM_, raw_alloc, raw_free, prepare);
    std::string err;
    void *p = &p, *q = nullptr;
    hook_rc = EHOOK_;
    CHECK(c.alloc(&p, 3 * MiB, "fresh block, hook fails", err) == EHOOK_ && p == nullptr);
    CHECK(kinds() == "a");                                      // the block went back to the cache, not to the raw free
    STATE(c, 0, 3 * MiB);
    CHECK(c.alloc(&p, 3 * MiB, "cached block, hook fails", err) == EHOOK_ && p == nullptr && kinds() == "a");
    STATE(c, 0, 3 * MiB);
    hook_rc = 0;
    CHECK(c.alloc(&q, 3 * MiB, "hook recovers", err) == 0 && q == journal[0].p && kinds() == "a");
    STATE(c, 1, 0);
    c.free(q);
    STATE(c, 0, 3 * MiB);
    c.trim();
    STATE(c, 0, 0);
    CHECK(kinds() == "af" && raw_live.empty());
}

static void test_cap_and_strangers()
{
    journal.clear();
    BlockCache c(3 * MiB, ENOMEM_, raw_alloc, raw_free, prepare);      // a small cap
    std::string err;
    void *a = nullptr, *b = nullptr, *d = nullptr;
    CHECK(c.alloc(&a, 2 * MiB, "a", err) == 0 && c.alloc(&b, MiB, "b", err) == 0 && c.alloc(&d, MiB, "d", err) == 0);
    STATE(c, 3, 0);
    c.free(a);
    STATE(c, 2, 2 * MiB);
    c.free(b);                                                  // exactly the cap: kept
    STATE(c, 1, 3 * MiB);
    CHECK(kinds() == "aaa");
    c.free(d);                                                  // beyond it: to the raw free, and the cache forgets the block
    CHECK(kinds() == "aaaf" && journal[3].p == d);
    STATE(c, 0, 3 * MiB);
    void *stranger = malloc(8);                                 // a pointer the cache never handed out
    if (!stranger) abort();
    raw_live.push_back(stranger);
    c.free(stranger);
    CHECK(kinds() == "aaaff" && journal[4].p == stranger);
    STATE(c, 0, 3 * MiB);
    void *p = &p;
    CHECK(c.alloc(&p, 9 * MiB, "e", err) == 0);
    STATE(c, 1, 3 * MiB);
    c.trim();                                                   // trim leaves live blocks alone
    STATE(c, 1, 0);
    CHECK(kinds() == "aaaffaff" && raw_live.size() == 1);
    c.free(p);
    c.trim();
    STATE(c, 0, 0);
    CHECK(raw_live.empty());
}

// a raw allocator that fails for another reason: its code and its reason come back, and there is no retry although blocks are cached
static void test_other_raw_failure()
{
    journal.clear();
    BlockCache c((size_t) 24 << 30, ENOMEM_, raw_alloc, raw_free, prepare);
    std::string err;
    void *s = nullptr, *p = &p;
    CHECK(c.alloc(&s, MiB, "s", err) == 0);
    c.free(s);
    STATE(c, 0, MiB);
    raw_broken = true;
    CHECK(c.alloc(&p, 2 * MiB, "broken", err) == EOTHER_ && !p && err == "raw: broken" && kinds() == "ax");
    raw_broken = false;
    STATE(c, 0, MiB);
    c.trim();
    STATE(c, 0, 0);
    CHECK(raw_live.empty());
}

int main()
{
    test_classes();
    test_oom_retry();
    test_injected_failure();
    test_prepare_fails();
    test_cap_and_strangers();
    test_other_raw_failure();
    CHECK(raw_live.empty());
    printf("pool ok\n");
    return 0;
}
