/* Stand-alone host program (tests/test_filter_hold.py builds it with -fsanitize=address,undefined): the reference-counted holder of a filter
 * batch's one allocation (xapiand_amd/csrc/xgm_filter_hold.h) as xgm_filter_free uses it — every free order, and frees from many threads at once.
 * malloc stands in for the device allocation: the sanitizer reports a use after the last reference, a double free and a leak. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "xgm_filter_hold.h"

namespace {

struct Filter { unsigned char* bits; FilterBatchHold* hold; };
std::atomic<int> g_frees{0};

std::vector<Filter*> build(uint32_t n, size_t bytes_each) {
    FilterBatchHold* h = new FilterBatchHold();
    h->d_mem = malloc(n * bytes_each);
    memset(h->d_mem, 0x5a, n * bytes_each);
    h->refs.store(n, std::memory_order_relaxed);
    std::vector<Filter*> out;
    for (uint32_t i = 0; i < n; ++i) out.push_back(new Filter{(unsigned char*)h->d_mem + i * bytes_each, h});
    return out;
}

/* xgm_filter_free's handling of a batch filter */
void filter_free(Filter* f) {
    if (f->hold->drop()) { free(f->hold->d_mem); delete f->hold; ++g_frees; }
    delete f;
}

int fail(const char* what) { fprintf(stderr, "filter_hold: %s\n", what); return 1; }

}  // namespace

int main() {
    const size_t each = 256;
    /* every order: forward, reverse, odd ones then even ones; the survivors' bytes stay readable and writable until their own free */
    for (int order = 0; order < 3; ++order) {
        for (uint32_t n : {1u, 2u, 25u, 64u}) {
            std::vector<Filter*> fs = build(n, each);
            std::vector<uint32_t> seq;
            if (order == 0) for (uint32_t i = 0; i < n; ++i) seq.push_back(i);
            if (order == 1) for (uint32_t i = n; i-- > 0;) seq.push_back(i);
            if (order == 2) { for (uint32_t i = 1; i < n; i += 2) seq.push_back(i); for (uint32_t i = 0; i < n; i += 2) seq.push_back(i); }
            const int before = g_frees.load();
            for (size_t k = 0; k < seq.size(); ++k) {
                for (size_t j = k; j < seq.size(); ++j) {                    /* every filter not yet freed still owns live memory */
                    if (fs[seq[j]]->bits[each - 1] != 0x5a) return fail("a surviving filter's bytes changed");
                    fs[seq[j]]->bits[0] = 0x5a;
                }
                if (g_frees.load() != before) return fail("the allocation went before the last filter");
                filter_free(fs[seq[k]]);
            }
            if (g_frees.load() != before + 1) return fail("the last filter did not free the allocation exactly once");
        }
    }
    /* 8 threads free the 64 filters of one batch, eight each, all at once; and 8 threads each build and free batches of their own */
    for (int rep = 0; rep < 50; ++rep) {
        std::vector<Filter*> fs = build(64, each);
        const int before = g_frees.load();
        std::vector<std::thread> ts;
        for (int t = 0; t < 8; ++t)
            ts.emplace_back([&fs, t] { for (int i = 0; i < 8; ++i) { Filter* f = fs[(size_t)(i * 8 + t)]; f->bits[1] = (unsigned char)t; filter_free(f); } });
        for (std::thread& t : ts) t.join();
        if (g_frees.load() != before + 1) return fail("concurrent frees: not exactly one free of the allocation");
    }
    {
        const int before = g_frees.load();
        std::vector<std::thread> ts;
        for (int t = 0; t < 8; ++t)
            ts.emplace_back([t] { for (int r = 0; r < 20; ++r) { std::vector<Filter*> fs = build(8, 256); for (size_t i = 0; i < 8; ++i) filter_free(fs[(i + (size_t)t) % 8]); } });
        for (std::thread& t : ts) t.join();
        if (g_frees.load() != before + 160) return fail("per-thread batches: a batch was not freed exactly once");
    }
    puts("filter_hold ok");
    return 0;
}
