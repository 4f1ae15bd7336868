// The store-form policy (netflow_amd/csrc/nfcs_store_policy.h) as a pure function of its observation
// history. Stand-alone: no device, no runtime. tests/test_store_policy.py builds and runs it, once plain
// and once with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>

#include "nfcs_store_policy.h"

using nfcs::StorePolicy;
using nfcs::kStoreFormDeferred;
using nfcs::kStoreFormSparse;

static int g_fail = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

// 4,096 sampled packets: at the threshold exactly, and one packet under it
static const uint32_t kS = 4096;
static const uint32_t kAt = kS * nfcs::kSparseMaxNum / nfcs::kSparseMaxDen;

int main() {
    {  // the start state
        StorePolicy p;
        CHECK(p.form == kStoreFormDeferred);
        CHECK(p.obs_sampled == 0 && p.obs_storing == 0);
    }
    {  // two low observations needed before sparse
        StorePolicy p;
        p.observe(1, kS, 0);
        CHECK(p.form == kStoreFormDeferred);
        CHECK(p.obs_gen == 1 && p.obs_sampled == kS && p.obs_storing == 0);
        p.observe(2, kS, kAt - 1);
        CHECK(p.form == kStoreFormSparse);
        p.observe(3, kS, 0);
        CHECK(p.form == kStoreFormSparse);
    }
    {  // the threshold itself is "at or over": not low
        StorePolicy p;
        p.observe(1, kS, kAt);
        p.observe(2, kS, kAt);
        CHECK(p.form == kStoreFormDeferred);
        CHECK(!StorePolicy::low(kS, kAt) && StorePolicy::low(kS, kAt - 1));
        CHECK(!StorePolicy::low(0, 0));
    }
    {  // one high observation sends a sparse context back, and two lows are needed again
        StorePolicy p;
        p.observe(1, kS, 0);
        p.observe(2, kS, 0);
        CHECK(p.form == kStoreFormSparse);
        p.observe(3, kS, kS);
        CHECK(p.form == kStoreFormDeferred);
        CHECK(p.obs_storing == kS);
        p.observe(4, kS, 0);
        CHECK(p.form == kStoreFormDeferred);
        p.observe(5, kS, 0);
        CHECK(p.form == kStoreFormSparse);
    }
    {  // stale generations are ignored: a repeated read, an older one, generation 0, an empty sample
        StorePolicy p;
        p.observe(5, kS, 0);
        p.observe(5, kS, 0);  // the same word read twice is one observation
        CHECK(p.form == kStoreFormDeferred);
        p.observe(4, kS, 0);
        p.observe(0, kS, 0);
        p.observe(6, 0, 0);
        CHECK(p.form == kStoreFormDeferred && p.obs_gen == 5);
        p.observe(6, kS, 0);
        CHECK(p.form == kStoreFormSparse);
        p.observe(3, kS, kS);  // a late high one of an earlier call does not turn it back
        CHECK(p.form == kStoreFormSparse && p.obs_gen == 6);
    }
    {  // alternating low and high observations never go sparse
        StorePolicy p;
        for (uint32_t g = 1; g <= 64; ++g) {
            p.observe(g, kS, (g & 1u) ? 0u : kS);
            CHECK(p.form == kStoreFormDeferred);
        }
    }
    {  // generations in serial-number order across the wrap
        StorePolicy p;
        p.last_gen = 0xFFFFFFFDu;  // a context that has counted up to there
        p.observe(0xFFFFFFFEu, kS, 0);
        p.observe(0xFFFFFFFFu, kS, kS);
        p.observe(1, kS, 0);
        CHECK(p.form == kStoreFormDeferred && p.obs_gen == 1);
        p.observe(2, kS, 0);
        CHECK(p.form == kStoreFormSparse);
        p.observe(0xFFFFFFFFu, kS, kS);
        CHECK(p.form == kStoreFormSparse);
    }
    {  // reset: deferred, and every generation up to the one given is skipped
        StorePolicy p;
        p.observe(1, kS, 0);
        p.observe(2, kS, 0);
        p.reset(4);
        CHECK(p.form == kStoreFormDeferred && p.obs_sampled == 0);
        p.observe(3, kS, 0);
        p.observe(4, kS, 0);
        CHECK(p.form == kStoreFormDeferred && p.obs_sampled == 0);
        p.observe(5, kS, 0);
        p.observe(6, kS, 0);
        CHECK(p.form == kStoreFormSparse);
    }
    {  // a count above the sample (counters shared by concurrent calls) is high and reported clamped
        StorePolicy p;
        p.observe(1, kS, 0xFFFFFFFFu);
        CHECK(p.form == kStoreFormDeferred && p.obs_storing == kS);
    }
    std::printf(g_fail ? "store_policy_test: %d failed\n" : "store_policy_test: ok\n", g_fail);
    return g_fail ? 1 : 0;
}
