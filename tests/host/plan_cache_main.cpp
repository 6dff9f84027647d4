// plan_cache_main.cpp -- the per-device host state of the shim (fnft_amd/csrc/nft_plan_cache.h) on fake handles, as a
// stand-alone program: no HIP, no emulator, nothing loaded into Python.  tests/test_plan_cache_cpu.py builds it plain,
// under ThreadSanitizer and under AddressSanitizer and runs each.  Exit status 0 only if every check held and no handle
// was ever destroyed while a call was using it.
#include <atomic>
#include <cstdio>
#include <latch>
#include <mutex>
#include <thread>

#include "../../fnft_amd/csrc/nft_plan_cache.h"

namespace {
struct Fake {
    int device, key;
    bool in_use = false;   // written and read under the lock of the device that owns the handle
    int payload;
};
std::atomic<int> g_live{0}, g_destroyed{0}, g_destroyed_in_use{0}, g_failures{0};

void fake_destroy(Fake *h)
{
    if (h->in_use) g_destroyed_in_use++;
    g_destroyed++;
    g_live--;
    delete h;
}

// a device's state as hip_backend.hip keeps it: the host-call lock and the cache it covers
struct State {
    std::mutex mtx;
    PlanCache<int, Fake, fake_destroy> cache;
};
DeviceRegistry<State> g_devices;

int find_or_create(State &s, int device, int key, Fake **out, int fail_with = 0)
{
    return s.cache.get(key, out, [&](Fake **h) {
        if (fail_with) return fail_with;
        *h = new Fake{device, key, false, 1000 * device + key};
        g_live++;
        return 0;
    });
}

#define CHECK(cond) \
    do { \
        if (!(cond)) { \
            std::fprintf(stderr, "plan_cache_main.cpp:%d: CHECK(%s) failed\n", __LINE__, #cond); \
            g_failures++; \
        } \
    } while (0)

// one thread inside a call on device 0 while another takes device 1 past its capacity
void two_devices()
{
    std::latch a_in_call(1), b_done(1);
    int a_read = -1;
    std::thread A([&] {
        State &s = g_devices.of(0);
        std::lock_guard<std::mutex> lk(s.mtx);
        Fake *h = nullptr;
        CHECK(find_or_create(s, 0, 7, &h) == 0);
        h->in_use = true;
        a_in_call.count_down();
        b_done.wait();
        a_read = h->payload;   // the plan this call is running on
        h->in_use = false;
    });
    std::thread B([&] {
        a_in_call.wait();
        State &s = g_devices.of(1);
        for (int key = 0; key < 6; key++) {
            std::lock_guard<std::mutex> lk(s.mtx);
            Fake *h = nullptr;
            CHECK(find_or_create(s, 1, key, &h) == 0);
            CHECK(h && h->device == 1 && h->key == key);
        }
        b_done.count_down();
    });
    A.join();
    B.join();
    CHECK(a_read == 7);
    CHECK(g_destroyed == 4);                  // device 1's first four, at its fifth key
    CHECK(g_devices.of(0).cache.size() == 1 && g_devices.of(1).cache.size() == 2);
}

void one_device()
{
    State &s = g_devices.of(2);
    CHECK(&s == &g_devices.of(2) && &s != &g_devices.of(0));   // a stable reference, a state of its own
    Fake *h[5] = {}, *again = nullptr;
    for (int key = 0; key < 3; key++) CHECK(find_or_create(s, 2, key, &h[key]) == 0);
    CHECK(find_or_create(s, 2, 1, &again) == 0 && again == h[1]);          // a hit returns the same handle
    const int live = g_live, destroyed = g_destroyed;
    Fake *none = nullptr;
    CHECK(find_or_create(s, 2, 9, &none, 5) == 5 && none == nullptr);      // below capacity: a failing create...
    CHECK(g_live == live && g_destroyed == destroyed && s.cache.size() == 3);
    CHECK(find_or_create(s, 2, 2, &again) == 0 && again == h[2]);          // ...leaves the cache as it was
    CHECK(find_or_create(s, 2, 3, &h[3]) == 0 && s.cache.size() == 4);
    const size_t others = g_devices.of(0).cache.size() + g_devices.of(1).cache.size();
    CHECK(find_or_create(s, 2, 4, &h[4]) == 0);                            // a miss at capacity
    CHECK(g_destroyed == destroyed + 4 && s.cache.size() == 1);            // destroys exactly this device's four
    CHECK(g_devices.of(0).cache.size() + g_devices.of(1).cache.size() == others);
}

void clear_one_device()
{
    const int live = g_live;
    const size_t n1 = g_devices.of(1).cache.size();
    Fake *kept = nullptr, *again = nullptr;
    CHECK(find_or_create(g_devices.of(0), 0, 7, &kept) == 0);
    {
        State &s = g_devices.of(1);
        std::lock_guard<std::mutex> lk(s.mtx);
        s.cache.clear();
    }
    CHECK(g_live == live - (int)n1 && g_devices.of(1).cache.size() == 0);
    CHECK(find_or_create(g_devices.of(0), 0, 7, &again) == 0 && again == kept && kept->payload == 7);
}
}  // namespace

int main()
{
    two_devices();
    one_device();
    clear_one_device();
    for (int d = 0; d < 3; d++) g_devices.of(d).cache.clear();
    CHECK(g_live == 0);                                                    // nothing is live at exit
    CHECK(g_destroyed_in_use == 0);
    if (g_failures || g_destroyed_in_use) {
        std::fprintf(stderr, "plan_cache_main: %d check(s) failed, %d handle(s) destroyed in use\n", g_failures.load(),
                     g_destroyed_in_use.load());
        return 1;
    }
    std::puts("plan_cache_main: ok");
    return 0;
}
