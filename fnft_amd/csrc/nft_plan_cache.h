// nft_plan_cache.h -- what the host-pointer entry points keep between calls, without any HIP in it: a bounded cache of
// plan handles and a registry that gives every device a state object of its own.  hip_backend.hip puts a device's
// host-call lock, its caches and its peeler into one such object, so two devices never share a lock, a cache or an
// eviction; tests/host/plan_cache_main.cpp runs both templates on fake handles.
#pragma once
#include <cstddef>
#include <map>
#include <memory>
#include <mutex>

// Find-or-create cache of at most Cap handles.  Not locked: the owner's lock covers the lookup AND the use of the handle
// it returns, because a later miss may destroy that handle.
template <class Key, class H, void (*Destroy)(H *), size_t Cap = 4> class PlanCache {
public:
    PlanCache() = default;
    PlanCache(const PlanCache &) = delete;
    PlanCache &operator=(const PlanCache &) = delete;
    ~PlanCache() { clear(); }

    // *out = the handle of `key`, made by create(&handle) -> 0 or an error code on a miss.  A miss at capacity destroys
    // every cached handle first (the footprint stays bounded, and a create gets the memory they held); a create that
    // fails adds nothing and its code is returned.
    template <class Create> int get(const Key &key, H **out, Create create)
    {
        auto it = map.find(key);
        if (it == map.end()) {
            if (map.size() >= Cap) clear();
            H *h = nullptr;
            const int rc = create(&h);
            if (rc != 0) return rc;
            it = map.emplace(key, h).first;
        }
        *out = it->second;
        return 0;
    }
    void clear()
    {
        for (auto &kv : map) Destroy(kv.second);
        map.clear();
    }
    size_t size() const { return map.size(); }

private:
    std::map<Key, H *> map;
};

// One State per device, made on first use and never moved: of(device) returns a reference that stays valid for the
// registry's life.  The registry's own lock covers the lookup only; what a State needs it brings itself.
template <class State> class DeviceRegistry {
public:
    State &of(int device)
    {
        std::lock_guard<std::mutex> lk(mtx);
        std::unique_ptr<State> &slot = states[device];
        if (!slot) slot.reset(new State());
        return *slot;
    }

private:
    std::mutex mtx;
    std::map<int, std::unique_ptr<State>> states;
};
