// dev_owner.hpp -- the one owner of a context's device memory (host code only).  vaeb_ctx,
// vaeb_ae and vaeb_clf (through their StackCore) and h16c::BfState each hold a DevOwner; every buffer is registered where it is
// allocated and release_all frees the list, so no second list has to be kept in step with the
// allocations.  Interior pointers (a second array inside one block) are never registered.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

namespace vaeb {

struct DevOwner {
    std::vector<void*> owned;

    // n (at least one) zeroed elements, owned from here on.
    template <class T>
    int alloc(T** p, int64_t n) {
        return take(reinterpret_cast<void**>(p), sizeof(T) * (size_t)std::max<int64_t>(n, 1));
    }
    // A buffer that exists from its first use on.
    template <class T>
    int lazy(T** p, int64_t n) { return *p ? 0 : alloc(p, n); }
    // Frees *p (when this owner holds it) and leaves it null.
    template <class T>
    void drop(T** p) {
        auto it = std::find(owned.begin(), owned.end(), (void*)*p);
        if (it != owned.end()) {
            hipFree(*p);
            owned.erase(it);
        }
        *p = nullptr;
    }
    // Replaces *p by a fresh buffer of n elements (contents are not kept).
    template <class T>
    int replace(T** p, int64_t n) {
        drop(p);
        return alloc(p, n);
    }
    // A grow-only buffer: at least n elements.
    template <class T>
    int grow(T** p, int64_t* cap, int64_t n) {
        if (n <= *cap) return 0;
        *cap = 0;
        if (int rc = replace(p, n)) return rc;
        *cap = n;
        return 0;
    }
    void release_all() {
        for (void* p : owned) hipFree(p);
        owned.clear();
    }

private:
    int take(void** p, size_t bytes);   // vaeb_hip.hip: dalloc, then the registration
};

// A call's local scratch: freed on every return.
struct DevScratch : DevOwner {
    DevScratch() = default;
    DevScratch(const DevScratch&) = delete;
    DevScratch& operator=(const DevScratch&) = delete;
    ~DevScratch() { release_all(); }
};

}  // namespace vaeb
