// gm_dev_array.hpp -- the one owner of device and page-locked memory: DevArray<T>, its pinned sibling HostArray<T>, and
// Carve.  Host code only; needs nothing but the HIP runtime API (it is also compiled by plain g++, host/gm_dev_array_test.cpp).
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <atomic>

namespace gm {

// blocks the owners of this process hold right now, device and pinned (gm_debug_live_buffers: tests)
inline std::atomic<long long> g_live_buffers{0};

struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void *p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void *p) { return hipHostFree(p); }
};

// A grow-only array, freed with its owner (on the owner's device).  reserve frees before it allocates (the peak is the
// larger block, never both), does not preserve the contents and never shrinks; after a failure the array is empty.
// reserve(0) on an empty array leaves it empty (p == nullptr): a caller that promises non-null scratch asks for one element.
// Reads like a T * everywhere (kernel arguments, arithmetic, ->, tests for null); only reserve and release change it.
template <class T, class Mem>
struct OwnedArray {
    T *p = nullptr;
    uint64_t cap = 0;   // elements
    OwnedArray() = default;
    OwnedArray(OwnedArray &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }   // (a std::vector of owners grows)
    OwnedArray(const OwnedArray &) = delete;
    OwnedArray &operator=(const OwnedArray &) = delete;
    ~OwnedArray() { release(); }
    operator T *() const { return p; }
    T *operator->() const { return p; }
    // moved: counts the reallocations (also a failed one: the old block is gone).  A slot passes its alloc_gen, the word
    // that retires captured graphs; a reserve that keeps the block leaves the word alone.
    hipError_t reserve(uint64_t n, uint32_t *moved = nullptr)
    {
        if (cap >= n) return hipSuccess;
        release();
        if (moved) ++*moved;
        const hipError_t e = Mem::alloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = n;
        g_live_buffers.fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    void release()
    {
        if (p) {
            (void)Mem::free(p);
            g_live_buffers.fetch_sub(1, std::memory_order_relaxed);
        }
        p = nullptr;
        cap = 0;
    }
};
template <class T> using DevArray = OwnedArray<T, DeviceMem>;
template <class T> using HostArray = OwnedArray<T, PinnedMem>;

// Consecutive arrays inside one DevArray<uint8_t> block.  Every such block is laid out by the count of the call that
// uses it, not by the block's capacity: what a call touches is dense at the front, whatever larger call sized the block.
struct Carve {
    uint8_t *at;
    template <class T>
    T *take(uint64_t n)
    {
        T *r = reinterpret_cast<T *>(at);
        at += n * sizeof(T);
        return r;
    }
};

}  // namespace gm
