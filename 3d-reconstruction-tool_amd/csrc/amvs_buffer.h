// amvs_buffer.h -- how the library owns device memory: every allocation is a DeviceBuffer (one block, grown only)
// or a lease from the ScratchCache of its context.  hipMalloc / hipFree appear in the library only here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <map>
#include <vector>

// In a function that runs on the stream `st` and returns hipError_t: return the error of `call`, after `st` has
// drained -- the scratch leases of the function go back to the cache with nothing in flight (Ordering, below).
#define STCHK(call)                                                 \
    do {                                                            \
        hipError_t e_ = (call);                                     \
        if (e_ != hipSuccess) { (void)hipStreamSynchronize(st); return e_; } \
    } while (0)

namespace amvs {

// A context's cache of device blocks for the post-steps' SHORT-LIVED buffers (the neighbour statistic of the stereo
// outlier filter, the scratch arrays of fusion / filter / voxel grid): hipMalloc + hipFree cost 0.1-0.2 ms a pair and
// a post-step takes a dozen pairs per call (measured, round 4: 2.7 of the 12.6 ms of amvs_knn_mean_distance on a
// 500 000-point cloud).  A lease is served from a block given back earlier when one of at most 2 x size + 4 KiB is
// cached; a lease that ends keeps its block here (at most 4 GiB per context); the context's destruction frees them.
//
// Ordering: a block can be leased again while work that used it is still queued.  That is safe because the cache is
// used only on its context's stream (in order), and every entry point that uses it synchronises that stream before it
// returns -- so no cached block is in use when the next call starts, on that stream or on another one
// (amvs_set_stream between calls).  There is no lock: a context is driven by one thread at a time.
class ScratchCache {
public:
    // a block of the cache, given back when the lease ends
    class Lease {
    public:
        Lease() = default;
        Lease(const Lease &) = delete;
        Lease &operator=(const Lease &) = delete;
        ~Lease() { reset(); }
        template <class T = void> T *get() const { return static_cast<T *>(p_); }
        void reset()
        {
            if (p_) owner_->give_back(p_, size_);
            p_ = nullptr; size_ = 0;
        }

    private:
        friend class ScratchCache;
        ScratchCache *owner_ = nullptr;
        void *p_ = nullptr;
        size_t size_ = 0;
    };

    ScratchCache() = default;
    ScratchCache(const ScratchCache &) = delete;
    ScratchCache &operator=(const ScratchCache &) = delete;
    ~ScratchCache() { clear(); }

    // Every device allocation of a context (the buffers too: DeviceBuffer::reserve): on out-of-memory the cache is
    // emptied to make room and the allocation tried once more.
    hipError_t allocate(void **p, size_t bytes)
    {
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipErrorOutOfMemory) return e;
        (void)hipGetLastError();
        clear();
        return hipMalloc(p, bytes);
    }

    // A block of at least `bytes` into `l`.  The block `l` holds already is kept when it is large enough, else it
    // goes back first (a scratch array grown for the largest of a run of requests).
    hipError_t lease(Lease &l, size_t bytes)
    {
        if (l.p_ && l.size_ >= bytes) return hipSuccess;
        l.reset();
        const size_t size = (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
        auto it = free_.lower_bound(size);
        if (it != free_.end() && it->first <= 2 * size + 4096) {
            l.p_ = it->second.back();
            l.size_ = it->first;
            it->second.pop_back();
            cached_ -= it->first;
            if (it->second.empty()) free_.erase(it);
        } else {
            void *p = nullptr;
            hipError_t e = allocate(&p, size);
            if (e != hipSuccess) return e;
            l.p_ = p;
            l.size_ = size;
        }
        l.owner_ = this;
        return hipSuccess;
    }

    // every cached block back to the driver
    void clear()
    {
        for (auto &kv : free_)
            for (void *p : kv.second) (void)hipFree(p);
        free_.clear();
        cached_ = 0;
    }

private:
    static constexpr size_t MAX_CACHED = size_t(4) << 30;   // beyond this, blocks go back to the driver

    void give_back(void *p, size_t size)
    {
        if (cached_ + size > MAX_CACHED) { (void)hipFree(p); return; }
        free_[size].push_back(p);
        cached_ += size;
    }

    std::map<size_t, std::vector<void *>> free_;   // size -> cached blocks
    size_t cached_ = 0;
};

// One device allocation of `capacity()` elements, freed by the destructor or release().  reserve() only grows and
// discards the contents: nothing happens when the capacity is already at least n, else the block is freed first and
// then the new one allocated (the cache is emptied to make room on out-of-memory: ScratchCache::allocate).
template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { release(); }

    hipError_t reserve(size_t n, ScratchCache &cache)
    {
        if (n <= n_) return hipSuccess;
        release();
        void *p = nullptr;
        hipError_t e = cache.allocate(&p, sizeof(T) * n);
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p);
        n_ = n;
        return hipSuccess;
    }
    T *get() const { return p_; }
    size_t capacity() const { return n_; }
    void release()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace amvs
