// amvs_handles.h -- how the library owns streams and events: every one it creates is a Stream, an Event or a slot of
// an EventPool, destroyed with its owner.  hipStreamCreate* / hipStreamDestroy / hipEventCreate* / hipEventDestroy
// appear in the library only here.  (A stream the caller supplies -- amvs_set_stream -- stays a borrowed raw handle.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace amvs {

// One non-blocking stream, destroyed by the destructor.  create() replaces the stream held, if any.
class Stream {
public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept
    {
        if (this != &o) {
            reset();
            s_ = o.s_;
            o.s_ = nullptr;
        }
        return *this;
    }
    ~Stream() { reset(); }

    hipError_t create()
    {
        reset();
        return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    }
    hipError_t create(int priority)
    {
        reset();
        return hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, priority);
    }
    hipStream_t get() const { return s_; }      // nullptr until created
    void reset()
    {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }

private:
    hipStream_t s_ = nullptr;
};

// A pair of streams, each of the device's most (`urgent`) or least urgent priority -- distinct priorities land on distinct
// hardware queues -- created whole or not at all: a failure leaves `pair` as it was.
inline hipError_t create_stream_pair(Stream (&pair)[2], bool urgent0, bool urgent1)
{
    int lo = 0, hi = 0;                 // (numerically: hi <= lo)
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    Stream made[2];
    if (e == hipSuccess) e = made[0].create(urgent0 ? hi : lo);
    if (e == hipSuccess) e = made[1].create(urgent1 ? hi : lo);
    if (e != hipSuccess) return e;
    pair[0] = std::move(made[0]);
    pair[1] = std::move(made[1]);
    return hipSuccess;
}

// One event, with timing (hipEventElapsedTime) or without (ordering only), destroyed by the destructor.
class Event {
public:
    Event() = default;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) {
            reset();
            e_ = o.e_;
            o.e_ = nullptr;
        }
        return *this;
    }
    ~Event() { reset(); }

    hipError_t create(bool timing)
    {
        reset();
        return timing ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, hipEventDisableTiming);
    }
    hipEvent_t get() const { return e_; }       // nullptr until created
    void reset()
    {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }

private:
    hipEvent_t e_ = nullptr;
};

// Events of one kind that are only ever added to: reserve(n) creates the ones missing up to n, [i] is the i-th.
// An event already created keeps its handle for the life of the pool.
class EventPool {
public:
    explicit EventPool(bool timing) : timing_(timing) {}
    EventPool(const EventPool &) = delete;
    EventPool &operator=(const EventPool &) = delete;
    ~EventPool()
    {
        for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    }

    hipError_t reserve(size_t n)
    {
        while (ev_.size() < n) {
            hipEvent_t e;
            hipError_t err = timing_ ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (err != hipSuccess) return err;
            ev_.push_back(e);
        }
        return hipSuccess;
    }
    const hipEvent_t &operator[](size_t i) const { return ev_[i]; }

private:
    std::vector<hipEvent_t> ev_;
    bool timing_;
};

}  // namespace amvs
