// ndtgpu_resource.h -- the four owning types of the C-ABI's handles (ndtgpu_host.h includes this): device buffer, pinned host
// buffer, fence (an event and whether it has been recorded) and stream.  Host side only, internal.  Each is move-only, releases
// what it holds in its destructor and ignores HIP errors there.
//
// ORDER OF MEMBERS.  Members are destroyed in reverse declaration order, and a Stream's destructor waits for its work: a handle
// declares its streams AFTER the buffers and fences that their work uses, so the streams go first.  That holds for the members
// that bundle buffers as well -- HostStage and LatticeTables (ndtgpu_host.h) own blocks that the handle's stream copies to and
// from, and no stream or fence: they stand in front of the handle's `used` and `hst`.  A *_destroy waits for the work on streams
// the handle does not own (the caller's), then deletes the handle (handle_destroy, ndtgpu_host.h).
//
// Objects with static storage keep raw HIP handles instead (g_coop_order in ndtgpu_matcher.hip): at process exit the runtime may
// be gone before their destructors would run.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

#pragma GCC visibility push(hidden)

// what ndtgpu_live_resources reports: bumped where the types below allocate or release, nowhere else
enum { LIVE_DEVICE, LIVE_PINNED, LIVE_EVENT, LIVE_STREAM };
inline std::atomic<uint64_t> g_live[4];
inline void live_add(int kind, int64_t d) { g_live[kind].fetch_add((uint64_t)d, std::memory_order_relaxed); }

class Fence;

// n elements of T in device (PINNED: page-locked host) memory
template <class T, bool PINNED>
class Buffer {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept
    {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~Buffer() { release(); }
    T *get() const { return p_; }
    size_t capacity() const { return n_; }
    void release()
    {
        if (!p_) return;
        if (PINNED) (void)hipHostFree(p_); else (void)hipFree(p_);
        live_add(PINNED ? LIVE_PINNED : LIVE_DEVICE, -1);
        p_ = nullptr;
        n_ = 0;
    }
    // a new block of n elements (what was held is released first); {nullptr, 0} after a failure
    hipError_t alloc(size_t n)
    {
        release();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p_, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p_, n * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = n;
        live_add(PINNED ? LIVE_PINNED : LIVE_DEVICE, 1);
        return hipSuccess;
    }
    // ... that also fills a kernel view's pointer
    hipError_t alloc(size_t n, T **view)
    {
        const hipError_t e = alloc(n);
        *view = p_;
        return e;
    }
    // Grow-only: room for n elements, contents NOT kept.  The block that is replaced may still be in use on the device: the caller
    // names what to wait for -- `last_use`, recorded behind the last launch that uses the block (the host waits for it only when
    // the block is replaced) -- or, with the one-argument form, has waited itself on the line before.
    hipError_t reserve(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }
    hipError_t reserve(size_t n, const Fence &last_use);
};
template <class T> using DeviceBuffer = Buffer<T, false>;
template <class T> using PinnedBuffer = Buffer<T, true>;

// An event "recorded behind the last launch that uses X" and whether it has been recorded: the next user of X waits for it on
// its stream (order), the host before it reads, frees or reuses X (sync).  Created on the first record (hipEventDisableTiming),
// or by create() where the handle's create function makes it (and for the timed events of the profiling hooks).
class Fence {
    hipEvent_t ev_ = nullptr;
    bool valid_ = false;
    unsigned flags_ = hipEventDisableTiming;   // the kind create() was asked for: a create that failed is repeated with it by record()

public:
    Fence() = default;
    Fence(Fence &&o) noexcept : ev_(o.ev_), valid_(o.valid_), flags_(o.flags_) { o.ev_ = nullptr; o.valid_ = false; }
    Fence &operator=(Fence &&o) noexcept
    {
        if (this != &o) { destroy(); ev_ = o.ev_; valid_ = o.valid_; flags_ = o.flags_; o.ev_ = nullptr; o.valid_ = false; }
        return *this;
    }
    ~Fence() { destroy(); }
    hipEvent_t get() const { return ev_; }
    bool valid() const { return valid_; }
    void clear() { valid_ = false; }
    hipError_t create(unsigned flags = hipEventDisableTiming)
    {
        if (ev_) return hipSuccess;
        flags_ = flags;
        const hipError_t e = flags == hipEventDefault ? hipEventCreate(&ev_) : hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) { ev_ = nullptr; return e; }
        live_add(LIVE_EVENT, 1);
        return hipSuccess;
    }
    hipError_t record(hipStream_t st)
    {
        hipError_t e = create(flags_);          // (no-op once the event exists; a timed event stays a timed event)
        if (e == hipSuccess) e = hipEventRecord(ev_, st);
        if (e == hipSuccess) valid_ = true;
        return e;
    }
    hipError_t order(hipStream_t st) const { return valid_ ? hipStreamWaitEvent(st, ev_, 0) : hipSuccess; }
    hipError_t sync() const { return valid_ ? hipEventSynchronize(ev_) : hipSuccess; }

private:
    void destroy()
    {
        if (!ev_) return;
        (void)hipEventDestroy(ev_);
        live_add(LIVE_EVENT, -1);
        ev_ = nullptr;
        valid_ = false;
    }
};

template <class T, bool PINNED>
hipError_t Buffer<T, PINNED>::reserve(size_t n, const Fence &last_use)
{
    if (n <= n_) return hipSuccess;
    const hipError_t e = last_use.sync();
    return e != hipSuccess ? e : alloc(n);
}

// A stream the library created: one create function per form in use.  The destructor waits for the stream's work, then destroys it.
class Stream {
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept
    {
        if (this != &o) { destroy(); s_ = o.s_; o.s_ = nullptr; }
        return *this;
    }
    ~Stream() { destroy(); }
    hipStream_t get() const { return s_; }
    hipError_t create(unsigned flags) { return made(hipStreamCreateWithFlags(&s_, flags)); }
    hipError_t create(unsigned flags, int priority) { return made(hipStreamCreateWithPriority(&s_, flags, priority)); }
    hipError_t create_cu_mask(uint32_t n_words, const uint32_t *mask) { return made(hipExtStreamCreateWithCUMask(&s_, n_words, mask)); }

private:
    hipError_t made(hipError_t e)
    {
        if (e != hipSuccess) s_ = nullptr; else live_add(LIVE_STREAM, 1);
        return e;
    }
    void destroy()
    {
        if (!s_) return;
        (void)hipStreamSynchronize(s_);
        (void)hipStreamDestroy(s_);
        live_add(LIVE_STREAM, -1);
        s_ = nullptr;
    }
};

#pragma GCC visibility pop
