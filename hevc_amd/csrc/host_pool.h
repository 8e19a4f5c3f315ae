// hevc_amd/csrc/host_pool.h — what a process shares between its sessions (worker threads, cached allocations, cached streams) and the move-only
// handles a session holds them by: a handle gives its resource back when it goes out of scope, with the size it was taken with.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace mihevc {

// Host worker pool for the CABAC jobs.  ONE pool per process, shared by every session and grown to the largest size a session asks for: a batch
// codes many clips back to back, and starting / joining 16 threads per clip was 2 ms of every 80 ms 1080p clip (bench step_phases open + close).
// The threads live until the process exits (they are parked on a condition variable); a session waits for ITS jobs, never for the threads.
class ThreadPool {
public:
    static ThreadPool &shared(int n)
    {
        static ThreadPool *p = new ThreadPool();      // never destroyed: no join at process exit, the threads hold no session state
        p->grow(n);
        return *p;
    }
    void submit(std::function<void()> f)
    {
        {
            std::lock_guard<std::mutex> l(m_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }

private:
    void grow(int n)
    {
        std::lock_guard<std::mutex> l(m_);
        while ((int)threads_.size() < n) { threads_.emplace_back([this] { run(); }); threads_.back().detach(); }
    }
    void run()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [this] { return !q_.empty(); });
                f = std::move(q_.front());
                q_.pop_front();
            }
            f();
        }
    }
    std::vector<std::thread> threads_;
    std::deque<std::function<void()>> q_;
    std::mutex m_;
    std::condition_variable cv_;
};

// Process-wide cache of device / pinned-host allocations keyed by (device, size): a batch transcodes many clips of
// the same geometry back to back (gui/mainwindow.py queue), and hipMalloc/hipHostMalloc/hipFree cost tens of ms
// per session otherwise (bench step_phases: close 51 ms).  Buffers return to the cache when their CachedBlock lets go.
class BufferCache {
public:
    static BufferCache &get() { static BufferCache c; return c; }
    hipError_t alloc(int dev, size_t n, bool pinned, void **out)
    {
        {
            std::lock_guard<std::mutex> l(m_);
            auto &v = free_[key(dev, n, pinned)];
            if (!v.empty()) { *out = v.back(); v.pop_back(); bytes_ -= n; return hipSuccess; }
        }
        return pinned ? hipHostMalloc(out, n, hipHostMallocDefault) : hipMalloc(out, n);
    }
    void release(int dev, size_t n, bool pinned, void *p)
    {
        if (!p) return;
        std::lock_guard<std::mutex> l(m_);
        if (bytes_ + n > kMaxBytes) { if (pinned) (void)hipHostFree(p); else (void)hipFree(p); return; }
        bytes_ += n;
        free_[key(dev, n, pinned)].push_back(p);
    }
private:
    static constexpr size_t kMaxBytes = (size_t)24 << 30;      // 24 GiB of 288: plenty for a few clip geometries
    static std::string key(int dev, size_t n, bool pinned) { return std::to_string(dev) + (pinned ? "h" : "d") + std::to_string(n); }
    std::mutex m_;
    std::map<std::string, std::vector<void *>> free_;
    size_t bytes_ = 0;
};

// the same for the sessions' two streams (create + destroy: about a millisecond per session)
class StreamCache {
public:
    static StreamCache &get() { static StreamCache c; return c; }
    hipError_t acquire(int dev, hipStream_t *out)
    {
        {
            std::lock_guard<std::mutex> l(m_);
            auto &v = free_[dev];
            if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
        }
        return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    }
    void release(int dev, hipStream_t st)
    {
        if (!st) return;
        std::lock_guard<std::mutex> l(m_);
        auto &v = free_[dev];
        if (v.size() >= 16) { (void)hipStreamDestroy(st); return; }
        v.push_back(st);
    }
private:
    std::mutex m_;
    std::map<int, std::vector<hipStream_t>> free_;
};

// One block from BufferCache, of T.  Empty by default; reads as its pointer.  The bytes it goes back under are the bytes it was taken with.
template <typename T> class CachedBlock {
public:
    CachedBlock() = default;
    CachedBlock(CachedBlock &&o) noexcept { swap(o); }
    CachedBlock &operator=(CachedBlock &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~CachedBlock() { reset(); }
    hipError_t alloc(int dev, size_t bytes, bool pinned)
    {
        reset();
        void *p = nullptr;
        if (hipError_t e = BufferCache::get().alloc(dev, bytes, pinned, &p)) return e;
        p_ = (T *)p; dev_ = dev; bytes_ = bytes; pinned_ = pinned;
        return hipSuccess;
    }
    void reset() { BufferCache::get().release(dev_, bytes_, pinned_, p_); p_ = nullptr; bytes_ = 0; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t bytes() const { return bytes_; }
private:
    void swap(CachedBlock &o) { std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(bytes_, o.bytes_); std::swap(pinned_, o.pinned_); }
    T *p_ = nullptr;
    int dev_ = 0;
    size_t bytes_ = 0;
    bool pinned_ = false;
};

// A stream from StreamCache.  It goes back as it is: whoever lets go of it has made it idle first.
class CachedStream {
public:
    CachedStream() = default;
    CachedStream(CachedStream &&o) noexcept : st_(std::exchange(o.st_, nullptr)), dev_(o.dev_) {}
    CachedStream &operator=(CachedStream &&o) noexcept { std::swap(st_, o.st_); std::swap(dev_, o.dev_); return *this; }
    ~CachedStream() { StreamCache::get().release(dev_, st_); }
    hipError_t acquire(int dev) { dev_ = dev; return StreamCache::get().acquire(dev, &st_); }
    operator hipStream_t() const { return st_; }
private:
    hipStream_t st_ = nullptr;
    int dev_ = 0;
};

// An event of the current device, created with `flags`; empty by default, and when creating it failed.
class Event {
public:
    Event() = default;
    explicit Event(unsigned flags) { if (hipEventCreateWithFlags(&ev_, flags) != hipSuccess) ev_ = nullptr; }
    Event(Event &&o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    Event &operator=(Event &&o) noexcept { std::swap(ev_, o.ev_); return *this; }
    ~Event() { if (ev_) (void)hipEventDestroy(ev_); }
    operator hipEvent_t() const { return ev_; }
private:
    hipEvent_t ev_ = nullptr;
};

// Two pinned blocks taken in turn: the host side of a device block that is rewritten by copies on one stream.  A block is written again only behind the event
// of the copy that read it, two sets back
struct PinnedPair {
    CachedBlock<uint8_t> host[2];
    Event ev[2];
    int64_t sets = 0;
    // the block of this turn, `bytes` long (one of another size is replaced), once the copy that last read it is through
    hipError_t acquire(int dev, size_t bytes, uint8_t *&block)
    {
        const int k = (int)(sets & 1);
        if (ev[k]) { if (hipError_t e = hipEventSynchronize(ev[k])) return e; }
        else if (!(ev[k] = Event(hipEventDisableTiming))) return hipErrorOutOfMemory;
        if (host[k].bytes() != bytes) if (hipError_t e = host[k].alloc(dev, bytes, true)) return e;
        block = host[k].get();
        return hipSuccess;
    }
    // the first `bytes` of that block go to dst on `st`, the event behind the copy; the turn passes to the other block
    hipError_t commit(void *dst, size_t bytes, hipStream_t st)
    {
        const int k = (int)(sets++ & 1);
        if (hipError_t e = hipMemcpyAsync(dst, host[k], bytes, hipMemcpyHostToDevice, st)) return e;
        return hipEventRecord(ev[k], st);
    }
};

}  // namespace mihevc
