// recc_devmem.hip.h -- who owns the handle's HIP objects: every hipMalloc / hipHostMalloc allocation, every event and every stream
// of the library belongs to one of the owners below and is released by it, and host-resident input reaches the device through one
// staging path (HostStage).  Plain structs: the growth policy, the sizes, the moment of creation and the order of destruction stay
// with the code that uses them.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

// a HIP call that must succeed: says which one failed and returns the library's error code for it
#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            std::fprintf(stderr, "amps_recc: %s failed: %s\n", #expr, hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? -ENOMEM : -EIO;                          \
        }                                                                               \
    } while (0)

namespace amps {

// The library's environment switches: a name and a test of its value (never null).  env_is reads a switch when its call site is
// first reached and keeps the answer for the life of the process; env_read reads it now.
typedef bool (*env_test_t)(const char *value);
inline bool env_one(const char *v) { return v[0] == '1'; }             // NAME=1
inline bool env_read(const char *name, env_test_t test) { const char *e = std::getenv(name); return e && test(e); }
#define env_is(name, test) ([] { static const bool v_ = amps::env_read(name, test); return v_; }())

// One device allocation of `capacity()` elements.  Move-only (the move constructor rules copies out); the destructor frees.
template <typename T> class DevBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); } return *this; }
    ~DevBuf() { reset(); }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    size_t capacity() const { return cap_; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    // a fresh allocation of n elements (n = 0: of one, so that a buffer that exists is never null); what was held is freed first
    int alloc(size_t n)
    {
        reset();
        if (n == 0) n = 1;
        if (hipMalloc((void **)&p_, n * sizeof(T)) != hipSuccess) { p_ = nullptr; return -ENOMEM; }
        cap_ = n;
        return 0;
    }
    // grow-only, exactly to n: contents are not kept, and a failure leaves the buffer empty
    int reserve(size_t n) { return n <= cap_ ? 0 : alloc(n); }
};

// One allocation of pinned host memory, mapped unless alloc is told otherwise: the kernels write through dev(), the host reads host()
// without a copy call (record lists, kept-burst lists, list headers).  With hipHostMallocDefault it is pinned only: dev() stays null.
template <typename T> class MappedBuf {
    T *host_ = nullptr, *dev_ = nullptr;
public:
    MappedBuf() = default;
    MappedBuf(MappedBuf &&o) noexcept : host_(std::exchange(o.host_, nullptr)), dev_(std::exchange(o.dev_, nullptr)) {}
    MappedBuf &operator=(MappedBuf &&o) noexcept { if (this != &o) { reset(); host_ = std::exchange(o.host_, nullptr); dev_ = std::exchange(o.dev_, nullptr); } return *this; }
    ~MappedBuf() { reset(); }
    T *host() const { return host_; }
    T *dev() const { return dev_; }
    explicit operator bool() const { return host_ != nullptr; }
    void reset() { if (host_) (void)hipHostFree(host_); host_ = nullptr; dev_ = nullptr; }
    int alloc(size_t n, unsigned flags = hipHostMallocMapped)
    {
        reset();
        if (hipHostMalloc((void **)&host_, n * sizeof(T), flags) != hipSuccess) { host_ = nullptr; return -ENOMEM; }
        if ((flags & hipHostMallocMapped) && hipHostGetDevicePointer((void **)&dev_, host_, 0) != hipSuccess) { reset(); return -ENOMEM; }
        return 0;
    }
};

// One event, created when its user says so: with hipEventDisableTiming for an ordering event, with no flags for a timing event.
class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); } return *this; }
    ~Event() { reset(); }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    int create(unsigned flags = hipEventDefault)
    {
        reset();
        if ((flags == hipEventDefault ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, flags)) != hipSuccess) { e_ = nullptr; return -ENOMEM; }
        return 0;
    }
};

// One stream: a non-blocking one of the library's own (create), destroyed with its owner, or the caller's (borrow), never destroyed.
class Stream {
    hipStream_t s_ = nullptr;
    bool own_ = false;
public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)), own_(std::exchange(o.own_, false)) {}
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s_ = std::exchange(o.s_, nullptr); own_ = std::exchange(o.own_, false); } return *this; }
    ~Stream() { reset(); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
    void reset() { if (own_ && s_) (void)hipStreamDestroy(s_); s_ = nullptr; own_ = false; }
    int create()
    {
        reset();
        if (hipStreamCreateWithFlags(&s_, hipStreamNonBlocking) != hipSuccess) { s_ = nullptr; return -EIO; }
        own_ = true;
        return 0;
    }
    void borrow(hipStream_t s) { reset(); s_ = s; }
};

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_constructible<MappedBuf<float>>::value &&
              !std::is_copy_constructible<Event>::value && !std::is_copy_constructible<Stream>::value, "an owner is moved, never copied");

// the guard inside a HostStage (below): an event, created by the first arm, behind the last kernel that reads the staging buffer
// (a fence that was moved from has no event and waits for nothing)
struct StageFence {
    Event ev;
    bool armed = false;
    int wait()
    {
        if (armed && ev) { if (hipEventSynchronize(ev.get()) != hipSuccess) return -EIO; armed = false; }
        return 0;
    }
    int arm(hipStream_t s)
    {
        if (!ev && ev.create(hipEventDisableTiming)) return -ENOMEM;
        if (hipEventRecord(ev.get(), s) != hipSuccess) return -EIO;
        armed = true;
        return 0;
    }
};

// The device staging buffer of one seam for host-resident input, and its guard.  Copies from pageable host memory are neither
// ordered after earlier kernels of a non-blocking stream nor guaranteed to have read their source when an Async call returns:
// back-to-back pushes without a drain in between corrupted samples in the staging buffer while the previous push's kernels
// were still reading it (found by scripts/fuzz_parity.py: intermittent wrong slicer bits), and blocks the caller freed right
// after the call were copied late.  A host push therefore goes through stage() -- wait until the previous push's kernels have
// released the buffer (before it is touched, freed to grow included), then copy SYNCHRONOUSLY, so the caller's block is free
// when the push returns and the kernels are enqueued behind a finished copy -- enqueues its kernels, and calls arm() behind the
// last one that reads the buffer.  An error return between the two arms nothing: nothing was enqueued that reads the buffer.
struct HostStage {
    DevBuf<uint8_t> buf;
    StageFence fence;
    // `rows` rows of `n` elements from the host block `src` (row pitch `ld` elements) into a buffer of at least `reserve`
    // elements, rows packed: *dev is the device copy and *dev_ld = n its pitch
    template <typename T> int stage(const T *src, size_t ld, size_t n, size_t rows, size_t reserve, const T **dev, uint64_t *dev_ld)
    {
        if (int rc = fence.wait()) return rc;
        if (int rc = buf.reserve(std::max(reserve, rows * n) * sizeof(T))) return rc;
        const hipError_t e = rows == 1 ? hipMemcpy(buf.get(), src, n * sizeof(T), hipMemcpyHostToDevice)
                                       : hipMemcpy2D(buf.get(), n * sizeof(T), src, ld * sizeof(T), n * sizeof(T), rows, hipMemcpyHostToDevice);
        if (e != hipSuccess) return -EIO;
        *dev = (const T *)buf.get();
        *dev_ld = n;
        return 0;
    }
    int arm(hipStream_t s) { return fence.arm(s); }
};

} // namespace amps
