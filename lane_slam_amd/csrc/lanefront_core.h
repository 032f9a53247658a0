// What the six opaque handles of the C ABI (lf_handle, lf_map, lf_lane_filter, lf_odometry, lf_motion, lf_places) share on the host:
// the fields every one of them carries, the error text, the HIP check, and one life cycle -- a creator's error buffer and its
// check (CreateError, LF_CREATE_TRY), the device, stream and events of a handle (open_core, close_core), the bodies of
// *_synchronize, *_set_profiling and *_get_timing (core_*) -- then the three classes of stream, the two kinds of clock, the
// scratch grower, the staging of a caller's host arrays and the ordering of a handle's stream against an lf_handle's
// (after_handle, release_handle).  A new handle type derives from Core and writes only what is its own.
// Host code only; common.h does not include it (tests/hostsim builds lsd_grow.h on the CPU).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include <mutex>
#include <vector>
#include "common.h"

namespace lf {

// every handle type derives from it
struct Core {
    int device = 0;
    hipStream_t stream = nullptr;
    char err[512] = "";
    int err_code = 0;
    bool profiling = false;
};

inline void vset_error(Core* c, int code, const char* fmt, va_list ap)
{
    if (!c) return;
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    c->err_code = code;
}

__attribute__((format(printf, 3, 4))) inline void set_error(Core* c, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vset_error(c, code, fmt, ap);
    va_end(ap);
}

#define LF_HIP_CHECK(core, expr)                                                                                             \
    do {                                                                                                                     \
        hipError_t _e = (expr);                                                                                              \
        if (_e != hipSuccess) {                                                                                              \
            lf::set_error((core), LF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);    \
            return LF_ERR_HIP;                                                                                               \
        }                                                                                                                    \
    } while (0)

// Why a handle type's last creator failed: what its *_last_error(NULL) returns.  One object per type, so that a failing creator
// of one type leaves the text of every other type alone.
struct CreateError {
    char text[512] = "no error";

    // a refused argument: the text, and LF_ERR_BAD_ARG
    __attribute__((format(printf, 2, 3))) int refuse(const char* fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return LF_ERR_BAD_ARG;
    }

    // a creator's check of device_id: LF_OK, or the message with the creator's name in front
    int check_device(int device_id, const char* who)
    {
        int ndev = 0;
        const hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0) {
            snprintf(text, sizeof(text), "%s: no HIP device (%s); lanefront has no CPU fallback", who, e != hipSuccess ? hipGetErrorString(e) : "device count 0");
            return LF_ERR_HIP;
        }
        return device_id < 0 || device_id >= ndev ? refuse("%s: device %d out of range (%d devices)", who, device_id, ndev) : LF_OK;
    }

    // a half-made handle failed with rc: its text is kept, the handle destroyed
    template <typename Handle>
    int fail(Handle* h, int rc, void (*destroy)(Handle*))
    {
        snprintf(text, sizeof(text), "%s", h->err);
        destroy(h);
        return rc;
    }
};

// a creator's HIP call: `fail` is its `[&](int rc) { return <the type's CreateError>.fail(handle, rc, <the type's destroyer>); }`
#define LF_CREATE_TRY(core, fail, expr)                                                                                      \
    do {                                                                                                                     \
        hipError_t _e = (expr);                                                                                              \
        if (_e != hipSuccess) {                                                                                              \
            lf::set_error((core), LF_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));                                \
            return fail(LF_ERR_HIP);                                                                                         \
        }                                                                                                                    \
    } while (0)

// (the configurations' doubles: neither infinite nor NaN)
inline bool is_finite(double x) { return x - x == 0; }

// The three classes of stream the library makes.  The runtime gives every stream one of the process's hardware queues (GPU_MAX_HW_QUEUES
// of them for the normal priority, four by default; another priority has queues of its own), a new stream the queue with the fewest
// streams, and streams that share a queue serialise.
//   CHAIN  lf_map's: one stream, the serial chain of a pipelined front end (lf_map_create) -- the greatest priority where the device
//          has a range, and with it a queue of its own.
//   BATCH  lf_handle's: many streams, each a pipeline of independent batches, at the normal priority.  What matters is that they are
//          dealt EVENLY: eight handles on four queues that already carry the default stream land 3 / 2 / 2 / 1, and the queue with three
//          sets the cycle of all.  So the first BATCH stream of a device is preceded by idle streams that fill the level the default
//          stream has begun (pad_normal_streams); from there on the handles are dealt 2 / 2 / 2 / 2, eighteen of them 5 / 5 / 4 / 4.
//          (The least priority would give the handles a pool of their own without any padding, and does: it was measured 10 % slower
//          than the uneven placement)
//   PLAIN  lf_lane_filter's, lf_odometry's, lf_motion's and lf_places': one stream of short side work at the normal priority, made
//          as it comes, without the padding: it takes the queue with the fewest streams at that moment.  (As BATCH streams they
//          would take part in the deal of the handles and shift it.)
enum class StreamClass { BATCH, CHAIN, PLAIN };

// Idle streams, made once per device and kept for the life of the process, that make the normal-priority streams which are no
// handle's -- the default stream and these -- a multiple of the hardware queue count.  GPU_MAX_HW_QUEUES is read, never set; with
// more than eight queues nothing is made (a handful of handles rarely share a queue there, and the idle streams would be many).  An
// application with normal-priority streams of its own that are not a multiple of the queue count shifts the deal by as many.
inline hipError_t pad_normal_streams()
{
    static std::mutex mu;
    static bool padded[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= 64) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (padded[dev]) return hipSuccess;
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    const int queues = q && *q ? atoi(q) : 4;
    for (int i = 1; i < queues && queues <= 8; ++i) {          // (the default stream is the first of the level)
        hipStream_t idle = nullptr;
        if ((e = hipStreamCreateWithFlags(&idle, hipStreamNonBlocking)) != hipSuccess) return e;
    }
    padded[dev] = true;
    return hipSuccess;
}

// a stream of the class on the current device
inline hipError_t create_stream(hipStream_t* s, StreamClass cls)
{
    int least = 0, greatest = 0;
    if (cls == StreamClass::CHAIN && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
        return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
    if (cls == StreamClass::BATCH) { const hipError_t e = pad_normal_streams(); if (e != hipSuccess) return e; }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

// the priority of the core's stream and the device's range (least == greatest: the device has one); any of them may be null
inline int stream_priority(Core* c, int* priority, int* least, int* greatest)
{
    int p = 0, lo = 0, hi = 0;
    LF_HIP_CHECK(c, hipSetDevice(c->device));
    LF_HIP_CHECK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    LF_HIP_CHECK(c, hipStreamGetPriority(c->stream, &p));
    if (priority) *priority = p;
    if (least) *least = lo;
    if (greatest) *greatest = hi;
    return LF_OK;
}

// A creator's first step, c->err set where it fails: the device, the core's stream of the class, and the events named, each made
// without timing.  (lf_create orders its own: it validates the configuration between the device and the stream.)
inline int open_core(Core* c, int device, StreamClass cls, std::initializer_list<hipEvent_t*> events)
{
    auto fail = [](int rc) { return rc; };
    c->device = device;
    LF_CREATE_TRY(c, fail, hipSetDevice(device));
    LF_CREATE_TRY(c, fail, create_stream(&c->stream, cls));
    for (hipEvent_t* ev : events) LF_CREATE_TRY(c, fail, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return LF_OK;
}

// A destroyer's: waits for the core's stream, then destroys the events named (null: never made) and the stream.  The owner deletes
// its handle afterwards; the buffers free themselves.
inline void close_core(Core* c, std::initializer_list<hipEvent_t> events)
{
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : events) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

// the bodies of *_synchronize and *_set_profiling behind their null checks (*_get_timing's: core_take_timing, below the clocks)
inline int core_synchronize(Core* c)
{
    LF_HIP_CHECK(c, hipSetDevice(c->device));
    LF_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return LF_OK;
}

inline int core_set_profiling(Core* c, int on)
{
    c->profiling = on != 0;
    return LF_OK;
}

// a scratch buffer of at least `bytes`; what it held is lost (kernels queued on the core's stream may still use it: they are
// waited for first)
template <typename T>
inline int scratch(Core* c, DevArray<T>& b, size_t bytes)
{
    if (b.bytes >= bytes) return LF_OK;
    if (b.p) { LF_HIP_CHECK(c, hipStreamSynchronize(c->stream)); b.reset(); }
    LF_HIP_CHECK(c, b.alloc(bytes + bytes / 4 + 256));
    return LF_OK;
}

// One entry of a fetch: `bytes` at the device address `src` to the host address `dst`.
struct Fetch { void* dst; const void* src; size_t bytes; };

// Results to the host: one copy per entry on the core's stream, then ONE wait for the stream.  Skipped: an entry with a null
// destination, a null source or no bytes (an array the caller did not ask for, or the call did not make), and one whose source is
// its destination -- a device caller's own array, as Staging::out named it.  A fetch that has nothing to copy does not wait
// either: the device form of a call returns with its work queued.
inline int fetch(Core* c, std::initializer_list<Fetch> list)
{
    bool queued = false;
    for (const Fetch& f : list) {
        if (!f.dst || !f.src || !f.bytes || f.dst == f.src) continue;
        LF_HIP_CHECK(c, hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyDeviceToHost, c->stream));
        queued = true;
    }
    if (queued) LF_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return LF_OK;
}

// The arrays of one call that its caller holds on the host or on the device (the entry point's on_device flags).  An array on the
// device is the caller's own, and nothing is queued for it.  For one on the host in() and out() name a scratch buffer of the
// handle and grow it, and upload() then queues the copies of the inputs: every growth of a call comes before its first copy
// (scratch() may wait for the stream and free, and where one fails nothing has been queued).  fetch() brings the outputs back.
struct Staging {
    explicit Staging(Core* c) : c_(c) {}

    // the device address of an input of `bytes`; its scratch buffer holds at least `room` bytes, so that an empty input has an
    // address all the same
    template <typename T, typename B>
    const T* in(int on_device, const T* src, size_t bytes, DevArray<B>& buf, size_t room = 0)
    {
        if (on_device) return src;
        grow(buf, bytes > room ? bytes : room);
        if (bytes) up_.push_back({ buf.p, src, bytes });
        return static_cast<const T*>(static_cast<const void*>(buf.p));
    }

    // (an input named through a pointer to non-const, such as a field of lf_segments)
    template <typename T, typename B>
    T* in(int on_device, T* src, size_t bytes, DevArray<B>& buf, size_t room = 0)
    {
        return const_cast<T*>(in(on_device, static_cast<const T*>(src), bytes, buf, room));
    }

    // the device address of an output of `bytes`
    template <typename T, typename B>
    T* out(int on_device, T* dst, size_t bytes, DevArray<B>& buf)
    {
        if (on_device) return dst;
        grow(buf, bytes);
        return static_cast<T*>(static_cast<void*>(buf.p));
    }

    // the first failed growth, or the inputs named so far on their way
    int upload()
    {
        if (rc_ != LF_OK) return rc_;
        for (const Up& u : up_) LF_HIP_CHECK(c_, hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, c_->stream));
        up_.clear();
        return LF_OK;
    }

private:
    struct Up { void* dst; const void* src; size_t bytes; };
    Core* c_;
    std::vector<Up> up_;
    int rc_ = LF_OK;

    template <typename B>
    void grow(DevArray<B>& buf, size_t bytes) { if (rc_ == LF_OK) rc_ = scratch(c_, buf, bytes); }
};

// stream `waits` waits for everything queued so far on stream `on`; ev is an event of the core's, kept for this
inline int stream_after(Core* c, hipEvent_t ev, hipStream_t waits, hipStream_t on)
{
    LF_HIP_CHECK(c, hipEventRecord(ev, on));
    LF_HIP_CHECK(c, hipStreamWaitEvent(waits, ev, 0));
    return LF_OK;
}

// The order of a core's stream against the stream of the lf_handle whose batch it reads (h null: nothing to order).  `who` is
// what stands before "bad handle" in the error text: the entry point and ": ", or "".
inline int order_with_handle(Core* c, hipEvent_t ev, lf_handle* h, const char* who, bool core_waits)
{
    if (!h) return LF_OK;
    void* s = nullptr;
    if (lf_get_stream(h, &s) != LF_OK) { set_error(c, LF_ERR_BAD_ARG, "%sbad handle", who); return LF_ERR_BAD_ARG; }
    const hipStream_t hs = static_cast<hipStream_t>(s);
    return core_waits ? stream_after(c, ev, c->stream, hs) : stream_after(c, ev, hs, c->stream);
}

// the core's stream waits for everything queued so far on the handle's stream
inline int after_handle(Core* c, hipEvent_t ev, lf_handle* h, const char* who) { return order_with_handle(c, ev, h, who, true); }
// the handle's later work (its next batch overwrites the segment arrays) waits for what the core has queued so far
inline int release_handle(Core* c, hipEvent_t ev, lf_handle* h, const char* who) { return order_with_handle(c, ev, h, who, false); }

// What a handle remembers of the batch it queued last (lf_process_batch_async): the caller's device block, the frames, and a serial
// number no other batch of any handle has.  The live map compares it with its snapshot of a batch's arrays (lanefront_map.hip).
struct LastBatch {
    lf_segments out{};
    int n_frames = 0;
    unsigned long long serial = 0;           // 0: no batch yet
};
LastBatch last_batch_of(const lf_handle* h);     // lanefront_api.hip; h null: none

// Per-stage time accumulated over many calls, with HIP events recorded on the core's stream.  Events are only recorded inside
// the pipeline (no host synchronisation); resolve() turns them into milliseconds.  A launch is counted whether or not the core
// is profiling.  At most `cap` records stay outstanding: then a clock either resolves them on the spot (resolve_when_full) or
// leaves the bracket at hand untimed.
struct StageClock {
    struct Rec { hipEvent_t a, b; int st; };
    std::vector<double> ms;
    std::vector<int32_t> launches;

    StageClock(int n_stages, size_t cap, bool resolve_when_full) : ms(n_stages, 0.0), launches(n_stages, 0), cap_(cap), resolve_when_full_(resolve_when_full) {}
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock()
    {
        for (std::vector<Rec>* v : { &used_, &free_ })
            for (Rec& r : *v) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    }

    // event pairs made ahead, not inside the first profiled calls
    void prefill(size_t n)
    {
        Rec r;
        while (free_.size() < n && make(&r)) free_.push_back(r);
    }

    // the events recorded so far become milliseconds of their stages (waits for them)
    void resolve()
    {
        for (Rec& r : used_) {
            (void)hipEventSynchronize(r.b);
            float t = 0;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) ms[r.st] += t;
            free_.push_back(r);
        }
        used_.clear();
    }

    // read and reset the stages [first, first + count) (count < 0: all from first): the first n of them go to ms_out and
    // launches_out, either of which may be null
    void take(double* ms_out, int32_t* launches_out, int n, int first = 0, int count = -1)
    {
        resolve();
        const int end = count < 0 ? (int)ms.size() : first + count;
        for (int i = first; i < end; ++i) {
            if (i - first < n && ms_out) ms_out[i - first] = ms[i];
            if (i - first < n && launches_out) launches_out[i - first] = launches[i];
            ms[i] = 0; launches[i] = 0;
        }
    }

    // brackets what is queued on the core's stream within its lifetime as one launch of stage st
    struct Scope {
        Core* c; StageClock* k; int st; Rec r; bool on;
        Scope(Core* c_, StageClock& k_, int st_) : c(c_), k(&k_), st(st_), on(c_->profiling && k_.acquire(&r))
        {
            if (on) { r.st = st; (void)hipEventRecord(r.a, c->stream); }
        }
        Scope(const Scope&) = delete;
        Scope& operator=(const Scope&) = delete;
        ~Scope()
        {
            if (on) { (void)hipEventRecord(r.b, c->stream); k->used_.push_back(r); }
            k->launches[st] += 1;
        }
    };

private:
    std::vector<Rec> free_, used_;
    size_t cap_;
    bool resolve_when_full_;

    static bool make(Rec* r)
    {
        r->st = 0;
        if (hipEventCreate(&r->a) != hipSuccess) return false;
        if (hipEventCreate(&r->b) != hipSuccess) { (void)hipEventDestroy(r->a); return false; }
        return true;
    }
    bool acquire(Rec* r)
    {
        if (free_.empty()) {
            if (used_.size() >= cap_) {
                if (!resolve_when_full_) return false;
                resolve();
            } else {
                Rec n;
                if (!make(&n)) return false;
                free_.push_back(n);
            }
        }
        *r = free_.back(); free_.pop_back();
        return true;
    }
};

// the body of *_get_timing behind its null check: every stage of the clock read and reset, the first n of them given out
inline int core_take_timing(Core* c, StageClock& clock, double* ms, int32_t* launches, int n)
{
    LF_HIP_CHECK(c, hipSetDevice(c->device));
    clock.take(ms, launches, n);
    return LF_OK;
}

// The per-stage times of the LAST call of one entry point: a pair of events per stage, made by the first profiled call and
// reused by the later ones.
struct CallClock {
    bool timed = false;                 // the last call ran with profiling on

    explicit CallClock(int n_stages) : ev_(2 * n_stages, nullptr) {}
    CallClock(const CallClock&) = delete;
    CallClock& operator=(const CallClock&) = delete;
    ~CallClock()
    {
        for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e);
    }

    // a call starts: it is timed when its core is profiling
    int begin(Core* c)
    {
        timed = false;
        stream_ = c->stream;
        if (c->profiling) for (hipEvent_t& e : ev_) if (!e) LF_HIP_CHECK(c, hipEventCreate(&e));
        timed = c->profiling;
        return LF_OK;
    }

    struct Scope {
        CallClock* k; int st;
        Scope(CallClock& k_, int st_) : k(&k_), st(st_) { if (k->timed) (void)hipEventRecord(k->ev_[2 * st], k->stream_); }
        Scope(const Scope&) = delete;
        Scope& operator=(const Scope&) = delete;
        ~Scope() { if (k->timed) (void)hipEventRecord(k->ev_[2 * st + 1], k->stream_); }
    };

    // the milliseconds of the last timed call's n_stages stages (waits for the last of them)
    int read(Core* c, int n_stages, double* ms)
    {
        LF_HIP_CHECK(c, hipSetDevice(c->device));
        LF_HIP_CHECK(c, hipEventSynchronize(ev_[2 * n_stages - 1]));
        for (int st = 0; st < n_stages; ++st) {
            float t = 0.f;
            LF_HIP_CHECK(c, hipEventElapsedTime(&t, ev_[2 * st], ev_[2 * st + 1]));
            ms[st] = t;
        }
        return LF_OK;
    }

private:
    std::vector<hipEvent_t> ev_;
    hipStream_t stream_ = nullptr;
};

}  // namespace lf
