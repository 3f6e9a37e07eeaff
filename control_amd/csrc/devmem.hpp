// Owners of the library's HIP resources.  Every hipMalloc, stream, event, pinned allocation and
// graph capture of the library is in this header (the vectors handed out by kkt_vec_alloc excepted:
// their caller owns them).
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

namespace kkt {

void hip_check(hipError_t e, const char *what, const char *file, int line);
#define HIPCHK(x) ::kkt::hip_check((x), #x, __FILE__, __LINE__)

// Owner of one allocation: members and function-local temporaries.  One hipMalloc per buffer;
// n == 0 allocates one element, so that no owner of a buffer holds a null pointer.
template <class T>
class DevBuf {
   public:
    DevBuf() = default;
    static DevBuf alloc(size_t n) {
        void *p = nullptr;
        if (n == 0) n = 1;
        HIPCHK(hipMalloc(&p, n * sizeof(T)));
        DevBuf b;
        b.p_.reset(static_cast<T *>(p));
        return b;
    }
    static DevBuf upload(const T *h, size_t n) {
        DevBuf b = alloc(n);
        if (n) HIPCHK(hipMemcpy(b.get(), h, n * sizeof(T), hipMemcpyHostToDevice));
        return b;
    }
    T *get() const { return p_.get(); }
    T *release() { return p_.release(); }   // to DevPool::adopt, or to a caller who frees it
    void reset() { p_.reset(); }

   private:
    struct Free {
        void operator()(T *p) const { (void)hipFree((void *)p); }
    };
    std::unique_ptr<T, Free> p_;
};

// Owner of many allocations with one lifetime.  Hands out plain pointers, stable until release();
// still one hipMalloc per request.
class DevPool {
   public:
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() { release(); }
    template <class T>
    T *alloc(size_t n) {
        return adopt(DevBuf<T>::alloc(n));
    }
    template <class T>
    T *upload(const T *h, size_t n) {
        return adopt(DevBuf<T>::upload(h, n));
    }
    template <class T>
    T *adopt(DevBuf<T> b) {
        ptrs_.push_back(nullptr);   // the slot first: a failed push_back must not strand the buffer
        ptrs_.back() = (void *)b.get();
        return b.release();
    }
    void release() {
        for (void *p : ptrs_) (void)hipFree(p);
        ptrs_.clear();
    }

   private:
    std::vector<void *> ptrs_;
};

// Owner of a stream (non-blocking).  Empty until create(): the side streams are made on first use.
class Stream {
   public:
    Stream() = default;
    static Stream create() {
        hipStream_t s = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        Stream o;
        o.p_.reset(s);
        return o;
    }
    hipStream_t get() const { return p_.get(); }
    operator hipStream_t() const { return get(); }

   private:
    struct Destroy {
        void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
    };
    std::unique_ptr<std::remove_pointer_t<hipStream_t>, Destroy> p_;
};

// Owner of an event, with timing (the clocks) or without (ordering between streams).
class Event {
   public:
    Event() = default;
    static Event create(bool timing) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming));
        Event o;
        o.p_.reset(e);
        return o;
    }
    hipEvent_t get() const { return p_.get(); }
    operator hipEvent_t() const { return get(); }

   private:
    struct Destroy {
        void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
    };
    std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroy> p_;
};

// Owner of pinned host memory.
template <class T>
class PinnedBuf {
   public:
    PinnedBuf() = default;
    static PinnedBuf alloc(size_t n) {
        void *p = nullptr;
        HIPCHK(hipHostMalloc(&p, n * sizeof(T), 0));
        PinnedBuf b;
        b.p_.reset(static_cast<T *>(p));
        return b;
    }
    T *get() const { return p_.get(); }
    operator T *() const { return get(); }

   private:
    struct Free {
        void operator()(T *p) const { (void)hipHostFree((void *)p); }
    };
    std::unique_ptr<T, Free> p_;
};

// Owner of a captured graph and its executable.  Declare it AFTER the buffers its nodes point at
// (members are destroyed in reverse order of declaration).
struct GraphExec {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    GraphExec() = default;
    GraphExec(GraphExec &&o) noexcept : graph(o.graph), exec(o.exec) { o.graph = nullptr, o.exec = nullptr; }
    GraphExec &operator=(GraphExec &&o) noexcept {
        std::swap(graph, o.graph);
        std::swap(exec, o.exec);
        return *this;
    }
    ~GraphExec() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

// `launches` on `st` as a graph: captured and instantiated on the first call, launched on every
// call.  A HIP error on the way (cleared) sets `usable` to false and issues the launches plainly;
// the caller then stops coming here.  This is the only place where a capture begins, and every way
// out of it -- done, HIP error, an exception from `launches` -- ends the capture first: the stream
// is never left capturing.
template <class F>
void run_captured(hipStream_t st, GraphExec &g, bool &usable, F &&launches) {
    if (!g.exec) {
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            try {
                launches();
            } catch (...) {
                GraphExec partial;   // discarded
                (void)hipStreamEndCapture(st, &partial.graph);
                (void)hipGetLastError();
                throw;
            }
            e = hipStreamEndCapture(st, &g.graph);
            if (e == hipSuccess) e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            g = GraphExec{};
            usable = false;
            launches();
            return;
        }
    }
    HIPCHK(hipGraphLaunch(g.exec, st));
}

}  // namespace kkt
