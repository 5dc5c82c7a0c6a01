// torj_host_util.hpp -- host plumbing shared by every host part of the library:
// the thread's last error (fail / HIPCK), the environment knobs' parsers, the
// grow-only device buffer and the small upload / download helpers.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// ===========================================================================
// error handling
// ===========================================================================
static thread_local std::string g_err;

static int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

#define HIPCK(expr)                                                                       \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ===========================================================================
// environment knobs (TORJ_*; INTEGRATION.md lists every one): the value parsed
// as the knob always was (atoi / atol / atof), or `dflt` when it is unset.
// A knob read per call goes through these at its use; one read once is a
// function-local `static const` initialised from them.
// ===========================================================================
static inline bool env_has(const char *name) { return getenv(name) != nullptr; }
static inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
static inline long env_long(const char *name, long dflt) {
    const char *e = getenv(name);
    return e ? atol(e) : dflt;
}
static inline double env_double(const char *name, double dflt) {
    const char *e = getenv(name);
    return e ? atof(e) : dflt;
}

// a grow-only device buffer: reserve() keeps it when it is large enough, else
// frees it and allocates `bytes` (the contents are scratch, not carried over)
struct GrowBuf {
    void *d = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (cap >= bytes) return 0;
        if (d) HIPCK(hipFree(d));
        d = nullptr;
        cap = 0;
        HIPCK(hipMalloc(&d, bytes));
        cap = bytes;
        return 0;
    }
};

// ---- device helpers ----
template <typename T>
static int dupload(T **d, const T *h, size_t n, hipStream_t s) {
    *d = nullptr;
    if (!h || n == 0) return 0;
    HIPCK(hipMalloc(d, n * sizeof(T)));
    HIPCK(hipMemcpyAsync(*d, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    return 0;
}
template <typename T>
static int dalloc(T **d, size_t n, bool want) {
    *d = nullptr;
    if (!want || n == 0) return 0;
    HIPCK(hipMalloc(d, n * sizeof(T)));
    return 0;
}
template <typename T>
static int ddownload(T *h, const T *d, size_t n, hipStream_t s) {
    if (!h || !d || n == 0) return 0;
    HIPCK(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    return 0;
}

struct DevBufs {
    std::vector<void *> ptrs;
    ~DevBufs() {
        for (void *q : ptrs)
            if (q) (void)hipFree(q);
    }
    template <typename T>
    T *track(T *q) {
        ptrs.push_back((void *)q);
        return q;
    }
    // dupload / dalloc whose buffer is owned from the moment it exists (freed
    // on every early return, a failed copy after a good allocation included)
    template <typename T>
    int up(T **d, const T *h, size_t n, hipStream_t s) {
        const int r = dupload(d, h, n, s);
        track(*d);
        return r;
    }
    template <typename T>  // ... into a field that is an input where it is used (RayIO's, EntryIO's)
    int up(const T **d, const T *h, size_t n, hipStream_t s) {
        return up(const_cast<T **>(d), h, n, s);
    }
    template <typename T>
    int alloc(T **d, size_t n, bool want) {
        const int r = dalloc(d, n, want);
        track(*d);
        return r;
    }
};

static inline int nblocks(int n, int b) { return (n + b - 1) / b; }

