// sph_devobj.hpp -- what the objects behind the C-ABI share on the host: the error sink and the HIP check, the device picker, and for the
// two frame objects (SphSurface, SphRender) the stream with its stage clocks and the growable device buffer.  Host code, included by
// sph_api.hip before the handle is defined.
#pragma once

static thread_local std::string g_create_error;   // what a failed create leaves for *_last_error(NULL)

struct ErrSink { std::string err; };

// set the object's message (no object: the create error) and return the code
static int fail(ErrSink *o, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    (o ? o->err : g_create_error) = buf;
    return code;
}
static const char *last_error(ErrSink *o) { return o ? o->err.c_str() : g_create_error.c_str(); }

#define HIPCHK(o, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((o), SPH_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// the device of a create (requested < 0: the current one), made current; `who` is the create's name in the messages
static int pick_device(const char *who, int requested, int *dev_out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, SPH_ERR_NO_DEVICE, "%s: no HIP device visible (libsph_hip has no CPU path)", who);
    int dev = requested;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) return fail(nullptr, SPH_ERR_NO_DEVICE, "%s: device %d not present", who, dev);
    hipDeviceProp_t prop;
    if (hipSetDevice(dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail(nullptr, SPH_ERR_HIP, "%s: device %d unusable", who, dev);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, SPH_ERR_NO_DEVICE, "%s: device %d is %s, this library is built for gfx950 only", who, dev, prop.gcnArchName);
    *dev_out = dev;
    return SPH_OK;
}

static float ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0.0f; hipEventElapsedTime(&ms, a, b); return ms; }

// the events between the stages of one pass sequence on a stream
struct StageClock {
    hipEvent_t ev[6] = {};
    hipStream_t stream = nullptr;
    hipError_t mark(int k) { return hipEventRecord(ev[k], stream); }
    float ms(int a, int b) const { return ev_ms(ev[a], ev[b]); }
};

// a device buffer that only grows
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    void release() { if (p) hipFree(p); p = nullptr; bytes = 0; }
    // room for `need` bytes.  A buffer that is too small is freed and replaced; with keep_prefix_bytes its first bytes (as far as it
    // reaches) are copied over on `st` before it goes
    int reserve(ErrSink *o, size_t need, size_t keep_prefix_bytes = 0, hipStream_t st = nullptr) {
        if (need <= bytes) return SPH_OK;
        const size_t keep = std::min(keep_prefix_bytes, bytes);
        if (!keep) release();
        void *q = nullptr;
        HIPCHK(o, hipMalloc(&q, need));
        if (keep) {
            hipError_t e_ = hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, st);
            if (e_ == hipSuccess) e_ = hipStreamSynchronize(st);
            if (e_ != hipSuccess) { hipFree(q); return fail(o, SPH_ERR_HIP, "mesh list: copy failed: %s", hipGetErrorString(e_)); }
            release();
        }
        p = q;
        bytes = need;
        return SPH_OK;
    }
};

// base of the frame objects: two clocks, the object's passes and its second stage (post-processing, mesh frames)
struct DevObj : ErrSink {
    const Launch *L = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    StageClock clk[2];
};

static int devobj_open(DevObj *o, const char *who, int dev, bool fast_math) {
    o->device = dev;
    o->L = fast_math ? sph_launch_fast() : sph_launch_strict();
    if (hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking) != hipSuccess) return fail(nullptr, SPH_ERR_HIP, "%s: stream", who);
    for (StageClock &c : o->clk) {
        c.stream = o->stream;
        for (hipEvent_t &e : c.ev)
            if (hipEventCreate(&e) != hipSuccess) return fail(nullptr, SPH_ERR_HIP, "%s: event", who);
    }
    return SPH_OK;
}

// the end of an object (opened or not): wait for its stream, then buffers, events and stream go
static void devobj_close(DevObj *o, DevBuf *buf, int nbuf) {
    hipSetDevice(o->device);
    if (o->stream) hipStreamSynchronize(o->stream);
    for (int k = 0; k < nbuf; ++k) buf[k].release();
    for (StageClock &c : o->clk)
        for (hipEvent_t e : c.ev) if (e) hipEventDestroy(e);
    if (o->stream) hipStreamDestroy(o->stream);
}
