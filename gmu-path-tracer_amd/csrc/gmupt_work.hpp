// The handle of a tree stage that runs on a stream of its own: the LBVH builder (gmupt_lbvh, gmupt_capi_accel.hip) and the treelet
// optimiser (gmupt_treeopt, gmupt_capi_treeopt.hip).  A stream, two events and the scratch of the largest input so far; what the two
// C-API units do alike with it.  `fn` is the caller's name as gmupt_last_error quotes it.
#pragma once
#include "gmupt_internal.hpp"

#pragma GCC visibility push(hidden)
struct gmupt_work {
    gmupt_device* dev = nullptr; hipStream_t stream = nullptr; EventPair ev; DevMem scratch;
    // (cap, sortTemp) is "large enough for every input so far", not "what the capacity needs": the sort's temporary storage is asked
    // for per input (a host-only call), a smaller input is not assumed to need less than the capacity did, and a later input may grow
    // either once more
    uint32_t cap = 0; size_t sortTemp = 0;
    ~gmupt_work() { if (stream) (void)hipStreamDestroy(stream); }        // work_destroy has synchronised it

    // scratch for an input of n items whose sorts need `temp` bytes; bytesFor(capacity, temp) is the stage's size of it
    int reserve(uint32_t n, size_t temp, size_t (*bytesFor)(uint32_t, size_t))
    {
        if (n <= cap && temp <= sortTemp) return GMUPT_OK;
        const uint32_t grown = std::max(n, cap);
        cap = 0; sortTemp = 0;                                           // should the scratch fail to grow
        GMUPT_TRY(scratch.grow(stream, bytesFor(grown, temp)));
        cap = grown; sortTemp = temp;
        return GMUPT_OK;
    }
};
struct gmupt_lbvh : gmupt_work {};
struct gmupt_treeopt : gmupt_work {};

template <class H> void work_destroy(H* h)
{
    if (!h) return;
    (void)hipSetDevice(h->dev->id);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
}

template <class H> int work_create(const char* fn, gmupt_device* dev, H** out)
{
    if (!dev || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    *out = nullptr;
    H* h = new (std::nothrow) H();
    if (!h) return fail(GMUPT_ERR_OUT_OF_MEMORY, "%s: out of host memory", fn);
    h->dev = dev;
    hipError_t e = hipSetDevice(dev->id);
    if (e == hipSuccess) e = hipStreamCreate(&h->stream);
    if (e != hipSuccess) { work_destroy(h); return fail(GMUPT_ERR_HIP, "%s: %s", fn, hipGetErrorString(e)); }
    *out = h;
    return GMUPT_OK;
}

// a gmupt_buffer of `elems` elements filled from device memory on stream s (the caller synchronises)
inline int output_buffer(gmupt_device* dev, gmupt_buffer_kind kind, size_t elems, const void* src, hipStream_t s, const char* fn, gmupt_buffer** out)
{
    hipError_t e = hipSuccess;
    gmupt_buffer* b = buffer_alloc(dev, kind, elems, elems * kind_stride(kind), &e);
    if (!b) return fail(GMUPT_ERR_OUT_OF_MEMORY, "%s: out of host memory", fn);
    if (e == hipSuccess) e = hipMemsetAsync((char*)b->dptr + b->bytes, 0, 16, s);      // the slack
    if (e == hipSuccess) e = hipMemcpyAsync(b->dptr, src, b->bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { gmupt_buffer_destroy(b); return fail(GMUPT_ERR_HIP, "%s(%zu bytes): %s", fn, elems * kind_stride(kind), hipGetErrorString(e)); }
    *out = b;
    return GMUPT_OK;
}
#pragma GCC visibility pop
