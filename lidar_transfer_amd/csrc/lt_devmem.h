// lt_devmem.h -- how the host side of liblidarhip.so holds device memory: two things and nothing else.
//
//   lt_carve          the layout of ONE allocation carved into 256-byte-aligned arrays: a running offset.  Pure size_t
//                     arithmetic, no HIP: the layouts built on it (lt_layouts.h) compile with any C++ compiler.
//   lt_dev_replace    the one way a device array of this library grows: a GROUP of arrays that share one capacity is
//                     replaced, all or none.  lt_dev_grow is the same for one array behind its "does it hold `need`" test.
//
// The two rules of a replacement: WHO WAITS -- the site says what has to finish before its old arrays may go (the device,
// one stream, or nothing: lt_wait_*), and the wait happens only when there is an old array; WHAT A FAILURE LEAVES -- every
// pointer of the group NULL and the capacity 0, so that the next call allocates again instead of trusting a capacity whose
// arrays are gone.  Pointers and capacities stay plain fields of the (calloc'ed) structs the kernels' arguments are read from.
#pragma once
#include <stddef.h>

struct lt_carve {
  size_t off = 0;
  // the offset of the next array of `bytes` bytes; the one after it starts at the next multiple of 256
  size_t take(size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
  }
};

// headroom of an array whose demand varies from scan to scan (meshes, clouds): a quarter more, and 1024 elements
static inline size_t lt_headroom(size_t need) { return need + need / 4 + 1024; }

#ifdef __HIPCC__
#include "lt_internal.h"

struct lt_wait { enum { NONE, STREAM, DEVICE } what; hipStream_t stream; };
static inline lt_wait lt_wait_none() { return {lt_wait::NONE, nullptr}; }  // (hipFree waits by itself)
static inline lt_wait lt_wait_stream(hipStream_t s) { return {lt_wait::STREAM, s}; }
static inline lt_wait lt_wait_device() { return {lt_wait::DEVICE, nullptr}; }

struct lt_dev_array { void** p; size_t bytes; };  // bytes == 0: the array is dropped and stays NULL

// Replace the arrays of `group`, whose shared capacity is *cap: wait (if one of them exists), free them all, allocate them
// all, *cap = new_cap.  On failure the group is empty, *cap is 0 and lt_last_error() names `who`.
template <class C, size_t N>
static int lt_dev_replace(const char* who, lt_wait w, C* cap, C new_cap, const lt_dev_array (&group)[N]) {
  bool any = false;
  for (const lt_dev_array& g : group) any = any || *g.p;
  hipError_t e = hipSuccess;
  if (any && w.what != lt_wait::NONE) e = w.what == lt_wait::DEVICE ? hipDeviceSynchronize() : hipStreamSynchronize(w.stream);
  if (e != hipSuccess) {
    lt_set_error("%s: waiting for the device before a reallocation failed: %s", who, hipGetErrorString(e));
    return LT_ERR_HIP;
  }
  auto drop = [&]() {
    for (const lt_dev_array& g : group) {
      if (*g.p) (void)hipFree(*g.p);
      *g.p = nullptr;
    }
    *cap = 0;
  };
  drop();
  size_t failed = 0;
  for (const lt_dev_array& g : group)
    if (e == hipSuccess && g.bytes && (e = hipMalloc(g.p, g.bytes)) != hipSuccess) failed = g.bytes;
  if (e != hipSuccess) {
    drop();
    (void)hipGetLastError();
    lt_set_error("%s: hipMalloc of %zu bytes failed: %s", who, failed, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? LT_ERR_NO_MEMORY : LT_ERR_HIP;
  }
  *cap = new_cap;
  return LT_OK;
}

// ... of a group without a capacity of its own (arrays created once, or sized by a fixed property of their object)
template <size_t N>
static int lt_dev_replace(const char* who, lt_wait w, const lt_dev_array (&group)[N]) {
  int cap = 0;
  return lt_dev_replace(who, w, &cap, 0, group);
}

// One array of *cap elements that must hold `need`: replaced by one of `alloc` elements when it does not (or does not exist).
template <class T, class C>
static int lt_dev_grow(const char* who, lt_wait w, T** p, C* cap, size_t need, size_t alloc) {
  if (need <= (size_t)*cap && *p) return LT_OK;
  const lt_dev_array one[] = {{(void**)p, alloc * sizeof(T)}};
  return lt_dev_replace(who, w, cap, (C)alloc, one);
}
#endif
