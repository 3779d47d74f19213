// resident_call.h -- host plumbing of the calls answered from a plan's resident baskets (query.hip,
// rquery.hip, propagate.hip): scratch carving and growth, the LDS opt-in, the timed spans of a call
// and the read-and-clear of the bounded-probe error word. What is decided before the device is
// touched lives in resident_args.h.
#pragma once
#include <cstdlib>

#include "plan.h"
#include "resident_args.h"

inline size_t rnd256(size_t b) { return (b + 255) & ~(size_t)255; }

// arrays of a device buffer, one behind the other, each 256-B aligned
struct Carve {
  unsigned char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t n) {
    T* r = reinterpret_cast<T*>(base + off);
    off += rnd256(n * sizeof(T));
    return r;
  }
};

// grow-only device buffer cached on the plan, with 25 % + 4 KB of slack so that calls of slowly
// growing size do not reallocate every time (the merge path's ensure_dev, grank.hip, allocates
// exactly what it needs: its footprint is accounted for)
inline int ensure_scratch(unsigned char** ptr, size_t* cap, size_t need) {
  if (need <= *cap) return PPR_OK;
  if (*ptr) hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  need += need / 4 + 4096;
  if (hipMalloc((void**)ptr, need) != hipSuccess) return PPR_ERR_OOM;
  *cap = need;
  return PPR_OK;
}

// a test knob, read per call
inline int64_t env_i64(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  return e ? atoll(e) : dflt;
}

// a kernel that may be launched with `lds` bytes of dynamic LDS: above 64 KB it has to opt in
inline int set_lds(const void* fn, size_t lds) {
  if (lds <= 64 * 1024) return PPR_OK;
  if (lds > 160 * 1024) return PPR_ERR_RANGE;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess ? PPR_OK
                                                                                                       : PPR_ERR_HIP;
}

// one call: the plan's device, stream and slab, the slot rule, and the device time of its spans
struct ResidentCall {
  ppr_plan* p = nullptr;
  hipStream_t s = nullptr;
  DevSlab slab;
  int sA = 0, sB = 0;  // current slot of a partition-0 / partition-1 node
  double dev_ms = 0.0;
  int begin(ppr_plan* plan, int32_t iterations_run) {
    HIP_OK(hipSetDevice(plan->device));
    p = plan;
    s = plan->stream;
    slab = dev_slab(plan);
    const pprres::SlotPair sp = pprres::slot_pair(iterations_run);
    sA = sp.sA;
    sB = sp.sB;
    return PPR_OK;
  }
  int lap() {  // kernels between ev_m0 and ev_m1 (waits for them)
    HIP_OK(hipEventRecord(p->ev_m1, s));
    HIP_OK(hipEventSynchronize(p->ev_m1));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, p->ev_m0, p->ev_m1));
    dev_ms += ms;
    return PPR_OK;
  }
};

// PPR_ERR_PROBE once a bounded probe of this module's kernels ran out (ppr_device.h probe_fail),
// and the word cleared; a device-wide sync. g_probe_err is `static __device__`: every translation
// unit has a word of its own, set by its own kernels. So this has to stay a `static inline` function
// of a header, compiled into each module that calls it, where it reads that module's word -- one
// out-of-line function (or one linker-merged inline copy) would read only the word of the file it
// was compiled in.
static inline int take_probe_err() {
  unsigned int v = 0u;
  HIP_OK(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_probe_err), sizeof(v), 0, hipMemcpyDeviceToHost));
  if (!v) return PPR_OK;
  const unsigned int z = 0u;
  HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_probe_err), &z, sizeof(z), 0, hipMemcpyHostToDevice));
  return PPR_ERR_PROBE;
}
