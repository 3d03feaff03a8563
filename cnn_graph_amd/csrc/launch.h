// What the host launch code at the bottom of every .hip file shares: the
// opt-in for more than 64 KB of dynamic LDS, the resident-workgroup count, the
// per-device CU count and wall-clock rate, and the launch itself.
//
// The first part, like occupancy_cache.h under it (ResidentCache,
// persistent_grid), is host-only and free of HIP types so that
// tests/test_launch_cpu.py can compile it with g++ against counting stand-ins;
// the HIP-facing part at the end is a few lines on top of it.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <thread>

#include "occupancy_cache.h"

namespace cg {

// What k_xbasis makes of the count: unknown means one workgroup per CU on 256 CUs.
inline int xbasis_resident(int resident) { return resident > 0 ? resident : 256; }

// What k_lstm_seq's residency check makes of it: its pairs wait for each
// other, so an unknown count is an error and not a guess.
enum GridFit { kGridFits = 0, kGridTooLarge, kGridUnknown };
inline GridFit grid_fit(int64_t blocks, int resident) {
  return resident <= 0 ? kGridUnknown : blocks > resident ? kGridTooLarge : kGridFits;
}

// set() -> status (>= 0) runs once per (device, kernel): the first caller for a
// pair runs it, every caller gets its status, and none returns before it has
// returned.  A function attribute belongs to the function on ONE device, so a
// per-process static would leave every device but the first launch's unset.
//
// A hit is a hash, the slot's key and the device's state word: three loads, no
// lock (config B's step is three launches in about 52 us).  Slots are claimed
// by compare-and-swap on the key and never freed: kernels are functions of the
// library, far fewer than kSlots.  A device past kDevices or a full table is
// served by running set() on every call: slower, never unset.
class OncePerDevice {
 public:
  static constexpr int kDevices = 16, kSlots = 256;

  template <typename Set>
  int get(int device, const void* kernel, Set&& set) {
    std::atomic<int>* st = device >= 0 && device < kDevices ? state(kernel, device) : nullptr;
    if (!st) return set();
    int v = st->load(std::memory_order_acquire);
    if (v >= kDone) return v - kDone;
    if (v == kUnset && st->compare_exchange_strong(v, kBusy, std::memory_order_acq_rel,
                                                   std::memory_order_acquire)) {
      const int status = set();
      st->store(status + kDone, std::memory_order_release);
      return status;
    }
    while ((v = st->load(std::memory_order_acquire)) < kDone) std::this_thread::yield();
    return v - kDone;
  }

 private:
  enum { kUnset = 0, kBusy = 1, kDone = 2 };  // kDone + status once set() has returned
  struct Slot {
    std::atomic<const void*> key{nullptr};
    std::atomic<int> st[kDevices] = {};
  };
  std::atomic<int>* state(const void* kernel, int device) {
    const unsigned h = unsigned((reinterpret_cast<uintptr_t>(kernel) >> 4) * 0x9E3779B1u);
    for (unsigned i = 0; i < unsigned(kSlots); ++i) {
      Slot& s = slots_[(h + i) % kSlots];
      const void* k = s.key.load(std::memory_order_acquire);
      if (k == nullptr && s.key.compare_exchange_strong(k, kernel, std::memory_order_acq_rel,
                                                        std::memory_order_acquire))
        k = kernel;
      if (k == kernel) return &s.st[device];
    }
    return nullptr;
  }
  Slot slots_[kSlots];
};

// One positive int per device (the CU count, the wall-clock rate), queried
// once: query() -> the value, <= 0 when it failed.  Returns -1 when unknown;
// the caller keeps its own fallback.
class DeviceInt {
 public:
  template <typename Query>
  int get(int device, Query&& query) {
    const bool cached = device >= 0 && device < OncePerDevice::kDevices;
    int v = cached ? v_[device].load(std::memory_order_relaxed) : 0;
    if (v != 0) return v;
    v = query();
    if (v <= 0) v = -1;
    if (cached) v_[device].store(v, std::memory_order_relaxed);  // racing threads store the same
    return v;
  }

 private:
  std::atomic<int> v_[OncePerDevice::kDevices] = {};
};

}  // namespace cg

#ifdef __HIPCC__
#include "cg_internal.h"

namespace cg {

inline int current_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}

template <typename... P>
const void* kernel_ptr(void (*k)(P...)) {
  return reinterpret_cast<const void*>(k);
}

// Allows kernel k up to `limit` bytes of dynamic LDS on the current device
// (`dev`, for a launcher that has read it already): hipFuncSetAttribute the
// first time k is asked for there, that call's status then and ever after.
// The first call for a (device, kernel) sets its limit; a kernel with a limit
// of its own (k_lstm_seq) passes it on every call.
inline hipError_t allow_big_lds(const void* k, int limit = kLdsBytes, int dev = current_device()) {
  static OncePerDevice once;
  return hipError_t(once.get(dev, k, [&] {
    return int(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, limit));
  }));
}

// CUs of `device`, -1 when the query failed.
inline int device_cus(int device) {
  static DeviceInt cus;
  return cus.get(device, [&] {
    int v = 0;
    return hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess ? v : -1;
  });
}

// Wall-clock rate of `device` in kHz, -1 when the query failed.
inline int device_wall_clock_khz(int device) {
  static DeviceInt rate;
  return rate.get(device, [&] {
    int v = 0;
    return hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, device) == hipSuccess ? v : -1;
  });
}

// Workgroups of k (threads, lds bytes of dynamic LDS) resident at once on the
// current device, -1 when unknown: what each caller does then is its own
// policy.  Past 64 KB the occupancy query needs the opt-in, so it comes first;
// a launcher that returns the opt-in's status, or whose kernel has a limit of
// its own, has called allow_big_lds before and this one is a hit.
inline int resident_blocks(const void* k, int threads, size_t lds, int dev = current_device()) {
  static ResidentCache cache;
  return cache.get(dev, k, threads, lds, [&](const void* kf, int thr, size_t l, int* per_cu, int* cus) {
    if (l > size_t(64) * 1024) (void)allow_big_lds(kf, kLdsBytes, dev);
    *cus = device_cus(dev);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kf, thr, l) == hipSuccess;
  });
}

template <typename T>
struct same {
  using type = T;
};

// hipLaunchKernel with the kernel's own parameter types: every argument is
// converted to its parameter as a <<<>>> launch converts it.  Returns what
// hipGetLastError returns after it, as hipLaunchKernelGGL's callers read it.
template <typename... P>
hipError_t launch(void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                  const typename same<P>::type&... p) {
  void* args[] = {const_cast<void*>(static_cast<const void*>(&p))...};
  (void)hipLaunchKernel(kernel_ptr(k), grid, block, args, lds, s);
  return hipGetLastError();
}

// launch() of a kernel that may take more than 64 KB of dynamic LDS: the
// opt-in for k on the current device first, its status if it failed.
template <typename... P>
hipError_t launch_big_lds(void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                          const typename same<P>::type&... p) {
  const hipError_t attr = allow_big_lds(kernel_ptr(k));
  return attr != hipSuccess ? attr : launch(k, grid, block, lds, s, p...);
}

}  // namespace cg
#endif  // __HIPCC__
