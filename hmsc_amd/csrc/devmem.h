// Ownership of device resources: the only place that creates or releases device buffers,
// pinned host buffers, streams and events.  A chain (State::own) and every one-shot entry
// point hold a DeviceOwner; what it hands out are plain pointers / handles (views), and it
// releases all of them in its destructor, so an exception half way through a setup frees
// what the setup had made.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <unordered_set>
#include <vector>

#include "common.h"

namespace hmsc {

// Chains may live on concurrent host threads (sampleMcmc nParallel, one stream each).  A
// stream capture must not overlap another thread's device-wide synchronising calls
// (hipMalloc / hipFree / hipDeviceSynchronize): those would invalidate it.  Captures,
// chain construction / destruction and every other allocation take this lock.
inline std::recursive_mutex& device_mutex() {
  static std::recursive_mutex mu;
  return mu;
}

struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int d) {
    HIP_OK(hipGetDevice(&prev));
    if (prev != d) HIP_OK(hipSetDevice(d));
  }
  ~DeviceGuard() { (void)hipSetDevice(prev); }
};

// Live resources held by all owners of the process (hmsc_debug_live_resources): a leak of a
// 256-byte buffer or of an event does not show in hipMemGetInfo, it shows here.
enum LiveKind { LIVE_BUFFERS = 0, LIVE_PINNED = 1, LIVE_STREAMS = 2, LIVE_EVENTS = 3, LIVE_KINDS = 4 };
inline std::atomic<int64_t> g_live[LIVE_KINDS];
inline void live_add(LiveKind k, int64_t d) { g_live[k].fetch_add(d, std::memory_order_relaxed); }

// Host <-> device copies and fills go through non-blocking streams, never the legacy null
// stream: a legacy-stream operation in one thread while another thread's chain is capturing
// its sweep graph fails with "operation would make the legacy stream depend on a capturing
// blocking stream" (several chains driven from host threads of one process).  The per-thread
// streams live as long as the process.
inline hipStream_t thread_stream() {
  thread_local std::map<int, hipStream_t> streams;
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  hipStream_t& st = streams[dev];
  if (!st) HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  return st;
}
inline void copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st = nullptr) {
  if (!st) st = thread_stream();
  HIP_OK(hipMemcpyAsync(dst, src, bytes, kind, st));
  HIP_OK(hipStreamSynchronize(st));
}
// fill with a byte value, complete on return
inline void fill_sync(void* dst, int byte, size_t bytes) {
  const hipStream_t st = thread_stream();
  HIP_OK(hipMemsetAsync(dst, byte, bytes, st));
  HIP_OK(hipStreamSynchronize(st));
}

class DeviceOwner {
 public:
  DeviceOwner() = default;
  DeviceOwner(const DeviceOwner&) = delete;
  DeviceOwner& operator=(const DeviceOwner&) = delete;
  ~DeviceOwner() { release(); }

  // n elements (at least one), zero-filled: one hipMalloc per buffer
  template <class T>
  T* alloc(size_t n) {
    void* p = nullptr;
    n = std::max<size_t>(1, n);
    HIP_OK(hipMalloc(&p, n * sizeof(T)));
    bufs_.push_back(p);
    live_add(LIVE_BUFFERS, 1);
    fill_sync(p, 0, n * sizeof(T));
    return static_cast<T*>(p);
  }
  // ... holding h[0 .. n).  st: the copy is queued on it (the caller's later work on st sees
  // it); without one it is complete on return
  template <class T>
  T* upload(const T* h, size_t n, hipStream_t st = nullptr) {
    T* p = alloc<T>(n);
    if (h && n) {
      if (st)
        HIP_OK(hipMemcpyAsync(p, h, n * sizeof(T), hipMemcpyHostToDevice, st));
      else
        copy_sync(p, h, n * sizeof(T), hipMemcpyHostToDevice);
    }
    return p;
  }
  template <class T>
  T* pinned(size_t n, unsigned flags) {
    void* p = nullptr;
    HIP_OK(hipHostMalloc(&p, n * sizeof(T), flags));
    pinned_.push_back(p);
    live_add(LIVE_PINNED, 1);
    return static_cast<T*>(p);
  }
  hipStream_t stream() {
    hipStream_t st = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    streams_.push_back(st);
    live_add(LIVE_STREAMS, 1);
    return st;
  }
  hipEvent_t event(unsigned flags = hipEventDefault) {
    hipEvent_t e = nullptr;
    HIP_OK(hipEventCreateWithFlags(&e, flags));
    events_.insert(e);
    live_add(LIVE_EVENTS, 1);
    return e;
  }
  // early release of a device buffer of this owner (null: nothing)
  void free(void* p) {
    if (!p) return;
    auto it = std::find(bufs_.rbegin(), bufs_.rend(), p);
    HMSC_REQUIRE(it != bufs_.rend(), "internal: a device buffer is released by an owner that does not hold it");
    bufs_.erase(std::next(it).base());
    live_add(LIVE_BUFFERS, -1);
    HIP_OK(hipFree(p));
  }
  void free_event(hipEvent_t e) {
    if (events_.erase(e) == 0) return;
    live_add(LIVE_EVENTS, -1);
    (void)hipEventDestroy(e);
  }
  // field <- a fresh zeroed buffer of n elements, once `drain` has finished with the old one.
  // The old buffer goes first, so the peak is the larger of the two and not their sum, and the
  // field is null while the allocation can still throw.
  template <class T>
  void regrow(T*& field, size_t n, hipStream_t drain) {
    std::lock_guard<std::recursive_mutex> dev_lock(device_mutex());
    HIP_OK(hipStreamSynchronize(drain));
    T* old = field;
    field = nullptr;
    free(old);
    field = alloc<T>(n);
  }
  // streams drained, then buffers, pinned buffers, events, streams
  void release() {
    for (hipStream_t st : streams_) (void)hipStreamSynchronize(st);
    for (void* p : bufs_) (void)hipFree(p);
    for (void* p : pinned_) (void)hipHostFree(p);
    for (hipEvent_t e : events_) (void)hipEventDestroy(e);
    for (hipStream_t st : streams_) (void)hipStreamDestroy(st);
    live_add(LIVE_BUFFERS, -(int64_t)bufs_.size());
    live_add(LIVE_PINNED, -(int64_t)pinned_.size());
    live_add(LIVE_EVENTS, -(int64_t)events_.size());
    live_add(LIVE_STREAMS, -(int64_t)streams_.size());
    bufs_.clear();
    pinned_.clear();
    events_.clear();
    streams_.clear();
  }

 private:
  std::vector<void*> bufs_, pinned_;
  std::vector<hipStream_t> streams_;
  std::unordered_set<hipEvent_t> events_;
};

}  // namespace hmsc
