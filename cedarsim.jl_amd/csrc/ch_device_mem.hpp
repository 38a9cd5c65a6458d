// ch_device_mem.hpp — ownership of device and pinned host memory for the engine host code: the per-circuit arena, DevBuf,
// RAII holders for a call's solve workspace, pinned buffers and events, and the HIPCHK early-return macro.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

// inside a member (or a scope with set_err in reach): record the failing call and return CH_ERR_DEVICE
#define HIPCHK(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) { set_err(std::string(#call) + ": " + hipGetErrorString(e_)); return CH_ERR_DEVICE; } \
  } while (0)

namespace chip {

// LDS of one gfx950 CU; a kernel's static __shared__ variables come out of the same budget, and the dynamic part is granted in
// units of 256 bytes: what a kernel with `static_bytes` of its own may be raised to
constexpr int LDS_BYTES_PER_CU = 160 * 1024;
inline int lds_dynamic_ceiling(int static_bytes) { return (LDS_BYTES_PER_CU - static_bytes) & ~255; }

// All device buffers of a circuit are carved out of a few large allocations: the Newton kernel's
// prologue touches a dozen different arrays, and with one hipMalloc per array every launch paid a
// cold translation miss per array (measured: prologue 9 us -> see profiles/r01_notes.md).
struct Arena {
  std::vector<char*> chunks; size_t used = 0, cap = 0;
  static constexpr size_t CHUNK = 32u << 20;
  ~Arena() { for (char* c : chunks) (void)hipFree(c); }
  void* take(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    if (bytes > CHUNK / 2) { char* p = nullptr; if (hipMalloc((void**)&p, bytes) != hipSuccess) return nullptr; chunks.insert(chunks.begin(), p); return p; }
    if (chunks.empty() || used + bytes > cap) { char* p = nullptr; if (hipMalloc((void**)&p, CHUNK) != hipSuccess) return nullptr; chunks.push_back(p); used = 0; cap = CHUNK; }
    void* r = chunks.back() + used; used += bytes; return r;
  }
};
static thread_local Arena* g_arena = nullptr;  // set while a circuit builds / rebuilds its buffers
// Every entry point that may (re)allocate device buffers of a circuit opens one of these: allocations made inside the
// call come from THAT circuit's arena and the pointer never outlives the call (a stale pointer would let a later call on
// another circuit carve its buffers out of this circuit's arena, which is freed with this circuit).
struct ArenaScope {
  Arena* prev;
  explicit ArenaScope(Arena* a) : prev(g_arena) { g_arena = a; }
  ~ArenaScope() { g_arena = prev; }
  ArenaScope(const ArenaScope&) = delete; ArenaScope& operator=(const ArenaScope&) = delete;
};

template <class T>
struct DevBuf {
  T* p = nullptr; size_t n = 0; bool owned = false;
  ~DevBuf() { if (p && owned) (void)hipFree(p); }
  hipError_t alloc(size_t count) {
    if (p && count <= n && count > 0) { return hipSuccess; }  // reuse
    if (p && owned) (void)hipFree(p);
    p = nullptr; n = count;
    const size_t bytes = std::max<size_t>(1, count) * sizeof(T);
    if (g_arena) { p = (T*)g_arena->take(bytes); owned = false; return p ? hipSuccess : hipErrorOutOfMemory; }
    owned = true;
    return hipMalloc((void**)&p, bytes);
  }
  hipError_t upload(const std::vector<T>& h, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (h.size() > n || !p) e = alloc(h.size());
    if (e != hipSuccess) return e;
    if (h.empty()) return hipSuccess;
    e = hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
  }
};

// The global workspace of one call's dense solves: its own hipMalloc, freed when the scope ends.  Never from the arena, which would
// hold it (up to 1 GiB) for the circuit's lifetime.  hipFree waits for the device, so a return between two launches is safe.
struct ScopedWorkspace {
  double* p = nullptr;
  ScopedWorkspace() = default;
  ScopedWorkspace(const ScopedWorkspace&) = delete; ScopedWorkspace& operator=(const ScopedWorkspace&) = delete;
  ~ScopedWorkspace() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t doubles) { return hipMalloc((void**)&p, doubles * sizeof(double)); }
};

// pinned host memory (mapped into the device's address space with hipHostMallocMapped); converts to T* like the raw pointer it replaces
template <class T>
struct PinnedBuf {
  T* p = nullptr; size_t n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
  hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) {   // drops the old contents
    release();
    const hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), flags);
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
  operator T*() const { return p; }
};
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete; DevEvent& operator=(const DevEvent&) = delete;
  ~DevEvent() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return hipEventCreate(&e); }
  operator hipEvent_t() const { return e; }
};

}  // namespace chip
