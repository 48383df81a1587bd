// Owners of the host driver's GPU resources (included by vofod_hip.hip ahead of everything that holds one): device buffers,
// pinned host buffers, events and streams.  Move-only; each converts to the raw pointer / handle, so kernel launches, copies and
// pointer arithmetic read as they would with the raw value.  These are the only places where the driver frees or destroys.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

struct DeviceMem
{
  static hipError_t get(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
  static void put(void* p) { (void)hipFree(p); }
};
struct PinnedMem
{
  static hipError_t get(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
  static void put(void* p) { (void)hipHostFree(p); }
};

// n elements of T in the memory `Mem` hands out.  n is the capacity: set only when the allocation succeeded, 0 (and p null) otherwise.
template <class T, class Mem>
struct Buf
{
  T* p = nullptr;
  size_t n = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  Buf& operator=(Buf&& o) noexcept
  {
    if (this != &o)
    {
      reset();
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }
  operator T*() const { return p; }
  void reset()
  {
    if (p)
      Mem::put(p);
    p = nullptr, n = 0;
  }
  // frees what it held, then allocates max(n_, 1) elements
  hipError_t alloc(size_t n_, unsigned flags = 0)
  {
    reset();
    n_ = std::max<size_t>(n_, 1);
    const hipError_t e = Mem::get(reinterpret_cast<void**>(&p), n_ * sizeof(T), flags);
    if (e == hipSuccess)
      n = n_;
    else
      p = nullptr;
    return e;
  }
  // grow only: nothing happens while n_ elements fit
  hipError_t reserve(size_t n_) { return n_ <= n ? hipSuccess : alloc(n_); }
};
template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T>
using PinBuf = Buf<T, PinnedMem>;

// An event or a stream.  create(hipEventCreateWithFlags, hipEventDisableTiming) forwards to the runtime's own constructor.
template <class H, hipError_t (*Destroy)(H)>
struct DevHandle
{
  H h = nullptr;
  DevHandle() = default;
  DevHandle(DevHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
  DevHandle& operator=(DevHandle&& o) noexcept
  {
    if (this != &o)
    {
      reset();
      h = o.h;
      o.h = nullptr;
    }
    return *this;
  }
  ~DevHandle() { reset(); }
  operator H() const { return h; }
  void reset()
  {
    if (h)
      (void)Destroy(h);
    h = nullptr;
  }
  template <class Make, class... Args>
  hipError_t create(Make make, Args... args)
  {
    reset();
    const hipError_t e = make(&h, args...);
    if (e != hipSuccess)
      h = nullptr;
    return e;
  }
};
using DevEvent = DevHandle<hipEvent_t, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamDestroy>;
