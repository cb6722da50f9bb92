// host_owned.h — memory that frees itself, shared by the host layers of libmi_rtjpeg.so (rtj_host_buf.h) and libmi_dv.so
// (dv_host_buf.h).  Host only; depends on nothing but HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

namespace {

// `cap` elements at `p`, owned: move-only, freed by the destructor
template <class T, hipError_t (*Free)(void*)>
struct Owned {
  T* p = nullptr;
  uint64_t cap = 0;

  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(cap, o.cap);
    }
    return *this;
  }
  ~Owned() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)Free(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace
