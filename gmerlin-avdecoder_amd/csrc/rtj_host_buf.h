// rtj_host_buf.h — what libmi_rtjpeg.so's host layer has beside the shared base (host_base.h): pinned host memory with
// hipHostMalloc's flags.  Included by mi_rtjpeg.hip (one translation unit); not a kernel header.
#pragma once
#include "host_base.h"

namespace {

// Pinned host memory allocated with flags (mapped memory's device address is the caller's to ask for).
template <class T>
struct FlagPinnedBuf : PinnedBuf<T> {
  hipError_t alloc(uint64_t n, unsigned flags = hipHostMallocDefault) {
    this->release();
    const hipError_t e = hipHostMalloc((void**)&this->p, sizeof(T) * (size_t)n, flags);
    if (e == hipSuccess) this->cap = n;
    else this->p = nullptr;
    return e;
  }
};

}  // namespace
