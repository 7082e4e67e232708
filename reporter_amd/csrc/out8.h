// out8.h -- the GPU writers' byte sink (responses.hip, flush.hip): a piece's
// text gathered 8 bytes at a time and stored as whole 8-byte words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pyrepr.h"

namespace otm {

// a piece's bytes, gathered 8 at a time and stored as whole 8-byte words
// (slots are 8-byte aligned; the last word may run past the piece into its
// slot's slack): a byte store per character cost a 64-line store instruction
struct Out {
  char* p;
  int n;
  uint64_t acc;
  __device__ __forceinline__ void put(char c) {
    acc |= (uint64_t)(uint8_t)c << (8 * (n & 7));
    if ((++n & 7) == 0) {
      *(uint64_t*)(p + n - 8) = acc;
      acc = 0;
    }
  }
  // m <= 8 bytes at once (w: byte j the j-th, zero above m)
  __device__ __forceinline__ void put8(uint64_t w, int m) {
    const int sh = 8 * (n & 7);
    acc |= w << sh;
    if ((n & 7) + m >= 8) {
      *(uint64_t*)(p + (n & ~7)) = acc;
      acc = sh ? w >> (64 - sh) : 0;
    }
    n += m;
  }
  // a literal, 8 characters a step, packed into constants at compile time (a
  // loop over the literal had read it from memory a byte at a time: one load
  // round trip per character)
  template <int N>
  __device__ __forceinline__ void lit(const char (&s)[N]) {
#pragma unroll
    for (int k0 = 0; k0 < N - 1; k0 += 8) {
      uint64_t w = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k0 + j < N - 1) w |= (uint64_t)(uint8_t)s[k0 + j] << (8 * j);
      put8(w, N - 1 - k0 < 8 ? N - 1 - k0 : 8);
    }
  }
  __device__ __forceinline__ void i64(int64_t v) { pyrepr::put_i64(v, *this); }
  __device__ __forceinline__ bool f64(double d) { return pyrepr::py_repr(d, *this); }
  __device__ __forceinline__ int done() {
    if (n & 7) *(uint64_t*)(p + (n & ~7)) = acc;
    return n;
  }
};

}  // namespace otm
