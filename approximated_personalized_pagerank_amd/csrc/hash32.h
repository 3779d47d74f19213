// hash32.h -- the 32-bit mixer behind every hash table, row order and tie rule of the library, for
// both sides: kernels probe tables with it (ppr_device.h) and the host builds table images that
// those kernels probe (rquery.hip's target table). One definition, so the two cannot drift. Plain
// C++ without hipcc: tests/cpp/resident_args_test.cpp pins five values.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PPR_HASH_HD __host__ __device__ __forceinline__
#else
#define PPR_HASH_HD inline
#endif

namespace pprd {

PPR_HASH_HD uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}

}  // namespace pprd
