// Stable device sort of (key, value) pairs of 32-bit unsigned integers by the low `bits` bits of the key
// (sort_pairs.hip: rocPRIM's radix sort, in a translation unit of its own so that no other file pays for its headers).
// The temporary storage is the caller's: sort_pairs_temp_bytes(n, bits) bytes, a function of n and bits alone.  Pairs with equal keys
// keep their input order, so the result is the same on every run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace plfem {
size_t sort_pairs_temp_bytes(size_t n, int bits);
hipError_t sort_pairs(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in,
                      uint32_t* vals_out, size_t n, int bits, hipStream_t stream);
}  // namespace plfem
