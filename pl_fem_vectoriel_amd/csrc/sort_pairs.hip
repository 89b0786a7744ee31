// sort_pairs.h on rocPRIM's header-only radix sort (LSD passes over the key's low bits: stable).
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "sort_pairs.h"

namespace plfem {

size_t sort_pairs_temp_bytes(size_t n, int bits) {
  size_t bytes = 0;
  const uint32_t* kin = nullptr;
  uint32_t* kout = nullptr;
  // (a size query: launches nothing and reads no pointer)
  if (rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, kin, kout, n, 0, (unsigned)bits, nullptr, false) != hipSuccess) return 0;
  return bytes;
}

hipError_t sort_pairs(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in,
                      uint32_t* vals_out, size_t n, int bits, hipStream_t stream) {
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, (unsigned)bits, stream, false);
}

}  // namespace plfem
