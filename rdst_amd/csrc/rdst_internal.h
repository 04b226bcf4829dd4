// rdst_internal.h — hooks between the library's translation units.  Not part of the C ABI (include/rdst_hip.h).
#ifndef RDST_INTERNAL_H
#define RDST_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdst_hip.h"

namespace rdst_internal {

// Records `what` (and the HIP error, if any) for rdst_hip_last_error and returns `code`.
int set_error(int code, const char* what, hipError_t e = hipSuccess);

// The current device's sticky error word (kernels OR bits into it; rdst_hip_device_status reports and clears it).
int device_error_word(uint32_t** out);

// [u8; N] rows with N in 1..16, in place on `s`: widened to 4-, 8- or 16-byte integers in `scratch`, sorted by the integer
// route, narrowed back (the path rdst_hip_sort takes for these widths).  Asynchronous.
uint64_t widened_scratch_bytes(uint64_t len, uint32_t nb);
int sort_bytes_widened(void* dev_rows, uint64_t len, uint32_t nb, void* scratch, hipStream_t s);

// rdst_bytes.hip: a host slice of `len` rows of `row_bytes` bytes ordered by the byte string at (key_offset, key_bytes),
// equal keys in input order.  Blocking; the slice is written only after the device reported success.  Arguments are
// checked by the caller.
int sort_bytes_rows_host(void* host_rows, uint64_t len, uint32_t row_bytes, uint32_t key_offset, uint32_t key_bytes,
                         const rdst_hip_opts* opts);

}  // namespace rdst_internal

#endif  // RDST_INTERNAL_H
