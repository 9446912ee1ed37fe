// Host-side helpers of the epilogue's hand-over to the caller (host_io.hip).
#pragma once
#include <cstddef>

#include "oiva_internal.h"

namespace oiva {

constexpr int kHostRingSlots = 3;
constexpr size_t kStageBytes = (size_t)256 << 20;   // staging of complex128 input and of small complex128 output
// the process-wide ring of pinned staging buffers, each of at least `bytes` (grown on demand, freed at exit)
hipError_t host_ring_slots(size_t bytes, void** slots);
// dst[r][0 .. row_bytes) = src[r][0 .. row_bytes) for r < nrows, by the pool's threads (the caller is one of them)
void host_copy_rows(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t row_bytes, long long nrows);
// fault the pages of [ptr, ptr + bytes) in for writing, contents kept, by the pool's threads (MADV_POPULATE_WRITE; where the
// kernel lacks it and may_touch, a read-modify-write of one byte per page -- only for ranges nobody else writes meanwhile)
void host_prefault(void* ptr, size_t bytes, bool may_touch);
int host_io_threads();

enum class Mem;
// rows of row_elems complex numbers between a host array of complex128 (row pitch `pitch` bytes; 0: a flat array) and a dense device array of
// complex64, cast on the device: slabs of whole rows through a staging buffer of at most stage_bound bytes (one row at least),
// allocated as `kind` on `device` for the call.  to_device: copy, cast, wait per slab; else cast, wait, copy.  Synchronous on `s`.
hipError_t staged_copy_c128(bool to_device, hipStream_t s, void* host, size_t pitch, float2* dev, size_t row_elems, long long rows,
                            size_t stage_bound, int device, Mem kind);

}  // namespace oiva
