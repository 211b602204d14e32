// fi_capture.h -- the host arithmetic of output capture (fi_run_sites_capture,
// DESIGN.md §4i): argument check, row pitch, chunk sizing and the copy from
// the pinned staging to the caller's arrays.  Plain C++ with no HIP in it, so
// that a stand-alone host program can run it under the sanitizers
// (tools/capture_host_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "fi_engine.h"

namespace fi {

// NULL when the arguments are fine, else what is wrong with them.
inline const char *capture_args_error(const fi_site *sites, uint64_t n, uint32_t cap_bytes, const uint8_t *out_buf) {
    if (cap_bytes == 0) return "cap_bytes is 0 (capture of nothing: use fi_run_sites)";
    if (cap_bytes > FI_CAPTURE_MAX_BYTES) return "cap_bytes above 1 MiB";
    if (n && !sites) return "sites is NULL";
    if (n && !out_buf) return "out_buf is NULL";
    return nullptr;
}

// Device row pitch: the kernels around the pass store 16 bytes per thread.
inline uint32_t capture_stride(uint32_t cap_bytes) { return (cap_bytes + 15u) & ~15u; }

// Trials per chunk of a capture call: the rows of both streams and of both
// chunks in flight (4 x rows x stride bytes) within `budget`, and one
// stream's rows of a chunk within kCaptureStage (the pinned staging mirrors
// the device rows); at least one, at most `want`.
constexpr uint64_t kCaptureStage = (uint64_t)256 << 20;
inline uint64_t capture_rows_for(uint64_t want, uint64_t budget, uint32_t stride) {
    const uint64_t fit = std::min<uint64_t>(budget / ((uint64_t)4 * stride), kCaptureStage / stride);
    return std::max<uint64_t>(1, std::min(want, fit));
}

// Staged rows (pitch `stride`) to the caller's array (pitch `bytes`).
inline void capture_rows(uint8_t *dst, const uint8_t *src, uint64_t k, uint32_t bytes, uint32_t stride) {
    if (bytes == stride) {
        memcpy(dst, src, k * bytes);
        return;
    }
    for (uint64_t i = 0; i < k; i++) memcpy(dst + i * bytes, src + i * stride, bytes);
}

}  // namespace fi
