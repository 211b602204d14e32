// capture_host_check -- the host arithmetic of output capture
// (shrewd_amd/csrc/fi_capture.h) as fi_run_sites_capture, chunk_end and
// chunk_deliver use it, with plain vectors in the place of the device rows
// and the pinned staging: a stand-alone host program, so that it runs under
// AddressSanitizer and UBSan.  It checks those inline helpers only; the
// engine's own allocation, error paths and chunk offsets need a device and
// are covered by tests/test_gpu_capture.py.  Build (no HIP needed):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ishrewd_amd/csrc tools/capture_host_check.cpp -o capture_host_check
// Prints "capture_host_check ok" and exits 0, or names what failed.
#include <cstdio>
#include <vector>

#include "fi_capture.h"

using namespace fi;

static int fails = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAILED line %d: %s\n", __LINE__, #x);         \
            fails++;                                              \
        }                                                         \
    } while (0)

// A run of n trials in chunks, as run_chunks does it: each chunk's "device"
// rows (pitch stride, every byte written) go through a staging buffer of the
// chunk size to the caller's arrays (pitch cap_bytes).
static void run(uint64_t n, uint32_t cap_bytes, uint64_t budget, uint64_t max_trials) {
    const uint32_t stride = capture_stride(cap_bytes);
    CHECK(stride % 16 == 0 && stride >= cap_bytes && stride < cap_bytes + 16);
    const uint64_t want = std::min(n, max_trials);
    const uint64_t rows = capture_rows_for(want, budget, stride);
    CHECK(rows >= 1 && rows <= want);
    CHECK(rows == 1 || 4 * rows * stride <= budget);
    CHECK(rows == 1 || rows * stride <= kCaptureStage);
    std::vector<uint8_t> out(n * cap_bytes, 0xEE), stage(rows * stride), dev(rows * stride);
    for (uint64_t done = 0; done < n;) {
        const uint64_t k = std::min(n - done, rows);
        for (uint64_t i = 0; i < k; i++)
            for (uint32_t b = 0; b < stride; b++) dev[i * stride + b] = b < cap_bytes ? (uint8_t)((done + i) * 31 + b) : 0xAA;
        memcpy(stage.data(), dev.data(), k * stride);
        capture_rows(out.data() + done * cap_bytes, stage.data(), k, cap_bytes, stride);
        done += k;
    }
    bool same = true;
    for (uint64_t i = 0; i < n && same; i++)
        for (uint32_t b = 0; b < cap_bytes && same; b++) same = out[i * cap_bytes + b] == (uint8_t)(i * 31 + b);
    CHECK(same);
}

int main() {
    fi_site s{};
    uint8_t byte = 0;
    CHECK(capture_args_error(&s, 1, 0, &byte) != nullptr);
    CHECK(capture_args_error(&s, 1, FI_CAPTURE_MAX_BYTES + 1, &byte) != nullptr);
    CHECK(capture_args_error(&s, 1, 0xFFFFFFFFu, &byte) != nullptr);
    CHECK(capture_args_error(&s, 1, 64, nullptr) != nullptr);
    CHECK(capture_args_error(nullptr, 1, 64, &byte) != nullptr);
    CHECK(capture_args_error(nullptr, 0, 64, nullptr) == nullptr);
    CHECK(capture_args_error(&s, 1, 1, &byte) == nullptr);
    CHECK(capture_args_error(&s, 1, FI_CAPTURE_MAX_BYTES, &byte) == nullptr);
    // sizing at the extremes: no overflow, never 0 rows
    CHECK(capture_rows_for(1u << 21, 0, capture_stride(FI_CAPTURE_MAX_BYTES)) == 1);
    CHECK(capture_rows_for(1u << 21, ~0ull, 16) == 1u << 21);
    CHECK(capture_rows_for(1u << 21, ~0ull, capture_stride(FI_CAPTURE_MAX_BYTES)) == 256);
    CHECK(capture_rows_for(1u << 21, 1ull << 30, capture_stride(4096)) == 65536);
    for (uint32_t cap : {1u, 8u, 15u, 16u, 17u, 200u, 4096u})
        for (uint64_t n : {1ull, 2ull, 1000ull, 3001ull})
            for (uint64_t budget : {0ull, 4096ull, 1ull << 20, 1ull << 34}) run(n, cap, budget, 1024);
    run(3, FI_CAPTURE_MAX_BYTES, 1ull << 23, 2);
    if (!fails) printf("capture_host_check ok\n");
    return fails ? 1 : 0;
}
