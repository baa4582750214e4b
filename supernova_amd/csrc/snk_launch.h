// snk_launch.h -- the one place a kernel is launched from.
//
// HIP cuts a launch of 2^32 or more work items short WITHOUT an error ("round 6" (5): 87 % of the provisional
// unitig bases were never written), and the kernels index with 32-bit expressions (blockIdx.x * TB + threadIdx.x).  So the grid
// is computed in 64 bits, judged on the host, and a shape that does not fit is an error before anything runs.  A kernel whose
// items may outgrow that strides over them behind a capped grid.
//
// The arithmetic is plain C++ (no HIP needed: tests/launch_shape_host.cc builds it with the host compiler).
#pragma once
#include <stdint.h>

// workgroups for `items` work items at `per_block` a group: ceiling division that cannot wrap
static inline uint64_t snk_blocks(uint64_t items, uint64_t per_block) { return items / per_block + (items % per_block != 0); }
// ... clamped to [1, cap]: the grid of a kernel that strides over what is left
static inline uint64_t snk_blocks_capped(uint64_t items, uint64_t per_block, uint64_t cap) {
    const uint64_t b = snk_blocks(items, per_block);
    return b < 1 ? 1 : b > cap ? cap : b;
}
// Is grid x block a launch that runs whole?  An empty grid is (nothing to do); otherwise fewer than 2^31 workgroups and fewer
// than 2^32 work items.  The bound is the conservative one: where exactly the runtime starts to drop work was not measured.
static inline bool snk_launch_shape_ok(uint64_t grid, uint32_t block) {
    return grid == 0 || (grid <= 0x7FFFFFFFull && grid * block < (1ull << 32));
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// Launch kernel(args...) on a 1-D grid.  grid == 0 means no items: success, nothing launched.  A shape that would lose work is
// hipErrorInvalidConfiguration; otherwise the launch's own error.  Drops into SNK_HIP_TRY and its local variants, whose message
// names the kernel (the expression), file and line.
template <typename Kernel, typename... Args>
static inline hipError_t snk_launch(Kernel kernel, uint64_t grid, uint32_t block, size_t lds_bytes, hipStream_t stream, Args... args) {
    if (grid == 0) return hipSuccess;
    if (!snk_launch_shape_ok(grid, block)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(block), lds_bytes, stream, args...);
    return hipGetLastError();
}
#endif
