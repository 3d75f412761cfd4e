// hgym_fill.hip -- zero_f32_async (hgym_common.hpp): n floats to +0.0 by a launch, for any translation unit of the library.
//
// A translation unit of its own, so that no existing device code object changes.  hgym_bc_grad clears its gradient vector with it.  That
// clear was one hipMemsetAsync until a cloning step first ran inside a captured update (the RND predictor's; DESIGN.md section 27 records
// what was observed): a launch replays as every other launch of the update does.
#include "hgym_common.hpp"

namespace hgym {

constexpr int FILL_THREADS = 256;
constexpr int64_t FILL_MAX_BLOCKS = 1024;      // workgroups walk the range with this stride beyond it

__global__ __launch_bounds__(FILL_THREADS) void zero_f32_kernel(int64_t n, float* __restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FILL_THREADS) x[i] = 0.0f;
}

int32_t zero_f32_async(float* x, int64_t n, hipStream_t stream) {
    HG_REQUIRE(x && n >= 1, HGYM_E_BADARG, "zero_f32_async: x=%p n=%lld", (void*)x, (long long)n);
    const int64_t blocks = (n + FILL_THREADS - 1) / FILL_THREADS;
    hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)(blocks < FILL_MAX_BLOCKS ? blocks : FILL_MAX_BLOCKS)), dim3(FILL_THREADS), 0, stream, n, x);
    HG_CHECK_LAUNCH("zero_f32_kernel");
    return HGYM_OK;
}

}  // namespace hgym
