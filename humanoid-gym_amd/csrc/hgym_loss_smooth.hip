// hgym_loss_smooth.hip -- ppo_loss_smooth_kernel<T> (hgym_loss.hpp): the layer-by-layer path's loss head with the smoothness regulariser
// (hgym_ppo_grad_smooth), fp32 and bf16, in a device code object of its own.  Host code reaches them through launch_ppo_loss_smooth only.
#include "hgym_loss.hpp"

namespace hgym {

int32_t launch_ppo_loss_smooth(const LossArgs& a, const LossSmooth& sm, bool bf16, int nblocks, hipStream_t s) {
    if (bf16) hipLaunchKernelGGL((ppo_loss_smooth_kernel<__bf16>), dim3(nblocks), dim3(256), 0, s, a, sm);
    else hipLaunchKernelGGL((ppo_loss_smooth_kernel<float>), dim3(nblocks), dim3(256), 0, s, a, sm);
    HG_CHECK_LAUNCH("ppo_loss_smooth_kernel");
    return HGYM_OK;
}

}  // namespace hgym
