// hgym_loss_mirror.hip -- ppo_loss_kernel<T, VU, ML = true> (hgym_loss.hpp): the layer-by-layer path's loss head with the mirror loss of
// left-right symmetry (HgymPPOConfig.mirror_coef > 0), fp32 and bf16, clipped and unclipped value loss, in a device code object of its
// own.  Host code reaches them through launch_ppo_loss_mirror only.
#include "hgym_loss.hpp"

namespace hgym {

int32_t launch_ppo_loss_mirror(const LossArgs& a, bool bf16, bool unclipped, int nblocks, hipStream_t s) {
    if (bf16) {
        if (unclipped) hipLaunchKernelGGL((ppo_loss_kernel<__bf16, true, true>), dim3(nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((ppo_loss_kernel<__bf16, false, true>), dim3(nblocks), dim3(256), 0, s, a);
    } else {
        if (unclipped) hipLaunchKernelGGL((ppo_loss_kernel<float, true, true>), dim3(nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((ppo_loss_kernel<float, false, true>), dim3(nblocks), dim3(256), 0, s, a);
    }
    HG_CHECK_LAUNCH("ppo_loss_kernel<mirror>");
    return HGYM_OK;
}

}  // namespace hgym
