// hgym_update_bc.hip -- mlp_fb_bc_kernel<.., GA = false> (hgym_fused.hpp): the ACTOR's update tile with the behaviour-cloning head
// (hgym_bc_grad), ELU(1), in a device code object of its own: six kernels, one per first hidden width (256 / 512 / 768) and input form
// (fp32 rows, bf16 shadow).  Also the small kernels of a cloning step that both paths share (hgym_loss.hpp): bc_loss_kernel, the
// layer-by-layer path's head in both operand precisions, and bc_scalars_kernel.  The generic-activation tiles are hgym_update_act_bc.hip's.
// Host code reaches them through the three launch functions only.
#include "hgym_loss.hpp"

namespace hgym {

int32_t launch_mlp_fb_bc(const FwdArgs& fb, const FbLoss& fl, const FbBC& bc, bool shadow, int tiles, hipStream_t s) {
    return launch_mlp_fb_bc_form<false>(fb, fl, bc, shadow, tiles, s);
}

int32_t launch_bc_loss(const BcLossArgs& a, bool bf16, int nblocks, hipStream_t s) {
    if (bf16) hipLaunchKernelGGL((bc_loss_kernel<__bf16>), dim3(nblocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((bc_loss_kernel<float>), dim3(nblocks), dim3(256), 0, s, a);
    HG_CHECK_LAUNCH("bc_loss_kernel");
    return HGYM_OK;
}

int32_t launch_bc_scalars(const BcScalArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((bc_scalars_kernel<512>), dim3(1), dim3(512), 0, s, a);
    HG_CHECK_LAUNCH("bc_scalars_kernel");
    return HGYM_OK;
}

}  // namespace hgym
