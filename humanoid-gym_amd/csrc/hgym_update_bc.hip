// hgym_update_bc.hip -- the device code object of mlp_fb_bc_kernel<G1, XB16, GA = false> (hgym_fused.hpp): the actor's update tile with
// the behaviour-cloning head (hgym_bc_grad), ELU(1).  Six kernels: first hidden width 256 / 512 / 768 x input form (fp32 rows, bf16
// shadow).  Also the small kernels of a cloning step that both paths share (hgym_loss.hpp): bc_loss_kernel, the layer-by-layer path's
// head in both operand precisions, and bc_scalars_kernel, behind their launch functions.
#include "hgym_loss.hpp"

namespace hgym {

template int32_t launch_mlp_fb_head<false, FbBC>(const FwdArgs&, const FbLoss&, const FbBC&, bool, int, hipStream_t);

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
