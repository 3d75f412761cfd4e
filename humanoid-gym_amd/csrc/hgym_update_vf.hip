// hgym_update_vf.hip -- the device code object of a critic-only step (hgym_vf_grad, hgym_bc_vf_grad; hgym_loss.hpp): vf_loss_kernel, the
// layer-by-layer path's value head in both operand precisions and both value-loss forms, and vf_scalars_kernel, behind their launch
// functions.  The critic's tiles of the fused path run through the kernels they always had (hgym_update.hip and its siblings): none is here.
#include "hgym_loss.hpp"

namespace hgym {

int32_t launch_vf_loss(const VfLossArgs& a, bool bf16, bool unclipped, int nblocks, hipStream_t s) {
    if (bf16) {
        if (unclipped) hipLaunchKernelGGL((vf_loss_kernel<__bf16, true>), dim3(nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((vf_loss_kernel<__bf16, false>), dim3(nblocks), dim3(256), 0, s, a);
    } else {
        if (unclipped) hipLaunchKernelGGL((vf_loss_kernel<float, true>), dim3(nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((vf_loss_kernel<float, false>), dim3(nblocks), dim3(256), 0, s, a);
    }
    HG_CHECK_LAUNCH("vf_loss_kernel");
    return HGYM_OK;
}

int32_t launch_vf_scalars(const VfScalArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((vf_scalars_kernel<512>), dim3(1), dim3(512), 0, s, a);
    HG_CHECK_LAUNCH("vf_scalars_kernel");
    return HGYM_OK;
}

}  // namespace hgym
