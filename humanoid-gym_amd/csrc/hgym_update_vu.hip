// hgym_update_vu.hip -- mlp_fb_kernel<shadow, VU = true>: the update tile with the unclipped value loss (R - V)^2
// (HgymPPOConfig.value_loss_unclipped), in a device code object of its own beside hgym_update.hip's clipped kernels.
#include "hgym_fused.hpp"

namespace hgym {

int32_t launch_mlp_fb_unclipped(const FwdArgs& fb, const FbLoss& fl, bool shadow, int tiles, int nets, size_t lds, hipStream_t s) {
    return launch_mlp_fb_form<true>(fb, fl, shadow, tiles, nets, lds, s);
}

}  // namespace hgym
