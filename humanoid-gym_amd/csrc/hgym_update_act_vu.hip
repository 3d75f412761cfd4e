// hgym_update_act_vu.hip -- mlp_fb_act_kernel<.., VU = true>: the update tile with any resolved activation and the unclipped value loss
// (R - V)^2 (HgymPPOConfig.value_loss_unclipped), in a device code object of its own beside hgym_update_act.hip's clipped kernels.
#include "hgym_fused.hpp"

namespace hgym {

int32_t launch_mlp_fb_act_unclipped(const FwdArgs& fb, const FbLoss& fl, bool shadow, int tiles, int nets, hipStream_t s, int first) {
    return launch_mlp_fb_act_form<true>(fb, fl, shadow, tiles, nets, s, first);
}

}  // namespace hgym
