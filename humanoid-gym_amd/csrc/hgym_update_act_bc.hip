// hgym_update_act_bc.hip -- mlp_fb_bc_kernel<.., GA = true> (hgym_fused.hpp): the actor's update tile with the behaviour-cloning head
// (hgym_bc_grad) and any resolved activation (HgymNetConfig.fused_activation), in a device code object of its own beside
// hgym_update_bc.hip's ELU(1) kernels.  Host code reaches them through launch_mlp_fb_act_bc only.
#include "hgym_fused.hpp"

namespace hgym {

int32_t launch_mlp_fb_act_bc(const FwdArgs& fb, const FbLoss& fl, const FbBC& bc, bool shadow, int tiles, hipStream_t s) {
    return launch_mlp_fb_bc_form<true>(fb, fl, bc, shadow, tiles, s);
}

}  // namespace hgym
