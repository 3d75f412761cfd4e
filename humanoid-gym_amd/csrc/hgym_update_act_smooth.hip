// hgym_update_act_smooth.hip -- mlp_fb_smooth_kernel<.., GA = true> (hgym_fused.hpp): the actor's update tile with the smoothness
// regulariser in its head and any resolved activation (HgymNetConfig.fused_activation), in a device code object of its own beside
// hgym_update_smooth.hip's ELU(1) kernels.  Host code reaches them through launch_mlp_fb_act_smooth only.
#include "hgym_fused.hpp"

namespace hgym {

int32_t launch_mlp_fb_act_smooth(const FwdArgs& fb, const FbLoss& fl, const FbSmooth& sm, bool shadow, int tiles, hipStream_t s) {
    return launch_mlp_fb_smooth_form<true>(fb, fl, sm, shadow, tiles, s);
}

}  // namespace hgym
