// hgym_update_act_mirror.hip -- mlp_fb_mirror_kernel<.., GA = true> (hgym_fused.hpp): the actor's update tile with the mirror loss in its
// head and any resolved activation (HgymNetConfig.fused_activation), in a device code object of its own beside hgym_update_mirror.hip's
// ELU(1) kernels.  Host code reaches them through launch_mlp_fb_act_mirror only.
#include "hgym_fused.hpp"

namespace hgym {

int32_t launch_mlp_fb_act_mirror(const FwdArgs& fb, const FbLoss& fl, const FbMirror& mr, bool shadow, int tiles, hipStream_t s) {
    return launch_mlp_fb_mirror_form<true>(fb, fl, mr, shadow, tiles, s);
}

}  // namespace hgym
