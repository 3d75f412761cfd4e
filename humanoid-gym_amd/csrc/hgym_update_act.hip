// hgym_update_act.hip -- mlp_fb_act_kernel (hgym_fused.hpp): the update's tile with any resolved activation (HgymNetConfig.fused_activation),
// clipped value loss, in a device code object of its own beside hgym_update.hip's ELU(1) kernels: eight kernels, one per tile body
// (first hidden width 256 / 512 / 768, the auxiliary head) and input form (fp32 rows, bf16 shadow).  The unclipped form is
// hgym_update_act_vu.hip's.  Host code reaches them through launch_mlp_fb_act only.
#include "hgym_fused.hpp"
#include "hgym_loss.hpp"      // (the declaration of what this file defines for hgym_net.hip)

namespace hgym {

int32_t launch_mlp_fb_act_unclipped(const FwdArgs& fb, const FbLoss& fl, bool shadow, int tiles, int nets, hipStream_t s, int first);

// first: the first net launched (0; 1 when the actor's tiles carry the mirror loss -- hgym_update_act_mirror.hip launches those)
int32_t launch_mlp_fb_act(const FwdArgs& fb, const FbLoss& fl, bool shadow, bool unclipped, int tiles, int nets, hipStream_t s, int first) {
    if (unclipped) return launch_mlp_fb_act_unclipped(fb, fl, shadow, tiles, nets, s, first);
    return launch_mlp_fb_act_form<false>(fb, fl, shadow, tiles, nets, s, first);
}

}  // namespace hgym
