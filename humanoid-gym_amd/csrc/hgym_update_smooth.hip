// hgym_update_smooth.hip -- mlp_fb_smooth_kernel<.., GA = false> (hgym_fused.hpp): the ACTOR's update tile with the smoothness regulariser
// in its head (hgym_ppo_grad_smooth), ELU(1), in a device code object of its own: six kernels, one per first hidden width (256 / 512 /
// 768) and input form (fp32 rows, bf16 shadow).  The value-loss form does not enter -- it is the critic's, whose tiles (and the auxiliary
// head's) run through hgym_update.hip / hgym_update_vu.hip's kernels as ever.  The generic-activation kernels are
// hgym_update_act_smooth.hip's.  Host code reaches them through launch_mlp_fb_smooth only.
#include "hgym_fused.hpp"

namespace hgym {

int32_t launch_mlp_fb_smooth(const FwdArgs& fb, const FbLoss& fl, const FbSmooth& sm, bool shadow, int tiles, hipStream_t s) {
    return launch_mlp_fb_smooth_form<false>(fb, fl, sm, shadow, tiles, s);
}

}  // namespace hgym
