// hgym_update_act_guide.hip -- the device code object of mlp_fb_head_kernel<FbGuide, G1, XB16, GA = true> (hgym_fused.hpp): the actor's
// update tile with the frozen teacher's cloning term in its head (hgym_ppo_grad_guide), any resolved activation
// (HgymNetConfig.fused_activation).  Six kernels: first hidden width 256 / 512 / 768 x input form (fp32 rows, bf16 shadow).
#include "hgym_fused.hpp"

namespace hgym {

template int32_t launch_mlp_fb_head<true, FbGuide>(const FwdArgs&, const FbLoss&, const FbGuide&, bool, int, hipStream_t);

}  // namespace hgym
