// hgym_update_act_mirror.hip -- the device code object of mlp_fb_head_kernel<FbMirror, G1, XB16, GA = true> (hgym_fused.hpp): the actor's update
// tile with the mirror loss in its head (HgymPPOConfig.mirror_coef > 0), any resolved activation (HgymNetConfig.fused_activation).
// Six kernels: first hidden width 256 / 512 / 768 x input form (fp32 rows, bf16 shadow).
#include "hgym_fused.hpp"

namespace hgym {

template int32_t launch_mlp_fb_head<true, FbMirror>(const FwdArgs&, const FbLoss&, const FbMirror&, bool, int, hipStream_t);

}  // namespace hgym
