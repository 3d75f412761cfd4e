// hgym_update_act_bc.hip -- the device code object of mlp_fb_bc_kernel<G1, XB16, GA = true> (hgym_fused.hpp): the actor's update tile
// with the behaviour-cloning head (hgym_bc_grad), any resolved activation (HgymNetConfig.fused_activation).
// Six kernels: first hidden width 256 / 512 / 768 x input form (fp32 rows, bf16 shadow).
#include "hgym_fused.hpp"

namespace hgym {

template int32_t launch_mlp_fb_head<true, FbBC>(const FwdArgs&, const FbLoss&, const FbBC&, bool, int, hipStream_t);

}  // namespace hgym
