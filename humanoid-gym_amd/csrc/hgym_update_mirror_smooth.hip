// hgym_update_mirror_smooth.hip -- the device code object of mlp_fb_head_kernel<FbMirrorSmooth, G1, XB16, GA = false> (hgym_fused.hpp): the
// actor's update tile with the mirror loss and the smoothness regulariser in one head (hgym_ppo_grad_smooth_mirror), ELU(1).
// Six kernels: first hidden width 256 / 512 / 768 x input form (fp32 rows, bf16 shadow).
#include "hgym_fused.hpp"

namespace hgym {

template int32_t launch_mlp_fb_head<false, FbMirrorSmooth>(const FwdArgs&, const FbLoss&, const FbMirrorSmooth&, bool, int, hipStream_t);

}  // namespace hgym
