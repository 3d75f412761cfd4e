// hgym_update.hip -- mlp_fb_kernel (hgym_fused.hpp: the update's forward + PPO loss + dZ chain of a 64-row tile) in a translation unit,
// i.e. a device code object, of its own.  Its two instantiations are 250 KB of code; inside hgym_net.hip they put that file's code
// object at 868 KB of the 960 KiB build.py allows (a device code object beyond ~1 MiB made 8-process runs on one GPU abort at random in
// round 4: DESIGN.md section 7).  Host code reaches the kernel through launch_mlp_fb only.  This file holds the clipped value loss
// (the default); the two kernels of the unclipped form are hgym_update_vu.hip's.
#include "hgym_fused.hpp"
#include "hgym_loss.hpp"      // (the declaration of what this file defines for hgym_net.hip)

namespace hgym {

int32_t launch_mlp_fb_unclipped(const FwdArgs& fb, const FbLoss& fl, bool shadow, int tiles, int nets, size_t lds, hipStream_t s);

int32_t launch_mlp_fb(const FwdArgs& fb, const FbLoss& fl, bool shadow, bool unclipped, int tiles, int nets, size_t lds, hipStream_t s) {
    if (unclipped) return launch_mlp_fb_unclipped(fb, fl, shadow, tiles, nets, lds, s);
    return launch_mlp_fb_form<false>(fb, fl, shadow, tiles, nets, lds, s);
}

}  // namespace hgym
