// hgym_fwd_act.hip -- mlp_fwd_act_kernel (hgym_fused.hpp): the fused forward with any resolved activation
// (HgymNetConfig.fused_activation), in a device code object of its own: eight kernels, one per tile shape (32 rows x 8 wavefronts,
// 64 rows x 16) and tile body (first hidden width 256 / 512 / 768, the auxiliary head's wide head).  Host code reaches them through
// launch_mlp_fwd_act only.
#include "hgym_fused.hpp"
#include "hgym_loss.hpp"      // (the declaration of what this file defines for hgym_net.hip)

namespace hgym {

template <int BM, int NW, int D, int G1U, bool WIDE>
static int32_t launch_one(const FwdArgs& a, int tiles, size_t lds, hipStream_t s) {
    const int32_t rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&mlp_fwd_act_kernel<BM, NW, D, G1U, WIDE>), lds, "mlp_fwd_act_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL((mlp_fwd_act_kernel<BM, NW, D, G1U, WIDE>), dim3(tiles), dim3(NW * 64), lds, s, a);
    return HGYM_OK;
}

template <int BM, int NW, int D>
static int32_t launch_net(const FwdArgs& a, hipStream_t s) {
    const FusedNet& n = a.net[a.net0];
    const int tiles = ceil_div(a.M, BM), g1 = n.layer[0].NB / 16;      // first hidden width 256 / 512 / 768
    const size_t lds = (size_t)fwd_lds_bytes(n, BM);
    if (n.layer[3].NB > 1) return g1 == 2 ? launch_one<BM, NW, D, 2, true>(a, tiles, lds, s) : HGYM_E_UNSUPPORTED;      // wide head: the auxiliary net
    if (g1 == 1) return launch_one<BM, NW, D, 1, false>(a, tiles, lds, s);
    if (g1 == 2) return launch_one<BM, NW, D, 2, false>(a, tiles, lds, s);
    if (g1 == 3) return launch_one<BM, NW, D, 3, false>(a, tiles, lds, s);
    return HGYM_E_UNSUPPORTED;
}

// nets [a0.net0, a0.net0 + nets) of a0, one launch each; tiles of 64 rows x 16 wavefronts (wide) or 32 rows x 8
int32_t launch_mlp_fwd_act(const FwdArgs& a0, int nets, bool wide, int64_t dbg_tiles, hipStream_t s) {
    for (int i = 0; i < nets; ++i) {
        FwdArgs a = a0;
        a.net0 = a0.net0 + i;
        a.nets = 1;
        if (a.dbg) a.dbg += (int64_t)i * dbg_tiles * 8;      // phase stamps: this net's slots
        const int32_t rc = wide ? launch_net<64, 16, 2>(a, s) : launch_net<32, 8, 4>(a, s);
        if (rc) return rc;
    }
    return HGYM_OK;
}

}  // namespace hgym
