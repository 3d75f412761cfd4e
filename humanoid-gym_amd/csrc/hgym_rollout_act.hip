// hgym_rollout_act.hip -- rollout_step_act_kernel (hgym_rollout.hpp): the one-launch rollout / evaluation step with any resolved activation
// (HgymNetConfig.fused_activation), in a device code object of its own beside hgym_rollout.hip's ELU(1) kernels; built with
// -ffp-contract=off like that file (the env arithmetic), hgym_fused.hpp restores the policy tiles' own setting for its part.
// The forms WITHOUT critic tiles only (values = NULL: the critic once over the stored rows, hgym_critic_values; the evaluation step): with
// the generic epilogues of an actor AND a critic tile the inline forms measure 131 856 .. 140 792 bytes of code, beyond build.py's
// 128 KiB per kernel; these are 85 016 .. 92 816.
#define HGYM_TU_CONTRACT_OFF 1
#include "hgym_rollout.hpp"

namespace hgym {

template <bool FIN, bool EVAL>
static int32_t launch_form(dim3 grid, size_t lds, hipStream_t s, const FwdArgs& f, const EnvArgs& e, const FinArgs& fin, const RolloutPP& pp) {
    const int32_t rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&rollout_step_act_kernel<FIN, EVAL>), lds,
                                          "rollout_step_act_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL((rollout_step_act_kernel<FIN, EVAL>), grid, dim3(RO_NT), lds, s, f, e, fin, pp);
    return HGYM_OK;
}

int32_t launch_rollout_step_act(int form, dim3 grid, size_t lds, hipStream_t s, const FwdArgs& f, const EnvArgs& e, const FinArgs& fin,
                                const RolloutPP& pp) {
    switch (form) {
        case RO_NOCRITIC_FIRST: return launch_form<false, false>(grid, lds, s, f, e, fin, pp);
        case RO_NOCRITIC_NEXT: return launch_form<true, false>(grid, lds, s, f, e, fin, pp);
        case RO_EVAL: return launch_form<true, true>(grid, lds, s, f, e, fin, pp);
    }
    HG_FAIL(HGYM_E_BADARG, "rollout form %d", form);
}

}  // namespace hgym
