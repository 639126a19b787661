// demcz_bridge_inst.hip -- the instantiations of the bridge-sampling kernels (demcz_kernels_bridge.h): bridge_posterior_kernel<D> and
// bridge_proposal_kernel<TARGET, D> of the three built-in targets for every d = 1..32, and the three kernels of the iteration.
// demcz_capi.hip launches them through the functions below and does not instantiate them.
#define DEMCZ_NO_AUX_KERNELS
#define DEMCZ_BRIDGE_INST
#include "demcz_kernels.h"
#include "demcz_kernels_bridge.h"

#include "../../include/demcz.h"

namespace demcz {

#define BRIDGE_DIMS(X)                                                                                                          \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22)   \
    X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

const void* bridge_posterior_fn(int d)
{
    switch (d) {
#define X(DD) case DD: return reinterpret_cast<const void*>(&bridge_posterior_kernel<DD>);
        BRIDGE_DIMS(X)
#undef X
    default: return nullptr;
    }
}

template <int T>
static const void* proposal_of(int d)
{
    switch (d) {
#define X(DD) case DD: return reinterpret_cast<const void*>(&bridge_proposal_kernel<T, DD>);
        BRIDGE_DIMS(X)
#undef X
    default: return nullptr;
    }
}

const void* bridge_proposal_fn(int target_kind, int d)
{
    switch (target_kind) {
    case DEMCZ_TARGET_MVNORMAL: return proposal_of<TARGET_MVNORMAL>(d);
    case DEMCZ_TARGET_ISO_QUAD: return proposal_of<TARGET_ISO_QUAD>(d);
    case DEMCZ_TARGET_LINREG_SSE: return proposal_of<TARGET_LINREG_SSE>(d);
    default: return nullptr;
    }
}

const void* bridge_rho0_fn() { return reinterpret_cast<const void*>(&bridge_rho0_kernel); }
const void* bridge_sum_fn() { return reinterpret_cast<const void*>(&bridge_sum_kernel); }
const void* bridge_finish_fn() { return reinterpret_cast<const void*>(&bridge_finish_kernel); }

}  // namespace demcz
