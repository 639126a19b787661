// demcz_snooker_inst.hip -- the built-in instantiations of snooker_kernel (demcz_kernels_snooker.h): the dimensions the one-lane
// dispatch specialises, and the run-time-d form for every other d <= MAX_D.  demcz_capi.hip launches them through
// snooker_kernel_fn and does not instantiate them.
#define DEMCZ_NO_AUX_KERNELS
#include "demcz_kernels_snooker.h"

#include "../../include/demcz.h"

namespace demcz {

#define SNK(T, DD) case DD: return reinterpret_cast<const void*>(&snooker_kernel<T, DD>);
#define SNK_GENERIC(T)                                                          \
    default:                                                                    \
        *dyn_lds = (size_t)(2 * d) * WINDOW_BS * sizeof(double);                \
        return reinterpret_cast<const void*>(&snooker_kernel_generic<T>);

const void* snooker_kernel_fn(int target_kind, int d, size_t* dyn_lds)
{
    *dyn_lds = 0;
    if (d < 2 || d > MAX_D) return nullptr;
    switch (target_kind) {
    case DEMCZ_TARGET_MVNORMAL:
        switch (d) {
        SNK(TARGET_MVNORMAL, 2) SNK(TARGET_MVNORMAL, 3) SNK(TARGET_MVNORMAL, 4) SNK(TARGET_MVNORMAL, 5) SNK(TARGET_MVNORMAL, 8)
        SNK(TARGET_MVNORMAL, 10) SNK(TARGET_MVNORMAL, 20) SNK_GENERIC(TARGET_MVNORMAL)
        }
    case DEMCZ_TARGET_ISO_QUAD:
        switch (d) { SNK(TARGET_ISO_QUAD, 10) SNK_GENERIC(TARGET_ISO_QUAD) }
    case DEMCZ_TARGET_LINREG_SSE:
        switch (d) { SNK(TARGET_LINREG_SSE, 10) SNK(TARGET_LINREG_SSE, 26) SNK_GENERIC(TARGET_LINREG_SSE) }
    default: return nullptr;
    }
}
#undef SNK
#undef SNK_GENERIC

}  // namespace demcz
