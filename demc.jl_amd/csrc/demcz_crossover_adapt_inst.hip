// demcz_crossover_adapt_inst.hip -- the ADAPT twins of the built-in instantiations of window_kernel_cr (demcz_kernels_crossover.h,
// demcz_crossover_inst.hip): the kernels a handle with demcz_set_crossover_adapt runs for life, and cr_adapt_kernel, the update of
// the weights.  demcz_capi.hip launches them through crossover_kernel_fn(..., adapt = true) and crossover_adapt_update_fn.
#define DEMCZ_NO_AUX_KERNELS
#include "demcz_kernels_crossover.h"

#include "../../include/demcz.h"

namespace demcz {

#define CRK(T, DD)                                                                                                              \
    case DD:                                                                                                                    \
        return reinterpret_cast<const void*>(                                                                                   \
            static_cast<void (*)(const WindowParams, const CrossoverParams, const CrossoverAdaptParams)>(&window_kernel_cr<T, DD, true, CrossoverAdaptParams>));
#define CRK_GENERIC(T)                                                                                                          \
    default:                                                                                                                    \
        *dyn_lds = (size_t)(2 * d) * WINDOW_BS * sizeof(double);                                                                \
        return reinterpret_cast<const void*>(                                                                                   \
            static_cast<void (*)(const WindowParams, const CrossoverParams, const CrossoverAdaptParams)>(&window_kernel_cr_generic<T, true, CrossoverAdaptParams>));

const void* crossover_adapt_kernel_fn(int target_kind, int d, size_t* dyn_lds)
{
    *dyn_lds = 0;
    if (d < 2 || d > MAX_D) return nullptr;
    switch (target_kind) {
    case DEMCZ_TARGET_MVNORMAL:
        switch (d) {
        CRK(TARGET_MVNORMAL, 2) CRK(TARGET_MVNORMAL, 3) CRK(TARGET_MVNORMAL, 4) CRK(TARGET_MVNORMAL, 5) CRK(TARGET_MVNORMAL, 8)
        CRK(TARGET_MVNORMAL, 10) CRK(TARGET_MVNORMAL, 20) CRK_GENERIC(TARGET_MVNORMAL)
        }
    case DEMCZ_TARGET_ISO_QUAD:
        switch (d) { CRK(TARGET_ISO_QUAD, 10) CRK_GENERIC(TARGET_ISO_QUAD) }
    case DEMCZ_TARGET_LINREG_SSE:
        switch (d) { CRK(TARGET_LINREG_SSE, 10) CRK(TARGET_LINREG_SSE, 26) CRK_GENERIC(TARGET_LINREG_SSE) }
    default: return nullptr;
    }
}
#undef CRK
#undef CRK_GENERIC

const void* crossover_adapt_update_fn() { return reinterpret_cast<const void*>(&cr_adapt_kernel<64>); }

}  // namespace demcz
