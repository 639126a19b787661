// demcz_mlr_inst.inc -- body of the translation units demcz_mlr_inst_<g>.hip (MLR_GROUP = g): window_kernel_ml<LINREG_SSE, d, 16> for
// the dimensions d in 2..28 with d % 2 == g, with and without helper waves (COOP), behind mlr_kernel_g<g> (demcz_mlr_dispatch.h).
#define DEMCZ_NO_AUX_KERNELS 1
#include "demcz_kernels_ml.h"
#include "demcz_mlr_dispatch.h"

#if MLR_GROUP == 0
#define MLR_DIMS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28)
#elif MLR_GROUP == 1
#define MLR_DIMS(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) X(23) X(25) X(27)
#else
#error "MLR_GROUP must be 0 or 1"
#endif
#define MLR_CAT2(a, b) a##b
#define MLR_CAT(a, b) MLR_CAT2(a, b)

namespace demcz {

const void* MLR_CAT(mlr_kernel_g, MLR_GROUP)(int d, bool coop)
{
    switch (d) {
#if ML_LRDPP
#define MLR_CASE(DD)                                                                                                                        \
    case DD:                                                                                                                                \
        return coop ? reinterpret_cast<const void*>(&window_kernel_ml<TARGET_LINREG_SSE, DD, 16, false, false, true>)                        \
                    : reinterpret_cast<const void*>(&window_kernel_ml<TARGET_LINREG_SSE, DD, 16>);
#else       // (no helper-wave instantiations: the caller never asks for them, ml_coop)
#define MLR_CASE(DD)                                                                                                                        \
    case DD:                                                                                                                                \
        return coop ? nullptr : reinterpret_cast<const void*>(&window_kernel_ml<TARGET_LINREG_SSE, DD, 16>);
#endif
        MLR_DIMS(MLR_CASE)
#undef MLR_CASE
    }
    return nullptr;
}

}  // namespace demcz
