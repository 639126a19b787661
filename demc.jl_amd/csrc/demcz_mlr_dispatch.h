// demcz_mlr_dispatch.h -- window_kernel_ml<LINREG_SSE, d, 16> (demcz_kernels_ml.h: the regression target on sixteen lanes per chain,
// with and without its helper waves) is instantiated for every dimension from 2 to 28: 54 kernels.  They live in two translation
// units of their own (demcz_mlr_inst_<g>.hip, dimension d in unit d % 2; compiled in parallel by demc.jl_amd/_lib.py) behind the
// function below, which hands out their host symbols; demcz_capi.hip launches them and does not instantiate them.
#pragma once

#include "demcz_kernels.h"

namespace demcz {

constexpr int MLR_D_MIN = 2, MLR_D_MAX = 28;

// the host symbol of the kernel for dimension d, nullptr where it is not built.  coop: a workgroup is one chain wave (four chains)
// + its helper waves (64 * ML_COOP_WAVES threads); otherwise it is one to ML_WAVES chain waves.
const void* mlr_kernel_g0(int d, bool coop);
const void* mlr_kernel_g1(int d, bool coop);

inline const void* mlr_kernel(int d, bool coop)
{
    if (d < MLR_D_MIN || d > MLR_D_MAX) return nullptr;
    return (d % 2 == 0) ? mlr_kernel_g0(d, coop) : mlr_kernel_g1(d, coop);
}

}  // namespace demcz
