// demcz_pw_dispatch.h -- window_kernel_pw (demcz_kernels_pw.h) is instantiated for every dimension from 6 to 32, both targets it
// evaluates, six forms each: 324 kernels.  They live in eight translation units of their own (demcz_pw_inst_<g>.hip, dimension d
// in unit d % 8; compiled in parallel by demc.jl_amd/_lib.py) behind the function below, which hands out their host symbols;
// demcz_capi.hip launches them and knows nothing of the template.
#pragma once

#include "demcz_kernels.h"

namespace demcz {

constexpr int PW_GROUPS = 8;
constexpr int PW_D_MIN = 6, PW_D_MAX = 32;
enum { PW_FORM_GENERAL = 0, PW_FORM_REGULAR = 1, PW_FORM_MATRIX = 2 };
// the host symbol of window_kernel_pw<target, d, live, temper, form> (for hipLaunchKernel and the attribute / occupancy queries: a
// stub's address taken in one translation unit of the library is valid in every other), nullptr where it is not built
#define DEMCZ_PW_DECL(g) const void* pw_kernel_g##g(int target, int d, bool live, bool temper, int form);
DEMCZ_PW_DECL(0) DEMCZ_PW_DECL(1) DEMCZ_PW_DECL(2) DEMCZ_PW_DECL(3) DEMCZ_PW_DECL(4) DEMCZ_PW_DECL(5) DEMCZ_PW_DECL(6) DEMCZ_PW_DECL(7)
#undef DEMCZ_PW_DECL

inline const void* pw_kernel(int target, int d, bool live, bool temper, int form)
{
    if (d < PW_D_MIN || d > PW_D_MAX) return nullptr;
    switch (d % PW_GROUPS) {
    case 0: return pw_kernel_g0(target, d, live, temper, form);
    case 1: return pw_kernel_g1(target, d, live, temper, form);
    case 2: return pw_kernel_g2(target, d, live, temper, form);
    case 3: return pw_kernel_g3(target, d, live, temper, form);
    case 4: return pw_kernel_g4(target, d, live, temper, form);
    case 5: return pw_kernel_g5(target, d, live, temper, form);
    case 6: return pw_kernel_g6(target, d, live, temper, form);
    default: return pw_kernel_g7(target, d, live, temper, form);
    }
}

}  // namespace demcz
