// demcz_pw_inst.inc -- body of the translation units demcz_pw_inst_<g>.hip (PW_GROUP = g): window_kernel_pw for the dimensions
// d in 6..32 with d % 8 == g, MvNormal and the isotropic quadratic, in its six forms (LIVE x tempered, general and regular
// launches; d = 20, MvNormal: the matrix form too), behind pw_kernel_g<g> (demcz_pw_dispatch.h).
#define DEMCZ_NO_AUX_KERNELS 1
#include "demcz_kernels_pw.h"
#include "demcz_pw_dispatch.h"

#if PW_GROUP == 0
#define PW_DIMS(X) X(8) X(16) X(24) X(32)
#elif PW_GROUP == 1
#define PW_DIMS(X) X(9) X(17) X(25)
#elif PW_GROUP == 2
#define PW_DIMS(X) X(10) X(18) X(26)
#elif PW_GROUP == 3
#define PW_DIMS(X) X(11) X(19) X(27)
#elif PW_GROUP == 4
#define PW_DIMS(X) X(12) X(20) X(28)
#elif PW_GROUP == 5
#define PW_DIMS(X) X(13) X(21) X(29)
#elif PW_GROUP == 6
#define PW_DIMS(X) X(6) X(14) X(22) X(30)
#elif PW_GROUP == 7
#define PW_DIMS(X) X(7) X(15) X(23) X(31)
#else
#error "PW_GROUP must be 0..7"
#endif
#define PW_CAT2(a, b) a##b
#define PW_CAT(a, b) PW_CAT2(a, b)

namespace demcz {
namespace {

// the kernel of (LIVE, tempered, form), nullptr where that form is not built: the matrix form exists at d = 20, MvNormal, and it and
// the regular form only as LIVE kernels
template <int TARGET, int D>
const void* kernel_td(bool live, bool temper, int form)
{
#define PW_FN(...) reinterpret_cast<const void*>(&window_kernel_pw<TARGET, D, __VA_ARGS__>)
    if (form == PW_FORM_MATRIX) {
        if constexpr (D == 20 && TARGET == TARGET_MVNORMAL) {
            if (!live) return nullptr;
            return temper ? PW_FN(true, true, true) : PW_FN(true, false, true);
        } else {
            return nullptr;
        }
    }
    if (form == PW_FORM_REGULAR) {
        if (!live) return nullptr;
        return temper ? PW_FN(true, true, false, true) : PW_FN(true, false, false, true);
    }
    if (temper) return live ? PW_FN(true, true) : PW_FN(false, true);
    return live ? PW_FN(true, false) : PW_FN(false, false);
#undef PW_FN
}

}  // namespace

const void* PW_CAT(pw_kernel_g, PW_GROUP)(int target, int d, bool live, bool temper, int form)
{
#define PW_CASE(DD)                                                                                                     \
    case DD:                                                                                                            \
        return (target == TARGET_MVNORMAL) ? kernel_td<TARGET_MVNORMAL, DD>(live, temper, form)                        \
               : (target == TARGET_ISO_QUAD) ? kernel_td<TARGET_ISO_QUAD, DD>(live, temper, form) : nullptr;
    switch (d) {
        PW_DIMS(PW_CASE)
    default: return nullptr;
    }
#undef PW_CASE
}

}  // namespace demcz
