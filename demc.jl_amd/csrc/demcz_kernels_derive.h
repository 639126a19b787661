// demcz_kernels_derive.h -- derived quantities (demcz_derive, include/demcz.h): m user-written functions of every draw of a
// history window, written out as an N x m x w history of their own.
//
// The library includes this header for the launch constants only.  The kernel is compiled at run time, in a unit of its own
// (demcz_program.hip, compose: UNIT_DERIVE) that defines DEMCZ_DERIVE_UNIT, DEMCZ_D, DEMCZ_M and, in front of this header,
// the user's
//     __device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out);
// Nothing else of the library is in that unit: no window kernel, no Philox, no target.
#pragma once

#include <stdint.h>

namespace demcz {

constexpr int DERIVE_THREADS = 256;      // lanes (= draws in flight) per workgroup
constexpr int DERIVE_MAX_WG = 2048;      // workgroups of a launch at the most: 256 CUs x 8; the draws beyond them are strided over
constexpr int DERIVE_MAX_M = 32;         // derived quantities per draw at the most

}  // namespace demcz

#ifdef DEMCZ_DERIVE_UNIT
namespace demcz {

// One lane per draw, draws numbered i = c + N*t over the window's `total` = N*w draws (c: chain, t: generation of the window,
// history slot s0 + t).  The 64 lanes of a wave read 64 consecutive chains of one parameter column -- 512 contiguous bytes, or
// two runs where the wave crosses from one generation into the next -- and write their outputs the same way.  x and o are
// indexed by unrolled compile-time loops only and live in registers.  A draw is read once and written once: (d + 1 + m) * 8
// bytes, nothing shared between lanes, nothing kept.
//   chain   N x DEMCZ_D x Gcap  history of the source handle        logobj  N x Gcap, or nullptr: logp is NaN
//   out     N x DEMCZ_M x w     the derived history
// (i, c, t) advance by the launch's stride without a division in the loop: stride = q*N + r, so c += r, t += q, one carry.
__global__ __launch_bounds__(DERIVE_THREADS) void derive_kernel(const double* __restrict__ chain, const double* __restrict__ logobj,
                                                               int64_t N, int64_t s0, int64_t total,
                                                               const double* __restrict__ data, int64_t ndata, double* __restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * DERIVE_THREADS;
    const int64_t q = stride / N, r = stride - q * N;
    int64_t i = (int64_t)blockIdx.x * DERIVE_THREADS + threadIdx.x;
    int64_t t = i / N, c = i - t * N;
    for (; i < total; i += stride) {
        const int64_t slot = s0 + t;
        const double* src = chain + c + N * DEMCZ_D * slot;
        double x[DEMCZ_D], o[DEMCZ_M];
#pragma unroll
        for (int p = 0; p < DEMCZ_D; ++p) x[p] = src[N * p];
        const double logp = logobj ? logobj[c + N * slot] : __builtin_nan("");
#pragma unroll
        for (int k = 0; k < DEMCZ_M; ++k) o[k] = __builtin_nan("");
        demcz_derive(x, logp, data, ndata, o);
        double* dst = out + c + N * DEMCZ_M * t;
#pragma unroll
        for (int k = 0; k < DEMCZ_M; ++k) dst[N * k] = o[k];
        c += r;
        t += q;
        if (c >= N) { c -= N; t += 1; }
    }
}

}  // namespace demcz
#endif
