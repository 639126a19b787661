// demcz_kernels_pointwise.h -- pointwise log-likelihoods (demcz_pointwise, include/demcz.h): the user's log-likelihood of
// observations obs_from .. obs_from + mc - 1 at every draw of a history window, written out as an N x mc x w history of its own
// -- the input of demcz_loo_columns (demcz_kernels_loo.h).
//
// The library itself does not compile this header (the launch constants are demcz_kernels_derive.h's); it embeds its text.  The
// kernel is compiled at run time, in a unit of its own (demcz_program.hip, compose: UNIT_POINTWISE) that defines
// DEMCZ_POINTWISE_UNIT, DEMCZ_D and, in front of this header, the user's
//     __device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i);
// Nothing else of the library is in that unit.  mc is a run-time argument: one compiled unit serves every chunk of observations.
#pragma once

#include <stdint.h>

#include "demcz_kernels_derive.h"

#ifdef DEMCZ_POINTWISE_UNIT
namespace demcz {

// derive_kernel's stream: one lane per draw, draws numbered i = c + N*t over the window's `total` = N*w draws, (i, c, t) advanced
// by the launch's stride without a division in the loop, 64-bit index arithmetic.  A lane loads its x ONCE, by the unrolled
// compile-time loop, into registers, then walks the chunk's observations: the bounds obs_from and mc are the same in every lane,
// so a likelihood that reads data[i*k + ...] reads one address per wave.  Each result goes straight to
// out[c + N*k + N*mc*t]: there is no array of results, nothing to send to scratch memory.
//   chain   N x DEMCZ_D x Gcap  history of the source handle
//   out     N x mc x w          the log-likelihoods; k < mc, t < w under the lane's own predicate i < total
__global__ __launch_bounds__(DERIVE_THREADS) void pointwise_kernel(const double* __restrict__ chain, int64_t N, int64_t s0, int64_t total,
                                                                  const double* __restrict__ data, int64_t ndata, int64_t obs_from,
                                                                  int mc, double* __restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * DERIVE_THREADS;
    const int64_t q = stride / N, r = stride - q * N;
    int64_t i = (int64_t)blockIdx.x * DERIVE_THREADS + threadIdx.x;
    int64_t t = i / N, c = i - t * N;
    for (; i < total; i += stride) {
        const double* src = chain + c + N * DEMCZ_D * (s0 + t);
        double x[DEMCZ_D];
#pragma unroll
        for (int p = 0; p < DEMCZ_D; ++p) x[p] = src[N * p];
        double* dst = out + c + N * mc * t;
        for (int k = 0; k < mc; ++k) dst[N * k] = demcz_loglik(x, data, ndata, obs_from + k);
        c += r;
        t += q;
        if (c >= N) { c -= N; t += 1; }
    }
}

}  // namespace demcz
#endif
