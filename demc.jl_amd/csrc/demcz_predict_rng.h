// demcz_predict_rng.h -- the random stream of one draw, as a predictive program sees it (demcz_predict, include/demcz.h; DESIGN.md
// section 3, "the random stream of a draw").  Part of the predict unit only (demcz_program.hip, compose: UNIT_PREDICT), behind
// demcz_device.h and in front of the user's source; global namespace, so that the program writes demcz_normal(rng).
//
// The draw of global chain c at generation g owns the Philox4x32-10 stream of key `seed` and subsequence S = (g << 32) | c: block b
// is the ten rounds on the counter {b lo, b hi, c, g} -- rocRAND's layout, rng_seek(st, seed, S, 0) followed by b + 1 calls of
// rng_next.  Nothing of rocRAND's 16-word state is kept: the state is b, (c, g), the key, one spare word, one spare normal and the
// two flags that say whether they are held.
#pragma once

#include <stdint.h>

#pragma clang fp contract(off)

struct demcz_rng {
    uint64_t b;              // the next block of the stream
    uint32_t c, g;           // S = (g << 32) | c
    uint32_t k0, k1;         // seed, low and high word (the same in every lane)
    uint64_t spare_word;     // r2 of the block demcz_uniform took last, where has_word
    double spare_normal;     // z1 of the pair demcz_normal made last, where has_normal
    bool has_word, has_normal;
};

__device__ __forceinline__ void demcz_rng_seed(demcz_rng* rng, uint64_t seed, uint32_t g, uint32_t c)
{
    rng->b = 0;
    rng->c = c;
    rng->g = g;
    rng->k0 = (uint32_t)seed;
    rng->k1 = (uint32_t)(seed >> 32);
    rng->spare_word = 0;
    rng->spare_normal = 0.0;
    rng->has_word = false;
    rng->has_normal = false;
}

// Block b of the stream as two 64-bit words (little-endian pairs of the four output words), then b += 1.  Touches no spare.
__device__ __forceinline__ void demcz_bits(demcz_rng* rng, uint64_t* r1, uint64_t* r2)
{
    uint32_t c0 = (uint32_t)rng->b, c1 = (uint32_t)(rng->b >> 32), c2 = rng->c, c3 = rng->g;
    uint32_t k0 = rng->k0, k1 = rng->k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    *r1 = (uint64_t)c0 | ((uint64_t)c1 << 32);
    *r2 = (uint64_t)c2 | ((uint64_t)c3 << 32);
    rng->b += 1;
}

// A uniform in (0, 1): u_open of the held spare word if there is one, else of r1 of a fresh block, whose r2 is held.
__device__ __forceinline__ double demcz_uniform(demcz_rng* rng)
{
    if (rng->has_word) {
        rng->has_word = false;
        return demcz::u_open(rng->spare_word);
    }
    uint64_t r1, r2;
    demcz_bits(rng, &r1, &r2);
    rng->spare_word = r2;
    rng->has_word = true;
    return demcz::u_open(r1);
}

// A standard normal: the held spare if there is one, else z0 of the Box-Muller pair of a fresh block, whose z1 is held.
__device__ __forceinline__ double demcz_normal(demcz_rng* rng)
{
    if (rng->has_normal) {
        rng->has_normal = false;
        return rng->spare_normal;
    }
    uint64_t r1, r2;
    demcz_bits(rng, &r1, &r2);
    double z0, z1;
    demcz::normal_pair(r1, r2, z0, z1);
    rng->spare_normal = z1;
    rng->has_normal = true;
    return z0;
}

// A standard exponential
__device__ __forceinline__ double demcz_exponential(demcz_rng* rng)
{
    return -demcz::dm_log(demcz_uniform(rng));
}
