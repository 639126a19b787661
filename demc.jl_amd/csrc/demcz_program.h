// demcz_program.h -- host-side interface of demcz_program.hip (program targets, DEMCZ_TARGET_PROGRAM, and derive programs,
// demcz_derive) for demcz_capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "demcz_kernels_derive.h"      // (the launch constants; the kernel itself is compiled at run time only)

#include <memory>
#include <string>
#include <vector>

namespace demcz_prog {

constexpr int MAX_PROGRAM_D = 32;
constexpr int MAX_DERIVE_M = demcz::DERIVE_MAX_M;

// The two units a program can be compiled into (demcz_program.hip, compose): the one-lane window kernel, or the wave-per-chain
// consumers of the split layout (DEMCZ_LAYOUT_PROGRAM_WAVE: window_kernel_ps for d = 2..5, window_kernel_pw for d = 6..32).
// A derive program (demcz_derive, include/demcz.h) has a unit of its own: the user's demcz_derive and derive_kernel of
// demcz_kernels_derive.h, nothing else.
// A pointwise program (demcz_pointwise) likewise: the user's demcz_loglik and pointwise_kernel of demcz_kernels_pointwise.h.
// A program target's bridge unit (demcz_bridge_proposal): the user's demcz_logobj and bridge_proposal_program_kernel of
// demcz_kernels_bridge.h.
// A predictive program (demcz_predict, demcz_ppc): demcz_device.h, the demcz_rng of demcz_predict_rng.h, the user's demcz_predict,
// and predict_kernel and ppc_kernel of demcz_kernels_predict.h.
enum { UNIT_ONE_LANE = 0, UNIT_WAVE = 1, UNIT_DERIVE = 2, UNIT_POINTWISE = 3, UNIT_BRIDGE = 4, UNIT_PREDICT = 5 };
constexpr int WAVE_MIN_D = 2;

// One compiled program: the gfx950 code object and the mangled names of its kernels.
struct Code {
    std::vector<char> object;
    std::string window_full;      // window_kernel<TARGET_PROGRAM, d, true>: one block covering 0..d-1 in order
    std::string window_blocks;    // window_kernel<TARGET_PROGRAM, d, false>: blocks from the CSR tables
    std::string snooker;          // snooker_kernel<TARGET_PROGRAM, d> (demcz_kernels_snooker.h): one-lane unit only
    std::string crossover;        // window_kernel_cr<TARGET_PROGRAM, d> (demcz_kernels_crossover.h): one-lane unit only
    std::string logp;             // logp_kernel<TARGET_PROGRAM>: the initial log_objcurrent (both units)
    std::string wave[2][2];       // UNIT_WAVE: window_kernel_ps / _pw<TARGET_PROGRAM, d, LIVE, TEMPER>, [LIVE][TEMPER] (the one-lane
                                  // kernels are not in that unit, and these not in the one-lane unit)
    std::string derive;           // UNIT_DERIVE: derive_kernel, the only kernel of that unit; UNIT_POINTWISE: pointwise_kernel;
                                  // UNIT_BRIDGE: bridge_proposal_program_kernel; UNIT_PREDICT: predict_kernel
    std::string ppc;              // UNIT_PREDICT: ppc_kernel
    int d = 0;
    int m = 0;                    // UNIT_DERIVE, UNIT_PREDICT: derived quantities per draw (DEMCZ_M)
    int unit = UNIT_ONE_LANE;
};

// A code object loaded on one device (kept until the process exits).
struct Module {
    hipModule_t module = nullptr;
    hipFunction_t window_full = nullptr, window_blocks = nullptr, snooker = nullptr, crossover = nullptr, logp = nullptr;
    hipFunction_t wave[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    hipFunction_t derive = nullptr;   // (UNIT_POINTWISE: pointwise_kernel; UNIT_BRIDGE: bridge_proposal_program_kernel; UNIT_PREDICT: predict_kernel)
    hipFunction_t ppc = nullptr;      // UNIT_PREDICT: ppc_kernel
    std::shared_ptr<const Code> code;
};

// Compile `source` for dimension d into `unit` (or take it from the process-wide cache, whose key includes the unit).  Needs no
// device.  Returns 0, or 1 with the compiler log (or what else went wrong) in err.  m: UNIT_DERIVE and UNIT_PREDICT only, 1..32 (part of
// the key).
int32_t get_code(int d, const char* source, const char* options, int unit, std::shared_ptr<const Code>& out, std::string& err, int m = 0);
// Load a code object on `device` (or take it from the cache).  Returns 0, or 2 (a HIP error) with the message in err.
int32_t get_module(const std::shared_ptr<const Code>& code, int device, Module& out, std::string& err);

}  // namespace demcz_prog
