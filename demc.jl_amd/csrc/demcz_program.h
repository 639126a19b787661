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

// The units a program can be compiled into: each is one row of the table in demcz_program.hip, which says what the unit consists
// of.  A program target runs in the one-lane unit or, on the wave-per-chain layout (DEMCZ_LAYOUT_PROGRAM_WAVE), in the wave unit;
// the bridge unit evaluates such a target at a proposal's draws (demcz_bridge_proposal).  Derive, pointwise and predictive programs
// (demcz_derive, demcz_pointwise, demcz_predict / demcz_ppc) have a unit each.
enum { UNIT_ONE_LANE = 0, UNIT_WAVE = 1, UNIT_DERIVE = 2, UNIT_POINTWISE = 3, UNIT_BRIDGE = 4, UNIT_PREDICT = 5, UNIT_COUNT };
constexpr int WAVE_MIN_D = 2;

// The kernels of each unit: indices into Code::names and Module::fn, in the order of the unit's row.
enum {
    LANE_FULL = 0,         // window_kernel<TARGET_PROGRAM, d, true>: one block covering 0..d-1 in order
    LANE_BLOCKS,           // window_kernel<TARGET_PROGRAM, d, false>: blocks from the CSR tables
    LANE_SNOOKER,          // snooker_kernel<TARGET_PROGRAM, d> (demcz_kernels_snooker.h)
    LANE_CROSSOVER,        // window_kernel_cr<TARGET_PROGRAM, d> (demcz_kernels_crossover.h)
    LANE_LOGP,             // logp_kernel<TARGET_PROGRAM>: the initial log_objcurrent
    LANE_CROSSOVER_ADAPT   // window_kernel_cr<TARGET_PROGRAM, d, true>: the crossover generation with adapted class weights
};
enum {
    WAVE_KERNEL = 0,       // + 2 * LIVE + TEMPER: window_kernel_ps (d <= 5) / _pw<TARGET_PROGRAM, d, LIVE, TEMPER>
    WAVE_LOGP = 4          // logp_kernel<TARGET_PROGRAM>
};
enum { DERIVE_KERNEL = 0 };                        // derive_kernel
enum { POINTWISE_KERNEL = 0 };                     // pointwise_kernel
enum { BRIDGE_KERNEL = 0 };                        // bridge_proposal_program_kernel
enum { PREDICT_KERNEL = 0, PREDICT_PPC = 1 };      // predict_kernel, ppc_kernel
constexpr int MAX_KERNELS = 6;

// One compiled program: the gfx950 code object and the mangled names of its unit's kernels.
struct Code {
    std::vector<char> object;
    std::string names[MAX_KERNELS];
    int d = 0;
    int m = 0;                    // the units with DEMCZ_M: derived quantities per draw
    int unit = UNIT_ONE_LANE;
};

// A code object loaded on one device (kept until the process exits).
struct Module {
    hipModule_t module = nullptr;
    hipFunction_t fn[MAX_KERNELS] = {};
    std::shared_ptr<const Code> code;
};

// Compile `source` for dimension d into `unit` (or take it from the process-wide cache, whose key includes the unit).  Needs no
// device.  Returns 0, or 1 with the compiler log (or what else went wrong) in err.  m: UNIT_DERIVE and UNIT_PREDICT only, 1..32 (part of
// the key).
int32_t get_code(int d, const char* source, const char* options, int unit, std::shared_ptr<const Code>& out, std::string& err, int m = 0);
// Load a code object on `device` (or take it from the cache).  Returns 0, or 2 (a HIP error) with the message in err.
int32_t get_module(const std::shared_ptr<const Code>& code, int device, Module& out, std::string& err);

}  // namespace demcz_prog
