// demcz_program.h -- host-side interface of demcz_program.hip (program targets, DEMCZ_TARGET_PROGRAM) for demcz_capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

namespace demcz_prog {

constexpr int MAX_PROGRAM_D = 32;

// One compiled program: the gfx950 code object and the mangled names of its three kernels.
struct Code {
    std::vector<char> object;
    std::string window_full;      // window_kernel<TARGET_PROGRAM, d, true>: one block covering 0..d-1 in order
    std::string window_blocks;    // window_kernel<TARGET_PROGRAM, d, false>: blocks from the CSR tables
    std::string logp;             // logp_kernel<TARGET_PROGRAM>: the initial log_objcurrent
    int d = 0;
};

// A code object loaded on one device (kept until the process exits).
struct Module {
    hipModule_t module = nullptr;
    hipFunction_t window_full = nullptr, window_blocks = nullptr, logp = nullptr;
    std::shared_ptr<const Code> code;
};

// Compile `source` for dimension d (or take it from the process-wide cache).  Needs no device.  Returns 0, or 1 with the
// compiler log (or what else went wrong) in err.
int32_t get_code(int d, const char* source, const char* options, std::shared_ptr<const Code>& out, std::string& err);
// Load a code object on `device` (or take it from the cache).  Returns 0, or 2 (a HIP error) with the message in err.
int32_t get_module(const std::shared_ptr<const Code>& code, int device, Module& out, std::string& err);

}  // namespace demcz_prog
