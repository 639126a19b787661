// demcz_program.hip -- program targets (DEMCZ_TARGET_PROGRAM): a log-density the user writes as HIP C++, compiled at run time
// with hipRTC for gfx950 together with the one-lane window kernel of demcz_kernels.h, and loaded as a module on the handle's
// device.  Host code only: the kernels of a program live in its code object, not in this library.
//
// The composed translation unit (compose):
//     #define DEMCZ_D <d> / DEMCZ_PROGRAM_TARGET / DEMCZ_NO_AUX_KERNELS, INFINITY and NAN as <math.h> has them
//     the user's source                      (#line 1 "program": compiler messages carry the user's own line numbers)
//     #include "demcz_kernels.h"             (its text and demcz_device.h's are embedded into this library at build time)
//     #include "demcz_kernels_snooker.h"     (the snooker generation's kernel: a program that cannot be built for it fails here)
//     #include "demcz_kernels_crossover.h"   (the crossover generation's kernel, in the same way)
//     explicit instantiations of window_kernel<TARGET_PROGRAM, DEMCZ_D, true / false>, snooker_kernel<TARGET_PROGRAM, DEMCZ_D>,
//     window_kernel_cr<TARGET_PROGRAM, DEMCZ_D>
//     and logp_kernel<TARGET_PROGRAM>
// The wave unit (UNIT_WAVE, handles created with DEMCZ_LAYOUT_PROGRAM_WAVE; composed and compiled only for them, cached under a
// key of its own) has the same head, then
//     #define ML_LRDPP 0 / PW_DDPP 0         (the generated DPP texts of the built-in targets are not part of the unit: the
//                                             candidate adds read their increments from LDS -- the same doubles,
//                                             tests/test_switch_variants.py -- and 54 generated files stay out of the library's
//                                             text and out of every first-use compile)
//     #include "demcz_kernels_pw.h"          (which brings _ps.h, _pc.h with the producer half, _ml.h, _rec.h, demcz_kernels.h)
//     window_kernel_ps<TARGET_PROGRAM, DEMCZ_D, LIVE, TEMPER> (d <= 5) or window_kernel_pw<TARGET_PROGRAM, DEMCZ_D, LIVE, TEMPER>,
//     LIVE and TEMPER both ways, and logp_kernel<TARGET_PROGRAM>
// The derive unit (UNIT_DERIVE, demcz_derive): #define DEMCZ_D <d> / DEMCZ_M <m> / DEMCZ_DERIVE_UNIT, INFINITY and NAN, the
// user's source (#line 1 "program"), #include "demcz_kernels_derive.h" and nothing else of the library: derive_kernel is its
// only kernel, and the unit compiles in a fraction of the time a program target takes.
// The pointwise unit (UNIT_POINTWISE, demcz_pointwise) is the derive unit with DEMCZ_POINTWISE_UNIT in place of DEMCZ_DERIVE_UNIT
// and DEMCZ_M, the user's demcz_loglik, and demcz_kernels_pointwise.h (which includes demcz_kernels_derive.h for the launch
// constants): pointwise_kernel is its only kernel.  Same options, same caches.
// The bridge unit (UNIT_BRIDGE, demcz_bridge_proposal): DEMCZ_D, DEMCZ_BRIDGE_UNIT, the user's demcz_logobj exactly as a program
// target defines it, then demcz_device.h (Philox, dm_log, the Box-Muller pair) and demcz_kernels_bridge.h, whose
// bridge_proposal_program_kernel is its only kernel.  No struct of the library's is in it.  A key of its own in the same caches.
// The predict unit (UNIT_PREDICT, demcz_predict and demcz_ppc): the derive unit's defines with DEMCZ_PREDICT_UNIT in place of
// DEMCZ_DERIVE_UNIT, demcz_device.h, demcz_predict_rng.h (the demcz_rng of a draw and its four helpers), the user's demcz_predict
// (#line 1 "program"), and demcz_kernels_predict.h with predict_kernel and ppc_kernel.  Same options, same caches, a key of its own.
// Compile options: --offload-arch=gfx950 -O3 -ffp-contract=off -I<rocm>/include, the library's own layout switches (not for
// the derive unit, which sees no struct of the library's), then the user's.  Code objects are cached per (composed text,
// options), loaded modules per (code object, device); both for the life of the process.
#include "demcz_program.h"

#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

namespace {

// The header text the library was built with (C23 #embed, accepted by hipcc as an extension)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wc23-extensions"
const char k_device_h[] = {
#embed "demcz_device.h"
    , 0};
const char k_kernels_h[] = {
#embed "demcz_kernels.h"
    , 0};
const char k_snooker_h[] = {
#embed "demcz_kernels_snooker.h"
    , 0};
const char k_crossover_h[] = {
#embed "demcz_kernels_crossover.h"
    , 0};
// the wave unit's headers
const char k_rec_h[] = {
#embed "demcz_kernels_rec.h"
    , 0};
const char k_ml_h[] = {
#embed "demcz_kernels_ml.h"
    , 0};
const char k_mlb_inc[] = {
#embed "demcz_mlb_dpp_20_5.inc"
    , 0};
const char k_pc_h[] = {
#embed "demcz_kernels_pc.h"
    , 0};
const char k_ps_h[] = {
#embed "demcz_kernels_ps.h"
    , 0};
const char k_pw_h[] = {
#embed "demcz_kernels_pw.h"
    , 0};
// the derive unit's only header
const char k_derive_h[] = {
#embed "demcz_kernels_derive.h"
    , 0};
// the pointwise unit's header (on top of the derive unit's)
const char k_pointwise_h[] = {
#embed "demcz_kernels_pointwise.h"
    , 0};
// the bridge unit's header (on top of demcz_device.h and the derive unit's launch constants)
const char k_bridge_h[] = {
#embed "demcz_kernels_bridge.h"
    , 0};
// the predict unit's headers (on top of demcz_device.h and the derive unit's launch constants)
const char k_predict_rng_h[] = {
#embed "demcz_predict_rng.h"
    , 0};
const char k_predict_h[] = {
#embed "demcz_kernels_predict.h"
    , 0};
#pragma clang diagnostic pop

// -D switches of the library build that change the layout of WindowParams: the program's kernels must see the same struct
const char* const k_layout_switches[] = {
#ifdef DEMCZ_STAMPS
    "-DDEMCZ_STAMPS",
#endif
    nullptr};

constexpr size_t LOG_MAX = 6000;      // bytes of compiler log handed back (the first errors are the useful ones)

std::mutex g_prog_mu;
std::map<std::string, std::shared_ptr<const demcz_prog::Code>> g_code_cache;                        // composed text + options
std::map<std::pair<const demcz_prog::Code*, int>, demcz_prog::Module> g_module_cache;               // (code object, device)

// <math.h>'s INFINITY and NAN, which hipRTC's built-in headers leave undefined: a log-density with bounded support returns -INFINITY
const char k_math_macros[] = "#ifndef INFINITY\n#define INFINITY (__builtin_inff())\n#endif\n#ifndef NAN\n#define NAN (__builtin_nanf(\"\"))\n#endif\n";

std::string compose(int d, int m, const std::string& source, int unit)
{
    std::ostringstream s;
    if (unit == demcz_prog::UNIT_DERIVE) {
        s << "#define DEMCZ_D " << d << "\n#define DEMCZ_M " << m << "\n#define DEMCZ_DERIVE_UNIT\n"
          << "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" << k_math_macros
          << "#line 1 \"program\"\n" << source << "\n"
          << "#line 1 \"demcz_unit_derive\"\n#include \"demcz_kernels_derive.h\"\n";
        return s.str();
    }
    if (unit == demcz_prog::UNIT_POINTWISE) {
        s << "#define DEMCZ_D " << d << "\n#define DEMCZ_POINTWISE_UNIT\n"
          << "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" << k_math_macros
          << "#line 1 \"program\"\n" << source << "\n"
          << "#line 1 \"demcz_unit_pointwise\"\n#include \"demcz_kernels_pointwise.h\"\n";
        return s.str();
    }
    if (unit == demcz_prog::UNIT_BRIDGE) {
        s << "#define DEMCZ_D " << d << "\n#define DEMCZ_BRIDGE_UNIT\n"
          << "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" << k_math_macros
          << "#line 1 \"program\"\n" << source << "\n"
          << "#line 1 \"demcz_unit_bridge\"\n#include \"demcz_kernels_bridge.h\"\n";
        return s.str();
    }
    if (unit == demcz_prog::UNIT_PREDICT) {
        s << "#define DEMCZ_D " << d << "\n#define DEMCZ_M " << m << "\n#define DEMCZ_PREDICT_UNIT\n"
          << "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" << k_math_macros
          << "#include \"demcz_device.h\"\n#include \"demcz_predict_rng.h\"\n"
          << "#line 1 \"program\"\n" << source << "\n"
          << "#line 1 \"demcz_unit_predict\"\n#include \"demcz_kernels_predict.h\"\n";
        return s.str();
    }
    if (unit == demcz_prog::UNIT_WAVE) {
        const char* kn = (d <= 5) ? "window_kernel_ps" : "window_kernel_pw";
        s << "#define DEMCZ_D " << d << "\n#define DEMCZ_PROGRAM_TARGET\n#define DEMCZ_NO_AUX_KERNELS\n#define ML_LRDPP 0\n#define PW_DDPP 0\n"
          << "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" << k_math_macros
          << "#line 1 \"program\"\n" << source << "\n"
          << "#line 1 \"demcz_program_wave_unit\"\n#include \"demcz_kernels_pw.h\"\n";
        for (int live = 0; live < 2; ++live)
            for (int temper = 0; temper < 2; ++temper)
                s << "template __global__ void demcz::" << kn << "<demcz::TARGET_PROGRAM, DEMCZ_D, " << (live ? "true" : "false") << ", "
                  << (temper ? "true" : "false") << ">(const demcz::WindowParams);\n";
        s << "template __global__ void demcz::logp_kernel<demcz::TARGET_PROGRAM>(demcz::TargetParams, int, const double*, int64_t, "
             "int64_t, double*);\n";
        return s.str();
    }
    s << "#define DEMCZ_D " << d << "\n#define DEMCZ_PROGRAM_TARGET\n#define DEMCZ_NO_AUX_KERNELS\n"
      << "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" << k_math_macros
      << "#line 1 \"program\"\n" << source << "\n"
      << "#line 1 \"demcz_program_unit\"\n#include \"demcz_kernels.h\"\n#include \"demcz_kernels_snooker.h\"\n#include \"demcz_kernels_crossover.h\"\n"
      << "template __global__ void demcz::window_kernel<demcz::TARGET_PROGRAM, DEMCZ_D, true>(const demcz::WindowParams);\n"
      << "template __global__ void demcz::window_kernel<demcz::TARGET_PROGRAM, DEMCZ_D, false>(const demcz::WindowParams);\n"
      << "template __global__ void demcz::snooker_kernel<demcz::TARGET_PROGRAM, DEMCZ_D>(const demcz::WindowParams, const demcz::SnookerParams);\n"
      << "template __global__ void demcz::logp_kernel<demcz::TARGET_PROGRAM>(demcz::TargetParams, int, const double*, int64_t, "
         "int64_t, double*);\n";
    s << "template __global__ void demcz::window_kernel_cr<demcz::TARGET_PROGRAM, DEMCZ_D>(const demcz::WindowParams, const demcz::CrossoverParams);\n";
    return s.str();
}

std::vector<std::string> split_options(const char* options)
{
    std::vector<std::string> out;
    std::istringstream in(options ? options : "");
    std::string w;
    while (in >> w) out.push_back(w);
    return out;
}

bool file_exists(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}

// ROCm's include directory (rocRAND's Philox header): ROCM_PATH, else the install libhiprtc was loaded from
bool rocm_include(std::string& dir, std::string& err)
{
    std::string root;
    if (const char* rp = getenv("ROCM_PATH"); rp && *rp) {
        root = rp;
    } else {
        Dl_info info{};
        if (dladdr(reinterpret_cast<void*>(&hiprtcCreateProgram), &info) && info.dli_fname) {
            std::string lib = info.dli_fname;                   // <rocm>/lib/libhiprtc.so.N
            const size_t a = lib.rfind('/');
            const size_t b = (a == std::string::npos || a == 0) ? std::string::npos : lib.rfind('/', a - 1);
            if (b != std::string::npos) root = lib.substr(0, b);
        }
    }
    dir = root + "/include";
    if (root.empty() || !file_exists(dir + "/rocrand/rocrand_philox4x32_10.h")) {
        err = "program target: rocRAND's header rocrand/rocrand_philox4x32_10.h was not found under '" + dir +
              "' (the ROCm install is taken from ROCM_PATH, or else from where libhiprtc was loaded; set ROCM_PATH to the ROCm root)";
        return false;
    }
    return true;
}

std::string trim_log(std::string log)
{
    if (log.size() > LOG_MAX) log = log.substr(0, LOG_MAX) + "\n... (compiler log cut)";
    return log;
}

#define RTCCHK(expr)                                                                             \
    do {                                                                                         \
        hiprtcResult r_ = (expr);                                                                \
        if (r_ != HIPRTC_SUCCESS) {                                                              \
            err = who + #expr ": " + hiprtcGetErrorString(r_);                                   \
            return false;                                                                        \
        }                                                                                        \
    } while (0)

// what a failed call says first: which of the two kinds of program it was about
const char* who_of(int unit)
{
    return unit == demcz_prog::UNIT_DERIVE ? "derive program: " : unit == demcz_prog::UNIT_POINTWISE ? "pointwise program: " :
           unit == demcz_prog::UNIT_PREDICT ? "predictive program: " : "program target: ";
}

bool compile(const std::string& text, const std::vector<std::string>& opts, int d, int m, int unit, demcz_prog::Code& code, std::string& err)
{
    hiprtcProgram prog = nullptr;
    const std::string who = who_of(unit);
    const char* headers[] = {k_device_h, k_kernels_h, k_rec_h, k_ml_h, k_mlb_inc, k_pc_h, k_ps_h, k_pw_h};
    const char* names[] = {"demcz_device.h", "demcz_kernels.h", "demcz_kernels_rec.h", "demcz_kernels_ml.h", "demcz_mlb_dpp_20_5.inc",
                           "demcz_kernels_pc.h", "demcz_kernels_ps.h", "demcz_kernels_pw.h"};
    const bool pointwise = unit == demcz_prog::UNIT_POINTWISE, bridge = unit == demcz_prog::UNIT_BRIDGE, predict = unit == demcz_prog::UNIT_PREDICT;
    const bool wave = unit == demcz_prog::UNIT_WAVE, derive = unit == demcz_prog::UNIT_DERIVE || pointwise || bridge || predict;   // (derive: a streaming unit)
    const char* lane_headers[] = {k_device_h, k_kernels_h, k_snooker_h, k_crossover_h};
    const char* lane_names[] = {"demcz_device.h", "demcz_kernels.h", "demcz_kernels_snooker.h", "demcz_kernels_crossover.h"};
    const char* derive_headers[] = {k_derive_h};
    const char* derive_names[] = {"demcz_kernels_derive.h"};
    const char* pointwise_headers[] = {k_derive_h, k_pointwise_h};
    const char* pointwise_names[] = {"demcz_kernels_derive.h", "demcz_kernels_pointwise.h"};
    const char* bridge_headers[] = {k_device_h, k_derive_h, k_bridge_h};
    const char* bridge_names[] = {"demcz_device.h", "demcz_kernels_derive.h", "demcz_kernels_bridge.h"};
    const char* predict_headers[] = {k_device_h, k_derive_h, k_predict_rng_h, k_predict_h};
    const char* predict_names[] = {"demcz_device.h", "demcz_kernels_derive.h", "demcz_predict_rng.h", "demcz_kernels_predict.h"};
    if (predict) RTCCHK(hiprtcCreateProgram(&prog, text.c_str(), "demcz_unit_predict.hip", 4, predict_headers, predict_names));
    else if (bridge) RTCCHK(hiprtcCreateProgram(&prog, text.c_str(), "demcz_unit_bridge.hip", 3, bridge_headers, bridge_names));
    else if (pointwise) RTCCHK(hiprtcCreateProgram(&prog, text.c_str(), "demcz_unit_pointwise.hip", 2, pointwise_headers, pointwise_names));
    else if (derive) RTCCHK(hiprtcCreateProgram(&prog, text.c_str(), "demcz_unit_derive.hip", 1, derive_headers, derive_names));
    else if (wave) RTCCHK(hiprtcCreateProgram(&prog, text.c_str(), "demcz_program_wave_unit.hip", 8, headers, names));
    else RTCCHK(hiprtcCreateProgram(&prog, text.c_str(), "demcz_program_unit.hip", 4, lane_headers, lane_names));
    struct Guard { hiprtcProgram& p; ~Guard() { if (p) (void)hiprtcDestroyProgram(&p); } } guard{prog};
    const std::string ds = std::to_string(d);
    std::vector<std::string> exprs;
    if (derive) {
        exprs = {predict ? "&demcz::predict_kernel" : bridge ? "&demcz::bridge_proposal_program_kernel" : pointwise ? "&demcz::pointwise_kernel" : "&demcz::derive_kernel"};
        if (predict) exprs.push_back("&demcz::ppc_kernel");
    } else if (wave) {
        const std::string kn = (d <= 5) ? "&demcz::window_kernel_ps<4, " : "&demcz::window_kernel_pw<4, ";
        for (int live = 0; live < 2; ++live)
            for (int temper = 0; temper < 2; ++temper)
                exprs.push_back(kn + ds + (live ? ", true" : ", false") + (temper ? ", true>" : ", false>"));
    } else {
        exprs = {"&demcz::window_kernel<4, " + ds + ", true>", "&demcz::window_kernel<4, " + ds + ", false>", "&demcz::snooker_kernel<4, " + ds + ">",
                 "&demcz::window_kernel_cr<4, " + ds + ">"};
    }
    if (!derive) exprs.push_back("&demcz::logp_kernel<4>");
    for (const auto& e : exprs) RTCCHK(hiprtcAddNameExpression(prog, e.c_str()));
    std::vector<const char*> argv;
    for (const auto& o : opts) argv.push_back(o.c_str());
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)argv.size(), argv.data());
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string log;
        if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
            log.resize(n);
            if (hiprtcGetProgramLog(prog, &log[0]) != HIPRTC_SUCCESS) log.clear();
            while (!log.empty() && log.back() == '\0') log.pop_back();
        }
        err = who + "compilation failed (" + std::string(hiprtcGetErrorString(rc)) + ")";
        if ((!derive || bridge) && text.find("demcz_logobj") == std::string::npos)   // (the library's own call is in demcz_kernels.h, not in `text`)
            err += "; the program does not define demcz_logobj -- it must define "
                   "__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)";
        if (pointwise && text.find("demcz_loglik") == std::string::npos)
            err += "; the program does not define demcz_loglik -- it must define "
                   "__device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i)";
        if (predict && text.find("demcz_predict(") == std::string::npos)    // (the unit's headers are included, not in `text`)
            err += "; the program does not define demcz_predict -- it must define "
                   "__device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata, demcz_rng* rng, double* out)";
        if (derive && !pointwise && !bridge && !predict && text.find("demcz_derive") == std::string::npos)    // (... and derive_kernel's in demcz_kernels_derive.h)
            err += "; the program does not define demcz_derive -- it must define "
                   "__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)";
        err += ":\n" + trim_log(log);
        return false;
    }
    size_t n = 0;
    RTCCHK(hiprtcGetCodeSize(prog, &n));
    code.object.resize(n);
    RTCCHK(hiprtcGetCode(prog, code.object.data()));
    if (const char* dump = getenv("DEMCZ_PROGRAM_DUMP"); dump && *dump) {
        // diagnosis (scripts/kernel_regs.py, llvm-objdump): the code object as a file in that directory
        const std::string path = std::string(dump) + "/demcz_program_" + (predict ? "predict" : bridge ? "bridge" : pointwise ? "pointwise" : derive ? "derive" : wave ? "wave" : "lane") + "_d" + ds + "_" +
                                 std::to_string(std::hash<std::string>{}(text) % 1000000007ull) + ".co";
        if (FILE* f = fopen(path.c_str(), "wb")) { (void)fwrite(code.object.data(), 1, code.object.size(), f); fclose(f); }
    }
    std::vector<std::string*> lowered;
    if (predict) lowered = {&code.derive, &code.ppc};
    else if (derive) lowered = {&code.derive};
    else if (wave) lowered = {&code.wave[0][0], &code.wave[0][1], &code.wave[1][0], &code.wave[1][1], &code.logp};
    else lowered = {&code.window_full, &code.window_blocks, &code.snooker, &code.crossover, &code.logp};
    for (size_t i = 0; i < lowered.size(); ++i) {
        const char* nm = nullptr;
        RTCCHK(hiprtcGetLoweredName(prog, exprs[i].c_str(), &nm));
        *lowered[i] = nm;
    }
    code.d = d;
    code.m = m;
    code.unit = unit;
    return true;
}
#undef RTCCHK

}  // namespace

namespace demcz_prog {

int32_t get_code(int d, const char* source, const char* options, int unit, std::shared_ptr<const Code>& out, std::string& err, int m)
{
    if (unit != UNIT_ONE_LANE && unit != UNIT_WAVE && unit != UNIT_DERIVE && unit != UNIT_POINTWISE && unit != UNIT_BRIDGE && unit != UNIT_PREDICT) {
        err = "program target: lanes_per_chain must be 0, 1 or DEMCZ_LAYOUT_PROGRAM_WAVE";
        return 1;
    }
    const std::string who = who_of(unit);
    if (d < 1 || d > MAX_PROGRAM_D) {
        err = who + "d must be in 1.." + std::to_string(MAX_PROGRAM_D);
        return 1;
    }
    if ((unit == UNIT_DERIVE || unit == UNIT_PREDICT) && (m < 1 || m > MAX_DERIVE_M)) {
        err = who + "m must be in 1.." + std::to_string(MAX_DERIVE_M);
        return 1;
    }
    if (unit == UNIT_WAVE && d < WAVE_MIN_D) {
        err = "program target: the wave-per-chain layout (DEMCZ_LAYOUT_PROGRAM_WAVE) needs d in " + std::to_string(WAVE_MIN_D) + ".." +
              std::to_string(MAX_PROGRAM_D);
        return 1;
    }
    if (!source) {
        err = who + "source is NULL";
        return 1;
    }
    std::string inc;
    if (!rocm_include(inc, err)) return 1;
    std::vector<std::string> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I" + inc};
    if (unit != UNIT_DERIVE && unit != UNIT_POINTWISE && unit != UNIT_BRIDGE && unit != UNIT_PREDICT)
        for (const char* const* s = k_layout_switches; *s; ++s) opts.push_back(*s);
    for (auto& o : split_options(options)) opts.push_back(o);
    // (the text is the key: it names the unit's kernel header and, for a derive unit, DEMCZ_M)
    const std::string text = compose(d, m, source, unit);
    std::string key = text;
    for (const auto& o : opts) key += '\0' + o;
    {
        std::lock_guard<std::mutex> lk(g_prog_mu);
        auto it = g_code_cache.find(key);
        if (it != g_code_cache.end()) { out = it->second; return 0; }
    }
    auto code = std::make_shared<Code>();
    if (!compile(text, opts, d, m, unit, *code, err)) return 1;
    std::lock_guard<std::mutex> lk(g_prog_mu);
    auto ins = g_code_cache.emplace(key, code);           // (another thread may have compiled the same program meanwhile)
    out = ins.first->second;
    return 0;
}

int32_t get_module(const std::shared_ptr<const Code>& code, int device, Module& out, std::string& err)
{
    std::lock_guard<std::mutex> lk(g_prog_mu);
    const auto key = std::make_pair(code.get(), device);
    auto it = g_module_cache.find(key);
    if (it != g_module_cache.end()) { out = it->second; return 0; }
    Module m;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipModuleLoadData(&m.module, code->object.data());
    const bool streaming = code->unit == UNIT_DERIVE || code->unit == UNIT_POINTWISE || code->unit == UNIT_BRIDGE || code->unit == UNIT_PREDICT;
    if (streaming) {
        if (e == hipSuccess) e = hipModuleGetFunction(&m.derive, m.module, code->derive.c_str());
        if (e == hipSuccess && code->unit == UNIT_PREDICT) e = hipModuleGetFunction(&m.ppc, m.module, code->ppc.c_str());
    } else if (code->unit == UNIT_WAVE) {
        for (int live = 0; live < 2; ++live)
            for (int temper = 0; temper < 2; ++temper)
                if (e == hipSuccess) e = hipModuleGetFunction(&m.wave[live][temper], m.module, code->wave[live][temper].c_str());
    } else {
        if (e == hipSuccess) e = hipModuleGetFunction(&m.window_full, m.module, code->window_full.c_str());
        if (e == hipSuccess) e = hipModuleGetFunction(&m.window_blocks, m.module, code->window_blocks.c_str());
        if (e == hipSuccess) e = hipModuleGetFunction(&m.snooker, m.module, code->snooker.c_str());
        if (e == hipSuccess) e = hipModuleGetFunction(&m.crossover, m.module, code->crossover.c_str());
    }
    if (!streaming && e == hipSuccess) e = hipModuleGetFunction(&m.logp, m.module, code->logp.c_str());
    if (e != hipSuccess) {
        if (m.module) (void)hipModuleUnload(m.module);
        err = std::string(who_of(code->unit)) + "loading the code object: " + hipGetErrorString(e);
        return 2;
    }
    m.code = code;          // (the cache keeps the code object alive with the module)
    g_module_cache.emplace(key, m);
    out = m;
    return 0;
}

}  // namespace demcz_prog
