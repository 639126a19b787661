// demcz_program.hip -- program targets (DEMCZ_TARGET_PROGRAM) and the other programs the user writes as HIP C++: compiled at run
// time with hipRTC for gfx950 together with kernels of the library's, and loaded as a module on the handle's device.  Host code
// only: the kernels of a program live in its code object, not in this library.
//
// What a unit consists of is its row of k_units (below); compose, compile, get_code and get_module read the row.  What the
// table does not show:
//   - the wave unit defines ML_LRDPP 0 / PW_DDPP 0: the generated DPP texts of the built-in targets are not part of the unit.  The
//     candidate adds read their increments from LDS -- the same doubles, tests/test_switch_variants.py -- and 54 generated files
//     stay out of the library's text and out of every first-use compile;
//   - the streaming units (derive, pointwise, bridge, predict) get no layout switches: they see no struct of the library's;
//   - the header texts are embedded into this library at build time, and the #line before the user's source gives compiler
//     messages the user's own line numbers.
// Compile options: --offload-arch=gfx950 -O3 -ffp-contract=off -I<rocm>/include, the library's own layout switches where the row
// says so, then the user's.  Code objects are cached per (composed text, options) -- the text names the unit's kernel header and
// DEMCZ_M, so every unit has keys of its own --, loaded modules per (code object, device); both for the life of the process.
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
const char k_derive_h[] = {
#embed "demcz_kernels_derive.h"
    , 0};
const char k_pointwise_h[] = {
#embed "demcz_kernels_pointwise.h"
    , 0};
const char k_bridge_h[] = {
#embed "demcz_kernels_bridge.h"
    , 0};
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

// ---- the units -----------------------------------------------------------------------------------------------------------------
struct Header { const char* name; const char* text; };
// A kernel of a unit: demcz::<name><targs>.  In targs {T} is the target and {d} the dimension -- 4 and the number in the name
// expression, demcz::TARGET_PROGRAM and DEMCZ_D in the explicit instantiation --; {k} in the name is Unit::stem(d).
struct Kernel { const char* name; const char* targs; const char* params; };
struct Unit {
    const char* tag;                        // in the name of the DEMCZ_PROGRAM_DUMP file
    const char* name;                       // the #line name of what follows the user's source; with ".hip", the translation unit's
    const char* who;                        // what an error message says first
    bool has_m = false;                     // DEMCZ_M is defined after DEMCZ_D: m is validated and part of the key
    const char* defines;                    // after DEMCZ_D (and DEMCZ_M)
    const char* before = "";                // the includes before the user's source
    const char* after;                      // the includes after it
    std::vector<Header> headers;            // the embedded headers the unit is given
    bool layout_switches = false;           // k_layout_switches are passed
    int min_d = 1;
    const char* min_d_what = "";            // what needs d >= min_d, for the message
    std::vector<Kernel> kernels;            // in the order of the unit's indices in demcz_program.h
    std::vector<int> instantiate = {};      // the kernels the text instantiates explicitly, in the text's order (the text is the cache
                                            // key: the order stays as it grew)
    const char* (*stem)(int d) = nullptr;   // {k}, where the kernel depends on d
    const char* needle;                     // the entry point the user must define, as searched in the composed text (the library's own
    const char* hint;                       // call is in an included header, not in the text); what a failed compile without it adds
};

const char k_logobj_hint[] = "; the program does not define demcz_logobj -- it must define "
                             "__device__ double demcz_logobj(const double* x, const double* data, int64_t ndata)";
const char k_window_params[] = "const demcz::WindowParams";
const Kernel k_logp = {"logp_kernel", "<{T}>", "demcz::TargetParams, int, const double*, int64_t, int64_t, double*"};

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wc++20-designator"
const Unit k_units[] = {
    {   // UNIT_ONE_LANE: the one-lane window kernel, the snooker and the crossover generation's kernels, the latter with and without
        // adapted class weights (a program that cannot be
        // built for them fails here) and logp_kernel
        .tag = "lane", .name = "demcz_program_unit", .who = "program target: ",
        .defines = "#define DEMCZ_PROGRAM_TARGET\n#define DEMCZ_NO_AUX_KERNELS\n",
        .after = "#include \"demcz_kernels.h\"\n#include \"demcz_kernels_snooker.h\"\n#include \"demcz_kernels_crossover.h\"\n",
        .headers = {{"demcz_device.h", k_device_h}, {"demcz_kernels.h", k_kernels_h}, {"demcz_kernels_snooker.h", k_snooker_h},
                    {"demcz_kernels_crossover.h", k_crossover_h}},
        .layout_switches = true,
        .kernels = {{"window_kernel", "<{T}, {d}, true>", k_window_params},
                    {"window_kernel", "<{T}, {d}, false>", k_window_params},
                    {"snooker_kernel", "<{T}, {d}>", "const demcz::WindowParams, const demcz::SnookerParams"},
                    {"window_kernel_cr", "<{T}, {d}>", "const demcz::WindowParams, const demcz::CrossoverParams"},
                    k_logp,
                    {"window_kernel_cr", "<{T}, {d}, true, demcz::CrossoverAdaptParams>",
                     "const demcz::WindowParams, const demcz::CrossoverParams, const demcz::CrossoverAdaptParams"}},
        .instantiate = {demcz_prog::LANE_FULL, demcz_prog::LANE_BLOCKS, demcz_prog::LANE_SNOOKER, demcz_prog::LANE_LOGP, demcz_prog::LANE_CROSSOVER,
                        demcz_prog::LANE_CROSSOVER_ADAPT},
        .needle = "demcz_logobj", .hint = k_logobj_hint,
    },
    {   // UNIT_WAVE: the wave-per-chain consumers of the split layout, LIVE and TEMPER both ways, and logp_kernel; demcz_kernels_pw.h
        // brings _ps.h, _pc.h with the producer half, _ml.h, _rec.h and demcz_kernels.h
        .tag = "wave", .name = "demcz_program_wave_unit", .who = "program target: ",
        .defines = "#define DEMCZ_PROGRAM_TARGET\n#define DEMCZ_NO_AUX_KERNELS\n#define ML_LRDPP 0\n#define PW_DDPP 0\n",
        .after = "#include \"demcz_kernels_pw.h\"\n",
        .headers = {{"demcz_device.h", k_device_h}, {"demcz_kernels.h", k_kernels_h}, {"demcz_kernels_rec.h", k_rec_h},
                    {"demcz_kernels_ml.h", k_ml_h}, {"demcz_mlb_dpp_20_5.inc", k_mlb_inc}, {"demcz_kernels_pc.h", k_pc_h},
                    {"demcz_kernels_ps.h", k_ps_h}, {"demcz_kernels_pw.h", k_pw_h}},
        .layout_switches = true, .min_d = demcz_prog::WAVE_MIN_D, .min_d_what = "the wave-per-chain layout (DEMCZ_LAYOUT_PROGRAM_WAVE)",
        .kernels = {{"{k}", "<{T}, {d}, false, false>", k_window_params}, {"{k}", "<{T}, {d}, false, true>", k_window_params},
                    {"{k}", "<{T}, {d}, true, false>", k_window_params}, {"{k}", "<{T}, {d}, true, true>", k_window_params}, k_logp},
        .instantiate = {0, 1, 2, 3, demcz_prog::WAVE_LOGP},
        .stem = [](int d) { return d <= 5 ? "window_kernel_ps" : "window_kernel_pw"; },
        .needle = "demcz_logobj", .hint = k_logobj_hint,
    },
    {   // UNIT_DERIVE: the user's demcz_derive and derive_kernel, nothing else of the library: it compiles in a fraction of the
        // time a program target takes
        .tag = "derive", .name = "demcz_unit_derive", .who = "derive program: ", .has_m = true,
        .defines = "#define DEMCZ_DERIVE_UNIT\n",
        .after = "#include \"demcz_kernels_derive.h\"\n",
        .headers = {{"demcz_kernels_derive.h", k_derive_h}},
        .kernels = {{"derive_kernel", "", nullptr}},
        .needle = "demcz_derive",
        .hint = "; the program does not define demcz_derive -- it must define "
                "__device__ void demcz_derive(const double* x, double logp, const double* data, int64_t ndata, double* out)",
    },
    {   // UNIT_POINTWISE: the user's demcz_loglik and pointwise_kernel (its header includes the derive unit's for the launch constants)
        .tag = "pointwise", .name = "demcz_unit_pointwise", .who = "pointwise program: ",
        .defines = "#define DEMCZ_POINTWISE_UNIT\n",
        .after = "#include \"demcz_kernels_pointwise.h\"\n",
        .headers = {{"demcz_kernels_derive.h", k_derive_h}, {"demcz_kernels_pointwise.h", k_pointwise_h}},
        .kernels = {{"pointwise_kernel", "", nullptr}},
        .needle = "demcz_loglik",
        .hint = "; the program does not define demcz_loglik -- it must define "
                "__device__ double demcz_loglik(const double* x, const double* data, int64_t ndata, int64_t i)",
    },
    {   // UNIT_BRIDGE: the user's demcz_logobj exactly as a program target defines it, and bridge_proposal_program_kernel, whose
        // header includes demcz_device.h (Philox, dm_log, the Box-Muller pair) itself
        .tag = "bridge", .name = "demcz_unit_bridge", .who = "program target: ",
        .defines = "#define DEMCZ_BRIDGE_UNIT\n",
        .after = "#include \"demcz_kernels_bridge.h\"\n",
        .headers = {{"demcz_device.h", k_device_h}, {"demcz_kernels_derive.h", k_derive_h}, {"demcz_kernels_bridge.h", k_bridge_h}},
        .kernels = {{"bridge_proposal_program_kernel", "", nullptr}},
        .needle = "demcz_logobj", .hint = k_logobj_hint,
    },
    {   // UNIT_PREDICT: the demcz_rng of a draw and its four helpers before the user's demcz_predict, then predict_kernel and ppc_kernel
        .tag = "predict", .name = "demcz_unit_predict", .who = "predictive program: ", .has_m = true,
        .defines = "#define DEMCZ_PREDICT_UNIT\n",
        .before = "#include \"demcz_device.h\"\n#include \"demcz_predict_rng.h\"\n",
        .after = "#include \"demcz_kernels_predict.h\"\n",
        .headers = {{"demcz_device.h", k_device_h}, {"demcz_kernels_derive.h", k_derive_h}, {"demcz_predict_rng.h", k_predict_rng_h},
                    {"demcz_kernels_predict.h", k_predict_h}},
        .kernels = {{"predict_kernel", "", nullptr}, {"ppc_kernel", "", nullptr}},
        .needle = "demcz_predict(",
        .hint = "; the program does not define demcz_predict -- it must define "
                "__device__ void demcz_predict(const double* x, double logp, const double* data, int64_t ndata, demcz_rng* rng, double* out)",
    },
};
#pragma clang diagnostic pop
static_assert(sizeof(k_units) / sizeof(k_units[0]) == demcz_prog::UNIT_COUNT, "one row per unit, in the order of the enum");

// a kernel's name expression, or its explicit instantiation
std::string kernel_text(const Unit& u, const Kernel& k, int d, bool instantiation)
{
    std::string s = std::string(instantiation ? "template __global__ void demcz::" : "&demcz::") + k.name + k.targs;
    auto put = [&s](const std::string& what, const std::string& with) {
        for (size_t p; (p = s.find(what)) != std::string::npos;) s.replace(p, what.size(), with);
    };
    if (u.stem) put("{k}", u.stem(d));
    put("{T}", instantiation ? "demcz::TARGET_PROGRAM" : "4");
    put("{d}", instantiation ? "DEMCZ_D" : std::to_string(d));
    return instantiation ? s + "(" + k.params + ");\n" : s;
}

std::string compose(int d, int m, const std::string& source, const Unit& u)
{
    std::ostringstream s;
    s << "#define DEMCZ_D " << d << "\n";
    if (u.has_m) s << "#define DEMCZ_M " << m << "\n";
    s << u.defines << "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" << k_math_macros << u.before
      << "#line 1 \"program\"\n" << source << "\n"
      << "#line 1 \"" << u.name << "\"\n" << u.after;
    for (int i : u.instantiate) s << kernel_text(u, u.kernels[i], d, true);
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

bool compile(const std::string& text, const std::vector<std::string>& opts, int d, int m, int unit, demcz_prog::Code& code, std::string& err)
{
    const Unit& u = k_units[unit];
    hiprtcProgram prog = nullptr;
    const std::string who = u.who;
    std::vector<const char*> headers, names;
    for (const Header& h : u.headers) { headers.push_back(h.text); names.push_back(h.name); }
    const std::string tu = std::string(u.name) + ".hip";
    RTCCHK(hiprtcCreateProgram(&prog, text.c_str(), tu.c_str(), (int)headers.size(), headers.data(), names.data()));
    struct Guard { hiprtcProgram& p; ~Guard() { if (p) (void)hiprtcDestroyProgram(&p); } } guard{prog};
    std::vector<std::string> exprs;
    for (const Kernel& k : u.kernels) exprs.push_back(kernel_text(u, k, d, false));
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
        if (text.find(u.needle) == std::string::npos) err += u.hint;
        err += ":\n" + trim_log(log);
        return false;
    }
    size_t n = 0;
    RTCCHK(hiprtcGetCodeSize(prog, &n));
    code.object.resize(n);
    RTCCHK(hiprtcGetCode(prog, code.object.data()));
    if (const char* dump = getenv("DEMCZ_PROGRAM_DUMP"); dump && *dump) {
        // diagnosis (scripts/kernel_regs.py, llvm-objdump): the code object as a file in that directory
        const std::string path = std::string(dump) + "/demcz_program_" + u.tag + "_d" + std::to_string(d) + "_" +
                                 std::to_string(std::hash<std::string>{}(text) % 1000000007ull) + ".co";
        if (FILE* f = fopen(path.c_str(), "wb")) { (void)fwrite(code.object.data(), 1, code.object.size(), f); fclose(f); }
    }
    for (size_t i = 0; i < exprs.size(); ++i) {
        const char* nm = nullptr;
        RTCCHK(hiprtcGetLoweredName(prog, exprs[i].c_str(), &nm));
        code.names[i] = nm;
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
    if (unit < 0 || unit >= UNIT_COUNT) {
        err = "program target: lanes_per_chain must be 0, 1 or DEMCZ_LAYOUT_PROGRAM_WAVE";
        return 1;
    }
    const Unit& u = k_units[unit];
    const std::string who = u.who;
    if (d < 1 || d > MAX_PROGRAM_D) {
        err = who + "d must be in 1.." + std::to_string(MAX_PROGRAM_D);
        return 1;
    }
    if (u.has_m && (m < 1 || m > MAX_DERIVE_M)) {
        err = who + "m must be in 1.." + std::to_string(MAX_DERIVE_M);
        return 1;
    }
    if (d < u.min_d) {
        err = who + u.min_d_what + " needs d in " + std::to_string(u.min_d) + ".." + std::to_string(MAX_PROGRAM_D);
        return 1;
    }
    if (!source) {
        err = who + "source is NULL";
        return 1;
    }
    std::string inc;
    if (!rocm_include(inc, err)) return 1;
    std::vector<std::string> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I" + inc};
    if (u.layout_switches)
        for (const char* const* s = k_layout_switches; *s; ++s) opts.push_back(*s);
    for (auto& o : split_options(options)) opts.push_back(o);
    const std::string text = compose(d, m, source, u);
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
    const Unit& u = k_units[code->unit];
    Module m;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipModuleLoadData(&m.module, code->object.data());
    for (size_t i = 0; i < u.kernels.size() && e == hipSuccess; ++i) e = hipModuleGetFunction(&m.fn[i], m.module, code->names[i].c_str());
    if (e != hipSuccess) {
        if (m.module) (void)hipModuleUnload(m.module);
        err = std::string(u.who) + "loading the code object: " + hipGetErrorString(e);
        return 2;
    }
    m.code = code;          // (the cache keeps the code object alive with the module)
    g_module_cache.emplace(key, m);
    out = m;
    return 0;
}

}  // namespace demcz_prog
