// Host driver of tests/test_oobleck_launches_host.py: runs the Oobleck codec's plan on the CPU and prints what it would launch.  Unlike
// dit_launch_dump.cpp, which stubs the plan's internal launchers, this driver is the HIP runtime itself: it links the real codec objects (the three
// builds of csrc/oobleck.hip and csrc/oobleck_plan.hip, compiled --cuda-host-only), so tile choice, grid, LDS bytes and the argument blocks are
// those of the real launchers, and the same driver links against any commit's codec sources.  Kernel registration (the objects' constructors) maps
// host stubs to device names; hipLaunchKernel prints one line: the kernel's name with its template arguments (namespaces and the
// parameter list dropped), grid, block, dynamic LDS bytes and every argument.  Memory and the other runtime calls: host_runtime.h.
// The test defines each object's __hip_fatbin_<hash> symbol as 1 (bf16), 2 (fp16), 3 (fp32): that is how a launch knows its build.
//   oobleck_launch_dump            every case, each behind a line "== <name>"
#include <cxxabi.h>

#include <map>

#include "host_runtime.h"
#include "oobleck_kernels.h"

// ------------------------------------------------------------------------------ kernel registration and launch
namespace {

struct Kernel {
    std::string name;
    int build;
};
std::map<const void*, Kernel>& kernels() {      // function-local: registration runs from the objects' global constructors
    static std::map<const void*, Kernel> m;
    return m;
}
const char* const BUILDS[] = {"?", "bf16", "f16", "f32"};

// "_ZN12_GLOBAL__N_116conv_pipe_kernelILi128E...EEvNS_8ConvArgsE" -> "conv_pipe_kernel<128,128,4,2,3>"
std::string base_name(const char* mangled) {
    std::string m = mangled;
    for (size_t i; (i = m.find("DF16_")) != std::string::npos;) m.replace(i, 5, "Dh");      // _Float16, for demanglers that predate the spelling
    int status = 0;
    char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &status);
    std::string s = status == 0 ? d : m;
    free(d);
    const std::string anon = "(anonymous namespace)::";
    for (size_t i; (i = s.find(anon)) != std::string::npos;) s.erase(i, anon.size());
    s = s.substr(0, s.find('('));
    if (s.rfind("void ", 0) == 0) s.erase(0, 5);
    const size_t lt = s.find('<'), ns = s.rfind("::", lt);
    if (ns != std::string::npos) s.erase(0, ns + 2);
    std::string o;
    for (char c : s)
        if (c != ' ') o += c;
    return o;
}

const Kernel& kernel_of(const void* f) {
    static const Kernel none{"unregistered", 0};
    auto it = kernels().find(f);
    return it == kernels().end() ? none : it->second;
}

void put_conv(std::string& o, const bf16::ConvArgs& a) {
    put(o, "in"); put(o, (const void*)a.in); put(o, a.Tin); put(o, a.Cin);
    put(o, "W"); put(o, (const void*)a.W); put(o, a.taps); put(o, a.N); put(o, a.M); put(o, a.stride); put(o, a.off0); put(o, a.doff);
    put(o, "bias"); put(o, (const void*)a.bias); put(o, a.Cout);
    put(o, "res"); put(o, (const void*)a.res);
    put(o, "out"); put(o, (const void*)a.out_raw); put(o, (const void*)a.out_snk);
    put(o, "sn"); put(o, (const void*)a.sn_a); put(o, (const void*)a.sn_ib);
    put(o, "flat"); put(o, a.out_bstride); put(o, a.out_shift); put(o, a.out_limit);
    put(o, "cf"); put(o, (const void*)a.out_cf); put(o, a.cf_channels);
    put(o, "zero"); put(o, (const void*)a.zero_page);
    put(o, "act"); put(o, a.act); put(o, a.tanh_out);
}

// the small kernels' parameters: p pointer, i int, z size_t
const std::map<std::string, const char*> SIGNATURES = {
    {"cf_to_cl_kernel", "ppiii"},          {"first_conv_kernel", "pppppippiiii"}, {"wn_invnorm_kernel", "pppi"},
    {"wn_pack_conv_kernel", "pppiiiii"},   {"wn_fold_f32_kernel", "pppiz"},       {"wn_pack_convT_kernel", "pppiiiii"},
    {"wn_pack_nearest_kernel", "pppiiiii"}, {"snake_params_kernel", "ppppii"},
};

struct FatbinWrapper {
    unsigned magic, version;
    const void* binary;
    void* unused;
};
struct CallConfig {
    dim3 grid, block;
    size_t lds;
    hipStream_t stream;
};
std::vector<CallConfig> g_calls;

// The build a kernel belongs to is printed when it changes ("build f16"), not on every line: a plan stays in one build, and the bf16 and fp16
// builds, which launch alike, then share their lines in the fixture.  Every case starts with no build (case_start)
int g_build = -1;
void note_build(int build) {
    if (build != g_build) line("build", BUILDS[build]);
    g_build = build;
}
void case_start(const std::string& name) {
    g_allocs = 0;
    g_build = -1;
    line("==", name.c_str());
}

}  // namespace

extern "C" {
void** __hipRegisterFatBinary(const void* wrapper) { return (void**)const_cast<void*>(wrapper); }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void** modules, const void* host_function, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    const uintptr_t build = (uintptr_t)((const FatbinWrapper*)modules)->binary;
    kernels()[host_function] = {base_name(device_name), build <= 3 ? (int)build : 0};
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    g_calls.push_back({grid, block, lds, stream});
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
    const CallConfig c = g_calls.back();
    g_calls.pop_back();
    *grid = c.grid; *block = c.block; *lds = c.lds; *stream = c.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
    const Kernel& k = kernel_of(f);
    note_build(k.build);
    std::string o = "launch";
    put(o, k.name.c_str());
    put(o, "grid"); put(o, (int)grid.x); put(o, (int)grid.y); put(o, (int)grid.z);
    put(o, "block"); put(o, (int)block.x); put(o, (int)block.y); put(o, (int)block.z);
    put(o, "lds"); put(o, lds);
    const std::string base = k.name.substr(0, k.name.find('<'));
    if (base == "conv_pipe_kernel") {
        put_conv(o, *(const bf16::ConvArgs*)args[0]);
    } else if (base == "ru_fused_kernel") {
        const bf16::RuArgs& r = *(const bf16::RuArgs*)args[0];
        put(o, "c7"); put_conv(o, r.c7);
        put(o, "c1"); put_conv(o, r.c1);
    } else if (SIGNATURES.count(base)) {
        const char* sig = SIGNATURES.at(base);
        for (int i = 0; sig[i]; ++i) {
            if (sig[i] == 'p') put(o, *(const void* const*)args[i]);
            else if (sig[i] == 'i') put(o, *(const int*)args[i]);
            else put(o, *(const size_t*)args[i]);
        }
    } else {
        put(o, "arguments unknown");
    }
    puts(o.c_str());
    return hipSuccess;
}
hipError_t hipGetLastError() { return hipSuccess; }
}

int sat_ensure_dynamic_lds(const void* kernel, int bytes) {
    const Kernel& k = kernel_of(kernel);
    note_build(k.build);
    return line("sat_ensure_dynamic_lds", k.name.c_str(), bytes);
}
int sat_launch_range_stats(const void* x, int dtype, int64_t rows, int64_t cols, int64_t pitch, uint64_t counted, sat_range_record* rec, hipStream_t) {
    return line("range_stats", x, dtype, (long long)rows, (long long)cols, (long long)pitch, (size_t)counted, (const void*)rec);
}

// ------------------------------------------------------------------------------ the cases
namespace {

const int BF16 = SAT_GEMM_BF16, F16 = SAT_GEMM_FP16, F32 = SAT_GEMM_FP32X;
const char* fmt_name(int dtype) { return dtype == F16 ? "fp16" : dtype == F32 ? "fp32" : "bf16"; }
const int ALL[] = {BF16, F16, F32};
hipStream_t const STREAM = (hipStream_t)(uintptr_t)0x100;

struct Vae {
    int channels;
    std::vector<int> c_mults, strides;
    int latent;                  // the decoder's latent_dim; the encoder emits 2 * latent
    sat_oobleck_options opt;      // activation, final_tanh, nearest_upsample (the last two: decoder)
};
const Vae STABLE_AUDIO = {128, {1, 2, 4, 8, 16}, {2, 4, 4, 8, 8}, 64, {SAT_OOBLECK_ACT_SNAKE, 0, 0}};
const Vae SMALL_VAE = {16, {1, 2, 4, 8, 16}, {2, 4, 4, 8, 8}, 64, {SAT_OOBLECK_ACT_SNAKE, 0, 0}};      // tests/golden/cases.py
// tests/golden/make_golden_codec_options.py, and a nearest-upsample decoder with odd strides
const Vae REF_DEFAULTS = {32, {1, 2, 4, 8}, {2, 4, 8, 8}, 32, {SAT_OOBLECK_ACT_ELU, 1, 0}};
const Vae NEAREST_SNAKE = {64, {1, 2, 4}, {2, 4, 4}, 64, {SAT_OOBLECK_ACT_SNAKE, 0, 1}};
const Vae NARROW_ALL = {48, {1, 2, 3}, {2, 4, 4}, 20, {SAT_OOBLECK_ACT_ELU, 1, 1}};
const Vae NEAREST_ODD = {32, {1, 2}, {3, 5}, 16, {SAT_OOBLECK_ACT_SNAKE, 0, 1}};
const Vae TWO_BLOCKS = {64, {2, 4}, {2, 4}, 64, {SAT_OOBLECK_ACT_SNAKE, 0, 0}};      // the range report's: units of 128 channels (fused while it is off) and of 64

sat_oobleck_cfg cfg_of(const Vae& v, bool decoder, int dtype) {
    sat_oobleck_cfg c{};
    c.is_decoder = decoder; c.io_channels = 2; c.channels = v.channels; c.latent_dim = decoder ? v.latent : 2 * v.latent;
    c.n_blocks = (int)v.strides.size(); c.gemm_dtype = dtype;
    for (int i = 0; i < c.n_blocks; ++i) { c.c_mults[i] = v.c_mults[i]; c.strides[i] = v.strides[i]; }
    return c;
}
sat_oobleck_options opt_of(const Vae& v, bool decoder) { return {v.opt.activation, decoder ? v.opt.final_tanh : 0, decoder ? v.opt.nearest_upsample : 0}; }

// every tensor the plan asks for at finalize, as the reference's modules name them; `skip` is withheld
void set_tensors(sat_oobleck_plan* p, const sat_oobleck_cfg& c, const sat_oobleck_options& o, Inputs& in, const std::string& skip = "") {
    auto t = [&](const std::string& name, size_t n) {
        if (name != skip) sat_oobleck_plan_set_tensor(p, name.c_str(), in.make(name, n), (int64_t)n);
    };
    auto snake = [&](const std::string& pf, int C) {
        if (o.activation == SAT_OOBLECK_ACT_SNAKE) { t(pf + "alpha", C); t(pf + "beta", C); }
    };
    auto conv = [&](const std::string& pf, int g, size_t v, int bias) {
        t(pf + "weight_g", g); t(pf + "weight_v", v);
        if (bias) t(pf + "bias", bias);
    };
    auto unit = [&](const std::string& pf, int C) {
        snake(pf + "layers.0.", C); conv(pf + "layers.1.", C, (size_t)C * C * 7, C);
        snake(pf + "layers.2.", C); conv(pf + "layers.3.", C, (size_t)C * C, C);
    };
    auto L = [](int i) { return "layers." + std::to_string(i) + "."; };
    const int nb = c.n_blocks, ch = c.channels, ctop = c.c_mults[nb - 1] * ch;
    if (c.is_decoder) {
        conv(L(0), ctop, (size_t)ctop * c.latent_dim * 7, ctop);
        for (int bi = 0; bi < nb; ++bi) {
            const int i = nb - bi, cin = c.c_mults[i - 1] * ch, cout = (i >= 2 ? c.c_mults[i - 2] : 1) * ch, st = c.strides[i - 1];
            const std::string pf = L(bi + 1);
            snake(pf + L(0), cin);
            if (o.nearest_upsample) conv(pf + "layers.1.1.", cout, (size_t)cout * cin * 2 * st, 0);
            else conv(pf + L(1), cin, (size_t)cin * cout * 2 * st, cout);
            for (int r = 0; r < 3; ++r) unit(pf + L(2 + r), cout);
        }
        snake(L(nb + 1), ch);
        conv(L(nb + 2), c.io_channels, (size_t)c.io_channels * ch * 7, 0);
    } else {
        conv(L(0), ch, (size_t)ch * c.io_channels * 7, ch);
        for (int bi = 0; bi < nb; ++bi) {
            const int cin = (bi == 0 ? 1 : c.c_mults[bi - 1]) * ch, cout = c.c_mults[bi] * ch, st = c.strides[bi];
            const std::string pf = L(bi + 1);
            for (int r = 0; r < 3; ++r) unit(pf + L(r), cin);
            snake(pf + L(3), cin);
            conv(pf + L(4), cout, (size_t)cout * cin * 2 * st, cout);
        }
        snake(L(nb + 1), ctop);
        conv(L(nb + 2), c.latent_dim, (size_t)c.latent_dim * ctop * 3, c.latent_dim);
    }
}

int ratio_of(const sat_oobleck_cfg& c) {
    int r = 1;
    for (int i = 0; i < c.n_blocks; ++i) r *= c.strides[i];
    return r;
}

// one decode or encode of B items of T latent frames, in a workspace of exactly the size the plan asks for
void run_codec(sat_oobleck_plan* p, const sat_oobleck_cfg& c, int B, int T) {
    Inputs in;
    size_t bytes = 0;
    RC(sat_oobleck_workspace_bytes, p, B, T, &bytes);
    line("workspace_bytes", B, T, bytes);
    void* ws = in.workspace(bytes);
    const size_t lat = (size_t)B * c.latent_dim * T, audio = (size_t)B * c.io_channels * T * ratio_of(c);
    if (c.is_decoder) RC(sat_oobleck_decode, p, in.make("z", lat), in.make("audio", audio), B, T, ws, bytes, STREAM);
    else RC(sat_oobleck_encode, p, in.make("audio", audio), in.make("latents", lat), B, T, ws, bytes, STREAM);
}

// create (through `_ex` unless the options are the defaults), finalize, the workspace at a second shape, one run
sat_oobleck_plan* make_plan(const Vae& v, bool decoder, int dtype, Inputs& weights) {
    const sat_oobleck_cfg c = cfg_of(v, decoder, dtype);
    const sat_oobleck_options o = opt_of(v, decoder);
    sat_oobleck_plan* p = nullptr;
    if (&v == &STABLE_AUDIO) RC(sat_oobleck_plan_create, &c, &p);
    else RC(sat_oobleck_plan_create_ex, &c, &o, sizeof o, &p);
    if (!p) return nullptr;
    set_tensors(p, c, o, weights);
    RC(sat_oobleck_plan_finalize, p, STREAM);
    return p;
}
void codec_case(const char* name, const Vae& v, bool decoder, int dtype, int B, int T) {
    case_start(std::string(name) + (decoder ? "_decoder_" : "_encoder_") + fmt_name(dtype));
    Inputs weights;
    sat_oobleck_plan* p = make_plan(v, decoder, dtype, weights);
    if (!p) return;
    size_t bytes = 0;
    RC(sat_oobleck_workspace_bytes, p, 3, 7, &bytes);
    line("workspace_bytes", 3, 7, bytes);
    run_codec(p, cfg_of(v, decoder, dtype), B, T);
    sat_oobleck_plan_destroy(p);
}

// the range report: on (the two-launch route and the range_stats lines), count and names, zeroing, read, off, read while off, the fused route again
void report_case(bool decoder, int dtype) {
    case_start(std::string("range_report") + (decoder ? "_decoder_" : "_encoder_") + fmt_name(dtype));
    Inputs weights, in;
    sat_oobleck_plan* p = make_plan(TWO_BLOCKS, decoder, dtype, weights);
    const sat_oobleck_cfg c = cfg_of(TWO_BLOCKS, decoder, dtype);
    RC(sat_oobleck_range_report, p, 2);          // nothing to zero yet
    RC(sat_oobleck_range_report, p, 1);
    RC(sat_oobleck_range_report, p, 1);          // already on
    int32_t n = 0;
    RC(sat_oobleck_range_report_count, p, &n);
    line("records", (int)n);
    for (int i = -1; i <= n; ++i) {
        const char* nm = sat_oobleck_range_report_name(p, i);
        line("name", i, nm ? nm : "(null)");
    }
    run_codec(p, c, 1, 2);
    RC(sat_oobleck_range_report, p, 2);
    sat_range_record* rec = (sat_range_record*)in.make("records", (size_t)n * sizeof(sat_range_record) / 4);
    RC(sat_oobleck_range_report_read, p, rec, n - 1, sizeof(sat_range_record), STREAM);
    RC(sat_oobleck_range_report_read, p, rec, n, sizeof(sat_range_record) + 8, STREAM);
    RC(sat_oobleck_range_report_read, p, rec, n, sizeof(sat_range_record), STREAM);
    RC(sat_oobleck_range_report, p, 3);
    RC(sat_oobleck_range_report, p, 0);
    RC(sat_oobleck_range_report, p, 0);
    RC(sat_oobleck_range_report_read, p, rec, n, sizeof(sat_range_record), STREAM);
    run_codec(p, c, 1, 2);
    sat_oobleck_plan_destroy(p);
}

// sat_oobleck_unit: every kind in one format
void unit_cases(int dtype) {
    case_start(std::string("units_") + fmt_name(dtype));
    const int eb = dtype == F32 ? 4 : 2, B = 2, L = 8;
    auto pad = [](int c) { return (c + 63) / 64 * 64; };
    auto run = [&](const char* what, int kind, int Ci, int Co, int act, int stride, int dilation, int two_launch, int tanh) {
        line("unit", what);
        Inputs in;
        auto opbuf = [&](const char* name, size_t elems) { return (void*)in.make(name, (elems * eb + 3) / 4); };
        sat_oobleck_unit_desc u{};
        u.kind = kind; u.gemm_dtype = dtype; u.activation = act; u.b = B; u.t_len = L; u.c_in = Ci; u.c_out = Co;
        u.stride = stride; u.dilation = dilation; u.two_launch = two_launch; u.final_tanh = tanh;
        const bool snake = act == SAT_OOBLECK_ACT_SNAKE;
        const bool resample = kind == SAT_OOBLECK_UNIT_CONVT || kind == SAT_OOBLECK_UNIT_NEAREST || kind == SAT_OOBLECK_UNIT_STRIDED;
        const bool to_cf = kind == SAT_OOBLECK_UNIT_FINAL_DEC || kind == SAT_OOBLECK_UNIT_FINAL_ENC;
        const bool from_cf = kind == SAT_OOBLECK_UNIT_FIRST_CONV || kind == SAT_OOBLECK_UNIT_CF_TO_CL;
        const int k = kind == SAT_OOBLECK_UNIT_CONV1_RES ? 1 : kind == SAT_OOBLECK_UNIT_FINAL_ENC ? 3 : resample ? 2 * stride : 7;
        const int Lout = kind == SAT_OOBLECK_UNIT_STRIDED ? L / stride : kind == SAT_OOBLECK_UNIT_CONVT || kind == SAT_OOBLECK_UNIT_NEAREST ? L * stride : L;
        if (kind != SAT_OOBLECK_UNIT_CF_TO_CL) {
            u.weight_g = in.make("weight_g", kind == SAT_OOBLECK_UNIT_CONVT ? Ci : Co);
            u.weight_v = in.make("weight_v", (size_t)Ci * Co * k);
            if (kind != SAT_OOBLECK_UNIT_NEAREST && kind != SAT_OOBLECK_UNIT_FINAL_DEC) u.bias = in.make("bias", Co);
            if (snake && !to_cf) { u.alpha = in.make("alpha", Co); u.beta = in.make("beta", Co); }
        }
        if (kind == SAT_OOBLECK_UNIT_RESIDUAL) {
            u.weight_g2 = in.make("weight_g2", Co); u.weight_v2 = in.make("weight_v2", (size_t)Co * Co); u.bias2 = in.make("bias2", Co);
            if (snake) { u.alpha2 = in.make("alpha2", Co); u.beta2 = in.make("beta2", Co); }
        }
        if (from_cf) u.in_cf = in.make("in_cf", (size_t)B * Ci * L);
        else u.in = opbuf("in", (size_t)B * L * pad(Ci));
        const int Cout = kind == SAT_OOBLECK_UNIT_CF_TO_CL ? Ci : Co;
        if (to_cf) {
            u.out_cf = in.make("out_cf", (size_t)B * Co * L);
        } else {
            if (kind == SAT_OOBLECK_UNIT_CONV1_RES || kind == SAT_OOBLECK_UNIT_RESIDUAL) u.res = u.out_raw = opbuf("res", (size_t)B * L * pad(Co));
            else u.out_raw = opbuf("out_raw", (size_t)B * Lout * pad(Cout));
            if (kind != SAT_OOBLECK_UNIT_CF_TO_CL) u.out_snk = opbuf("out_snk", (size_t)B * Lout * pad(Cout));
        }
        RC(sat_oobleck_unit, &u, sizeof u, STREAM);
    };
    const int SN = SAT_OOBLECK_ACT_SNAKE, ELU = SAT_OOBLECK_ACT_ELU;
    run("conv7", SAT_OOBLECK_UNIT_CONV7, 96, 80, SN, 0, 3, 0, 0);
    run("conv1_res", SAT_OOBLECK_UNIT_CONV1_RES, 128, 128, ELU, 0, 0, 0, 0);
    run("residual_128", SAT_OOBLECK_UNIT_RESIDUAL, 128, 128, SN, 0, 9, 0, 0);
    run("residual_128_two_launch", SAT_OOBLECK_UNIT_RESIDUAL, 128, 128, SN, 0, 9, 1, 0);
    run("residual_128_elu", SAT_OOBLECK_UNIT_RESIDUAL, 128, 128, ELU, 0, 1, 0, 0);
    run("residual_256", SAT_OOBLECK_UNIT_RESIDUAL, 256, 256, SN, 0, 3, 0, 0);
    run("residual_256_elu", SAT_OOBLECK_UNIT_RESIDUAL, 256, 256, ELU, 0, 3, 0, 0);
    run("residual_512", SAT_OOBLECK_UNIT_RESIDUAL, 512, 512, SN, 0, 1, 0, 0);
    run("residual_200", SAT_OOBLECK_UNIT_RESIDUAL, 200, 200, SN, 0, 1, 0, 0);
    run("convT", SAT_OOBLECK_UNIT_CONVT, 128, 64, SN, 4, 0, 0, 0);
    run("nearest", SAT_OOBLECK_UNIT_NEAREST, 64, 48, ELU, 3, 0, 0, 0);
    run("strided", SAT_OOBLECK_UNIT_STRIDED, 64, 128, SN, 4, 0, 0, 0);
    run("first_conv", SAT_OOBLECK_UNIT_FIRST_CONV, 2, 128, SN, 0, 0, 0, 0);
    run("first_conv_general", SAT_OOBLECK_UNIT_FIRST_CONV, 1, 48, ELU, 0, 0, 0, 0);
    run("final_dec", SAT_OOBLECK_UNIT_FINAL_DEC, 128, 2, SN, 0, 0, 0, 1);
    run("final_enc", SAT_OOBLECK_UNIT_FINAL_ENC, 256, 64, SN, 0, 0, 0, 0);
    run("cf_to_cl", SAT_OOBLECK_UNIT_CF_TO_CL, 20, 0, SN, 0, 0, 0, 0);
    // refused descriptors
    run("refused_kind", 10, 64, 64, SN, 0, 1, 0, 0);
    run("refused_dilation", SAT_OOBLECK_UNIT_CONV7, 64, 64, SN, 0, 2, 0, 0);
    run("refused_odd_convT", SAT_OOBLECK_UNIT_CONVT, 64, 64, SN, 3, 0, 0, 0);
    run("refused_strided_length", SAT_OOBLECK_UNIT_STRIDED, 64, 64, SN, 3, 0, 0, 0);
}

void refusals() {
    case_start("refusals");
    sat_oobleck_plan* p = nullptr;
    auto create = [&](const char* what, sat_oobleck_cfg c, const sat_oobleck_options* o, size_t bytes) {
        line("refusal", what);
        p = nullptr;
        RC(sat_oobleck_plan_create_ex, &c, o, bytes, &p);
        if (p) sat_oobleck_plan_destroy(p);
    };
    const sat_oobleck_options none = {SAT_OOBLECK_ACT_SNAKE, 0, 0};
    create("gemm_dtype_1", cfg_of(SMALL_VAE, true, SAT_GEMM_FP8), nullptr, 0);
    create("gemm_dtype_4", cfg_of(SMALL_VAE, true, 4), nullptr, 0);
    sat_oobleck_cfg c = cfg_of(SMALL_VAE, true, F16);
    c.n_blocks = 9;
    create("n_blocks_9", c, nullptr, 0);
    Vae odd = SMALL_VAE;
    odd.strides[1] = 3;
    create("odd_stride_transposed_decoder", cfg_of(odd, true, F16), nullptr, 0);
    odd.strides[1] = 1;
    create("stride_1_encoder", cfg_of(odd, false, F16), nullptr, 0);
    const sat_oobleck_options dec_opt = {SAT_OOBLECK_ACT_SNAKE, 1, 0}, near_opt = {SAT_OOBLECK_ACT_SNAKE, 0, 1}, bad_act = {2, 0, 0}, bad_flag = {0, 2, 0};
    create("final_tanh_on_encoder", cfg_of(SMALL_VAE, false, F16), &dec_opt, sizeof dec_opt);
    create("nearest_upsample_on_encoder", cfg_of(SMALL_VAE, false, F32), &near_opt, sizeof near_opt);
    create("activation_2", cfg_of(SMALL_VAE, true, F16), &bad_act, sizeof bad_act);
    create("final_tanh_2", cfg_of(SMALL_VAE, true, F16), &bad_flag, sizeof bad_flag);
    create("options_bytes", cfg_of(SMALL_VAE, true, F16), &none, sizeof none + 4);
    c = cfg_of(SMALL_VAE, true, F16);
    c.io_channels = 3;
    create("io_channels_3", c, nullptr, 0);
    c = cfg_of(SMALL_VAE, true, F16);
    c.latent_dim = 0;
    create("latent_dim_0", c, nullptr, 0);
    c = cfg_of(SMALL_VAE, true, F16);
    c.c_mults[2] = 0;
    create("c_mult_0", c, nullptr, 0);
    line("refusal", "null_arguments");
    c = cfg_of(SMALL_VAE, true, F16);
    RC(sat_oobleck_plan_create_ex, nullptr, nullptr, 0, &p);
    RC(sat_oobleck_plan_create_ex, &c, nullptr, 0, nullptr);
    RC(sat_oobleck_plan_create, nullptr, &p);
    line("refusal", "plan_create_contract");
    Vae v = SMALL_VAE;
    v.channels = 100;
    c = cfg_of(v, true, BF16);
    RC(sat_oobleck_plan_create, &c, &p);
    v.channels = 64; v.latent = 20;
    c = cfg_of(v, true, F32);
    RC(sat_oobleck_plan_create, &c, &p);
    c.gemm_dtype = SAT_GEMM_FP8;
    RC(sat_oobleck_plan_create, &c, &p);
    sat_oobleck_unit_desc u{};
    line("refusal", "unit_descriptor");
    RC(sat_oobleck_unit, nullptr, sizeof u, STREAM);
    RC(sat_oobleck_unit, &u, sizeof u - 8, STREAM);
    u.gemm_dtype = SAT_GEMM_FP8;
    RC(sat_oobleck_unit, &u, sizeof u, STREAM);

    line("refusal", "null_plan");
    size_t bytes = 0;
    int32_t n = 0;
    float x[4] = {};
    sat_range_record rec;
    sat_oobleck_plan_destroy(nullptr);
    RC(sat_oobleck_plan_set_tensor, nullptr, "layers.0.bias", x, 4);
    RC(sat_oobleck_plan_finalize, nullptr, STREAM);
    RC(sat_oobleck_workspace_bytes, nullptr, 1, 1, &bytes);
    RC(sat_oobleck_decode, nullptr, x, x, 1, 1, x, 16, STREAM);
    RC(sat_oobleck_encode, nullptr, x, x, 1, 1, x, 16, STREAM);
    RC(sat_oobleck_range_report, nullptr, 1);
    RC(sat_oobleck_range_report_count, nullptr, &n);
    line("name", sat_oobleck_range_report_name(nullptr, 0) ? "set" : "(null)");
    RC(sat_oobleck_range_report_read, nullptr, &rec, 1, sizeof rec, STREAM);
}

// call order and workspace errors on one small decoder (fp16) and encoder (fp32)
void state_errors() {
    case_start("state_errors");
    const Vae v = {64, {1, 2}, {2, 4}, 64, {SAT_OOBLECK_ACT_SNAKE, 0, 0}};
    for (int decoder = 1; decoder >= 0; --decoder) {
        const int dtype = decoder ? F16 : F32, B = 1, T = 2;
        line("plan", decoder ? "decoder" : "encoder");
        const sat_oobleck_cfg c = cfg_of(v, decoder, dtype);
        const sat_oobleck_options o = opt_of(v, decoder);
        sat_oobleck_plan* p = nullptr;
        RC(sat_oobleck_plan_create_ex, &c, &o, sizeof o, &p);
        Inputs weights, in;
        const size_t lat = (size_t)B * c.latent_dim * T, audio = (size_t)B * 2 * T * ratio_of(c);
        float *z = in.make("z", lat), *a = in.make("audio", audio);
        void* ws = in.workspace(1 << 20);
        size_t bytes = 0;
        RC(sat_oobleck_plan_set_tensor, p, nullptr, z, 4);
        RC(sat_oobleck_plan_set_tensor, p, "layers.0.bias", nullptr, 4);
        RC(sat_oobleck_plan_set_tensor, p, "layers.0.bias", z, 0);
        RC(sat_oobleck_workspace_bytes, p, B, T, &bytes);          // before finalize
        RC(sat_oobleck_decode, p, z, a, B, T, ws, 1 << 20, STREAM);
        RC(sat_oobleck_encode, p, a, z, B, T, ws, 1 << 20, STREAM);
        const std::string held = "layers.1.layers.2.layers.1.weight_v";
        set_tensors(p, c, o, weights, held);
        RC(sat_oobleck_plan_finalize, p, STREAM);                  // SAT_E_MISSING, the table is kept
        RC(sat_oobleck_workspace_bytes, p, B, T, &bytes);
        RC(sat_oobleck_plan_set_tensor, p, held.c_str(), weights.make(held, 3), 3);
        RC(sat_oobleck_plan_finalize, p, STREAM);                  // the wrong size
        const size_t C1 = (decoder ? (size_t)c.c_mults[0] : 1) * c.channels;
        RC(sat_oobleck_plan_set_tensor, p, held.c_str(), weights.make(held, C1 * C1 * 7), (int64_t)(C1 * C1 * 7));
        RC(sat_oobleck_plan_finalize, p, STREAM);
        RC(sat_oobleck_workspace_bytes, p, 0, T, &bytes);
        RC(sat_oobleck_workspace_bytes, p, B, T, nullptr);
        RC(sat_oobleck_workspace_bytes, p, B, T, &bytes);
        line("workspace_bytes", B, T, bytes);
        if (decoder) {
            RC(sat_oobleck_encode, p, a, z, B, T, ws, bytes, STREAM);          // the other direction
            RC(sat_oobleck_decode, p, z, a, B, T, ws, bytes - 1, STREAM);      // one byte short
            RC(sat_oobleck_decode, p, z, a, B, T, (char*)ws + 64, bytes, STREAM);
            RC(sat_oobleck_decode, p, nullptr, a, B, T, ws, bytes, STREAM);
            RC(sat_oobleck_decode, p, z, a, B, 0, ws, bytes, STREAM);
            RC(sat_oobleck_decode, p, z, a, B, T, ws, bytes, STREAM);
        } else {
            RC(sat_oobleck_decode, p, z, a, B, T, ws, bytes, STREAM);
            RC(sat_oobleck_encode, p, a, z, B, T, ws, bytes - 1, STREAM);
            RC(sat_oobleck_encode, p, a, z, B, T, (char*)ws + 64, bytes, STREAM);
            RC(sat_oobleck_encode, p, a, nullptr, B, T, ws, bytes, STREAM);
            RC(sat_oobleck_encode, p, a, z, 0, T, ws, bytes, STREAM);
            RC(sat_oobleck_encode, p, a, z, B, T, ws, bytes, STREAM);
        }
        RC(sat_oobleck_plan_finalize, p, STREAM);                  // a second finalize: the table is empty by now
        sat_oobleck_plan_destroy(p);
    }
}

}  // namespace

int main() {
    for (int dtype : ALL) {
        codec_case("stable_audio", STABLE_AUDIO, true, dtype, 1, 3);
        codec_case("stable_audio", STABLE_AUDIO, false, dtype, 1, 1);
    }
    for (int dtype : ALL) {
        codec_case("small_vae", SMALL_VAE, true, dtype, 2, 3);
        codec_case("small_vae", SMALL_VAE, false, dtype, 2, 1);
    }
    const struct { const char* name; const Vae* v; } options[] = {{"ref_defaults", &REF_DEFAULTS}, {"nearest_snake", &NEAREST_SNAKE}, {"narrow_all", &NARROW_ALL}, {"nearest_odd", &NEAREST_ODD}};
    for (auto& o : options)
        for (int dtype : {F16, F32}) {
            codec_case(o.name, *o.v, true, dtype, 2, 5);
            if (o.v->opt.activation == SAT_OOBLECK_ACT_ELU) codec_case(o.name, *o.v, false, dtype, 1, 2);      // the other options are the decoder's
        }
    for (int dtype : ALL)
        for (int decoder = 1; decoder >= 0; --decoder) report_case(decoder, dtype);
    for (int dtype : ALL) unit_cases(dtype);
    refusals();
    state_errors();
    return 0;
}
