// Host side of libr50hip.so: C ABI declared in include/r50.h, include/r50_hal.h, include/r50_smooth.h, include/r50_multiview.h,
// include/r50_kinematics.h, include/r50_refine.h, include/r50_track.h, include/r50_resample.h and include/r50_bootstrap.h.
// Builds the static ResNet-50 [:-1] schedule (upstream torchvision models/resnet.py, the module
// list the reference cuts at src/preprocess_resnet_features.py:207-209), folds BN, packs weights
// and launches the gfx950 kernels of kernels.h.
#include "kernels.h"
#include "smooth_kernels.h"
#include "multiview_kernels.h"
#include "kinematics_kernels.h"
#include "refine_kernels.h"
#include "track_kernels.h"
#include "resample_kernels.h"
#include "bootstrap_kernels.h"
#include "launch_plan.h"
#include "../../include/r50.h"
#include "../../include/r50_hal.h"
#include "../../include/r50_smooth.h"
#include "../../include/r50_multiview.h"
#include "../../include/r50_kinematics.h"
#include "../../include/r50_refine.h"
#include "../../include/r50_track.h"
#include "../../include/r50_resample.h"
#include "../../include/r50_bootstrap.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

namespace {

using namespace launch_plan;
static_assert(kBf16 == R50_PREC_BF16 && kFp32x == R50_PREC_FP32X && kBf16w2 == R50_PREC_BF16W2 && kFp16 == R50_PREC_FP16 && kFp8 == R50_PREC_FP8,
              "launch_plan.h restates the precisions of r50.h");

thread_local std::string g_err;   // errors raised without a handle (r50_create, r50_op_*)

struct Prof {
    const char* name;
    int64_t launches = 0;
    double ms = 0, flops = 0, bytes = 0;
};
enum ProfClass { PC_IGEMM = 0, PC_STEM_CONV, PC_MAXPOOL, PC_AVGPOOL, PC_STEM_PACK, PC_TAIL, PC_TAIL3, PC_BLOCK2, PC_CATCHAIN, PC_COUNT };
const char* kProfNames[PC_COUNT] = {"igemm", "conv1", "maxpool", "avgpool", "stem_pack", "bneck_tail", "bneck_tail3", "bneck_block2", "bneck_catchain"};

struct EvRec {
    hipEvent_t a, b;
    int cls;
    int layer;        // index into convs (per-layer breakdown) or -1
    double flops, bytes;
};

struct ConvLayer : ConvShape {
    std::string conv_key, bn_key;
    __bf16* w = nullptr;    // device, (cout, ks, ks, cin)
    float* bias = nullptr;  // device
    // fp8 mode, layer2-4: w holds e4m3 bytes with real value = byte value x wscale; bias_scaled = bias / (sx * wscale) once the
    // activation scales are known (r50_set_fp8_scales)
    float wscale = 1.0f;
    float* bias_scaled = nullptr;
    std::vector<float> bias_host;
    std::vector<float> w_host;   // fp8 mode, conv3 / downsample of a stage's first block: folded fp32 weights (OIHW), requantised
                                 // with a common accumulator scale once the activation scales are known
};

}  // namespace

struct r50_handle {
    int device = 0;
    int precision = R50_PREC_BF16;
    int max_batch = 0;
    int micro_batch = 0;
    int profile = 0;
    int tile_override = 0;
    int overlap_ds = 0;                 // downsample conv of a stage's first block on a side stream
    hipStream_t ds_stream = nullptr;
    hipEvent_t ev_ds_fork = nullptr, ev_ds_join = nullptr;
    int fused_stem = 1;                 // bf16 mode: conv1+bn1+relu+maxpool in one kernel
    int fuse_stem_c1 = 1;               // strip stem kernel also computes layer1.0.conv1
    std::vector<float> fp8_scales;      // R50_PREC_FP8: activation scales, execution order (r50_set_fp8_scales)
    float cat_acc_scale[4] = {0.f, 0.f, 0.f, 0.f};   // fp8 two-source conv of layer2.0 / 3.0 / 4.0: real value of one accumulator unit
    int fuse_ds_cat = 1;                // layer2.0 / 3.0 / 4.0: conv3 and the downsample conv as one GEMM over K = [t2 | x at stride 2]
    __bf16* cat_w[4] = {nullptr, nullptr, nullptr, nullptr};      // per stage: (cout, cmid + cin) = [W3 | Wd], device
    float* cat_bias[4] = {nullptr, nullptr, nullptr, nullptr};    // b3 + bd (fp32)
    int fuse_tail = 1;                  // bf16 mode, layer1: conv3 + identity + ReLU + the next block's conv1 in one kernel
    int fuse_fp8_handover = 1;          // fp8 mode: quantise layer1's output in layer1.2.conv3's epilogue instead of in a pass of its own
    int fuse_tail3 = 1;                 // layer3.1-.4: conv3 + identity + ReLU chained with the next block's conv1 through LDS (bneck_tail3_kernel)
    __bf16* catchain_wp = nullptr;      // layer2.0: [W3 | Wd] and layer2.1.conv1 in bneck_catchain_kernel's fragment-ordered stream
    int fuse_tail3_last = 1;            // layer3.5: conv3 + identity + ReLU through the pipelined tail kernel without a second GEMM
    int fuse_cat_chain = 1;             // layer2.0: conv3 + downsample + ReLU chained with layer2.1.conv1 in one launch (bneck_catchain_kernel)
    int sub_out = 1;                    // layer1.2 stores only the even rows / columns of its output (its readers: the fused layer2.0.conv1 and the stride-2 downsample
                                        // conv inside bneck_catchain_kernel); needs fuse_block1 >= 2 and the chained layer2.0 tail, else the full tensor is written
    __bf16* tail3_wp[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // per layer3 block b: [W3(b) | W1(b+1)] in the kernel's fragment order
    int fuse_block1 = 3;                // 1: layer1.1, 2 (default since round 3: with the loaders' position loop unrolled the c1 = 128 form takes 248 us against
                                        // 276 for conv2 + fused tail): also layer1.2 -- the bottleneck body in one launch (bneck_block1_kernel)
    int fuse_block2 = 1;                // layer2.1-.3: the whole bottleneck body (conv2 + conv3 + identity + ReLU [+ next conv1]) in one launch
    int inplace_out = 0;                // plain-identity blocks write their output over their input (same bits, fewer DRAM page switches)
    int n_streams = 1;                  // > 1: the batch is split over internal streams (forked from / joined to the caller's)
    hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    bool loaded = false;
    // r50_share_weights: this handle reads the weight buffers of `owner` (convs[].w / bias, cat_w / cat_bias, tail3_wp, catchain_wp, stem_w) and
    // frees none of them; the owner counts its sharers and, if destroyed first, stays alive (weights only) until the last sharer is gone
    r50_handle* owner = nullptr;
    int sharers = 0;
    bool zombie = false;
    std::string err;
    std::vector<ConvLayer> convs;       // execution order, convs[0] = stem
    char* stem_w = nullptr;             // packed stem weights (device)
    char* stem_xp = nullptr;            // packed input image (device)
    float* u8_table = nullptr;          // [3][256]: uint8 sample -> normalised fp32, for r50_forward_u8 (device)
    __bf16* buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t buf_bytes = 0;
    Prof prof[PC_COUNT];
    std::vector<Prof> prof_layer;       // one entry per conv, same order as convs
    std::vector<EvRec> ev_pending;
    std::vector<hipEvent_t> ev_free;
};

namespace {

int fail(r50_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    g_err = msg;
    return code;
}

// What fill_conv_args* and every launch_* function answer, by value: launched; refused before anything was queued (a size rule's refusal
// carries the quantity, its value and the bound; any other refusal carries no note); or what HIP said.  No string is built unless a
// message is: profiled() and Op::done() below are the two places that turn a Launch into a status and a text.
struct Launch {
    enum Kind { Launched, Refused, Hip } kind = Launched;
    hipError_t hip = hipSuccess;                                // Hip: the runtime's status
    const char *quantity = nullptr, *bound = nullptr;           // Refused by a size rule: "<quantity> = <value> must be < <bound>"
    long long value = 0;
    Launch(hipError_t e = hipSuccess) : kind(e == hipSuccess ? Launched : Hip), hip(e) {}
    static Launch refused() { Launch r; r.kind = Refused; return r; }
    bool ok() const { return kind == Launched; }
    std::string note(const char* unnoted = "") const {             // a size rule's note, else `unnoted`
        return quantity ? std::string(quantity) + " = " + std::to_string(value) + " must be < " + bound : std::string(unnoted);
    }
    std::string suffix() const { return quantity ? ": " + note() : std::string(); }     // behind a message that already names the op
    const char* hip_text() const { return hipGetErrorString(kind == Refused ? hipErrorInvalidValue : hip); }
};

// Size limits (include/r50.h states them per entry point; DESIGN.md section 4, "Size limits"): fill_conv_args and the launchers check them
// with size_over, which turns `r` into the refusal that names the quantity, its value and the bound.
bool size_over(Launch& r, const char* quantity, long long value, long long bound, const char* bound_text) {
    if (value < bound) return false;
    r = Launch::refused();
    r.quantity = quantity; r.value = value; r.bound = bound_text;
    return true;
}
constexpr long long k2p31 = 1ll << 31;

// The frame of an entry point: its name, once, and the three ways it answers.  Every r50_op_* hook makes one (`h` stays null: the text goes
// to r50_last_error(NULL)); r50_forward* make one with their handle for the alignment check.
//   aligned   Pointer alignment (include/r50.h): every device pointer annotated R50_ALIGNED(n) in a header is checked under the header's
//             parameter name before the entry point's first launch, copy or attribute call: after its null checks, or as its first
//             statement where those live in the launcher (NULL, allowed or not, counts as aligned, so a null pointer is still answered
//             by the null check).  0, or R50_ERR_INVALID with a message that names the parameter and the bytes.
//   refuse    R50_ERR_INVALID, "<name>: <why>".
//   done      the launcher's answer, or the runtime's last error: R50_OK, or "<name>: <the size note, else the HIP error string>".  A
//             launcher's refusal is R50_ERR_INVALID, and so is hipErrorInvalidValue from the runtime inside a launcher (DESIGN.md
//             section 4 records that conflation); every other failure is R50_ERR_HIP.
//   hip_failed  R50_ERR_HIP, "<name>: <what>", where no HIP status says more.
struct AlignedArg { const void* p; const char* name; unsigned bytes; };
struct Op {
    const char* name;
    r50_handle* h = nullptr;
    int aligned(std::initializer_list<AlignedArg> args) const {
        for (const AlignedArg& a : args)
            if ((uintptr_t)a.p & (uintptr_t)(a.bytes - 1u)) return refuse(std::string(a.name) + " must be " + std::to_string(a.bytes) + "-byte aligned");
        return 0;
    }
    int refuse(const std::string& why) const { return fail(h, R50_ERR_INVALID, std::string(name) + ": " + why); }
    int hip_failed(const char* what) const { return fail(h, R50_ERR_HIP, std::string(name) + ": " + what); }
    int done(hipError_t e = hipGetLastError()) const { return e != hipSuccess ? hip_failed(hipGetErrorString(e)) : R50_OK; }
    int done(const Launch& r) const {
        if (r.ok()) return R50_OK;
        if (r.kind == Launch::Hip && r.hip != hipErrorInvalidValue) return done(r.hip);
        return refuse(r.note(r.hip_text()));
    }
};

// Element-type dispatch: the <1, rest...> (IEEE half) or <0, rest...> (bf16) instantiation of a kernel or launcher template, as a pointer;
// and the launch of the one the element type selects.
#define R50_BY_ET(et, tmpl, ...) ((et) == 1 ? tmpl<1, ##__VA_ARGS__> : tmpl<0, ##__VA_ARGS__>)
#define R50_ET_LAUNCH(et, kern, grid, block, lds, stream, ...) \
    hipLaunchKernelGGL(R50_BY_ET(et, kern), grid, block, lds, (hipStream_t)(stream), __VA_ARGS__)

// Workgroups of 256 threads for n elements, at least one and at most `cap` (the kernels walk the rest in a grid-stride loop)
unsigned ew_grid(long long n, long long cap = 256 * 32) { return (unsigned)std::min<long long>(std::max<long long>((n + 255) / 256, 1), cap); }

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(h, R50_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)

inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

constexpr float kBnEps = 1e-5f;

std::vector<ConvLayer> make_specs() {       // the table of launch_plan.h, with room for the weights
    std::vector<ConvLayer> v;
    for (const ConvSpec& spec : conv_specs()) {
        ConvLayer L;
        static_cast<ConvShape&>(L) = spec.shape;
        L.conv_key = spec.conv_key; L.bn_key = spec.bn_key;
        v.push_back(L);
    }
    return v;
}

// BN fold in fp32, op order fixed (no contraction: built with -ffp-contract=off):
//   scale = gamma / sqrt(var + eps);  w' = w * scale;  b' = beta - mean * scale
void fold_bn(const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
             int cout, int per_out, std::vector<float>& wf, std::vector<float>& bf) {
    wf.resize((size_t)cout * per_out);
    bf.resize(cout);
    for (int o = 0; o < cout; ++o) {
        const float ve = var[o] + kBnEps;
        const float sd = std::sqrt(ve);
        const float scale = gamma[o] / sd;
        for (int i = 0; i < per_out; ++i) wf[(size_t)o * per_out + i] = w[(size_t)o * per_out + i] * scale;
        const float ms = mean[o] * scale;
        bf[o] = beta[o] - ms;
    }
}

// (cout, cin, k, k) fp32 -> (cout, k, k, cin) bf16
// fp32 -> IEEE half, round to nearest even, saturating at +-65504 (the kernels' conversion does the same)
inline uint16_t f32_to_f16_rne(float f) {
    if (f > 65504.0f) f = 65504.0f;
    if (f < -65504.0f) f = -65504.0f;
    const _Float16 hv = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &hv, 2);
    return u;
}

void pack_ohwi_f16(const float* wf, int cout, int cin, int ks, std::vector<uint16_t>& out) {
    out.resize((size_t)cout * ks * ks * cin);
    for (int o = 0; o < cout; ++o)
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < ks * ks; ++t)
                out[((size_t)o * ks * ks + t) * cin + c] = f32_to_f16_rne(wf[((size_t)o * cin + c) * ks * ks + t]);
}

// fp32 -> OCP e4m3 (fn: no infinities, S.1111.111 = NaN), round to nearest even, saturating at +-448
inline uint8_t f32_to_e4m3(float v) {
    const uint8_t sign = std::signbit(v) ? 0x80 : 0x00;
    float a = std::fabs(v);
    if (!(a == a)) return (uint8_t)(sign | 0x7f);
    if (a >= 448.0f) return (uint8_t)(sign | 0x7e);
    if (a < 0.015625f) {                                   // below 2^-6: subnormals, step 2^-9
        const int q = (int)std::nearbyint(a * 512.0f);     // 0 .. 8 (8 = the smallest normal)
        return (uint8_t)(sign | q);
    }
    int e;
    const float m = std::frexp(a, &e);                     // a = m * 2^e, m in [0.5, 1)
    int q = (int)std::nearbyint((m * 2.0f - 1.0f) * 8.0f); // mantissa steps of the binade [2^(e-1), 2^e)
    int ex = e - 1;
    if (q == 8) { q = 0; ++ex; }
    if (ex > 8 || (ex == 8 && q > 6)) return (uint8_t)(sign | 0x7e);
    return (uint8_t)(sign | ((ex + 7) << 3) | q);
}
// (cout, cin, k, k) fp32 -> (cout, k, k, cin) e4m3 bytes with one scale for the tensor (absmax / 448); returns the scale
float pack_ohwi_fp8(const float* wf, int cout, int cin, int ks, std::vector<uint16_t>& out) {
    const size_t total = (size_t)cout * ks * ks * cin;
    float amax = 0.f;
    for (size_t i = 0; i < total; ++i) amax = std::fmax(amax, std::fabs(wf[i]));
    const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
    out.assign((total + 1) / 2, 0);
    uint8_t* o = reinterpret_cast<uint8_t*>(out.data());
    for (int oc = 0; oc < cout; ++oc)
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < ks * ks; ++t)
                o[((size_t)oc * ks * ks + t) * cin + c] = f32_to_e4m3(wf[((size_t)oc * cin + c) * ks * ks + t] / scale);
    return scale;
}

inline float absmax_of(const std::vector<float>& v) {
    float a = 0.f;
    for (float x : v) a = std::fmax(a, std::fabs(x));
    return a;
}

void pack_ohwi_bf16(const float* wf, int cout, int cin, int ks, std::vector<uint16_t>& out) {
    out.resize((size_t)cout * ks * ks * cin);
    for (int o = 0; o < cout; ++o)
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < ks * ks; ++t)
                out[((size_t)o * ks * ks + t) * cin + c] = f32_to_bf16_rne(wf[((size_t)o * cin + c) * ks * ks + t]);
}

inline float bf16_to_f32(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// split mode: (cout, cin, k, k) fp32 -> (cout, k, k, [w_head(cin) | w_head(cin) | w_tail(cin)]) bf16,
// w_head = bf16(w), w_tail = bf16(w - w_head); pairs with X = [x_head | x_tail | x_head]
void pack_ohwi_split(const float* wf, int cout, int cin, int ks, std::vector<uint16_t>& out) {
    out.resize((size_t)cout * ks * ks * 3 * cin);
    for (int o = 0; o < cout; ++o)
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < ks * ks; ++t) {
                const float w = wf[((size_t)o * cin + c) * ks * ks + t];
                const uint16_t hd = f32_to_bf16_rne(w);
                const uint16_t tl = f32_to_bf16_rne(w - bf16_to_f32(hd));
                uint16_t* row = &out[((size_t)o * ks * ks + t) * 3 * cin];
                row[c] = hd; row[cin + c] = hd; row[2 * cin + c] = tl;
            }
}

// bf16w2 mode: (cout, cin, k, k) fp32 -> (cout, k, k, [w_head(cin) | w_tail(cin)]) bf16; pairs with X = [x | x]
// (the X chunk index wraps after cin/64, ConvArgs::x_wrap), i.e. x*w_head + x*w_tail with ONE fp32 accumulator.
void pack_ohwi_w2(const float* wf, int cout, int cin, int ks, std::vector<uint16_t>& out) {
    out.resize((size_t)cout * ks * ks * 2 * cin);
    for (int o = 0; o < cout; ++o)
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < ks * ks; ++t) {
                const float w = wf[((size_t)o * cin + c) * ks * ks + t];
                const uint16_t hd = f32_to_bf16_rne(w);
                const uint16_t tl = f32_to_bf16_rne(w - bf16_to_f32(hd));
                uint16_t* row = &out[((size_t)o * ks * ks + t) * 2 * cin];
                row[c] = hd; row[cin + c] = tl;
            }
}

inline int perm_row_to_cout(int rho) {   // LDS/MFMA row -> channel inside a 32-row group (kernels.h)
    return (rho & ~31) | (rho & 3) | (((rho >> 4) & 1) << 2) | (((rho >> 2) & 3) << 3);
}

// stem: (64,3,7,7) fp32 folded -> [kh][rho][j=0..7][c=0..3] bf16, j = kw + 1, zero elsewhere
void pack_stem(const float* wf, std::vector<uint16_t>& out, int part = 0) {   // part: 0 = bf16(w), 1 = tail bf16(w - head), 2 = fp16(w)
    out.assign((size_t)7 * 64 * 32, 0);
    for (int kh = 0; kh < 7; ++kh)
        for (int rho = 0; rho < 64; ++rho) {
            const int o = perm_row_to_cout(rho);
            for (int kw = 0; kw < 7; ++kw)
                for (int c = 0; c < 3; ++c)
                {
                    const float w = wf[(((size_t)o * 3 + c) * 7 + kh) * 7 + kw];
                    const uint16_t hd = f32_to_bf16_rne(w);
                    out[(((size_t)kh * 64 + rho) * 8 + (kw + 1)) * 4 + c] = part == 2 ? f32_to_f16_rne(w) : part ? f32_to_bf16_rne(w - bf16_to_f32(hd)) : hd;
                }
        }
}

// n / d for n < 2^31 as (umulhi(n, mul) >> shr): mul = ceil(2^(32+shr) / d), shr = ceil(log2 d) - 1
// (exact: the error term n*e/2^(32+shr) stays below 1/d because n < 2^31 <= 2^(32+shr)/d).
FastDiv make_fast_div(unsigned d) {
    FastDiv f{0u, 0u};
    if (d <= 1u) return f;
    unsigned L = 0;
    while ((1ull << L) < d) ++L;
    f.shr = L - 1;
    const unsigned long long num = 1ull << (32 + f.shr);
    f.mul = (unsigned)((num + d - 1) / d);
    return f;
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
// Tile-config ids of igemm_bf16_kernel (BC couts x BP pixels):
//   4 waves, 2 LDS stages:                1 = 128x128, 2 = 64x128, 3 = 64x256, 5 = 128x64
//   8 waves, 3 LDS stages, counted vmcnt: 6 = 256x128, 7 = 128x256, 8 = 128x128
//   8 waves, 2 LDS stages, 128 accumulator registers: 9 = 256x256 (wave 64c x 128p), 10 = 256x256 (wave 128c x 64p)
//   8 waves, 2 LDS stages, pixel counts that divide M = 2^10 * 49: 11 = 256x208 (wave 32c x 208p), 12 = 256x224 (wave 64c x 112p)
//   + 32: chip-sized persistent grid (tiles streamed through the LDS ring) instead of one tile per workgroup
constexpr int kPersistBit = 32;
int g_num_cus = 0;
// Workgroups a persistent launch may put on the chip: the CU count, or R50_CU_CAP / the "cu_cap" option when several internal streams
// share the chip (each stream's launches then take their share of the CUs and run beside the other streams' launches).
int g_cu_cap = [] { const char* v = std::getenv("R50_CU_CAP"); return v ? std::atoi(v) : 0; }();
int cu_budget(int device_cus) { return (g_cu_cap > 0 && g_cu_cap < device_cus) ? g_cu_cap : device_cus; }
int num_cus() {          // 0: the device could not be queried
    if (g_num_cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        g_num_cus = cu_budget(prop.multiProcessorCount);
    }
    return g_num_cus;
}

// A persistent kernel: at most one workgroup per CU of the budget, the workgroups stream `tiles` tiles.  The dynamic-LDS attribute is set on
// every launch: it is per device, and a process may hold handles on several devices.
template <typename K, typename... Args>
Launch launch_persistent(K kern, long long tiles, int threads, size_t lds, hipStream_t s, Args... args) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int cus = num_cus();
    if (cus == 0) return hipErrorInvalidDevice;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles < cus ? tiles : cus)), dim3(threads), lds, s, args...);
    return hipGetLastError();
}

template <int ET, int BC, int BP, int WC, int WP, int NSTAGE, bool SPLIT = false>
Launch launch_igemm_t(ConvArgs a, bool persistent, hipStream_t s) {
    a.n_ctiles = a.Cout / BC;
    a.n_blocks = a.n_ctiles * ((a.M + BP - 1) / BP);
    a.div_ctiles = make_fast_div((unsigned)a.n_ctiles);
    constexpr int kRowsPerPass = WC * WP * 8;
    const size_t lds = (size_t)NSTAGE * (BC + (BP + kRowsPerPass - 1) / kRowsPerPass * kRowsPerPass) * 128;
    auto kern = igemm_bf16_kernel<ET, BC, BP, WC, WP, NSTAGE, SPLIT>;
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    int grid = a.n_blocks;
    if (persistent) {
        const int cus = num_cus();
        if (cus == 0) return hipErrorInvalidDevice;
        // resident workgroups per CU (LDS / registers / wave slots).  No workgroup waits on another one,
        // so an optimistic answer only queues the surplus workgroups; it cannot deadlock.
        static int per_cu = 0;
        if (per_cu == 0) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, WC * WP * 64, lds) != hipSuccess || n < 1) n = 1;
            per_cu = n;
        }
        if (grid > cus * per_cu) grid = cus * per_cu;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WC * WP * 64), lds, s, a);
    return hipGetLastError();
}

// Tile choice.  For the 23 conv shapes of ResNet-50 at large batch the table holds the variant measured
// fastest on an MI355X at batch 256 (scripts/layer_bench.py, profiles/r01_layer_bench.txt); anything else
// falls back to a shape rule.
struct TunedTile { int h, cin, cout, ks, stride, res, tile; };
constexpr TunedTile kTuned[] = {
    {56, 64, 64, 1, 1, 0, 73},    {56, 64, 64, 3, 1, 0, 2},     {56, 64, 256, 1, 1, 1, 72},   {56, 64, 256, 1, 1, 0, 38},
    {56, 256, 64, 1, 1, 0, 73},    {56, 256, 128, 1, 1, 0, 40},  {56, 128, 128, 3, 2, 0, 65},   {28, 128, 512, 1, 1, 1, 72},
    {56, 256, 512, 1, 2, 0, 42},  {28, 512, 128, 1, 1, 0, 65},   {28, 128, 128, 3, 1, 0, 72},  {28, 512, 256, 1, 1, 0, 72},
    {28, 256, 256, 3, 2, 0, 44},  {14, 256, 1024, 1, 1, 1, 72}, {28, 512, 1024, 1, 2, 0, 72}, {14, 1024, 256, 1, 1, 0, 44},
    {14, 256, 256, 3, 1, 0, 68},  {14, 1024, 512, 1, 1, 0, 72}, {14, 512, 512, 3, 2, 0, 68},  {7, 512, 2048, 1, 1, 1, 43},
    {14, 1024, 2048, 1, 2, 0, 43}, {7, 2048, 512, 1, 1, 0, 72}, {7, 512, 512, 3, 1, 0, 68},
};

// Role-specialised kernel (loader waves + consumer waves), always one persistent workgroup per CU: tile id + 64
constexpr int kWsBit = 64;

template <int ET, int BC, int BP, int CWC, int CWP, int NLOAD, int NSTAGE>
Launch launch_igemm_ws_t(ConvArgs a, hipStream_t s) {
    a.n_ctiles = a.Cout / BC;
    a.n_blocks = a.n_ctiles * ((a.M + BP - 1) / BP);
    a.div_ctiles = make_fast_div((unsigned)a.n_ctiles);
    constexpr int kRowsPerPass = NLOAD * 8;
    const size_t lds = (size_t)NSTAGE * (BC + (BP + kRowsPerPass - 1) / kRowsPerPass * kRowsPerPass) * 128;
    return launch_persistent(igemm_ws_kernel<ET, BC, BP, CWC, CWP, NLOAD, NSTAGE>, a.n_blocks, (CWC * CWP + NLOAD) * 64, lds, s, a);
}

// layer1 conv2 shape (3x3 s1 p1, 64 -> 64, 56x56): filter bank resident in LDS (kernels.h: conv3x3_c64_kernel); tile id 64+16
constexpr int kTileC64 = kWsBit | 16;
bool is_c64_shape(const ConvArgs& a) {
    return a.ks == 3 && a.stride == 1 && a.pad == 1 && a.Cin == 64 && a.Cout == 64 && a.H == 56 && a.W == 56 && a.res == nullptr &&
           a.x_cstride == 64 && a.y_cstride == 64 && a.Ktot == 576;
}
template <int ET>
Launch launch_conv3x3_c64(const ConvArgs& a, hipStream_t s) {
    if (!is_c64_shape(a)) return Launch::refused();
    constexpr size_t lds = 9 * 64 * 128 + 2 * 352 * 128;      // 163,840 = all of the CU's LDS
    return launch_persistent(conv3x3_c64_kernel<ET>, a.N * 14, 512, lds, s, a);
}

// conv2 of the non-first blocks of layer2 / layer3 / layer4 (3x3 s1 p1, Cin = Cout): input-resident kernel (kernels.h: conv3x3_xres_kernel);
// tile id 64+17.  Chosen for these shapes at EVERY batch size: its K order differs from the generic kernel's.
constexpr int kTileXres = kWsBit | 17;
bool is_xres_shape(const ConvArgs& a) {
    if (!(a.ks == 3 && a.stride == 1 && a.pad == 1 && a.Cin == a.Cout && a.H == a.W && a.res == nullptr && a.x2 == nullptr &&
          a.x_cstride == a.Cin && a.y_cstride == a.Cout && a.Ktot == 9 * a.Cin && a.et != 2)) return false;
    return (a.H == 14 && a.Cin == 256) || (a.H == 7 && a.Cin == 512) || (a.H == 28 && a.Cin == 128);
}
template <int ET, int NI, int TR, int IW, int IH>
Launch launch_conv3x3_xres_t(ConvArgs a, hipStream_t s) {
    constexpr int BC = 128, NST = 3;
    constexpr int PW = IW == 28 ? 32 : 16;
    constexpr int PPT = IW == 7 ? 17 * 16 : NI * (TR + 2) * PW, XBUF = (PPT + 31) / 32 * 32 * 128;
    constexpr size_t lds = 2 * (size_t)XBUF + NST * (size_t)BC * 128;
    static_assert(lds <= 163840, "LDS budget");
    a.n_ctiles = a.Cout / BC;
    a.n_blocks = ((a.N + NI - 1) / NI) * (IH / TR) * a.n_ctiles;
    return launch_persistent(conv3x3_xres_kernel<ET, NI, TR, IW, IH>, a.n_blocks, 768, lds, s, a);
}
template <int ET>
Launch launch_conv3x3_xres(const ConvArgs& a, hipStream_t s) {
    if (!is_xres_shape(a)) return Launch::refused();
    // The row-block form (kernels.h): 128 couts x 196 pixels per tile, one tap per step, ring of three 16-KB weight stages, static loader schedule.
    // 14x14: one image per tile (512 tiles = two full rounds at batch 256); 28x28: a 7-row band; 7x7: four images (two pairs per 16-position row).
    // Rounds 2-3 carried eleven more schedules of this kernel (13-block addressing, mid-step barriers, rings of 4-5 stages, staggered SIMD partners,
    // 256 couts per tile, the 32x32x16 MFMA): all bit-identical, all measured slower or equal (profiles/r03_xres_variants.txt), removed in round 4.
    if (a.H == 14) return launch_conv3x3_xres_t<ET, 1, 14, 14, 14>(a, s);
    if (a.H == 28) return launch_conv3x3_xres_t<ET, 1, 7, 28, 28>(a, s);
    return launch_conv3x3_xres_t<ET, 4, 7, 7, 7>(a, s);
}

// conv2 of layer2.0 / layer3.0 / layer4.0 (3x3 STRIDE 2 p1, Cin = Cout, 56 -> 28 x 128, 28 -> 14 x 256, 14 -> 7 x 512): input resident by polyphase planes (kernels.h:
// conv3x3_s2_kernel); tile id 64+18.  Chosen for these shapes at EVERY batch size: its K order differs from the generic kernel's.
constexpr int kTileS2 = kWsBit | 18;
bool is_s2_shape(const ConvArgs& a) {
    if (!(a.ks == 3 && a.stride == 2 && a.pad == 1 && a.Cin == a.Cout && a.H == a.W && a.res == nullptr && a.x2 == nullptr &&
          a.x_cstride == a.Cin && a.y_cstride == a.Cout && a.Ktot == 9 * a.Cin && a.et != 2)) return false;
    return (a.H == 56 && a.Cin == 128) || (a.H == 28 && a.Cin == 256) || (a.H == 14 && a.Cin == 512);
}
template <int ET, int TR, int OW, int OH>
Launch launch_conv3x3_s2_t(ConvArgs a, hipStream_t s) {
    constexpr size_t lds = 3 * 32768 + 3 * 128 * 128;
    a.n_ctiles = a.Cout / 128;
    a.n_blocks = (OW == 7 ? (a.N + 3) / 4 : a.N * (OH / TR)) * a.n_ctiles;
    return launch_persistent(conv3x3_s2_kernel<ET, 128, TR, OW, OH>, a.n_blocks, 768, lds, s, a);
}
template <int ET>
Launch launch_conv3x3_s2(const ConvArgs& a, hipStream_t s) {
    if (!is_s2_shape(a)) return Launch::refused();
    if (a.H == 56) return launch_conv3x3_s2_t<ET, 7, 28, 28>(a, s);
    if (a.H == 14) return launch_conv3x3_s2_t<ET, 7, 7, 7>(a, s);          // four images per tile (two pairs)
    return launch_conv3x3_s2_t<ET, 14, 14, 14>(a, s);
}

// 1x1 convs with both operands streaming (layer3 / layer4, K >= 256) as a 256 x 256 / 256 x 224 GEMM tile on the eight-phase schedule
// (kernels.h: gemm8p_kernel); tile ids 64+19 (256 pixels) and 64+20 (224 pixels).  One or two K sources.  Same bits as tile ids 9 / 12.
constexpr int kTileG8 = kWsBit | 19;
constexpr int kTileG8N7 = kWsBit | 20;
bool is_g8_shape(const ConvArgs& a) {
    return a.ks == 1 && a.pad == 0 && a.Cout % 256 == 0 && a.et != 2 && a.x_wrap >= (1 << 30) && a.q_inv == 0.f &&
           a.y_cstride == a.Cout && a.nk >= 1 && (a.x2 ? (a.stride == 1 && a.cc1 >= 1 && a.cc1 < a.nk) : a.x_cstride == a.Cin);
}
template <int ET, int NR, bool DUAL>
Launch launch_gemm8p_t(ConvArgs a, hipStream_t s) {
    constexpr int BP = 32 * NR;
    constexpr size_t lds = 2 * 4 * 16384;
    a.n_ctiles = a.Cout / 256;
    a.n_blocks = a.n_ctiles * ((a.M + BP - 1) / BP);
    a.div_ctiles = make_fast_div((unsigned)a.n_ctiles);
    return launch_persistent(gemm8p_kernel<ET, NR, DUAL>, a.n_blocks, 512, lds, s, a);
}
template <int ET>
Launch launch_gemm8p(const ConvArgs& a, int tile, hipStream_t s) {
    if (!is_g8_shape(a)) return Launch::refused();
    if (a.x2) return tile == kTileG8N7 ? launch_gemm8p_t<ET, 7, true>(a, s) : launch_gemm8p_t<ET, 8, true>(a, s);
    return tile == kTileG8N7 ? launch_gemm8p_t<ET, 7, false>(a, s) : launch_gemm8p_t<ET, 8, false>(a, s);
}

// tiles a launch of tile id `tile` would have (0 if the id does not divide this Cout)
long long tiles_of(const ConvArgs& a, int tile) {
    int bc = 0, bp = 0;
    if (tile & kWsBit) {
        switch (tile & (kPersistBit - 1)) {
            case 1: bc = 128; bp = 128; break;  case 3: bc = 256; bp = 128; break;  case 4: case 8: bc = 128; bp = 224; break;
            case 9: bc = 64; bp = 224; break;   case 10: bc = 128; bp = 208; break;   case 19: bc = 256; bp = 256; break;   case 20: bc = 256; bp = 224; break;
            default: return 0;
        }
    } else {
        switch (tile & (kPersistBit - 1)) {
            case 1: case 8: bc = 128; bp = 128; break;  case 2: bc = 64; bp = 128; break;   case 3: bc = 64; bp = 256; break;
            case 5: bc = 128; bp = 64; break;           case 6: bc = 256; bp = 128; break;  case 7: bc = 128; bp = 256; break;
            case 9: case 10: bc = 256; bp = 256; break; case 11: bc = 256; bp = 208; break; case 12: bc = 256; bp = 224; break;
            default: return 0;
        }
    }
    if (a.Cout % bc) return 0;
    return (long long)(a.Cout / bc) * ((a.M + bp - 1) / bp);
}

int g_use_xres = [] { const char* v = std::getenv("R50_XRES"); return v ? std::atoi(v) : 1; }();      // A/B knob: 0 = generic igemm tiles for the 3x3 s1 shapes
int g_use_s2 = [] { const char* v = std::getenv("R50_S2"); return v ? std::atoi(v) : 1; }();          // A/B knob: 0 = generic igemm tiles for the 3x3 s2 shapes
// Eight-phase GEMM tiles for the streaming 1x1 convs: 0 = never, 1 = the shapes of kG8 (measured at batch 256), 2 / 3 = wherever the shape fits, 256 / 224 pixels
// (A/B knob: R50_G8 / option "use_g8").
int g_use_g8 = [] { const char* v = std::getenv("R50_G8"); return v ? std::atoi(v) : 1; }();
// Where the eight-phase tiles beat the tuned generic ones at batch 256 (scripts/time_g8.py, profiles/r04_time_g8.txt; same-process medians):
// layer3.1.conv1 32.3 against 33.9 us, layer4.0.conv1 56.8 against 60.0, the two-source conv3 + downsample GEMMs of layer3.0 / layer4.0 88.9 / 86.6
// against 90.7 / 88.6 -- all with 224-pixel tiles (whole blocks of the pixel counts 2^k x 49; 256-pixel tiles leave 23 % of the last round empty).
// NOT layer3.0.conv1 (HBM-bound, 3.5 rounds of 224-pixel tiles), layer4.x.conv1 (98-112 tiles on 256 CUs) and layer4.x.conv3 (K = 512: the
// tile's residual + store epilogue is as long as its K loop): the schedule's 1.36 PFLOP/s shows at K >= 2048 with whole rounds of tiles only.
struct G8Shape { int h, cin, cout, two_sources; };
constexpr G8Shape kG8[] = {{14, 1024, 256, 0}, {14, 1024, 512, 0}, {14, 768, 1024, 1}, {7, 1536, 2048, 1}};
int g8_tile(const ConvArgs& a) {
    if (!g_use_g8 || !is_g8_shape(a) || a.N < 48) return 0;
    if (g_use_g8 == 2) return kTileG8;
    if (g_use_g8 == 3) return kTileG8N7;
    for (const G8Shape& g : kG8)
        if (g.h == a.Ho && a.Ho == a.Wo && g.cin == a.Ktot && g.cout == a.Cout && (g.two_sources != 0) == (a.x2 != nullptr) && a.stride == 1 && !a.res)
            return tiles_of(a, kTileG8N7) >= 200 ? kTileG8N7 : 0;
    return 0;
}
int auto_tile(const ConvArgs& a) {
    if (is_c64_shape(a)) return kTileC64;
    if (const int t8 = g8_tile(a)) return t8;
    if (g_use_xres && is_xres_shape(a)) return kTileXres;
    if (g_use_s2 && is_s2_shape(a)) return kTileS2;
    const long long want = 200;           // of 256 CUs: below that a launch leaves too much of the chip idle
    if (a.N >= 48 && a.H == a.W)
        for (const TunedTile& t : kTuned)
            if (t.h == a.H && t.cin == a.Cin && t.cout == a.Cout && t.ks == a.ks && t.stride == a.stride &&
                t.res == (a.res != nullptr)) {
                // the table was measured at batch 256; a smaller batch may leave its (large) tiles too few to fill the chip
                if (tiles_of(a, t.tile) >= want) return t.tile;
                break;
            }
    // generic choice: the largest of these tiles that still gives the chip enough workgroups, else the one with the most
    const int cand[] = {kWsBit | 8, 1, 5, 2};        // 128x224 role-specialised, 128x128, 128x64, 64x128
    int best = 2;
    long long best_n = -1;
    for (int c : cand) {
        const long long n = tiles_of(a, c);
        if (n >= want) return c;
        if (n > best_n) { best_n = n; best = c; }
    }
    return best;
}

template <int ET>
Launch launch_igemm_et(const ConvArgs& a, int tile, hipStream_t s, bool split) {
    if (split && ET != 0) return Launch::refused();
    if (split) {       // fp32-class mode: two tile shapes are enough (it is the accuracy path, not the fast one)
        if (a.Cout % 128) return launch_igemm_t<0, 64, 128, 1, 4, 2, true>(a, false, s);
        return launch_igemm_t<0, 128, 128, 2, 2, 2, true>(a, false, s);
    }
    if (tile == 0) tile = auto_tile(a);
    if (a.x2 && (!(tile & kWsBit) || tile == kTileC64 || tile == kTileXres || tile == kTileS2)) return Launch::refused();     // two K sources: igemm_ws_kernel / gemm8p_kernel only
    if (tile == kTileG8 || tile == kTileG8N7) return launch_gemm8p<ET>(a, tile, s);
    const bool pers = (tile & kPersistBit) != 0;
    if (tile == kTileC64) return launch_conv3x3_c64<ET>(a, s);
    if (tile == kTileXres) return launch_conv3x3_xres<ET>(a, s);
    if (tile == kTileS2) return launch_conv3x3_s2<ET>(a, s);
    if (tile & kWsBit) {
        // <couts, pixels, consumer waves (couts x pixels), loader waves, LDS stages>
        switch (tile & (kPersistBit - 1)) {
            case 1: if (a.Cout % 128) return Launch::refused(); return launch_igemm_ws_t<ET, 128, 128, 2, 2, 4, 4>(a, s);
            case 3: if (a.Cout % 256) return Launch::refused(); return launch_igemm_ws_t<ET, 256, 128, 4, 2, 4, 3>(a, s);
            case 4: if (a.Cout % 128) return Launch::refused(); return launch_igemm_ws_t<ET, 128, 224, 2, 2, 4, 3>(a, s);
            case 8: if (a.Cout % 128) return Launch::refused(); return launch_igemm_ws_t<ET, 128, 224, 4, 2, 4, 3>(a, s);
            case 9: return launch_igemm_ws_t<ET, 64, 224, 2, 2, 4, 4>(a, s);
            // 208 = 13 x 16 pixels: M = 2^10 * 49 k gives 484 (layer3, 2 cout tiles) or 244 (layer4, 4 cout tiles) tiles of 13 blocks
            // where 224-wide tiles give 448 / 224 of 14: the same number of rounds on 256 CUs, 7 % less work per round
            case 10: if (a.Cout % 128) return Launch::refused(); return launch_igemm_ws_t<ET, 128, 208, 4, 1, 4, 3>(a, s);
            default: return Launch::refused();
        }
    }
    switch (tile & (kPersistBit - 1)) {
        case 1: if (a.Cout % 128) return Launch::refused(); return launch_igemm_t<ET, 128, 128, 2, 2, 2>(a, pers, s);
        case 2: return launch_igemm_t<ET, 64, 128, 1, 4, 2>(a, pers, s);
        case 3: return launch_igemm_t<ET, 64, 256, 1, 4, 2>(a, pers, s);
        case 5: if (a.Cout % 128) return Launch::refused(); return launch_igemm_t<ET, 128, 64, 2, 2, 2>(a, pers, s);
        case 6: if (a.Cout % 256) return Launch::refused(); return launch_igemm_t<ET, 256, 128, 4, 2, 3>(a, pers, s);
        case 7: if (a.Cout % 128) return Launch::refused(); return launch_igemm_t<ET, 128, 256, 2, 4, 3>(a, pers, s);
        case 8: if (a.Cout % 128) return Launch::refused(); return launch_igemm_t<ET, 128, 128, 2, 4, 3>(a, pers, s);
        case 9: if (a.Cout % 256) return Launch::refused(); return launch_igemm_t<ET, 256, 256, 4, 2, 2>(a, pers, s);
        case 10: if (a.Cout % 256) return Launch::refused(); return launch_igemm_t<ET, 256, 256, 2, 4, 2>(a, pers, s);
        case 11: if (a.Cout % 256) return Launch::refused(); return launch_igemm_t<ET, 256, 208, 8, 1, 2>(a, pers, s);
        case 12: if (a.Cout % 256) return Launch::refused(); return launch_igemm_t<ET, 256, 224, 4, 2, 2>(a, pers, s);
        default: return Launch::refused();
    }
}

Launch launch_igemm(const ConvArgs& a, int tile, hipStream_t s, bool split = false) {
    return R50_BY_ET(a.et, launch_igemm_et)(a, tile, s, split);
}

// fp8 (e4m3) operands: role-specialised kernel only, element type 2 (kernels.h)
Launch launch_igemm_fp8(const ConvArgs& a, int tile, hipStream_t s) {
    if (tile == 0) {
        tile = kWsBit | 9;
        // 128x224 with 8 consumer waves is the fastest or within 2 % of it at 16 of the 18 layer2-4 shapes (scripts/time_conv_fp8.py)
        for (int c : {kWsBit | 8, kWsBit | 3, kWsBit | 1})
            if (tiles_of(a, c) >= 200) { tile = c; break; }
    }
    if (!(tile & kWsBit) || tile == kTileC64) return Launch::refused();
    switch (tile & (kPersistBit - 1)) {
        case 1: if (a.Cout % 128) return Launch::refused(); return launch_igemm_ws_t<2, 128, 128, 2, 2, 4, 4>(a, s);
        case 3: if (a.Cout % 256) return Launch::refused(); return launch_igemm_ws_t<2, 256, 128, 4, 2, 4, 3>(a, s);
        case 4: if (a.Cout % 128) return Launch::refused(); return launch_igemm_ws_t<2, 128, 224, 2, 2, 4, 3>(a, s);
        case 8: if (a.Cout % 128) return Launch::refused(); return launch_igemm_ws_t<2, 128, 224, 4, 2, 4, 3>(a, s);
        case 9: return launch_igemm_ws_t<2, 64, 224, 2, 2, 4, 4>(a, s);
        default: return Launch::refused();
    }
}

Launch fill_conv_args(ConvArgs& a, const void* x, int n, int h, int w, int cin, const void* wt, const float* bias,
                      const void* res, void* y, int cout, int ks, int stride, int pad, int relu, bool split = false, bool w2 = false) {
    Launch r;
    if (!x || !wt || !bias || !y) return Launch::refused();
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cin % 64 || cout <= 0 || cout % 64) return Launch::refused();
    if (!(ks == 1 || ks == 3) || stride < 1 || pad < 0 || 2 * pad > ks - 1) return Launch::refused();
    a.x = (const __bf16*)x; a.w = (const __bf16*)wt; a.bias = bias; a.res = (const __bf16*)res; a.y = (__bf16*)y;
    a.N = n; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout;
    a.Ho = (h + 2 * pad - ks) / stride + 1;
    a.Wo = (w + 2 * pad - ks) / stride + 1;
    if (a.Ho <= 0 || a.Wo <= 0) return Launch::refused();
    a.ks = ks; a.stride = stride; a.pad = pad; a.relu = relu;
    const long long M = (long long)n * a.Ho * a.Wo;
    // 32-bit index budget of the kernel: pixel indices fit the FastDiv range (the byte checks below are the tighter ones in every mode)
    if (size_over(r, "output pixels n*ho*wo", M, (1ll << 30) + 1, "2^30 + 1")) return r;
    a.M = (int)M; a.HoWo = a.Ho * a.Wo;
    // split mode: X is [head(cin) | tail(cin)] per pixel, K per tap is 3*cin, Y is [head(cout) | tail(cout)]
    a.x_cstride = split ? 2 * cin : cin;
    a.y_cstride = split ? 2 * cout : cout;
    // bf16w2 mode: X plain, K per tap is 2*cin = [x | x] against [w_head | w_tail]
    const int kmul = split ? 3 : (w2 ? 2 : 1);
    a.x_wrap = split ? 2 * (cin / 64) : (w2 ? cin / 64 : (1 << 30));
    a.cin_chunks = kmul * (cin / 64); a.nk = ks * ks * a.cin_chunks; a.Ktot = ks * ks * kmul * cin;
    a.n_ctiles = 0; a.n_blocks = 0;
    // buffer descriptors of the kernel (kernels.h): every offset must stay below 2^31
    const long long x_bytes = (long long)n * h * w * a.x_cstride * 2;
    const long long x_back = ((long long)pad * w + pad) * a.x_cstride * 2;
    if (size_over(r, "x bytes + back reach, n*h*w*cx*2 + (pad*w+pad)*cx*2 (cx = channels per x pixel),", x_bytes + x_back, k2p31, "2^31") ||
        size_over(r, "w bytes, cout*K*2 (K = weight elements per cout),", (long long)cout * ks * ks * kmul * cin * 2, k2p31, "2^31") ||
        size_over(r, "y bytes, n*ho*wo*cy*2 (cy = channels per y pixel),", M * a.y_cstride * 2, k2p31, "2^31"))
        return r;
    a.x_back = (int)x_back;
    a.x_records = (unsigned)(x_bytes + a.x_back);
    a.w_bytes = (unsigned)((long long)cout * a.Ktot * 2);
    a.y_bytes = (unsigned)(M * a.y_cstride * 2);
    a.div_howo = make_fast_div((unsigned)a.HoWo);
    a.div_wo = make_fast_div((unsigned)a.Wo);
    a.div_ctiles = FastDiv{0u, 0u};
    a.et = 0;
    a.oscale = 1.0f; a.rscale = 1.0f; a.q_inv = 0.0f;
    a.x2 = nullptr; a.H2 = 0; a.W2 = 0; a.stride2 = 1; a.x2_cstride = 0; a.cc1 = 1 << 30; a.x2_records = 0u;
#if defined(R50_STAMP)
    a.dbg = nullptr;
#endif
    return r;
}

// profiling brackets
void prof_begin(r50_handle* h, hipStream_t s, EvRec& r, int cls, double flops, double bytes, int layer = -1) {
    if (!h || !h->profile) return;
    r.layer = layer;
    auto get = [&]() {
        hipEvent_t e;
        if (!h->ev_free.empty()) { e = h->ev_free.back(); h->ev_free.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    r.a = get(); r.b = get(); r.cls = cls; r.flops = flops; r.bytes = bytes;
    (void)hipEventRecord(r.a, s);
}
void prof_end(r50_handle* h, hipStream_t s, EvRec& r) {
    if (!h || !h->profile) return;
    (void)hipEventRecord(r.b, s);
    h->ev_pending.push_back(r);
}
// One launch between its profiling brackets.  A failure reads "<what>: <hip error>", or "<what> (<key><key_suffix>): <hip error>" with a conv key.
const std::string kNoKey;
template <typename F>
int profiled(r50_handle* h, hipStream_t s, int cls, double flops, double bytes, int layer, const char* what, const std::string& key, F&& launch,
             const char* key_suffix = "") {
    EvRec r{};
    prof_begin(h, s, r, cls, flops, bytes, layer);
    const Launch l = launch();
    prof_end(h, s, r);
    if (l.ok()) return R50_OK;
    return fail(h, R50_ERR_HIP, what + (key.empty() ? std::string() : " (" + key + key_suffix + ")") + ": " + l.hip_text() + l.suffix());
}

// conv3 (64 -> 256) + identity + ReLU + next conv1 (256 -> c1) in one launch (kernels.h: bneck_tail_kernel).
// wd/bd non-null: `res` is the block INPUT (m,64) and the identity is the downsample conv computed in the kernel.
template <int C1, bool DS, int NT>
Launch launch_bneck_tail_t(int et, const TailArgs& a, hipStream_t s) {
    const size_t lds = 256 * 128 * (DS ? 2 : 1) + (size_t)C1 * 512 + 256 * 4 * (DS ? 2 : 1) + (size_t)C1 * 4;
    const long long tiles = ((long long)a.M + 15) / 16;
    return launch_persistent(R50_BY_ET(et, bneck_tail_kernel, C1, DS, NT), (tiles + NT / 64 - 1) / (NT / 64), NT, lds, s, a);
}

// The size rules of r50_op_bneck_tail and r50_op_bneck_cat_chain (include/r50.h), once: for the launchers, and for the two hooks' own check
// before they queue the weight packing.  `out` is the largest tensor of a tail in every form.
bool tail_over(Launch& r, long long m, int cmid) {
    return size_over(r, "pixels m", m, k2p31, "2^31") || size_over(r, "out bytes, m*4*cmid*2,", m * 8 * cmid, k2p31, "2^31");
}
bool catchain_over(Launch& r, int n, int ow) {
    return size_over(r, "out bytes, n*ow*ow*512*2,", (long long)n * ow * ow * 1024, k2p31, "2^31") ||
           size_over(r, "x bytes, n*(2*ow)*(2*ow)*256*2,", (long long)n * 4 * ow * ow * 512, k2p31, "2^31");
}

#ifndef TAIL_NT_DS
#define TAIL_NT_DS 512
#endif
#ifndef TAIL_NT_C128
#define TAIL_NT_C128 256
#endif
Launch launch_bneck_tail(const void* y2, long long m, const void* w3, const float* b3, const void* res, const void* wd,
                             const float* bd, void* out, const void* w1, int c1, const float* b1, void* y1n, hipStream_t s, int et = 0) {
    if (!y2 || !w3 || !b3 || !res || !out || !w1 || !b1 || !y1n || m <= 0) return Launch::refused();
    if (Launch r; tail_over(r, m, 64)) return r;
    if ((c1 != 64 && c1 != 128) || ((wd == nullptr) != (bd == nullptr))) return Launch::refused();
    TailArgs a;
    a.y2 = (const __bf16*)y2; a.w3 = (const __bf16*)w3; a.b3 = b3; a.res = (const __bf16*)res; a.out = (__bf16*)out;
    a.wd = (const __bf16*)wd; a.bd = bd;
    a.w1 = (const __bf16*)w1; a.b1 = b1; a.y1n = (__bf16*)y1n; a.M = (int)m;
    // 4 waves per CU stream best (more waves lower the HBM rate); the downsample variant has 1.5x the MFMA work
    if (wd) return (c1 == 64 ? launch_bneck_tail_t<64, true, TAIL_NT_DS> : launch_bneck_tail_t<128, true, TAIL_NT_DS>)(et, a, s);
    return (c1 == 64 ? launch_bneck_tail_t<64, false, 256> : launch_bneck_tail_t<128, false, TAIL_NT_C128>)(et, a, s);
}

// layer2 shapes: conv3 (128 -> 512) + identity + ReLU + next conv1 (512 -> 128) (kernels.h: bneck_tail2_kernel)
Launch launch_bneck_tail2(const void* y2, long long m, const void* w3, const float* b3, const void* res, void* out,
                              const void* w1, const float* b1, void* y1n, hipStream_t s, int et = 0) {
    if (!y2 || !w3 || !b3 || !res || !out || !w1 || !b1 || !y1n || m <= 0) return Launch::refused();
    if (Launch r; tail_over(r, m, 128)) return r;
    Tail2Args a;
    a.y2 = (const __bf16*)y2; a.w3 = (const __bf16*)w3; a.b3 = b3; a.res = (const __bf16*)res; a.out = (__bf16*)out;
    a.w1 = (const __bf16*)w1; a.b1 = b1; a.y1n = (__bf16*)y1n; a.M = (int)m;
    const size_t lds = 2 * 8 * 8 * 1024 + 512 * 4 + 2 * 4096;
    return launch_persistent(R50_BY_ET(et, bneck_tail2_kernel), (m + 15) / 16, 512, lds, s, a);
}

// layer3 shapes: conv3 (256 -> 1024) + identity + ReLU chained with the next conv1 (1024 -> 256) (kernels.h: bneck_tail3_kernel)
// `wp`: both weight matrices in the kernel's fragment-ordered stream (1 MB; pack_tail3_weights).
// Pixel tile: at most 112 rows; chosen so the tiles fill whole rounds of the chip (batch 256: M = 50,176 -> 98 pixels, 512 tiles).
constexpr size_t kTail3PackedBytes = 1u << 20;
#if defined(R50_STAMP)
unsigned long long* g_dbg = nullptr;         // diagnostic build: set through r50_debug_buffer()
#endif
hipError_t pack_tail3_weights(const void* w3, const void* w1, void* wp, hipStream_t s) {
    if (!w3 || !w1 || !wp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tail3_pack_kernel, dim3(65536 / 256), dim3(256), 0, s, (const __bf16*)w3, (const __bf16*)w1, (__bf16*)wp);
    return hipGetLastError();
}
// bneck_tail3p_kernel (two-group pipeline, 112 LDS rows per slot).  Rounds 2-3 also carried bneck_tail3_kernel (consumer + helper waves) and a 98-row
// form of the pipeline: both measured slower (profiles/r03_tail3p_variants.txt) and were removed in round 4 (git history has them).
int g_tail3_bp = 0;        // option "tail3_bp": real pixels per tile of the chained layer3 tail (0 = whole rounds of the chip / full tiles)
Launch launch_bneck_tail3(const void* y2, long long m, const void* wp, const float* b3, const void* res, void* out,
                              const float* b1, void* y1n, hipStream_t s, int et = 0, int bp_override = 0, bool no_next = false) {
    if (no_next) { b1 = b3; y1n = out; }       // conv3 + identity + ReLU only (group B copies out): b1 / y1n are not used
    if (bp_override == 0) bp_override = g_tail3_bp;
    if (!y2 || !wp || !b3 || !res || !out || !b1 || !y1n || m <= 0) return Launch::refused();
    if (Launch r; tail_over(r, m, 256)) return r;
    const int cus = num_cus();
    if (cus == 0) return hipErrorInvalidDevice;
    Tail3Args a;
    a.y2 = (const __bf16*)y2; a.wp = (const __bf16*)wp; a.b3 = b3; a.res = (const __bf16*)res; a.out = (__bf16*)out;
    a.b1 = b1; a.y1n = (__bf16*)y1n; a.M = (int)m;
#if defined(R50_STAMP)
    a.dbg = g_dbg;
#endif
    constexpr int rows = 112;
    const long long rounds = ((m + rows - 1) / rows + cus - 1) / cus;
    long long bp = (m + rounds * cus - 1) / (rounds * cus);
    if (bp < 49) bp = 49;
    if (bp > rows) bp = rows;
    // more than one round of tiles: FULL tiles (batch 256: 448 tiles of 112 instead of 512 of 98 in 112 rows).  An eighth of the MFMA columns of a
    // 98-pixel tile multiply padding; the ragged last round that full tiles leave is filled by the other lane's launches (bench.py --lanes 2:
    // +0.9 % frames/s, two same-box pairs; neutral with one lane)
    if ((m + rows - 1) / rows > cus) bp = rows;
    if (bp_override >= 1 && bp_override <= rows) bp = bp_override;
    a.bp = (int)bp;
    a.n_tiles = (int)((m + bp - 1) / bp);
    const size_t ldsp = 8 * (size_t)rows * 128 + 256 * 4 + 1024 * 4;      // t2 (4 slots) + out_c (2 x 2) + b1 + b3
    return launch_persistent(no_next ? R50_BY_ET(et, bneck_tail3p_kernel, 112, true) : R50_BY_ET(et, bneck_tail3p_kernel, 112), a.n_tiles, 512,
                             ldsp, s, a);
}

// layer2.0 transition tail: conv3 + downsample (one conv over K = [t2 | x at stride 2]) + ReLU chained with the next block's conv1
// (kernels.h: bneck_catchain_kernel).  `wp`: both weight matrices in the kernel's fragment-ordered stream (512 KB; pack_catchain_weights).
constexpr size_t kCatChainPackedBytes = 1u << 19;
hipError_t pack_catchain_weights(const void* wcat, const void* w1, void* wp, hipStream_t s) {
    if (!wcat || !w1 || !wp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(catchain_pack_kernel, dim3(32768 / 256), dim3(256), 0, s, (const __bf16*)wcat, (const __bf16*)w1, (__bf16*)wp);
    return hipGetLastError();
}
// x_sub: x is the compact (N, ow, ow, 256) tensor of the block input's even rows and columns (what bneck_block1_kernel writes with out_sub)
Launch launch_bneck_catchain(const void* t2, const void* x, int n, int ow, const void* wp, const float* bcat, void* out,
                                 const float* b1, void* y1n, hipStream_t s, int et = 0, bool x_sub = false) {
    if (!t2 || !x || !wp || !bcat || !out || !b1 || !y1n || n <= 0 || ow != 28) return Launch::refused();
    const long long m = (long long)n * ow * ow;
    if (Launch r; catchain_over(r, n, ow)) return r;
    const int cus = num_cus();
    if (cus == 0) return hipErrorInvalidDevice;
    CatChainArgs a;
    a.t2 = (const __bf16*)t2; a.x = (const __bf16*)x; a.wp = (const __bf16*)wp; a.b3 = bcat; a.out = (__bf16*)out; a.b1 = b1; a.y1n = (__bf16*)y1n;
    a.M = (int)m; a.x_bytes = (unsigned)((long long)n * (x_sub ? 1 : 4) * ow * ow * 512); a.x_sub = x_sub ? 1 : 0;
#if defined(R50_STAMP)
    a.dbg = g_dbg;
#endif
    // full 112-pixel tiles when there is more than one round of them (batch 256: 1792 tiles = 7 per CU), else spread over the chip
    const long long full = (m + 111) / 112;
    long long bp = 112;
    if (full <= cus) { bp = (m + cus - 1) / cus; if (bp < 16) bp = 16; if (bp > 112) bp = 112; }
    a.bp = (int)bp;
    a.n_tiles = (int)((m + bp - 1) / bp);
    const size_t lds = 10 * 112 * 128 + 128 * 4 + 512 * 4 + 16;        // operand slots + out_c + b1 + b3 + 4 sync words
    return launch_persistent(R50_BY_ET(et, bneck_catchain_kernel, 28), a.n_tiles, 512, lds, s, a);
}

// layer2.1-.3 bottleneck body in one launch (kernels.h: bneck_block2_kernel): conv2 + conv3 + identity + ReLU [+ the next block's conv1]
Launch launch_bneck_block2(const void* t1, int n, const void* w2, const float* b2, const void* w3, const float* b3, const void* res,
                               void* out, const void* w1, const float* b1, void* y1n, hipStream_t s, int et = 0) {
    if (!t1 || !w2 || !b2 || !w3 || !b3 || !res || !out || n <= 0) return Launch::refused();
    if (Launch r; size_over(r, "out bytes, n*28*28*512*2,", (long long)n * 784 * 1024, k2p31, "2^31")) return r;
    if ((w1 == nullptr) != (b1 == nullptr) || (w1 == nullptr) != (y1n == nullptr)) return Launch::refused();
    Block2Args a;
    a.t1 = (const __bf16*)t1; a.w2 = (const __bf16*)w2; a.b2 = b2; a.w3 = (const __bf16*)w3; a.b3 = b3; a.res = (const __bf16*)res;
    a.out = (__bf16*)out; a.w1 = (const __bf16*)w1; a.b1 = b1; a.y1n = (__bf16*)y1n; a.N = n; a.n_tiles = 4 * n;
    const size_t lds = (w1 ? 3 * 208 * 128 + 224 * 128 : 4 * 208 * 128) + 3 * 16384 + 768 * 4;       // 160,768 / 158,720 (kernels.h: LDS map)
    return launch_persistent(w1 ? R50_BY_ET(et, bneck_block2_kernel, 128) : R50_BY_ET(et, bneck_block2_kernel, 0), a.n_tiles, 768, lds, s, a);
}

// layer1.1 / .2 bottleneck body in one launch (kernels.h: bneck_block1_kernel): conv2 + conv3 + identity + ReLU + the next conv1 (c1 = 64 or 128)
Launch launch_bneck_block1(const void* t1, int n, const void* w2, const float* b2, const void* w3, const float* b3, const void* res,
                               void* out, const void* w1, int c1, const float* b1, void* y1n, hipStream_t s, int et = 0,
                               const void* wd = nullptr, const float* bd = nullptr, bool out_sub = false) {
    if (!t1 || !w2 || !b2 || !w3 || !b3 || !res || !out || !w1 || !b1 || !y1n || n <= 0) return Launch::refused();
    if (Launch r; size_over(r, "out bytes, n*56*56*256*2,", (long long)n * 3136 * 512, k2p31, "2^31")) return r;
    if (c1 != 64 && c1 != 128) return Launch::refused();
    if ((wd == nullptr) != (bd == nullptr) || (wd && c1 != 64)) return Launch::refused();       // downsample form: layer1.0 (next conv1 256 -> 64)
    Block1Args a;
    a.t1 = (const __bf16*)t1; a.w2 = (const __bf16*)w2; a.b2 = b2; a.w3 = (const __bf16*)w3; a.b3 = b3; a.res = (const __bf16*)res;
    a.out = (__bf16*)out; a.w1 = (const __bf16*)w1; a.b1 = b1; a.y1n = (__bf16*)y1n; a.N = n; a.n_tiles = 14 * n;
    a.wd = (const __bf16*)wd; a.bd = bd; a.out_sub = out_sub ? 1 : 0;
    constexpr size_t lds = 11 * 32 * 128 + 3 * 224 * 128 + 3 * 8192 + (448 + 256) * 4;       // 158,464 (kernels.h: LDS map; bd behind b1)
    auto kern = wd ? R50_BY_ET(et, bneck_block1_kernel, 64, true) : c1 == 64 ? R50_BY_ET(et, bneck_block1_kernel, 64) : R50_BY_ET(et, bneck_block1_kernel, 128);
    return launch_persistent(kern, a.n_tiles, 768, lds, s, a);
}

// q_inv > 0: write the output as e4m3 = fp8(16-bit result * q_inv) (role-specialised tiles only; *q_done reports whether that happened)
int run_conv(r50_handle* h, const ConvLayer& L, const __bf16* x, int n, int hh, int ww, const __bf16* res,
             __bf16* y, int relu, hipStream_t s, int* ho, int* wo, float q_inv = 0.f, bool* q_done = nullptr) {
    ConvArgs a;
    const bool split = (h->precision == R50_PREC_FP32X);
    const bool w2 = (h->precision == R50_PREC_BF16W2);
    if (const Launch r = fill_conv_args(a, x, n, hh, ww, L.cin, L.w, L.bias, res, y, L.cout, L.ks, L.stride, L.pad, relu, split, w2); !r.ok())
        return fail(h, R50_ERR_INVALID, "conv args invalid for " + L.conv_key + r.suffix());
    a.et = (h->precision == R50_PREC_FP16) ? 1 : 0;
    const double flops = 2.0 * a.M * (double)a.Cout * L.ks * L.ks * L.cin;       // algorithmic (not the 3x of split mode)
    const double bytes = 2.0 * ((double)n * hh * ww * L.cin + (double)a.M * a.Cout * (res ? 2 : 1) + (double)a.Cout * L.ks * L.ks * L.cin);
    int tile = h->tile_override;
    if (q_done) *q_done = false;
    if (q_inv > 0.f && !split && !w2 && tile == 0) {
        const int t = auto_tile(a);
        if ((t & kWsBit) && t != kTileC64 && t != kTileXres) {      // the quantising epilogue lives in igemm_ws_kernel
            tile = t; a.q_inv = q_inv; a.y_bytes = (unsigned)((long long)a.M * a.y_cstride);
            if (q_done) *q_done = true;
        }
    }
    *ho = a.Ho; *wo = a.Wo;
    return profiled(h, s, PC_IGEMM, flops, bytes, (int)(&L - &h->convs[0]), "igemm launch", L.conv_key, [&] { return launch_igemm(a, tile, s, split); });
}

// 1x1 conv over two K sources: y = act([W1 | W2] . [x1 ; x2 at stride2] + bias).  x1 (n,h,w,c1) at the output resolution,
// x2 (n,h2,w2,c2) sampled at (ho*stride2, wo*stride2); wcat (cout, c1 + c2) K-major.  Role-specialised kernel only.
Launch fill_conv_args_cat(ConvArgs& a, const void* x1, int n, int h, int w, int c1, const void* x2, int h2, int w2, int c2, int stride2,
                          const void* wcat, const float* bias, void* y, int cout, int relu) {
    if (!x2 || c2 <= 0 || c2 % 64 || stride2 < 1 || h2 < 1 || w2 < 1) return Launch::refused();
    if ((h2 - 1) / stride2 + 1 != h || (w2 - 1) / stride2 + 1 != w) return Launch::refused();
    Launch r = fill_conv_args(a, x1, n, h, w, c1, wcat, bias, nullptr, y, cout, 1, 1, 0, relu);
    if (!r.ok()) return r;
    const long long x2_bytes = (long long)n * h2 * w2 * c2 * 2;
    if (size_over(r, "x2 bytes, n*h2*w2*c2*2,", x2_bytes, k2p31, "2^31") ||
        size_over(r, "wcat bytes, cout*(c1+c2)*2,", ((long long)c1 + c2) * cout * 2, k2p31, "2^31"))
        return r;
    a.Cin = c1 + c2;
    a.cin_chunks = (c1 + c2) / 64; a.nk = a.cin_chunks; a.Ktot = c1 + c2;
    a.w_bytes = (unsigned)((long long)cout * a.Ktot * 2);
    a.x2 = (const __bf16*)x2; a.H2 = h2; a.W2 = w2; a.stride2 = stride2; a.x2_cstride = c2; a.cc1 = c1 / 64;
    a.x2_records = (unsigned)x2_bytes;
    return r;
}
int cat_tile(const ConvArgs& a, int tile) {          // tile id for a two-source conv: role-specialised variants only
    if (tile == 0) {
        if (const int t8 = g8_tile(a)) return t8;
        if (a.N >= 48) {                               // measured at batch 256 (scripts/time_cat.py, profiles/r01_time_cat.txt)
            if (a.Cout % 256 == 0) return kWsBit | 3;      // 256x128, 8 consumer waves: fastest of the five at all three shapes
        }
        for (int c : {kWsBit | 8, kWsBit | 1, kWsBit | 9})
            if (tiles_of(a, c) >= 200) return c;
        return kWsBit | 9;
    }
    return (tile & kWsBit) ? tile : -1;
}
int run_conv_cat(r50_handle* h, int si, const ConvLayer& c3, const ConvLayer& cd, const __bf16* t2, const __bf16* xin, int n, int h2, int w2,
                 int hin, int win, __bf16* y, hipStream_t s) {
    ConvArgs a;
    if (const Launch r = fill_conv_args_cat(a, t2, n, h2, w2, c3.cin, xin, hin, win, cd.cin, cd.stride, h->cat_w[si], h->cat_bias[si], y, c3.cout, 1);
        !r.ok())
        return fail(h, R50_ERR_INVALID, "two-source conv args invalid for " + c3.conv_key + r.suffix());
    a.et = (h->precision == R50_PREC_FP16) ? 1 : 0;
    const double flops = 2.0 * a.M * (double)a.Cout * a.Ktot;
    const double bytes = 2.0 * ((double)a.M * (c3.cin + cd.cin) + (double)a.M * a.Cout + (double)a.Cout * a.Ktot);
    return profiled(h, s, PC_IGEMM, flops, bytes, (int)(&c3 - &h->convs[0]), "igemm launch", c3.conv_key,
                    [&] { return launch_igemm(a, cat_tile(a, 0), s, false); }, " + downsample");
}

template <typename TIN>
Launch launch_stem_pack(const TIN* x, void* xp, int n, hipStream_t s, int et = 0) {
    hipLaunchKernelGGL(R50_BY_ET(et, stem_pack_kernel, TIN), dim3(ew_grid((long long)n * STEM_HP * STEM_WP, 256 * 64)), dim3(256), 0, s, x,
                       (u32x2*)xp, n);
    return hipGetLastError();
}
Launch launch_stem_conv(const void* xp, const void* wpk, const float* bias, void* y, int n, hipStream_t s, int et = 0) {
    R50_ET_LAUNCH(et, stem_conv_kernel, dim3(n * (112 / STEM_ROWS_PER_WG)), dim3(256), STEM_LDS_BYTES, s,
                  (const char*)xp, (const char*)wpk, bias, (__bf16*)y);
    return hipGetLastError();
}
// fused stem (stem_fused3_kernel): a workgroup walks a strip of G consecutive pooled-row pairs of one image.  Strip length 0 = chosen from the
// batch, 1/2/4/7/14/28 = that many pairs per strip: r50_set_option("stem_strip") or R50_STEM_STRIP in the environment (A/B).
// (Removed in round 4: the per-pair kernel of round 1 and the strip kernel of rounds 2-3, whose phases ran in turn.)
static int g_stem_strip = [] { const char* v = std::getenv("R50_STEM_STRIP"); const int g = v ? std::atoi(v) : 0; return g > 0 && 28 % g == 0 ? g : 0; }();
// c1_w / c1_bias / y1 non-null: layer1.0.conv1 (+ bias + ReLU) of the pooled output into y1 in the same launch
template <typename TIN>
Launch launch_stem_fused(const TIN* x, const void* wpk, const float* bias, void* y, int n, hipStream_t s,
                             const float* u8_table, int et = 0, const void* c1_w = nullptr, const float* c1_bias = nullptr,
                             void* y1 = nullptr) {
    // G = the longest strip that still gives the chip ~200 workgroups (28 = the whole image from batch 200 up)
    int G = 1;
    if (g_stem_strip > 0) G = g_stem_strip;
    else
        for (int cand : {28, 14, 7, 4, 2})
            if (n * (28 / cand) >= 200) { G = cand; break; }
    const bool c1 = c1_w && c1_bias && y1;
    const int strips = n * (28 / G);
    // 16-B (fp32) / 4-B (uint8) loads of 4 pixels: image rows start at multiples of 896 / 224 bytes from the frame pointer
    if (reinterpret_cast<uintptr_t>(x) & (sizeof(TIN) == 1 ? 3u : 15u)) return Launch::refused();
    auto kern = c1 ? R50_BY_ET(et, stem_fused3_kernel, TIN, true) : R50_BY_ET(et, stem_fused3_kernel, TIN, false);
#if defined(R50_STAMP)
    return launch_persistent(kern, strips, SF3_THREADS, SF3_LDS_BYTES, s, x, (const char*)wpk, bias, (__bf16*)y, strips, G, u8_table,
                             (const __bf16*)c1_w, c1_bias, (__bf16*)y1, g_dbg);
#else
    return launch_persistent(kern, strips, SF3_THREADS, SF3_LDS_BYTES, s, x, (const char*)wpk, bias, (__bf16*)y, strips, G, u8_table,
                             (const __bf16*)c1_w, c1_bias, (__bf16*)y1);
#endif
}
template <typename TIN>
Launch launch_stem_split(const TIN* x, char* xp_head, char* xp_tail, const char* w_head, const char* w_tail,
                             const float* bias, void* y, int n, hipStream_t s) {
    hipLaunchKernelGGL(stem_pack_split_kernel<TIN>, dim3(ew_grid((long long)n * STEM_HP * STEM_WP, 256 * 64)), dim3(256), 0, s, x, (u32x2*)xp_head,
                       (u32x2*)xp_tail, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(stem_conv_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            STEM_SPLIT_LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stem_conv_split_kernel, dim3(n * (112 / STEM_ROWS_PER_WG)), dim3(256), STEM_SPLIT_LDS_BYTES, s,
                       (const char*)xp_head, (const char*)xp_tail, w_head, w_tail, bias, (__bf16*)y);
    return hipGetLastError();
}
Launch launch_maxpool_split(const void* x, void* y, int n, int h, int w, int c, hipStream_t s) {
    const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(maxpool3x3s2_split_kernel, dim3(ew_grid((long long)n * ho * wo * (c / 8), 256 * 64)), dim3(256), 0, s, (const __bf16*)x,
                       (__bf16*)y, n, h, w, c, ho, wo);
    return hipGetLastError();
}
Launch launch_avgpool_split(const void* x, float* y, int n, int hw, int c, hipStream_t s) {
    const int total = n * (c / 8);
    hipLaunchKernelGGL(avgpool_split_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (const __bf16*)x, y, n, hw, c,
                       1.0f / (float)hw);
    return hipGetLastError();
}
Launch launch_maxpool(const void* x, void* y, int n, int h, int w, int c, hipStream_t s, int et = 0) {
    const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    R50_ET_LAUNCH(et, maxpool3x3s2_kernel, dim3(ew_grid((long long)n * ho * wo * (c / 8), 256 * 64)), dim3(256), 0, s, (const __bf16*)x,
                  (__bf16*)y, n, h, w, c, ho, wo);
    return hipGetLastError();
}
Launch launch_avgpool(const void* x, float* y, int n, int hw, int c, hipStream_t s, int et = 0) {
    const int total = n * (c / 8);
    R50_ET_LAUNCH(et, avgpool_kernel, dim3((total + 255) / 256), dim3(256), 0, s, (const __bf16*)x, y, n, hw, c, 1.0f / (float)hw);
    return hipGetLastError();
}

// ---- R50_PREC_FP8: layer2-4 on e4m3 tensors ----------------------------------------------------------------------------
int run_conv_fp8(r50_handle* h, const ConvLayer& L, const void* x, int n, int hh, int ww, const void* res, void* y, int relu, float sx,
                 float sr, float sy, hipStream_t s, int* ho, int* wo) {
    ConvArgs a;
    if (const Launch r = fill_conv_args(a, x, n, hh, ww, L.cin / 2, L.w, L.bias_scaled, res, y, L.cout, L.ks, L.stride, L.pad, relu); !r.ok())
        return fail(h, R50_ERR_INVALID, "fp8 conv args invalid for " + L.conv_key + r.suffix());
    a.y_bytes = (unsigned)((long long)a.M * L.cout);
    a.et = 2; a.oscale = sx * L.wscale / sy; a.rscale = sr / sy;
    const double flops = 2.0 * a.M * (double)a.Cout * L.ks * L.ks * L.cin;
    const double bytes = (double)n * hh * ww * L.cin + (double)a.M * a.Cout * (res ? 2 : 1) + (double)a.Cout * L.ks * L.ks * L.cin;
    *ho = a.Ho; *wo = a.Wo;
    return profiled(h, s, PC_IGEMM, flops, bytes, (int)(&L - &h->convs[0]), "fp8 igemm launch", L.conv_key, [&] { return launch_igemm_fp8(a, 0, s); });
}

// buf[cur] holds layer1's output (n,56,56,256) as 16-bit elements: quantise it, run layer2-4 in fp8, pool.
int run_fp8_part(r50_handle* h, __bf16* const* buf, int cur, int n, float* out, hipStream_t s, bool already_fp8 = false) {
    if ((int)h->fp8_scales.size() != R50_FP8_NUM_SCALES)
        return fail(h, R50_ERR_STATE, "fp8 mode: call r50_set_fp8_scales (activation scales) before the first forward");
    const float* sc = h->fp8_scales.data();
    int k = 0;
    float s_in = sc[k++];
    int nxt = (cur + 1) % 5;
    int rc;
    if (!already_fp8) {
        const long long n4 = (long long)n * 56 * 56 * 256 / 4;
        rc = profiled(h, s, PC_MAXPOOL, 0, (double)n4 * 12, -1, "quant_to_fp8", kNoKey, [&] {
            hipLaunchKernelGGL(quant_to_fp8_kernel<0>, dim3(ew_grid(n4, 256 * 64)), dim3(256), 0, s,
                               (const unsigned short*)buf[cur], (unsigned*)buf[nxt], n4, 1.0f / s_in);
            return hipGetLastError();
        });
        if (rc) return rc;
        cur = nxt;
    }
    int hh = 56, ww = 56;
    size_t li = kFp8FirstConv;
    for (int si = 1; si < 4; ++si)
        for (int b = 0; b < kStages[si][1]; ++b) {
            int fr[4], nf = 0;
            for (int i = 0; i < 5; ++i)
                if (i != cur) fr[nf++] = i;
            const ConvLayer &c1 = h->convs[li], &c2 = h->convs[li + 1], &c3 = h->convs[li + 2];
            const float s_t1 = sc[k++], s_t2 = sc[k++];
            int h1, w1, h2, w2, h3, w3;
            if ((rc = run_conv_fp8(h, c1, buf[cur], n, hh, ww, nullptr, buf[fr[0]], 1, s_in, 1.f, s_t1, s, &h1, &w1))) return rc;
            if ((rc = run_conv_fp8(h, c2, buf[fr[0]], n, h1, w1, nullptr, buf[fr[1]], 1, s_t1, 1.f, s_t2, s, &h2, &w2))) return rc;
            const void* idn = buf[cur];
            float s_idn = s_in;
            const bool cat_ds = (b == 0) && h->fuse_ds_cat && h->cat_w[si] && h->cat_acc_scale[si] > 0.f;
            if (b == 0) {
                const float s_ds = sc[k++];        // unused by the two-source form: the downsample tensor is never formed
                if (!cat_ds) {
                    int hd, wd;
                    if ((rc = run_conv_fp8(h, h->convs[li + 3], buf[cur], n, hh, ww, nullptr, buf[fr[2]], 0, s_in, 1.f, s_ds, s, &hd, &wd))) return rc;
                    idn = buf[fr[2]]; s_idn = s_ds;
                }
            }
            const float s_out = sc[k++];
            if (cat_ds) {
                const ConvLayer& cd = h->convs[li + 3];
                ConvArgs a;
                if (const Launch r = fill_conv_args_cat(a, buf[fr[1]], n, h2, w2, c3.cin / 2, buf[cur], hh, ww, cd.cin / 2, cd.stride, h->cat_w[si],
                                                        h->cat_bias[si], buf[fr[3]], c3.cout, 1); !r.ok())
                    return fail(h, R50_ERR_INVALID, "fp8 two-source conv args invalid for " + c3.conv_key + r.suffix());
                a.y_bytes = (unsigned)((long long)a.M * c3.cout);
                a.et = 2; a.oscale = h->cat_acc_scale[si] / s_out; a.rscale = 0.f;
                const double flops = 2.0 * a.M * (double)a.Cout * (c3.cin + cd.cin);
                rc = profiled(h, s, PC_IGEMM, flops, (double)a.M * (c3.cin + cd.cin + a.Cout) + (double)a.Cout * (c3.cin + cd.cin), (int)(&c3 - &h->convs[0]),
                              "fp8 two-source igemm launch", c3.conv_key, [&] { return launch_igemm_fp8(a, 0, s); });
                if (rc) return rc;
                h3 = h2; w3 = w2;
            } else if ((rc = run_conv_fp8(h, c3, buf[fr[1]], n, h2, w2, idn, buf[fr[3]], 1, s_t2, s_idn, s_out, s, &h3, &w3))) return rc;
            cur = fr[3]; hh = h3; ww = w3; s_in = s_out;
            li += (b == 0) ? 4 : 3;
        }
    return profiled(h, s, PC_AVGPOOL, 0, (double)n * (hh * ww * 2048.0 + 2048.0 * 4), -1, "avgpool_fp8", kNoKey, [&] {
        hipLaunchKernelGGL(avgpool_fp8_kernel, dim3((n * 256 + 255) / 256), dim3(256), 0, s, (const unsigned char*)buf[cur], out, n, hh * ww, 2048,
                           s_in / (float)(hh * ww));
        return hipGetLastError();
    });
}

PlanInputs plan_inputs(const r50_handle* h, const char* tap) {
    PlanInputs in;
    in.precision = h->precision;
    in.fused_stem = h->fused_stem; in.fuse_stem_c1 = h->fuse_stem_c1; in.fuse_tail = h->fuse_tail; in.fuse_tail3 = h->fuse_tail3;
    in.fuse_tail3_last = h->fuse_tail3_last; in.fuse_ds_cat = h->fuse_ds_cat; in.fuse_cat_chain = h->fuse_cat_chain; in.sub_out = h->sub_out;
    in.fuse_block1 = h->fuse_block1; in.fuse_block2 = h->fuse_block2; in.inplace_out = h->inplace_out; in.overlap_ds = h->overlap_ds;
    in.fuse_fp8_handover = h->fuse_fp8_handover; in.tile_override = h->tile_override; in.profile = h->profile;
    for (int i = 0; i < 4; ++i) in.cat_w[i] = h->cat_w[i] != nullptr;
    for (int b = 0; b < 8; ++b) in.tail3_wp[b] = h->tail3_wp[b] != nullptr;
    in.catchain_wp = h->catchain_wp != nullptr;
    in.fp8_scales_complete = (int)h->fp8_scales.size() == R50_FP8_NUM_SCALES;
    in.tap = tap;
    for (int i = 0; i < kNumConvs; ++i) in.convs[i] = h->convs[i];
    return in;
}

// Runs `n` frames (n <= max_batch) through the stack: plans the launches (launch_plan.h) and executes the plan.  If `tap` is
// non-null, stops once the named activation is available and reports it through tap_ptr / dims.
template <typename TIN>
int run_stack(r50_handle* h, const TIN* x, int n, float* out, hipStream_t s, const char* tap,
              const __bf16** tap_ptr, int64_t dims[4], int slot0 = 0) {
    // slot0: first frame slot of the workspace this call may use (concurrent calls on different streams
    // work on disjoint frame ranges of the same buffers)
    const StackPlan plan = plan_stack(plan_inputs(h, tap));
    const bool split = (h->precision == R50_PREC_FP32X);
    const int et = (h->precision == R50_PREC_FP16) ? 1 : 0;      // element type of weights / activations (kernels.h)
    const int cmul = split ? 2 : 1;            // channels per pixel multiplier of every activation tensor
    __bf16* buf[5];
    for (int i = 0; i < 5; ++i) buf[i] = h->buf[i] + (size_t)slot0 * 112 * 112 * 64 * cmul;
    char* stem_xp = h->stem_xp + (size_t)slot0 * STEM_HP * STEM_WP * 8 * cmul;
    auto report = [&](const __bf16* p, int hh, int ww, int c) {
        *tap_ptr = p; dims[0] = n; dims[1] = hh; dims[2] = ww; dims[3] = c * cmul;
        return R50_OK;
    };
    int rc = R50_OK;
    const bool stem_c1 = plan.stem == Stem::FusedConv1;       // layer1.0.conv1 is computed by the stem kernel (into buf[2])
    switch (plan.stem) {
        case Stem::Split: {
            char* xp_tail = stem_xp + (size_t)n * STEM_HP * STEM_WP * 8;
            rc = profiled(h, s, PC_STEM_CONV, 2.0 * n * 112 * 112 * 64 * 147.0, (double)n * (3.0 * 224 * 224 * 4 + 112.0 * 112 * 128 * 2), -1, "stem (split)", kNoKey,
                          [&] { return launch_stem_split(x, stem_xp, xp_tail, h->stem_w, h->stem_w + STEM_W_BYTES, h->convs[0].bias, buf[0], n, s); });
            break;
        }
        case Stem::Fused: case Stem::FusedConv1: {
            // conv1 + bn1 + relu + maxpool in one kernel: frame in, (n,56,56,64) out
            // ... and layer1.0.conv1 (1x1, 64 -> 64) of the pooled rows into buf[2] while they are still in LDS
            const ConvLayer& l1c1 = h->convs[1];
            rc = profiled(h, s, PC_STEM_CONV, 2.0 * n * 112 * 112 * 64 * 147.0 + (stem_c1 ? 2.0 * n * 56 * 56 * 64 * 64 : 0.0),
                          (double)n * (3.0 * 224 * 224 * 4 + 56.0 * 56 * 64 * 2 * (stem_c1 ? 2 : 1)), -1, "stem_fused", kNoKey, [&] {
                              return launch_stem_fused(x, h->stem_w, h->convs[0].bias, buf[1], n, s, h->u8_table, et, stem_c1 ? l1c1.w : nullptr,
                                                       stem_c1 ? l1c1.bias : nullptr, stem_c1 ? buf[2] : nullptr);
                          });
            break;
        }
        case Stem::PackConv:
            rc = profiled(h, s, PC_STEM_PACK, 0, (double)n * (3.0 * 224 * 224 * 4 + (double)STEM_HP * STEM_WP * 8), -1, "stem_pack", kNoKey,
                          [&] { return launch_stem_pack(x, stem_xp, n, s, et); });
            if (rc) return rc;
            rc = profiled(h, s, PC_STEM_CONV, 2.0 * n * 112 * 112 * 64 * 147.0, (double)n * ((double)STEM_HP * STEM_WP * 8 + 112.0 * 112 * 64 * 2), -1, "stem_conv",
                          kNoKey, [&] { return launch_stem_conv(stem_xp, h->stem_w, h->convs[0].bias, buf[0], n, s, et); });
            break;
    }
    if (rc) return rc;
    if (plan.stem == Stem::Split || plan.stem == Stem::PackConv) {
        if (plan.tap == TapAt::Stem) return report(buf[0], 112, 112, 64);
        rc = profiled(h, s, PC_MAXPOOL, 0, (double)n * (112.0 * 112 + 56.0 * 56) * 64 * 2 * cmul, -1, "maxpool", kNoKey, [&] {
            return split ? launch_maxpool_split(buf[0], buf[1], n, 112, 112, 64, s) : launch_maxpool(buf[0], buf[1], n, 112, 112, 64, s, et);
        });
        if (rc) return rc;
    }
    if (plan.tap == TapAt::Pool) return report(buf[1], 56, 56, 64);

    int cur = 1, hh = 56, ww = 56;
    int pre_t1 = stem_c1 ? 2 : -1;      // buffer that already holds the coming block's conv1 output (Conv1::Ready), or -1
    bool layer1_out_fp8 = false;        // fp8 mode: layer1's output was written as e4m3 by its last conv's epilogue
    for (int i = 0; i < plan.n_blocks; ++i) {
        const BlockPlan& bp = plan.blocks[i];
        int fr[4], nf = 0;
        if (pre_t1 >= 0) fr[nf++] = pre_t1;
        for (int j = 0; j < 5; ++j)
            if (j != cur && j != pre_t1) fr[nf++] = j;
        pre_t1 = -1;
        const ConvLayer &c1 = h->convs[bp.li], &c2 = h->convs[bp.li + 1], &c3 = h->convs[bp.li + 2];
        const ConvLayer* nx = (bp.li_next < kNumConvs) ? &h->convs[bp.li_next] : nullptr;
        const ConvLayer* cdp = (bp.b == 0) ? &h->convs[bp.li + 3] : nullptr;
        int h1 = hh, w1 = ww, h2, w2, h3, w3;
        const __bf16* idn = buf[cur];
        if (bp.ds_side) {
            if (!h->ds_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->ds_stream, hipStreamNonBlocking));
            if (!h->ev_ds_fork) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_ds_fork, hipEventDisableTiming));
            if (!h->ev_ds_join) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_ds_join, hipEventDisableTiming));
            const hipStream_t sd = h->ds_stream;
            HIP_TRY(h, hipEventRecord(h->ev_ds_fork, s));          // block input complete
            HIP_TRY(h, hipStreamWaitEvent(sd, h->ev_ds_fork, 0));
            int hd, wd;
            rc = run_conv(h, *cdp, buf[cur], n, hh, ww, nullptr, buf[fr[2]], 0, sd, &hd, &wd);
            if (rc) return rc;
            HIP_TRY(h, hipEventRecord(h->ev_ds_join, sd));
            idn = buf[fr[2]];
        }
        if (bp.conv1 == Conv1::Launch) {
            rc = run_conv(h, c1, buf[cur], n, hh, ww, nullptr, buf[fr[0]], 1, s, &h1, &w1);
            if (rc) return rc;
        }
        // conv2 .. block output in ONE launch: t1 in buf[fr[0]], the block input as the identity, the output into buf[fr[3]], the next block's
        // conv1 output (chain_next) into buf[fr[1]].  Same bits as the launches it replaces.
        switch (bp.body) {
            case Body::Conv2: break;
            case Body::Block1Ds: {      // layer1.0: the downsample conv of the block input is the identity (bneck_block1_kernel<.., DS>)
                const double m = (double)n * 3136.0;
                rc = profiled(h, s, PC_BLOCK2, 2.0 * m * (64.0 * 576 + 2 * 256.0 * 64 + 64.0 * 256),
                              2.0 * (m * (64.0 + 64 + 256 + 64) + 64.0 * 576 + 2 * 256.0 * 64 + 64.0 * 256), bp.li + 1, "bneck_block1 (downsample) launch", c2.conv_key, [&] {
                                  return launch_bneck_block1(buf[fr[0]], n, c2.w, c2.bias, c3.w, c3.bias, buf[cur], buf[fr[3]], nx->w, 64, nx->bias, buf[fr[1]], s, et,
                                                             cdp->w, cdp->bias);
                              });
                break;
            }
            case Body::Block1: {        // layer1.1 / .2 (bneck_block1_kernel).  sub_out: only the even rows and columns of the output are stored, all that
                                        // its one reader, layer2.0's chained tail, looks at -- 103 MB instead of 411 MB at batch 256
                const double m = (double)n * 3136.0;
                rc = profiled(h, s, PC_BLOCK2, 2.0 * m * (64.0 * 576 + 256.0 * 64 + (double)nx->cout * 256),
                              2.0 * (m * (64.0 + 256 + (bp.sub_out ? 64.0 : 256.0) + nx->cout) + 64.0 * 576 + 256.0 * 64 + (double)nx->cout * 256), bp.li + 1,
                              "bneck_block1 launch", c2.conv_key, [&] {
                                  return launch_bneck_block1(buf[fr[0]], n, c2.w, c2.bias, c3.w, c3.bias, buf[cur], buf[fr[3]], nx->w, nx->cout, nx->bias, buf[fr[1]], s,
                                                             et, nullptr, nullptr, bp.sub_out);
                              });
                break;
            }
            case Body::Block2: {        // layer2.1-.3 (bneck_block2_kernel); .3 has no next conv1 that fits the chain
                const bool chain = bp.chain_next;
                const double m = (double)n * 784.0;
                rc = profiled(h, s, PC_BLOCK2, 2.0 * m * (128.0 * 1152 + 512.0 * 128 + (chain ? 128.0 * 512 : 0.0)),
                              2.0 * (m * (128.0 + 512 + 512 + (chain ? 128.0 : 0.0)) + 128.0 * 1152 + 512.0 * 128 + (chain ? 128.0 * 512 : 0.0)), bp.li + 1,
                              "bneck_block2 launch", c2.conv_key, [&] {
                                  return launch_bneck_block2(buf[fr[0]], n, c2.w, c2.bias, c3.w, c3.bias, buf[cur], buf[fr[3]], chain ? nx->w : nullptr,
                                                             chain ? nx->bias : nullptr, chain ? buf[fr[1]] : nullptr, s, et);
                              });
                break;
            }
        }
        if (bp.body != Body::Conv2) {
            if (rc) return rc;
            if (bp.chain_next) pre_t1 = fr[1];
            cur = fr[3];
            continue;
        }
        if (bp.tap == TapAt::T1) return report(buf[fr[0]], h1, w1, c1.cout);
        rc = run_conv(h, c2, buf[fr[0]], n, h1, w1, nullptr, buf[fr[1]], 1, s, &h2, &w2);
        if (rc) return rc;
        if (bp.tap == TapAt::T2) return report(buf[fr[1]], h2, w2, c2.cout);
        if (bp.ds_separate) {
            int hd, wd;
            rc = run_conv(h, *cdp, buf[cur], n, hh, ww, nullptr, buf[fr[2]], 0, s, &hd, &wd);
            if (rc) return rc;
            if (bp.tap == TapAt::Ds) return report(buf[fr[2]], hd, wd, cdp->cout);
            idn = buf[fr[2]];
        }
        if (bp.ds_side) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_ds_join, 0));   // conv3 needs the downsample output
        // inplace: a DRAM page that has just been read is written while it is still open -- a device add_ (read + write the same addresses)
        // streams 9 % faster than a copy on this chip (profiles/r02_hbm_copy_probe.txt)
        __bf16* const outb = bp.inplace ? buf[cur] : buf[fr[3]];
        const long long m = (long long)n * h2 * w2;
        const int layer = bp.li + 2;
        h3 = h2; w3 = w2;
        switch (bp.tail) {
            case Tail::Tail1: case Tail::Tail2: case Tail::Tail3:       // conv3 + identity + ReLU and the next block's conv1 in one pass over the pixels; Tail1 with
                                                                        // fuse_ds: the identity (downsample conv of the block input) is computed in the kernel as well
                rc = profiled(h, s, bp.tail == Tail::Tail3 ? PC_TAIL3 : PC_TAIL, 2.0 * m * ((double)c3.cout * c3.cin * (bp.fuse_ds ? 2 : 1) + (double)nx->cout * nx->cin),
                              2.0 * (m * ((double)c3.cin + (bp.fuse_ds ? c3.cin : c3.cout) + c3.cout + nx->cout) +
                                     (double)c3.cout * c3.cin * (bp.fuse_ds ? 2 : 1) + (double)nx->cin * nx->cout),
                              layer, "bneck_tail launch", c3.conv_key, [&] {
                                  if (bp.tail == Tail::Tail3) return launch_bneck_tail3(buf[fr[1]], m, h->tail3_wp[bp.b], c3.bias, idn, outb, nx->bias, buf[fr[0]], s, et);
                                  if (bp.tail == Tail::Tail2) return launch_bneck_tail2(buf[fr[1]], m, c3.w, c3.bias, idn, outb, nx->w, nx->bias, buf[fr[0]], s, et);
                                  return launch_bneck_tail(buf[fr[1]], m, c3.w, c3.bias, bp.fuse_ds ? buf[cur] : idn, bp.fuse_ds ? cdp->w : nullptr,
                                                           bp.fuse_ds ? cdp->bias : nullptr, outb, nx->w, nx->cout, nx->bias, buf[fr[0]], s, et);
                              });
                break;
            case Tail::CatChain: {      // layer2.0: the two-source conv3 + downsample GEMM chained with layer2.1.conv1 through LDS (bneck_catchain_kernel);
                                        // same bits as the two-source igemm launch followed by the 1x1 launch
                const double md = (double)n * 784.0;
                rc = profiled(h, s, PC_CATCHAIN, 2.0 * md * (512.0 * 384 + 128.0 * 512), 2.0 * (md * (128.0 + 256 + 512 + 128) + 512.0 * 384 + 128.0 * 512), layer,
                              "bneck_catchain launch", c3.conv_key, [&] {
                                  return launch_bneck_catchain(buf[fr[1]], buf[cur], n, 28, h->catchain_wp, h->cat_bias[1], outb, nx->bias, buf[fr[0]], s, et, bp.x_sub);
                              });
                break;
            }
            case Tail::Cat:             // the downsample tensor is never written or read back, and there is one launch instead of two
                rc = run_conv_cat(h, bp.si, c3, *cdp, buf[fr[1]], buf[cur], n, h2, w2, hh, ww, outb, s);
                break;
            case Tail::Tail3NoNext:     // same bits as the igemm launch, whose K = 256 tiles alternate between an MFMA phase and an epilogue phase
                rc = profiled(h, s, PC_TAIL3, 2.0 * m * (double)c3.cout * c3.cin, 2.0 * (m * ((double)c3.cin + 2.0 * c3.cout) + (double)c3.cout * c3.cin), layer,
                              "bneck_tail3 (no next conv1) launch", c3.conv_key, [&] {
                                  return launch_bneck_tail3(buf[fr[1]], m, h->tail3_wp[bp.b], c3.bias, idn, outb, nullptr, nullptr, s, et, 0, /*no_next=*/true);
                              });
                break;
            case Tail::Conv3:           // handover: the 16-bit tensor is neither written nor read back, the fp8 stack's input comes out of this conv's epilogue
                rc = run_conv(h, c3, buf[fr[1]], n, h2, w2, idn, outb, 1, s, &h3, &w3, bp.handover ? 1.0f / h->fp8_scales[0] : 0.f,
                              bp.handover ? &layer1_out_fp8 : nullptr);
                break;
        }
        if (rc) return rc;
        if (bp.chain_next) pre_t1 = fr[0];
        if (!bp.inplace) cur = fr[3];
        hh = h3; ww = w3;
        if (bp.tap == TapAt::Out) return report(buf[cur], hh, ww, c3.cout);
    }
    switch (plan.stop) {
        case Stop::Fp8TapRefused: return fail(h, R50_ERR_INVALID, "fp8 mode: activations beyond layer1 are e4m3 tensors, taps stop at layer1.2");
        case Stop::Fp8Part: return run_fp8_part(h, buf, cur, n, out, s, layer1_out_fp8);
        case Stop::UnknownTap: return fail(h, R50_ERR_INVALID, std::string("unknown layer name: ") + tap);
        case Stop::Tap: return fail(h, R50_ERR_STATE, "internal: the planned tap was not reached");
        case Stop::Avgpool: break;
    }
    return profiled(h, s, PC_AVGPOOL, 0, (double)n * (hh * ww * 2048.0 * 2 + 2048.0 * 4), -1, "avgpool", kNoKey, [&] {
        return split ? launch_avgpool_split(buf[cur], out, n, hh * ww, 2048, s) : launch_avgpool(buf[cur], out, n, hh * ww, 2048, s, et);
    });
}

void free_weights(r50_handle* h) {        // the buffers a sharer reads through its owner
    const bool own = (h->owner == nullptr);
    for (auto& L : h->convs) {
        if (own && L.w) (void)hipFree(L.w);
        if (own && L.bias) (void)hipFree(L.bias);
        if (L.bias_scaled) (void)hipFree(L.bias_scaled);
        L.w = nullptr; L.bias = nullptr; L.bias_scaled = nullptr;
    }
    for (auto& p : h->tail3_wp) { if (own && p) (void)hipFree(p); p = nullptr; }
    if (own && h->catchain_wp) (void)hipFree(h->catchain_wp);
    h->catchain_wp = nullptr;
    for (int i = 0; i < 4; ++i) {
        if (own && h->cat_w[i]) (void)hipFree(h->cat_w[i]);
        if (own && h->cat_bias[i]) (void)hipFree(h->cat_bias[i]);
        h->cat_w[i] = nullptr; h->cat_bias[i] = nullptr;
    }
    if (own && h->stem_w) (void)hipFree(h->stem_w);
    h->stem_w = nullptr;
}
void free_all(r50_handle* h, bool keep_weights = false) {
    if (!keep_weights) free_weights(h);
    if (h->stem_xp) (void)hipFree(h->stem_xp);
    if (h->u8_table) (void)hipFree(h->u8_table);
    for (auto& b : h->buf) { if (b) (void)hipFree(b); b = nullptr; }
    for (int i = 0; i < 4; ++i) {
        if (h->side[i]) (void)hipStreamDestroy(h->side[i]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
        h->side[i] = nullptr; h->ev_join[i] = nullptr;
    }
    if (h->ds_stream) (void)hipStreamDestroy(h->ds_stream);
    if (h->ev_ds_fork) (void)hipEventDestroy(h->ev_ds_fork);
    if (h->ev_ds_join) (void)hipEventDestroy(h->ev_ds_join);
    h->ds_stream = nullptr; h->ev_ds_fork = nullptr; h->ev_ds_join = nullptr;
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    h->ev_fork = nullptr;
    for (auto& r : h->ev_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto& e : h->ev_free) (void)hipEventDestroy(e);
    h->ev_pending.clear(); h->ev_free.clear();
}

template <typename TIN>
int forward_impl(r50_handle* h, const TIN* x, int n, float* out, void* stream) {
    if (!h) return fail(nullptr, R50_ERR_INVALID, "r50_forward: null handle");
    if (!h->loaded) return fail(h, R50_ERR_STATE, "r50_forward: weights not loaded");
    if (!x || !out) return fail(h, R50_ERR_INVALID, "r50_forward: null buffer");
    if (n < 0) return fail(h, R50_ERR_INVALID, "r50_forward: n < 0");
    // the fused stem loads 4 pixels at a time (16 bytes of fp32, 4 of uint8); the average pool stores f32x4
    const Op op{sizeof(TIN) == 1 ? "r50_forward_u8" : "r50_forward", h};
    if (int rc = op.aligned({{x, sizeof(TIN) == 1 ? "x_nchw_u8_dev" : "x_nchw_f32_dev", sizeof(TIN) == 1 ? 4u : 16u}, {out, "out_f32_dev", 16}}))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    int chunk = h->max_batch;
    if (h->micro_batch > 0 && h->micro_batch < chunk) chunk = h->micro_batch;
    hipStream_t user = (hipStream_t)stream;
    for (int i = 0; i < n; i += chunk) {
        const int m = (n - i < chunk) ? (n - i) : chunk;
        const int ns = (h->n_streams > 1 && m >= 2 * h->n_streams) ? h->n_streams : 1;
        if (ns == 1) {
            int rc = run_stack(h, x + (size_t)i * 3 * 224 * 224, m, out + (size_t)i * 2048, user, nullptr, nullptr, nullptr);
            if (rc) return rc;
            continue;
        }
        // fork: the side streams start after everything already queued on the caller's stream
        if (!h->ev_fork) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->ev_fork, user));
        const int per = (m + ns - 1) / ns;
        for (int k = 0; k < ns; ++k) {
            const int f0 = k * per, cnt = (m - f0 < per) ? (m - f0) : per;
            if (cnt <= 0) break;
            if (!h->side[k]) HIP_TRY(h, hipStreamCreateWithFlags(&h->side[k], hipStreamNonBlocking));
            if (!h->ev_join[k]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_join[k], hipEventDisableTiming));
            HIP_TRY(h, hipStreamWaitEvent(h->side[k], h->ev_fork, 0));
            int rc = run_stack(h, x + (size_t)(i + f0) * 3 * 224 * 224, cnt, out + (size_t)(i + f0) * 2048, h->side[k],
                               nullptr, nullptr, nullptr, f0);
            if (rc) return rc;
            HIP_TRY(h, hipEventRecord(h->ev_join[k], h->side[k]));
            HIP_TRY(h, hipStreamWaitEvent(user, h->ev_join[k], 0));    // join
        }
    }
    return R50_OK;
}

// Every option: where it lives (a field of the handle, or a process-wide knob shared with the r50_op_* hooks), the values r50_set_option
// accepts and whether r50_get_option serves it.  "max_batch" and "workspace_bytes" are read-only and live in r50_get_option alone.
enum OptionKind { OPT_BOOL, OPT_RANGE, OPT_ANY, OPT_STEM_STRIP };     // BOOL: stored as value ? 1 : 0; RANGE: lo <= value <= hi or range_error; ANY: stored as it comes
struct Option {
    const char* key;
    int r50_handle::*field;
    int* global;
    OptionKind kind;
    int64_t lo, hi;
    const char* range_error;
    bool gettable;
};
const Option kOptions[] = {
    {"micro_batch", &r50_handle::micro_batch, nullptr, OPT_RANGE, 0, INT64_MAX, "micro_batch < 0", true},
    {"profile", &r50_handle::profile, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"tile", &r50_handle::tile_override, nullptr, OPT_ANY, 0, 0, nullptr, true},
    {"fused_stem", &r50_handle::fused_stem, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_tail", &r50_handle::fuse_tail, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_tail3", &r50_handle::fuse_tail3, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_cat_chain", &r50_handle::fuse_cat_chain, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"sub_out", &r50_handle::sub_out, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_tail3_last", &r50_handle::fuse_tail3_last, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"tail3_bp", nullptr, &g_tail3_bp, OPT_RANGE, 0, 112, "tail3_bp must be 0 .. 112", true},
    {"fuse_fp8_handover", &r50_handle::fuse_fp8_handover, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_stem_c1", &r50_handle::fuse_stem_c1, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_ds_cat", &r50_handle::fuse_ds_cat, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"stem_strip", nullptr, &g_stem_strip, OPT_STEM_STRIP, 0, 28, "stem_strip must be 0 or a divisor of 28", true},
    {"overlap_ds", &r50_handle::overlap_ds, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"streams", &r50_handle::n_streams, nullptr, OPT_RANGE, 1, 4, "streams must be in [1,4]", true},
    {"inplace_out", &r50_handle::inplace_out, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_block2", &r50_handle::fuse_block2, nullptr, OPT_BOOL, 0, 1, nullptr, true},
    {"fuse_block1", &r50_handle::fuse_block1, nullptr, OPT_RANGE, 0, 3, "fuse_block1 must be 0 .. 3", true},
    {"use_g8", nullptr, &g_use_g8, OPT_RANGE, 0, 3, "use_g8 must be 0 .. 3", true},
    {"use_s2", nullptr, &g_use_s2, OPT_ANY, 0, 0, nullptr, false},        // 0 = generic tiles for the stride-2 3x3 shapes
    {"cu_cap", nullptr, &g_cu_cap, OPT_RANGE, 0, 4096, "cu_cap must be in [0,4096]", true},
};
const Option* find_option(const char* key) {
    for (const Option& o : kOptions)
        if (std::strcmp(o.key, key) == 0) return &o;
    return nullptr;
}

}  // namespace

// =================================================================================================
extern "C" {

const char* r50_version(void) { return "r50hip 0.1.0 (gfx950)"; }

const char* r50_last_error(r50_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int r50_create(r50_handle** out, int device_id, int precision, int max_batch) {
    if (!out) return fail(nullptr, R50_ERR_INVALID, "r50_create: out is null");
    *out = nullptr;
    if (precision != R50_PREC_BF16 && precision != R50_PREC_FP32X && precision != R50_PREC_BF16W2 && precision != R50_PREC_FP16 &&
        precision != R50_PREC_FP8)
        return fail(nullptr, R50_ERR_INVALID, "r50_create: unsupported precision");
    const int cmul = (precision == R50_PREC_FP32X) ? 2 : 1;
    // The kernels address every tensor through 31-bit buffer descriptors (fill_conv_args): the largest activation, layer1's
    // (n,56,56,256), is n x 1.6 MB in the 16-bit modes (n <= 1337) and twice that in fp32x mode ([head | tail] pairs: n <= 668).
    const int batch_cap = (precision == R50_PREC_FP32X) ? 640 : 1024;
    if (max_batch < 1 || max_batch > batch_cap)
        return fail(nullptr, R50_ERR_INVALID, "r50_create: max_batch must be in [1," + std::to_string(batch_cap) + "] for this precision");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, R50_ERR_HIP, "r50_create: no HIP device available");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, R50_ERR_INVALID, "r50_create: bad device_id");
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, R50_ERR_HIP, std::string("r50_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    r50_handle* h = new r50_handle();
    h->device = device_id; h->precision = precision; h->max_batch = max_batch;
    h->convs = make_specs();
    for (int i = 0; i < PC_COUNT; ++i) h->prof[i].name = kProfNames[i];
    h->prof_layer.resize(h->convs.size());
    for (size_t i = 0; i < h->convs.size(); ++i) h->prof_layer[i].name = h->convs[i].conv_key.c_str();
    h->buf_bytes = (size_t)max_batch * 112 * 112 * 64 * 2 * cmul;
    bool ok = true;
    for (int i = 0; i < 5 && ok; ++i) ok = hipMalloc((void**)&h->buf[i], h->buf_bytes) == hipSuccess;
    ok = ok && hipMalloc((void**)&h->stem_xp, (size_t)max_batch * STEM_HP * STEM_WP * 8 * cmul) == hipSuccess;
    ok = ok && hipMalloc((void**)&h->stem_w, STEM_W_BYTES * cmul) == hipSuccess;
    {   // the reference's host arithmetic, three fp32 operations per sample (src/dataset.py:148-149,242-245)
        static const float kMean[3] = {0.485f, 0.456f, 0.406f}, kStd[3] = {0.229f, 0.224f, 0.225f};
        std::vector<float> tab(3 * 256);
        for (int c = 0; c < 3; ++c)
            for (int v = 0; v < 256; ++v) {
                const float a = (float)v / 255.0f;
                const float b = a - kMean[c];
                tab[c * 256 + v] = b / kStd[c];
            }
        ok = ok && hipMalloc((void**)&h->u8_table, tab.size() * sizeof(float)) == hipSuccess &&
             hipMemcpy(h->u8_table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        free_all(h);
        delete h;
        return fail(nullptr, R50_ERR_NOMEM, "r50_create: device allocation failed");
    }
    *out = h;
    return R50_OK;
}

void r50_destroy(r50_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->sharers > 0) {                 // other handles still read this one's weights: everything else goes now, the weights with the last sharer
        free_all(h, /*keep_weights=*/true);
        h->zombie = true;
        return;
    }
    r50_handle* owner = h->owner;
    free_all(h);
    delete h;
    if (owner && --owner->sharers == 0 && owner->zombie) {
        free_weights(owner);
        delete owner;
    }
}

int r50_share_weights(r50_handle* h, r50_handle* from) {
    if (!h || !from) return fail(h, R50_ERR_INVALID, "r50_share_weights: null handle");
    if (h == from || h->owner || h->loaded) return fail(h, R50_ERR_STATE, "r50_share_weights: the handle already has weights");
    if (!from->loaded || from->zombie) return fail(h, R50_ERR_STATE, "r50_share_weights: the source handle has no weights loaded");
    if (from->owner) from = from->owner;
    if (h->device != from->device || h->precision != from->precision)
        return fail(h, R50_ERR_INVALID, "r50_share_weights: device and precision of the two handles must be the same");
    if (!is16(h->precision))
        return fail(h, R50_ERR_INVALID, "r50_share_weights: bf16 / fp16 handles only (the fp8 mode rewrites weight buffers per handle when its scales are set)");
    (void)hipSetDevice(h->device);
    if (h->stem_w) (void)hipFree(h->stem_w);                  // allocated by r50_create
    h->stem_w = from->stem_w;
    for (size_t i = 0; i < h->convs.size(); ++i) {
        ConvLayer& L = h->convs[i];
        const ConvLayer& S = from->convs[i];
        L.w = S.w; L.bias = S.bias; L.wscale = S.wscale; L.bias_host = S.bias_host; L.w_host = S.w_host;
    }
    for (int i = 0; i < 4; ++i) { h->cat_w[i] = from->cat_w[i]; h->cat_bias[i] = from->cat_bias[i]; h->cat_acc_scale[i] = from->cat_acc_scale[i]; }
    for (int b = 0; b < 8; ++b) h->tail3_wp[b] = from->tail3_wp[b];
    h->catchain_wp = from->catchain_wp;
    h->owner = from;
    ++from->sharers;
    h->loaded = true;
    return R50_OK;
}

int r50_load_weights(r50_handle* h, const r50_tensor_desc* tensors, int n_tensors) {
    if (!h) return fail(nullptr, R50_ERR_INVALID, "r50_load_weights: null handle");
    if (!tensors || n_tensors <= 0) return fail(h, R50_ERR_INVALID, "r50_load_weights: no tensors");
    // handles that take part in r50_share_weights: a sharer would write the folded weights into its OWNER's buffers (and leak what it allocates beside
    // them); an owner with sharers would repack the weights under lanes that may be in mid-forward on other streams
    if (h->owner || h->sharers > 0 || h->zombie)
        return fail(h, R50_ERR_STATE, "r50_load_weights: this handle shares its weight buffers (r50_share_weights): load into a fresh handle instead");
    HIP_TRY(h, hipSetDevice(h->device));
    std::map<std::string, const r50_tensor_desc*> by_name;
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name || !tensors[i].data) return fail(h, R50_ERR_INVALID, "r50_load_weights: null name/data");
        by_name[tensors[i].name] = &tensors[i];
    }
    auto need = [&](const std::string& k, int64_t numel, const float** p) -> int {
        auto it = by_name.find(k);
        if (it == by_name.end()) return fail(h, R50_ERR_INVALID, "r50_load_weights: missing tensor " + k);
        if (it->second->numel != numel)
            return fail(h, R50_ERR_INVALID, "r50_load_weights: tensor " + k + " has " + std::to_string(it->second->numel) +
                                                " elements, expected " + std::to_string(numel));
        *p = it->second->data;
        return R50_OK;
    };
    std::vector<float> wf, bf;
    std::vector<uint16_t> pk;
    // [W3 | Wd] and b3 + bd of layer2.0 / layer3.0 / layer4.0 (16-bit precisions): convs are stored c1, c2, c3, ds per first block
    const bool want_cat = is16(h->precision);
    std::map<size_t, std::pair<std::vector<uint16_t>, std::vector<float>>> kept;       // conv index -> (packed weights, bias)
    for (size_t i = 0; i < h->convs.size(); ++i) {
        ConvLayer& L = h->convs[i];
        const float *w, *g, *b, *m, *v;
        const int per_out = L.cin * L.ks * L.ks;
        int rc;
        if ((rc = need(L.conv_key + ".weight", (int64_t)L.cout * per_out, &w))) return rc;
        if ((rc = need(L.bn_key + ".weight", L.cout, &g))) return rc;
        if ((rc = need(L.bn_key + ".bias", L.cout, &b))) return rc;
        if ((rc = need(L.bn_key + ".running_mean", L.cout, &m))) return rc;
        if ((rc = need(L.bn_key + ".running_var", L.cout, &v))) return rc;
        fold_bn(w, g, b, m, v, L.cout, per_out, wf, bf);
        L.bias_host = bf;
        if (!L.bias) HIP_TRY(h, hipMalloc((void**)&L.bias, L.cout * sizeof(float)));
        HIP_TRY(h, hipMemcpy(L.bias, bf.data(), L.cout * sizeof(float), hipMemcpyHostToDevice));
        const bool split = (h->precision == R50_PREC_FP32X);
        if (i == 0) {
            pack_stem(wf.data(), pk, h->precision == R50_PREC_FP16 ? 2 : 0);
            HIP_TRY(h, hipMemcpy(h->stem_w, pk.data(), STEM_W_BYTES, hipMemcpyHostToDevice));
            if (split) {
                pack_stem(wf.data(), pk, 1);
                HIP_TRY(h, hipMemcpy(h->stem_w + STEM_W_BYTES, pk.data(), STEM_W_BYTES, hipMemcpyHostToDevice));
            }
        } else {
            if (split) pack_ohwi_split(wf.data(), L.cout, L.cin, L.ks, pk);
            else if (h->precision == R50_PREC_BF16W2) pack_ohwi_w2(wf.data(), L.cout, L.cin, L.ks, pk);
            else if (h->precision == R50_PREC_FP16) pack_ohwi_f16(wf.data(), L.cout, L.cin, L.ks, pk);
            else if (h->precision == R50_PREC_FP8 && i >= kFp8FirstConv) {
                L.wscale = pack_ohwi_fp8(wf.data(), L.cout, L.cin, L.ks, pk);
                if (L.ks == 1 && (L.conv_key.find(".0.conv3") != std::string::npos || L.conv_key.find(".downsample.0") != std::string::npos))
                    L.w_host = wf;
            }
            else pack_ohwi_bf16(wf.data(), L.cout, L.cin, L.ks, pk);
            if (!L.w) HIP_TRY(h, hipMalloc((void**)&L.w, pk.size() * 2));
            HIP_TRY(h, hipMemcpy(L.w, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
            if (want_cat && L.ks == 1 && (L.conv_key.find(".0.conv3") != std::string::npos || L.conv_key.find(".downsample.0") != std::string::npos))
                kept[i] = {pk, bf};
        }
    }
    if (want_cat) {
        size_t li = 1;
        for (int si = 0; si < 4; ++si) {
            const size_t i3 = li + 2, id = li + 3;
            if (si >= 1 && kept.count(i3) && kept.count(id)) {
                const ConvLayer &c3 = h->convs[i3], &cd = h->convs[id];
                const int k1 = c3.cin, k2 = cd.cin, co = c3.cout;
                std::vector<uint16_t> cat((size_t)co * (k1 + k2));
                std::vector<float> cb(co);
                for (int o = 0; o < co; ++o) {
                    std::memcpy(&cat[(size_t)o * (k1 + k2)], &kept[i3].first[(size_t)o * k1], (size_t)k1 * 2);
                    std::memcpy(&cat[(size_t)o * (k1 + k2) + k1], &kept[id].first[(size_t)o * k2], (size_t)k2 * 2);
                    cb[o] = kept[i3].second[o] + kept[id].second[o];
                }
                if (!h->cat_w[si]) HIP_TRY(h, hipMalloc((void**)&h->cat_w[si], cat.size() * 2));
                if (!h->cat_bias[si]) HIP_TRY(h, hipMalloc((void**)&h->cat_bias[si], co * sizeof(float)));
                HIP_TRY(h, hipMemcpy(h->cat_w[si], cat.data(), cat.size() * 2, hipMemcpyHostToDevice));
                HIP_TRY(h, hipMemcpy(h->cat_bias[si], cb.data(), co * sizeof(float), hipMemcpyHostToDevice));
            }
            li += 4 + 3 * (kStages[si][1] - 1);
        }
    }
    // layer3.1-.4: conv3 of block b and conv1 of block b+1 in the chained tail kernel's fragment-ordered stream (16-bit precisions)
    if (want_cat) {
        size_t li = 1;
        for (int si = 0; si < 4; ++si) {
            const int blocks = kStages[si][1];
            for (int b = 0; b < blocks; ++b) {
                const size_t i3 = li + 2, inx = li + ((b == 0) ? 4 : 3);
                if (si == 1 && b == 0 && h->cat_w[1] && inx < h->convs.size()) {
                    const ConvLayer& c3 = h->convs[i3];
                    const ConvLayer& cd = h->convs[li + 3];
                    const ConvLayer& nx = h->convs[inx];
                    if (c3.ks == 1 && c3.cin == 128 && c3.cout == 512 && cd.ks == 1 && cd.cin == 256 && cd.stride == 2 && nx.ks == 1 && nx.stride == 1 &&
                        nx.cin == 512 && nx.cout == 128) {
                        if (!h->catchain_wp) HIP_TRY(h, hipMalloc((void**)&h->catchain_wp, kCatChainPackedBytes));
                        HIP_TRY(h, pack_catchain_weights(h->cat_w[1], nx.w, h->catchain_wp, nullptr));
                    }
                }
                if (si == 2 && b > 0 && b < 8 && inx < h->convs.size()) {
                    const ConvLayer& c3 = h->convs[i3];
                    const ConvLayer& nx = h->convs[inx];
                    if (c3.ks == 1 && c3.cin == 256 && c3.cout == 1024 && nx.ks == 1 && nx.stride == 1 && nx.cin == 1024 && nx.cout == 256) {
                        if (!h->tail3_wp[b]) HIP_TRY(h, hipMalloc((void**)&h->tail3_wp[b], kTail3PackedBytes));
                        HIP_TRY(h, pack_tail3_weights(c3.w, nx.w, h->tail3_wp[b], nullptr));
                    } else if (b == blocks - 1 && c3.ks == 1 && c3.cin == 256 && c3.cout == 1024) {
                        // the stage's last block: conv3 + identity + ReLU alone through the pipelined kernel (its W1 slices are never read: W3 stands in)
                        if (!h->tail3_wp[b]) HIP_TRY(h, hipMalloc((void**)&h->tail3_wp[b], kTail3PackedBytes));
                        HIP_TRY(h, pack_tail3_weights(c3.w, c3.w, h->tail3_wp[b], nullptr));
                    }
                }
                li += (b == 0) ? 4 : 3;
            }
        }
        HIP_TRY(h, hipDeviceSynchronize());
    }
    h->loaded = true;
    h->fp8_scales.clear();              // new weights: bias_scaled must be rebuilt
    return R50_OK;
}

int r50_set_fp8_scales(r50_handle* h, const float* scales, int n) {
    if (!h || !scales) return fail(h, R50_ERR_INVALID, "r50_set_fp8_scales: null argument");
    if (h->precision != R50_PREC_FP8) return fail(h, R50_ERR_STATE, "r50_set_fp8_scales: handle is not in R50_PREC_FP8 mode");
    if (!h->loaded) return fail(h, R50_ERR_STATE, "r50_set_fp8_scales: weights not loaded");
    if (n != R50_FP8_NUM_SCALES) return fail(h, R50_ERR_INVALID, "r50_set_fp8_scales: expected R50_FP8_NUM_SCALES values");
    for (int i = 0; i < n; ++i)
        if (!(scales[i] > 0.f) || !std::isfinite(scales[i])) return fail(h, R50_ERR_INVALID, "r50_set_fp8_scales: scales must be positive and finite");
    HIP_TRY(h, hipSetDevice(h->device));
    // input scale of every fp8 conv, walking the blocks in execution order (same walk as run_fp8_part)
    size_t li = kFp8FirstConv;
    int k = 0;
    float s_in = scales[k++];
    std::vector<float> tmp;
    auto set_bias = [&](ConvLayer& L, float sx) -> int {
        tmp.resize(L.cout);
        for (int o = 0; o < L.cout; ++o) tmp[o] = L.bias_host[o] / (sx * L.wscale);
        if (!L.bias_scaled) HIP_TRY(h, hipMalloc((void**)&L.bias_scaled, L.cout * sizeof(float)));
        HIP_TRY(h, hipMemcpy(L.bias_scaled, tmp.data(), L.cout * sizeof(float), hipMemcpyHostToDevice));
        return R50_OK;
    };
    for (int si = 1; si < 4; ++si)
        for (int b = 0; b < kStages[si][1]; ++b) {
            const float s_t1 = scales[k++], s_t2 = scales[k++];
            int rc;
            if ((rc = set_bias(h->convs[li], s_in))) return rc;
            if ((rc = set_bias(h->convs[li + 1], s_t1))) return rc;
            if ((rc = set_bias(h->convs[li + 2], s_t2))) return rc;
            if (b == 0) {
                ++k;
                if ((rc = set_bias(h->convs[li + 3], s_in))) return rc;
                // conv3 + downsample as ONE fp8 accumulation over [t2 | x at the block's stride]: both products must land in the same
                // accumulator unit, s = s_t2 * s_w3' = s_x * s_wd'.  s = the larger of the two natural units, so neither weight matrix
                // clips; the other one is requantised a little coarser than its absmax would allow.
                ConvLayer &c3 = h->convs[li + 2], &cd = h->convs[li + 3];
                if (!c3.w_host.empty() && !cd.w_host.empty()) {
                    const float a3 = absmax_of(c3.w_host), ad = absmax_of(cd.w_host);
                    const float unit = std::fmax(s_t2 * (a3 > 0.f ? a3 / 448.0f : 1.0f), s_in * (ad > 0.f ? ad / 448.0f : 1.0f));
                    const float sw3 = unit / s_t2, swd = unit / s_in;
                    const int k1 = c3.cin, k2 = cd.cin, co = c3.cout;
                    std::vector<uint8_t> cat((size_t)co * (k1 + k2));
                    tmp.resize(co);
                    for (int o = 0; o < co; ++o) {
                        for (int c = 0; c < k1; ++c) cat[(size_t)o * (k1 + k2) + c] = f32_to_e4m3(c3.w_host[(size_t)o * k1 + c] / sw3);
                        for (int c = 0; c < k2; ++c) cat[(size_t)o * (k1 + k2) + k1 + c] = f32_to_e4m3(cd.w_host[(size_t)o * k2 + c] / swd);
                        tmp[o] = (c3.bias_host[o] + cd.bias_host[o]) / unit;
                    }
                    if (!h->cat_w[si]) HIP_TRY(h, hipMalloc((void**)&h->cat_w[si], cat.size()));
                    if (!h->cat_bias[si]) HIP_TRY(h, hipMalloc((void**)&h->cat_bias[si], co * sizeof(float)));
                    HIP_TRY(h, hipMemcpy(h->cat_w[si], cat.data(), cat.size(), hipMemcpyHostToDevice));
                    HIP_TRY(h, hipMemcpy(h->cat_bias[si], tmp.data(), co * sizeof(float), hipMemcpyHostToDevice));
                    h->cat_acc_scale[si] = unit;
                }
            }
            s_in = scales[k++];
            li += (b == 0) ? 4 : 3;
        }
    h->fp8_scales.assign(scales, scales + n);
    return R50_OK;
}

int r50_forward(r50_handle* h, const float* x, int n, float* out, void* stream) {
    return forward_impl<float>(h, x, n, out, stream);
}

int r50_forward_u8(r50_handle* h, const uint8_t* x, int n, float* out, void* stream) {
    return forward_impl<unsigned char>(h, x, n, out, stream);
}

int r50_forward_layer(r50_handle* h, const float* x, int n, const char* layer, void* out, int64_t cap,
                      int64_t dims_out[4], void* stream) {
    if (!h) return fail(nullptr, R50_ERR_INVALID, "r50_forward_layer: null handle");
    if (!h->loaded) return fail(h, R50_ERR_STATE, "r50_forward_layer: weights not loaded");
    if (!x || !out || !layer || !dims_out) return fail(h, R50_ERR_INVALID, "r50_forward_layer: null argument");
    if (n < 1 || n > h->max_batch) return fail(h, R50_ERR_INVALID, "r50_forward_layer: n must be in [1,max_batch]");
    const Op op{"r50_forward_layer", h};
    if (int rc = op.aligned({{x, "x_nchw_f32_dev", 16}, {out, "out_bf16_nhwc_dev", 2}})) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const __bf16* p = nullptr;
    int rc = run_stack(h, x, n, nullptr, (hipStream_t)stream, layer, &p, dims_out);
    if (rc) return rc;
    const int64_t bytes = dims_out[0] * dims_out[1] * dims_out[2] * dims_out[3] * 2;
    if (bytes > cap) return fail(h, R50_ERR_INVALID, "r50_forward_layer: output buffer too small");
    HIP_TRY(h, hipMemcpyAsync(out, p, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return R50_OK;
}

int r50_set_option(r50_handle* h, const char* key, int64_t value) {
    if (!h || !key) return fail(h, R50_ERR_INVALID, "r50_set_option: null argument");
    const Option* o = find_option(key);
    if (!o) return fail(h, R50_ERR_INVALID, std::string("r50_set_option: unknown key ") + key);
    if (o->kind == OPT_RANGE && (value < o->lo || value > o->hi)) return fail(h, R50_ERR_INVALID, o->range_error);
    if (o->kind == OPT_STEM_STRIP && !(value == 0 || (value > 0 && 28 % value == 0))) return fail(h, R50_ERR_INVALID, o->range_error);
    (o->field ? h->*(o->field) : *o->global) = (o->kind == OPT_BOOL) ? (value ? 1 : 0) : (int)value;
    if (o->global == &g_cu_cap) g_num_cus = 0;       // the budget is worked out again at the next launch
    return R50_OK;
}

int r50_get_option(r50_handle* h, const char* key, int64_t* value) {
    if (!h || !key || !value) return fail(h, R50_ERR_INVALID, "r50_get_option: null argument");
    const Option* o = find_option(key);
    if (o && o->gettable) *value = o->field ? h->*(o->field) : *o->global;
    else if (std::strcmp(key, "max_batch") == 0) *value = h->max_batch;
    else if (std::strcmp(key, "workspace_bytes") == 0) *value = (int64_t)(5 * h->buf_bytes + (size_t)h->max_batch * STEM_HP * STEM_WP * 8);
    else return fail(h, R50_ERR_INVALID, std::string("r50_get_option: unknown key ") + key);
    return R50_OK;
}

int r50_profile_reset(r50_handle* h) {
    if (!h) return R50_ERR_INVALID;
    for (auto& r : h->ev_pending) { h->ev_free.push_back(r.a); h->ev_free.push_back(r.b); }
    h->ev_pending.clear();
    for (int i = 0; i < PC_COUNT; ++i) { h->prof[i].launches = 0; h->prof[i].ms = h->prof[i].flops = h->prof[i].bytes = 0; }
    for (auto& p : h->prof_layer) { p.launches = 0; p.ms = p.flops = p.bytes = 0; }
    return R50_OK;
}

int r50_profile_collect(r50_handle* h) {
    if (!h) return R50_ERR_INVALID;
    for (auto& r : h->ev_pending) {
        HIP_TRY(h, hipEventSynchronize(r.b));
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, r.a, r.b));
        Prof& p = h->prof[r.cls];
        p.launches += 1; p.ms += ms; p.flops += r.flops; p.bytes += r.bytes;
        if (r.layer >= 0 && r.layer < (int)h->prof_layer.size()) {
            Prof& q = h->prof_layer[r.layer];
            q.launches += 1; q.ms += ms; q.flops += r.flops; q.bytes += r.bytes;
        }
        h->ev_free.push_back(r.a); h->ev_free.push_back(r.b);
    }
    h->ev_pending.clear();
    return R50_OK;
}

int r50_profile_count(r50_handle* h) { return h ? PC_COUNT + (int)h->prof_layer.size() - 1 : 0; }

int r50_profile_entry(r50_handle* h, int i, const char** name, int64_t* launches, double* total_ms, double* flops,
                      double* bytes) {
    if (!h || i < 0 || i >= PC_COUNT + (int)h->prof_layer.size() - 1) return R50_ERR_INVALID;
    const Prof& p = (i < PC_COUNT) ? h->prof[i] : h->prof_layer[i - PC_COUNT + 1];    // [0] is the stem conv: class "conv1"
    if (name) *name = p.name;
    if (launches) *launches = p.launches;
    if (total_ms) *total_ms = p.ms;
    if (flops) *flops = p.flops;
    if (bytes) *bytes = p.bytes;
    return R50_OK;
}

int r50_get_packed(r50_handle* h, const char* conv_key, int what, void* dst_host, int64_t capacity_bytes,
                   int64_t* bytes_out) {
    if (!h || !conv_key || !dst_host || !bytes_out) return fail(h, R50_ERR_INVALID, "r50_get_packed: null argument");
    if (!h->loaded) return fail(h, R50_ERR_STATE, "r50_get_packed: weights not loaded");
    HIP_TRY(h, hipSetDevice(h->device));
    for (size_t i = 0; i < h->convs.size(); ++i) {
        const ConvLayer& L = h->convs[i];
        if (L.conv_key != conv_key) continue;
        const void* src;
        int64_t bytes;
        if (what == 1) { src = L.bias; bytes = (int64_t)L.cout * 4; }
        else if (i == 0) { src = h->stem_w; bytes = STEM_W_BYTES; }
        else if (h->precision == R50_PREC_FP8 && i >= kFp8FirstConv) { src = L.w; bytes = (int64_t)L.cout * L.ks * L.ks * L.cin; }
        else { src = L.w; bytes = (int64_t)L.cout * L.ks * L.ks * L.cin * 2 * (h->precision == R50_PREC_FP32X ? 3 : h->precision == R50_PREC_BF16W2 ? 2 : 1); }
        *bytes_out = bytes;
        if (bytes > capacity_bytes) return fail(h, R50_ERR_INVALID, "r50_get_packed: buffer too small");
        HIP_TRY(h, hipMemcpy(dst_host, src, bytes, hipMemcpyDeviceToHost));
        return R50_OK;
    }
    return fail(h, R50_ERR_INVALID, std::string("r50_get_packed: unknown conv ") + conv_key);
}

// ---- op-level entry points -------------------------------------------------------------------
#if defined(R50_STAMP)      // diagnostic build only (not declared in include/r50.h): where the kernel's cycle sums go
extern "C" __attribute__((visibility("default"))) void r50_debug_buffer(void* p) { g_dbg = (unsigned long long*)p; }
#endif

static int op_conv2d_et(const Op& op, int et, const void* x, int n, int h, int w, int cin, const void* wt, const float* bias, const void* res,
                        void* y, int cout, int ksize, int stride, int pad, int relu, int tile, void* stream);

int r50_op_conv2d(const void* x, int n, int h, int w, int cin, const void* wt, const float* bias, const void* res,
                  void* y, int cout, int ksize, int stride, int pad, int relu, int tile, void* stream) {
    const Op op{"r50_op_conv2d"};
    if (int rc = op.aligned({{x, "x_nhwc_bf16", 16}, {wt, "w_ohwi_bf16", 16}, {bias, "bias_f32", 16},
                             {res, "residual_nhwc_bf16", 16}, {y, "y_nhwc_bf16", 16}}))
        return rc;
    return op_conv2d_et(op, 0, x, n, h, w, cin, wt, bias, res, y, cout, ksize, stride, pad, relu, tile, stream);
}

int r50_op_conv2d_f16(const void* x, int n, int h, int w, int cin, const void* wt, const float* bias, const void* res,
                      void* y, int cout, int ksize, int stride, int pad, int relu, int tile, void* stream) {
    const Op op{"r50_op_conv2d_f16"};
    if (int rc = op.aligned({{x, "x_nhwc_f16", 16}, {wt, "w_ohwi_f16", 16}, {bias, "bias_f32", 16},
                             {res, "residual_nhwc_f16", 16}, {y, "y_nhwc_f16", 16}}))
        return rc;
    return op_conv2d_et(op, 1, x, n, h, w, cin, wt, bias, res, y, cout, ksize, stride, pad, relu, tile, stream);
}

static int op_conv2d_et(const Op& op, int et, const void* x, int n, int h, int w, int cin, const void* wt, const float* bias, const void* res,
                        void* y, int cout, int ksize, int stride, int pad, int relu, int tile, void* stream) {
    ConvArgs a;
    if (const Launch r = fill_conv_args(a, x, n, h, w, cin, wt, bias, res, y, cout, ksize, stride, pad, relu); !r.ok())
        return op.refuse(r.note("invalid arguments"));
    a.et = et;
#if defined(R50_STAMP)
    a.dbg = g_dbg;
#endif
    // these two hooks answer the launcher's refusal (a tile id that does not fit the shape) with R50_ERR_HIP; the other convolution hooks,
    // through done(), with R50_ERR_INVALID
    const Launch r = launch_igemm(a, tile, (hipStream_t)stream);
    return r.ok() ? R50_OK : op.hip_failed(r.hip_text());
}

// The two pair precisions at kernel level: the ConvArgs run_conv builds for R50_PREC_BF16W2 / R50_PREC_FP32X, through the same launcher.
int r50_op_conv2d_w2(const void* x, int n, int h, int w, int cin, const void* w_pair, const float* bias, const void* res, void* y,
                     int cout, int ksize, int stride, int pad, int relu, int tile, void* stream) {
    const Op op{"r50_op_conv2d_w2"};
    if (int rc = op.aligned({{x, "x_nhwc_bf16", 16}, {w_pair, "w_pair_bf16", 16}, {bias, "bias_f32", 16},
                             {res, "residual_nhwc_bf16", 16}, {y, "y_nhwc_bf16", 16}}))
        return rc;
    ConvArgs a;
    if (const Launch r = fill_conv_args(a, x, n, h, w, cin, w_pair, bias, res, y, cout, ksize, stride, pad, relu, false, true); !r.ok())
        return op.refuse(r.note("invalid arguments"));
    // only igemm_bf16_kernel and igemm_ws_kernel wrap the X chunk index (ConvArgs::x_wrap): the shape-specialised kernels walk K on their own
    if (tile == kTileC64 || tile == kTileXres || tile == kTileS2 || tile == kTileG8 || tile == kTileG8N7)
        return op.refuse("tile id " + std::to_string(tile) + " does not read the weight pair");
    return op.done(launch_igemm(a, tile, (hipStream_t)stream));
}

int r50_op_conv2d_split(const void* x_pair, int n, int h, int w, int cin, const void* w_trip, const float* bias, const void* res_pair,
                        void* y_pair, int cout, int ksize, int stride, int pad, int relu, void* stream) {
    const Op op{"r50_op_conv2d_split"};
    if (int rc = op.aligned({{x_pair, "x_pair_bf16", 16}, {w_trip, "w_trip_bf16", 16}, {bias, "bias_f32", 16},
                             {res_pair, "residual_pair_bf16", 16}, {y_pair, "y_pair_bf16", 16}}))
        return rc;
    ConvArgs a;
    if (const Launch r = fill_conv_args(a, x_pair, n, h, w, cin, w_trip, bias, res_pair, y_pair, cout, ksize, stride, pad, relu, true, false); !r.ok())
        return op.refuse(r.note("invalid arguments"));
    return op.done(launch_igemm(a, 0, (hipStream_t)stream, true));
}

int r50_op_conv2d_fp8(const void* x, int n, int h, int w, int cin, const void* wt, const float* bias_scaled, const void* res, void* y,
                      int cout, int ksize, int stride, int pad, int relu, float oscale, float rscale, int tile, void* stream) {
    const Op op{"r50_op_conv2d_fp8"};
    if (int rc = op.aligned({{x, "x_nhwc_fp8", 16}, {wt, "w_ohwi_fp8", 16}, {bias_scaled, "bias_scaled_f32", 16},
                             {res, "residual_nhwc_fp8", 16}, {y, "y_nhwc_fp8", 16}}))
        return rc;
    if (cin <= 0 || cin % 128) return op.refuse("cin must be a multiple of 128");
    ConvArgs a;
    // the loaders move bytes: described in 2-byte units, an fp8 tensor with cin channels is a 16-bit tensor with cin / 2
    if (const Launch r = fill_conv_args(a, x, n, h, w, cin / 2, wt, bias_scaled, res, y, cout, ksize, stride, pad, relu); !r.ok())
        return fail(nullptr, R50_ERR_INVALID, std::string(op.name) + " (sizes as 16-bit pairs: cx = cin/2, cy = cout): " + r.note("invalid arguments"));
    a.y_bytes = (unsigned)((long long)a.M * cout);       // one byte per output element
    a.et = 2; a.oscale = oscale; a.rscale = rscale;
    return op.done(launch_igemm_fp8(a, tile, (hipStream_t)stream));
}

int r50_op_conv1x1_cat(const void* x1, int n, int h, int w, int c1, const void* x2, int h2, int w2, int c2, int stride2, const void* wcat,
                       const float* bias, void* y, int cout, int relu, int tile, int et, void* stream) {
    const Op op{"r50_op_conv1x1_cat"};
    if (int rc = op.aligned({{x1, "x1", 16}, {x2, "x2", 16}, {wcat, "wcat", 16},
                             {bias, "bias_f32", 16}, {y, "y", 16}}))
        return rc;
    ConvArgs a;
    if (const Launch r = fill_conv_args_cat(a, x1, n, h, w, c1, x2, h2, w2, c2, stride2, wcat, bias, y, cout, relu); !r.ok() || (et != 0 && et != 1))
        return op.refuse(r.note("invalid arguments"));
    a.et = et;
    return op.done(launch_igemm(a, cat_tile(a, tile), (hipStream_t)stream));
}

// Element type of the op-level hooks that have no argument for it (the fused tails, bodies and chain, the stem, the two pools): they run
// the bf16 instantiations unless R50_OP_ET=1 is in the environment, which selects the IEEE-half ones a handle in R50_PREC_FP16 launches
// (every tensor and weight is then fp16).  A test knob like R50_TAIL3_BP, read per call.
static int op_et() { const char* v = std::getenv("R50_OP_ET"); return (v && std::atoi(v) == 1) ? 1 : 0; }

int r50_op_bneck_tail(const void* y2, int64_t m, int cmid, const void* w3, const float* b3, const void* res, const void* wd,
                      const float* bd, void* out, const void* w1, int c1, const float* b1, void* y1n, void* stream) {
    const Op op{"r50_op_bneck_tail"};
    if (int rc = op.aligned({{y2, "y2_bf16", 16}, {w3, "w3_bf16", 16}, {b3, "b3", 16}, {res, "identity_bf16", 16}, {wd, "wd_bf16", 16},
                             {bd, "bd", 16}, {out, "out_bf16", 16}, {w1, "w1_bf16", 16}, {b1, "b1", 16}, {y1n, "y1n_bf16", 16}}))
        return rc;
    Launch r;
    const int et = op_et();
    // the size limit before anything is queued (the cmid = 256 forms pack their weights on the stream first)
    if ((cmid == 64 || cmid == 128 || cmid == 256) && m > 0 && tail_over(r, m, cmid)) return op.done(r);
    if (cmid == 64) r = launch_bneck_tail(y2, m, w3, b3, res, wd, bd, out, w1, c1, b1, y1n, (hipStream_t)stream, et);
    else if (cmid == 128 && c1 == 128 && !wd && !bd) r = launch_bneck_tail2(y2, m, w3, b3, res, out, w1, b1, y1n, (hipStream_t)stream, et);
    else if (cmid == 256 && c1 == 0 && !w1 && !b1 && !y1n && !wd && !bd) {
        // conv3 + identity + ReLU alone through the pipelined layer3 tail (the form layer3.5 runs in the network): W3 stands in for the unused W1 slices
        void* wp_scratch = nullptr;
        if (hipMallocAsync(&wp_scratch, kTail3PackedBytes, (hipStream_t)stream) != hipSuccess || !wp_scratch) return op.hip_failed("hipMallocAsync");
        r = pack_tail3_weights(w3, w3, wp_scratch, (hipStream_t)stream);
        if (r.ok()) r = launch_bneck_tail3(y2, m, wp_scratch, b3, res, out, nullptr, nullptr, (hipStream_t)stream, et, 0, /*no_next=*/true);
        const hipError_t ef = hipFreeAsync(wp_scratch, (hipStream_t)stream);
        if (r.ok()) r = ef;
    }
    else if (cmid == 256 && c1 == 256 && !wd && !bd) {
        const char* v = std::getenv("R50_TAIL3_BP");          // test / A-B knob of this debug hook: real pixels per tile (1..112); unset = automatic
        // the hook takes plain weight matrices: packed here, per call, into a buffer allocated AND freed in the caller's stream order on the
        // caller's current device (a process-wide scratch buffer would be shared by callers on other streams / devices: round-2 ADVICE)
        void* wp_scratch = nullptr;
        if (hipMallocAsync(&wp_scratch, kTail3PackedBytes, (hipStream_t)stream) != hipSuccess || !wp_scratch) return op.hip_failed("hipMallocAsync");
        r = pack_tail3_weights(w3, w1, wp_scratch, (hipStream_t)stream);
        if (r.ok()) r = launch_bneck_tail3(y2, m, wp_scratch, b3, res, out, b1, y1n, (hipStream_t)stream, et, v ? std::atoi(v) : 0);
        const hipError_t ef = hipFreeAsync(wp_scratch, (hipStream_t)stream);
        if (r.ok()) r = ef;
    }
    else r = Launch::refused();
    return op.done(r);
}

int r50_op_bneck_block2(const void* t1, int n, const void* w2, const float* b2, const void* w3, const float* b3, const void* res,
                        void* out, const void* w1, const float* b1, void* y1n, void* stream) {
    const Op op{"r50_op_bneck_block2"};
    if (int rc = op.aligned({{t1, "t1_bf16", 16}, {w2, "w2_bf16", 16}, {b2, "b2", 16}, {w3, "w3_bf16", 16}, {b3, "b3", 16},
                             {res, "identity_bf16", 16}, {out, "out_bf16", 16}, {w1, "w1_bf16", 16}, {b1, "b1", 16}, {y1n, "y1n_bf16", 16}}))
        return rc;
    return op.done(launch_bneck_block2(t1, n, w2, b2, w3, b3, res, out, w1, b1, y1n, (hipStream_t)stream, op_et()));
}

int r50_op_bneck_block1_ds(const void* t1, int n, const void* w2, const float* b2, const void* w3, const float* b3, const void* x, const void* wd,
                           const float* bd, void* out, const void* w1, const float* b1, void* y1n, void* stream) {
    const Op op{"r50_op_bneck_block1_ds"};
    if (int rc = op.aligned({{t1, "t1_bf16", 16}, {w2, "w2_bf16", 16}, {b2, "b2", 16}, {w3, "w3_bf16", 16}, {b3, "b3", 16}, {x, "x_bf16", 16},
                             {wd, "wd_bf16", 16}, {bd, "bd", 16}, {out, "out_bf16", 16}, {w1, "w1_bf16", 16}, {b1, "b1", 16}, {y1n, "y1n_bf16", 16}}))
        return rc;
    if (!wd || !bd) return op.refuse("null downsample weights");
    return op.done(launch_bneck_block1(t1, n, w2, b2, w3, b3, x, out, w1, 64, b1, y1n, (hipStream_t)stream, op_et(), wd, bd));
}

int r50_op_bneck_cat_chain(const void* t2, const void* x, int n, int ow, const void* wcat, const float* bcat, void* out, const void* w1,
                           const float* b1, void* y1n, void* stream) {
    const Op op{"r50_op_bneck_cat_chain"};
    if (int rc = op.aligned({{t2, "t2_bf16", 16}, {x, "x_bf16", 16}, {wcat, "wcat_bf16", 16}, {bcat, "bcat", 16},
                             {out, "out_bf16", 16}, {w1, "w1_bf16", 16}, {b1, "b1", 16}, {y1n, "y1n_bf16", 16}}))
        return rc;
    // plain weight matrices in, packed per call into a buffer allocated and freed in the caller's stream order (as r50_op_bneck_tail does)
    void* wp = nullptr;
    if (!wcat || !w1) return op.refuse("null weights");
    // the size limits before anything is queued (the weights are packed on the stream first)
    Launch r;
    if (n > 0 && ow == 28 && catchain_over(r, n, ow)) return op.done(r);
    if (hipMallocAsync(&wp, kCatChainPackedBytes, (hipStream_t)stream) != hipSuccess || !wp) return op.hip_failed("hipMallocAsync");
    r = pack_catchain_weights(wcat, w1, wp, (hipStream_t)stream);
    if (r.ok()) r = launch_bneck_catchain(t2, x, n, ow, wp, bcat, out, b1, y1n, (hipStream_t)stream, op_et());
    const hipError_t ef = hipFreeAsync(wp, (hipStream_t)stream);
    if (r.ok()) r = ef;
    return op.done(r);
}

int r50_op_bneck_block1(const void* t1, int n, const void* w2, const float* b2, const void* w3, const float* b3, const void* res,
                        void* out, const void* w1, int c1, const float* b1, void* y1n, void* stream) {
    const Op op{"r50_op_bneck_block1"};
    if (int rc = op.aligned({{t1, "t1_bf16", 16}, {w2, "w2_bf16", 16}, {b2, "b2", 16}, {w3, "w3_bf16", 16}, {b3, "b3", 16},
                             {res, "identity_bf16", 16}, {out, "out_bf16", 16}, {w1, "w1_bf16", 16}, {b1, "b1", 16}, {y1n, "y1n_bf16", 16}}))
        return rc;
    return op.done(launch_bneck_block1(t1, n, w2, b2, w3, b3, res, out, w1, c1, b1, y1n, (hipStream_t)stream, op_et()));
}

// Weight precision of ATen's native uint8 bilinear resize (antialias off) along one axis: the largest p with
// round(max_weight * 2^(p+1)) < 2^15, the maximum taken over every tap weight of the axis
// (aten/src/ATen/native/cpu/UpSampleKernel.cpp `_compute_index_ranges_int16_weights`; weights as in
// `_compute_indices_min_size_weights`, restated in oracle/resize_oracle.py:index_weights_int16 and, per thread, in
// kernels.h:resize_taps).
static int resize_weight_precision(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    double wt_max = 0.0;
    for (int i = 0; i < out_size; ++i) {
        double real = scale * (i + 0.5) - 0.5;
        if (real < 0.0) real = 0.0;
        long idx = (long)std::floor(real);
        if (idx > in_size - 1) idx = in_size - 1;
        double lam = real - (double)idx;
        lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
        const long umin = idx, umax = idx + 2;
        const long lo = umin > 0 ? umin : 0;
        const long size = (umax < in_size ? umax : in_size) - lo;
        double w[2] = {0.0, 0.0};
        long w_index = 0;
        for (int j = 0; j < 2; ++j) {
            const double x = std::fabs((double)j - lam);
            const double wj = x < 1.0 ? 1.0 - x : 0.0;
            if (umin + j <= 0) w_index = 0;
            else if (umin + j >= in_size - 1) w_index = size - 1;
            if (w_index == 0) w[0] += wj; else w[1] += wj;
            ++w_index;
        }
        if (w[0] > wt_max) wt_max = w[0];
        if (w[1] > wt_max) wt_max = w[1];
    }
    int precision = 0;
    for (; precision < 22; ++precision)
        if ((int)(0.5 + wt_max * (double)(1 << (precision + 1))) >= (1 << 15)) break;
    return precision;
}

int r50_op_crop_resize_u8(const void* frames, int t, int h, int w, int top, int left, int hh, int ww, void* out, int out_size,
                          int mode, int flags, void* stream) {
    const Op op{"r50_op_crop_resize_u8"};
    if (int rc = op.aligned({{out, "out_tchw_u8", 4}})) return rc;
    if (!frames || !out || t < 1 || h < 1 || w < 1 || hh < 1 || ww < 1 || top < 0 || left < 0 || top + hh > h || left + ww > w ||
        out_size < 4 || (out_size & 3) || out_size > 4096 || (long long)t * h * w * 3 >= (1ll << 40))
        return op.refuse("invalid arguments (the box must lie inside the frame; out_size % 4 == 0)");
    if (mode != R50_RESIZE_FLOAT && mode != R50_RESIZE_FIXED) return op.refuse("unknown mode");
    if (flags & ~(R50_AUG_HFLIP | R50_AUG_TREV)) return op.refuse("unknown flags");
    ResizeArgs a;
    a.hflip = (flags & R50_AUG_HFLIP) ? 1 : 0;
    a.trev = (flags & R50_AUG_TREV) ? 1 : 0;
    a.float_mode = (mode == R50_RESIZE_FLOAT);
    a.px = a.py = 1;
    if (!a.float_mode) {
        a.px = resize_weight_precision(ww, out_size);
        a.py = resize_weight_precision(hh, out_size);
        if (a.px < 1 || a.py < 1) return op.refuse("degenerate weights");
    }
    a.src = (const unsigned char*)frames; a.dst = (unsigned char*)out;
    a.T = t; a.H = h; a.W = w; a.top = top; a.left = left; a.hh = hh; a.ww = ww; a.out = out_size;
    const size_t lds = 2 * (size_t)((ww * 3 + 6) & ~3);                // two source rows of the crop, dword-padded
    if (lds > 160 * 1024 || (long long)t * out_size >= (1ll << 31)) return op.refuse("crop too wide");
    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(crop_resize_u8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return op.done(ea);
    hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)(t * out_size)), dim3(256), lds, (hipStream_t)stream, a);
    return op.done();
}

// ---- one box per output frame (include/r50_track.h, track_kernels.h, INTEGRATION.md section AA) ----
int r50_track_weight_precision(int in_size, int out_size) {
    if (in_size < 1 || out_size < 1) return -1;
    return resize_weight_precision(in_size, out_size);
}

int r50_op_crop_resize_boxes_u8(const void* src, int64_t src_bytes, const int64_t* table, int t, int max_ww, void* out, void* out_flip,
                                int out_size, int mode, void* stream) {
    const Op op{"r50_op_crop_resize_boxes_u8"};
    if (!src || !table || !out) return op.refuse("null pointer");
    if (int rc = op.aligned({{src, "src_u8", 4}, {out, "out_tchw_u8", 4}, {out_flip, "out_flip_tchw_u8", 4}, {table, "table_dev", 8}})) return rc;
    if (out_flip == out) return op.refuse("out_flip is not out");
    if (t < 1 || src_bytes < 1 || src_bytes >= (1ll << 40) || out_size < 4 || (out_size & 3) || out_size > 4096)
        return op.refuse("invalid arguments (need t >= 1, 1 <= src_bytes < 2^40, out_size % 4 == 0 in [4, 4096])");
    if (mode != R50_RESIZE_FLOAT && mode != R50_RESIZE_FIXED) return op.refuse("unknown mode");
    if (max_ww < 1 || max_ww > (160 * 1024 - 12) / 6 || (long long)t * out_size >= (1ll << 31)) return op.refuse("crop too wide");
    const size_t lds = 2 * (size_t)((max_ww * 3 + 6) & ~3);            // two source rows of the widest crop, dword-padded
    if (lds > 160 * 1024) return op.refuse("crop too wide");
    if (out_flip) {                                                     // the two outputs are written by one launch: they may not share a byte
        const long long n = (long long)t * 3 * out_size * out_size;
        const char *o = (const char*)out, *f = (const char*)out_flip;
        if (o < f + n && f < o + n) return op.refuse("out_flip overlaps out");
    }
    TrackArgs a;
    a.src = (const unsigned char*)src; a.src_bytes = (long long)src_bytes; a.table = (const long long*)table;
    a.dst = (unsigned char*)out; a.dst_flip = (unsigned char*)out_flip; a.out = out_size; a.float_mode = (mode == R50_RESIZE_FLOAT);
    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(crop_resize_boxes_u8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return op.done(ea);
    hipLaunchKernelGGL(crop_resize_boxes_u8_kernel, dim3((unsigned)(t * out_size)), dim3(256), lds, (hipStream_t)stream, a);
    return op.done();
}

int r50_op_resize_frames_u8(const void* frames, int n, int h, int w, const int* src_idx, int t, void* out, int out_size, void* stream) {
    const Op op{"r50_op_resize_frames_u8"};
    if (!frames || !src_idx || !out || n < 1 || h < 1 || w < 1 || t < 1 || out_size < 1 || out_size > 16384 ||
        (long long)n * h * w * 3 >= (1ll << 40) || (long long)t * out_size >= (1ll << 31))
        return op.refuse("invalid arguments");
    const size_t lds = 2 * (size_t)w * 3;                               // the two full-width source rows
    if (lds > 160 * 1024) return op.refuse("frames too wide");
    // the map lives on the device: read it back once (t ints, one stream synchronisation) so no index can reach past the frames
    std::vector<int> idx((size_t)t);
    hipStream_t s = (hipStream_t)stream;
    if (hipError_t e = hipMemcpyAsync(idx.data(), src_idx, (size_t)t * sizeof(int), hipMemcpyDeviceToHost, s)) return op.done(e);
    if (hipError_t e = hipStreamSynchronize(s)) return op.done(e);
    for (int i = 0; i < t; ++i)
        if (idx[i] < 0 || idx[i] >= n)
            return op.refuse("src_idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside [0, " + std::to_string(n) + ")");
    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(resize_frames_u8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return op.done(ea);
    hipLaunchKernelGGL(resize_frames_u8_kernel, dim3((unsigned)(t * out_size)), dim3(256), lds, s, (const unsigned char*)frames, src_idx,
                       h, w, out_size, (unsigned char*)out);
    return op.done();
}

// ---- skeleton drawing (kernels.h: draw_skeletons_u8_kernel).  Everything is checked here, before the launch: a refused call touches nothing.
int r50_op_draw_skeletons_u8(const void* bg, int bg_rgb, const float* pts, const void* style, const int* edges_host, int n_edges, int f,
                             int h, int w, int layers, int joints, float half_width, float joint_radius, void* out, void* stream) {
    const Op op{"r50_op_draw_skeletons_u8"};
    if (!pts || !style || !out) return op.refuse("null pointer (pts, style and out are required; only bg may be NULL)");
    if (f < 1 || h < 1 || w < 1) return op.refuse("need f, h, w >= 1");
    if (joints < 1 || joints > DRAW_MAX_JOINTS) return op.refuse("need 1 <= joints <= 64");
    if (layers < 1 || layers > DRAW_MAX_LAYERS) return op.refuse("need 1 <= layers <= 8");
    if (n_edges < 0 || n_edges > DRAW_MAX_EDGES) return op.refuse("need 0 <= n_edges <= 128");
    if (n_edges > 0 && !edges_host) return op.refuse("null pointer (edges_host with n_edges > 0)");
    if (!std::isfinite(half_width) || !std::isfinite(joint_radius) || half_width < 0.f || joint_radius < 0.f)
        return op.refuse("half_width and joint_radius must be finite and >= 0");
    if (bg_rgb < 0 || bg_rgb > 0xFFFFFF) return op.refuse("bg_rgb must be 0xRRGGBB");
    const long long bytes = (long long)f * h * w * 3;
    const long long tiles_x = (w + DRAW_TILE - 1) / DRAW_TILE, tiles_y = (h + DRAW_TILE - 1) / DRAW_TILE;
    if (bytes >= (1ll << 40) || tiles_x * tiles_y * f > INT32_MAX) return op.refuse("f * h * w is too large");
    if (bg) {
        const uintptr_t b0 = (uintptr_t)bg, o0 = (uintptr_t)out;
        if (b0 < o0 + (uintptr_t)bytes && o0 < b0 + (uintptr_t)bytes) return op.refuse("out may not alias bg");
    }
    DrawEdges ed;
    for (int q = 0; q < DRAW_MAX_EDGES; ++q) ed.ab[q] = 0;
    for (int q = 0; q < n_edges; ++q) {
        const int ea = edges_host[2 * q], eb = edges_host[2 * q + 1];
        if (ea < 0 || ea >= joints || eb < 0 || eb >= joints)
            return op.refuse("edge " + std::to_string(q) + " = (" + std::to_string(ea) + ", " + std::to_string(eb) + ") is outside [0, joints)");
        ed.ab[q] = (unsigned short)(ea | (eb << 8));
    }
    const size_t lds = draw_lds_bytes(layers, joints, n_edges);                        // <= 45,280 B: under the default 64 KB ceiling
    const bool vec = (w % 4 == 0) && (((uintptr_t)out | (uintptr_t)bg) & 3u) == 0;      // a NULL bg counts as aligned
    const dim3 grid((unsigned)(tiles_x * tiles_y * f));
    R50_ET_LAUNCH(vec, draw_skeletons_u8_kernel, grid, dim3(256), lds, stream, (const unsigned char*)bg, (unsigned)bg_rgb, pts,     // <1>: the 12-byte path
                  (const unsigned char*)style, ed, n_edges, h, w, layers, joints, (int)tiles_x, (int)tiles_y, half_width, joint_radius,
                  (unsigned char*)out);
    return op.done();
}

// ---- lifting head pieces (kernels.h: cast_rows_kernel, concat_pad_kernel, gn_relu_causal3_kernel); et: 0 = bf16, 1 = fp16
int r50_op_cast_rows(const float* src, int64_t rows, int c, void* dst, int cpad, int et, void* stream) {
    const Op op{"r50_op_cast_rows"};
    if (int rc = op.aligned({{dst, "dst", 4}})) return rc;
    if (!src || !dst || rows < 1 || c < 1 || cpad < c || (cpad & 1) || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, cast_rows_kernel, dim3(ew_grid(rows * (cpad / 2))), dim3(256), 0, stream, src, (unsigned short*)dst, (long long)rows, c, cpad);
    return op.done();
}

int r50_op_concat_pad(const void* phi, int d, const float* y, int ny, int64_t rows, void* dst, int dp, int et, void* stream) {
    const Op op{"r50_op_concat_pad"};
    if (int rc = op.aligned({{phi, "phi", 2}, {dst, "dst", 2}})) return rc;
    if (!phi || !y || !dst || rows < 1 || d < 1 || ny < 0 || dp < d + ny || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, concat_pad_kernel, dim3(ew_grid(rows * dp)), dim3(256), 0, stream, (const unsigned short*)phi, d, y, ny, (unsigned short*)dst,
                  (long long)rows, dp);
    return op.done();
}

int r50_op_add_rows(float* y, int ny, const void* dy, int dp, int64_t rows, int et, void* stream) {
    const Op op{"r50_op_add_rows"};
    if (int rc = op.aligned({{dy, "dy", 2}})) return rc;
    if (!y || !dy || rows < 1 || ny < 1 || dp < ny || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, add_rows_kernel, dim3(ew_grid(rows * ny)), dim3(256), 0, stream, y, ny, (const unsigned short*)dy, dp, (long long)rows);
    return op.done();
}

int r50_op_gn_relu_causal3(const void* x, int b, int t, int c, int groups, const float* gamma, const float* beta, float eps,
                           void* out, int et, void* stream) {
    const Op op{"r50_op_gn_relu_causal3"};
    if (int rc = op.aligned({{x, "x", 2}, {out, "out", 2}})) return rc;
    if (!x || !gamma || !beta || !out || b < 1 || t < 1 || c < 1 || groups < 1 || c % groups || (et != 0 && et != 1))
        return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, gn_relu_causal3_kernel, dim3((unsigned)(b * groups)), dim3(256), 0, stream, (const unsigned short*)x, gamma, beta,
                  (unsigned short*)out, t, c, groups, eps);
    return op.done();
}

int r50_op_gn_relu_causal3_tm(const void* x, int b, int t, int t0, int c, int groups, const float* gamma, const float* beta, float eps,
                              void* out, int et, void* stream) {
    const Op op{"r50_op_gn_relu_causal3_tm"};
    if (int rc = op.aligned({{x, "x", 2}, {out, "out", 2}})) return rc;
    if (!x || !gamma || !beta || !out || b < 1 || t < 1 || t0 < 0 || t0 >= t || c < 1 || groups < 1 || c % groups ||
        (et != 0 && et != 1) || (int64_t)b * groups > INT32_MAX || (int64_t)t * (c / groups) > INT32_MAX)
        return op.refuse("invalid arguments (need 0 <= t0 < t, c % groups == 0)");
    R50_ET_LAUNCH(et, gn_relu_causal3_tm_kernel, dim3((unsigned)(b * groups)), dim3(256), 0, stream, (const unsigned short*)x, gamma, beta,
                  (unsigned short*)out, b, t, t0, c, groups, eps);
    return op.done();
}

// ---- ColorJitter variant (kernels.h: cj_*_kernel) ----
int r50_op_color_jitter_u8(const void* frames_u8, int t, int hw, const int* order4, float brightness, float contrast, float saturation,
                           float hue, int normalize, float* out_f32, float* scratch_means, void* stream) {
    const Op op{"r50_op_color_jitter_u8"};
    if (!frames_u8 || !order4 || !out_f32 || !scratch_means || t < 1 || hw < 1) return op.refuse("invalid arguments");
    int seen = 0;
    for (int i = 0; i < 4; ++i) {
        if (order4[i] < 0 || order4[i] > 3) return op.refuse("order entries must be 0..3");
        seen |= 1 << order4[i];
    }
    if (seen != 15) return op.refuse("order must be a permutation of 0..3");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)t * 3 * hw;
    const unsigned grid = ew_grid(n);
    hipLaunchKernelGGL(cj_from_u8_kernel, dim3(grid), dim3(256), 0, s, (const unsigned char*)frames_u8, out_f32, n);
    const float factor[4] = {brightness, contrast, saturation, hue};
    for (int i = 0; i < 4; ++i) {
        const int op = order4[i];
        if (op == 3 && hue == 0.0f) continue;                       // adjust_hue returns its input for a zero factor
        if (op == 1) hipLaunchKernelGGL(cj_gray_mean_kernel, dim3(t), dim3(1024), 0, s, out_f32, hw, scratch_means);
        hipLaunchKernelGGL(cj_apply_kernel, dim3(grid), dim3(256), 0, s, out_f32, t, hw, op, factor[op], scratch_means);
    }
    if (normalize)
        hipLaunchKernelGGL(cj_normalize_kernel, dim3(grid), dim3(256), 0, s, out_f32, (long long)t * 3, hw, 0.485f, 0.456f, 0.406f, 0.229f,
                           0.224f, 0.225f);
    return op.done();
}

// ---- lifting head, backward + optimizer (kernels.h, "Lifting head, backward + optimizer") ----
int r50_op_transpose16(const void* src, int rows, int cols, void* dst, int ld, void* stream) {
    const Op op{"r50_op_transpose16"};
    if (int rc = op.aligned({{src, "src", 2}, {dst, "dst", 2}})) return rc;
    if (!src || !dst || rows < 1 || cols < 1 || ld < rows) return op.refuse("invalid arguments");
    hipLaunchKernelGGL(transpose16_kernel, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)src, (unsigned short*)dst, rows, cols, ld);
    return op.done();
}

int r50_op_mask_scale(void* x, const void* mask_u8, float scale, int64_t n, int et, void* stream) {
    const Op op{"r50_op_mask_scale"};
    if (int rc = op.aligned({{x, "x", 2}})) return rc;
    if (!x || !mask_u8 || n < 1 || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, mask_scale_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, (unsigned short*)x, (const unsigned char*)mask_u8, scale, (long long)n);
    return op.done();
}

int r50_op_relu_bwd(void* dy, const void* act, float scale, int64_t n, int et, void* stream) {
    const Op op{"r50_op_relu_bwd"};
    if (int rc = op.aligned({{dy, "dy", 2}, {act, "act", 2}})) return rc;
    if (!dy || !act || n < 1 || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, relu_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, (unsigned short*)dy, (const unsigned short*)act, scale, (long long)n);
    return op.done();
}

int r50_op_colsum(const void* x, int64_t rows, int cols, int ld, float scale, float* out, int accumulate, int et, void* stream) {
    const Op op{"r50_op_colsum"};
    if (int rc = op.aligned({{x, "x", 2}})) return rc;
    if (!x || !out || rows < 1 || cols < 1 || ld < cols || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, colsum_kernel, dim3((cols + 63) / 64), dim3(1024), 0, stream, (const unsigned short*)x, (long long)rows, cols, ld, scale, out,
                  accumulate);
    return op.done();
}

int r50_op_colsum_split(const void* x, int64_t rows, int cols, int ld, float scale, float* part, float* out, int accumulate, int et,
                        void* stream) {
    const Op op{"r50_op_colsum_split"};
    if (int rc = op.aligned({{x, "x", 2}})) return rc;
    if (!x || !part || !out || rows < 1 || cols < 1 || ld < cols || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, colsum_chain_kernel, dim3((cols + 63) / 64, 16), dim3(64), 0, stream, (const unsigned short*)x, (long long)rows, cols, ld, part);
    hipLaunchKernelGGL(colsum_chain_sum_kernel, dim3((cols + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, cols, scale, out, accumulate);
    return op.done();
}

int r50_op_colsum_f32(const float* x, int64_t rows, int cols, float scale, float* out, int accumulate, void* stream) {
    const Op op{"r50_op_colsum_f32"};
    if (!x || !out || rows < 1 || cols < 1) return op.refuse("invalid arguments");
    hipLaunchKernelGGL(colsum_f32_kernel, dim3((cols + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, (long long)rows, cols, scale, out, accumulate);
    return op.done();
}

int r50_op_grad_accum(const void* src, float scale, float* dst, int64_t n, int accumulate, int et, void* stream) {
    const Op op{"r50_op_grad_accum"};
    if (int rc = op.aligned({{src, "src", 2}})) return rc;
    if (!src || !dst || n < 1 || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, grad_accum_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, (const unsigned short*)src, scale, dst, (long long)n, accumulate);
    return op.done();
}

int r50_op_mse_loss_grad(const float* y, const float* gt, int64_t n, float loss_scale, float* dy, float* loss2, void* stream) {
    const Op op{"r50_op_mse_loss_grad"};
    if (!y || !gt || !dy || !loss2 || n < 3 || n % 3) return op.refuse("invalid arguments");
    hipLaunchKernelGGL(mse_loss_grad_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, y, gt, (long long)n, loss_scale, dy, loss2);
    return op.done();
}

int r50_op_pose_metrics(const float* pred, const float* gt, int64_t rows, int joints, double* acc, void* stream) {
    const Op op{"r50_op_pose_metrics"};
    if (!pred || !gt || !acc || rows < 1 || joints < 1 || rows > INT64_MAX / 3 / joints) return op.refuse("invalid arguments");
    hipLaunchKernelGGL(pose_metrics_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, pred, gt, (long long)(rows * joints), acc);
    return op.done();
}

int r50_op_horizon_metrics(const float* pred, const float* gt, int b, int p, int t_gt, int i0, int joints, double* acc, void* stream) {
    const Op op{"r50_op_horizon_metrics"};
    if (!pred || !gt || !acc || b < 1 || p < 1 || joints < 1 || i0 < 0 || t_gt < 1 || (int64_t)i0 + p > t_gt ||
        (int64_t)b * joints > INT32_MAX || (int64_t)b * t_gt * joints > INT64_MAX / 3)
        return op.refuse("invalid arguments (need b, p, joints >= 1 and 0 <= i0, i0 + p <= t_gt)");
    hipLaunchKernelGGL(horizon_metrics_kernel, dim3((unsigned)p), dim3(256), 0, (hipStream_t)stream, pred, gt, b, p, t_gt, i0, joints, acc);
    return op.done();
}

int r50_op_pose_protocols(const float* pred, const float* gt, const int* group, int b, int p, int t_gt, int i0, int joints, int root,
                          int n_groups, double* acc, void* stream) {
    const Op op{"r50_op_pose_protocols"};
    if (!pred || !gt || !group || !acc) return op.refuse("null pointer");
    if (b < 1 || p < 1 || n_groups < 1 || joints < 1 || joints > 64 || root < 0 || root >= joints || i0 < 0 || (int64_t)i0 + p > t_gt ||
        (int64_t)p * n_groups > INT32_MAX || (int64_t)b * t_gt > INT32_MAX)
        return op.refuse("invalid arguments (need b, p, n_groups >= 1, 1 <= joints <= 64, 0 <= root < joints and 0 <= i0, i0 + p <= t_gt)");
    hipLaunchKernelGGL(pose_protocols_kernel, dim3((unsigned)(p * n_groups)), dim3(256), 0, (hipStream_t)stream, pred, gt, group, b, p,
                       t_gt, i0, joints, root, n_groups, acc);
    return op.done();
}

int r50_op_pose_detail_metrics(const float* pred, const float* gt, const int* group, int b, int p, int t_gt, int i0, int joints, int root,
                               int n_groups, int n_thr, double thr_max, double* acc, void* stream) {
    const Op op{"r50_op_pose_detail_metrics"};
    if (!pred || !gt || !group || !acc) return op.refuse("null pointer");
    if (b < 1 || p < 1 || n_groups < 1 || joints < 1 || joints > 64 || root < 0 || root >= joints || i0 < 0 || (int64_t)i0 + p > t_gt ||
        (int64_t)p * n_groups > INT32_MAX || (int64_t)b * t_gt > INT32_MAX)
        return op.refuse("invalid arguments (need b, p, n_groups >= 1, 1 <= joints <= 64, 0 <= root < joints and 0 <= i0, i0 + p <= t_gt)");
    if (n_thr < 2 || n_thr > POSE_DETAIL_MAX_THR || !std::isfinite(thr_max) || !(thr_max > 0.0))
        return op.refuse("invalid arguments (need 2 <= n_thr <= 1024 and a finite thr_max > 0)");
    hipLaunchKernelGGL(pose_detail_metrics_kernel, dim3((unsigned)(p * n_groups)), dim3(256), 0, (hipStream_t)stream, pred, gt, group, b, p,
                       t_gt, i0, joints, root, n_groups, n_thr, thr_max, acc);
    return op.done();
}

int r50_op_dtw_protocols(const float* pred, const float* gt, const int* group, int b, int p, int t_gt, int i0, int q, int joints, int root,
                         int band, int n_groups, double* clip_out, int* path_out, double* acc, void* stream) {
    const Op op{"r50_op_dtw_protocols"};
    if (!pred || !gt || !group || !clip_out || !acc) return op.refuse("null pointer");
    if (b < 1 || p < 1 || p > DTW_MAX_LEN || q < 1 || q > DTW_MAX_LEN || n_groups < 1 || joints < 1 || joints > 64 || root < 0 ||
        root >= joints || i0 < 0 || (int64_t)i0 + q > t_gt || (int64_t)b * t_gt > INT32_MAX)
        return op.refuse("invalid arguments (need b, n_groups >= 1, 1 <= p, q <= 64, 1 <= joints <= 64, 0 <= root < joints and "
                         "0 <= i0, i0 + q <= t_gt)");
    if (band >= 0 && band < (p > q ? p - q : q - p)) return op.refuse("invalid arguments (a band >= 0 must be >= |p - q|)");
    const size_t lds = dtw_lds_bytes(p, q);
    if (lds > 65536) {
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dtw_align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return op.done(e);
    }
    hipLaunchKernelGGL(dtw_align_kernel, dim3((unsigned)b), dim3(256), lds, (hipStream_t)stream, pred, gt, p, t_gt, i0, q, joints, root, band,
                       clip_out, path_out);
    hipLaunchKernelGGL(dtw_group_sums_kernel, dim3((unsigned)n_groups), dim3(256), 0, (hipStream_t)stream, clip_out, group, b, p, n_groups,
                       acc);
    return op.done();
}

int r50_op_stitch_poses(const float* pred, const float* gt, int64_t rows, int joints, const int* offsets, const int* src, int frames, int t,
                        int mode, int ramp, float* fused, float* gt_out, float* spread, float* gt_gap, void* stream) {
    const Op op{"r50_op_stitch_poses"};
    if (!pred || !gt || !offsets || !src || !fused || !gt_out || !spread || !gt_gap) return op.refuse("null pointer");
    if (rows < 1 || rows > INT32_MAX || joints < 1 || joints > 64 || frames < 1 || t < 1 || rows % t != 0 || mode < 0 || mode > 2 || ramp < 1)
        return op.refuse("invalid arguments (need 1 <= rows < 2^31 a multiple of t >= 1, 1 <= joints <= 64, frames >= 1, mode in {0,1,2} and "
                         "ramp >= 1)");
    hipLaunchKernelGGL(stitch_poses_kernel, dim3((unsigned)((frames + STITCH_WAVES - 1) / STITCH_WAVES)), dim3(64 * STITCH_WAVES), 0,
                       (hipStream_t)stream, pred, gt, offsets, src, frames, joints, t, mode, ramp, fused, gt_out, spread, gt_gap);
    return op.done();
}

int r50_op_gather_window_rows(const float* src, int64_t src_rows, int c, const int* starts, int b, int t, void* dst, int et, void* stream) {
    const Op op{"r50_op_gather_window_rows"};
    if (!src || !starts || !dst) return op.refuse("null pointer");
    if (b < 1 || t < 1 || c < 8 || c % 8 != 0 || src_rows < t || src_rows > INT32_MAX || (et != 0 && et != 1) ||
        (long long)b * t > INT32_MAX / (c / 8))
        return op.refuse("invalid arguments (need b >= 1, 1 <= t <= src_rows < 2^31, c a positive multiple of 8, b * t * c / 8 < 2^31, et in {0,1})");
    if (int rc = op.aligned({{src, "src_f32", 16}, {dst, "dst", 16}})) return rc;
    const long long items = (long long)b * t * (c / 8);
    R50_ET_LAUNCH(et, gather_window_rows_kernel, dim3(ew_grid(items)), dim3(256), 0, stream, src, starts, (unsigned short*)dst, (unsigned)items,
                  (unsigned)t, (unsigned)(c / 8));
    return op.done();
}

int r50_op_merge_mirrored_poses(const float* a, const float* b_mirrored, int64_t rows, int joints, const int* perm, float* out,
                                void* stream) {
    const Op op{"r50_op_merge_mirrored_poses"};
    if (!a || !b_mirrored || !perm || !out) return op.refuse("null pointer");
    if (rows < 1 || joints < 1 || joints > 64 || rows > INT64_MAX / (3 * 64))
        return op.refuse("invalid arguments (need rows >= 1 and 1 <= joints <= 64)");
    const long long bytes = (long long)rows * joints * 3 * (long long)sizeof(float);
    const char *o0 = (const char*)out, *b0 = (const char*)b_mirrored, *a0 = (const char*)a;
    if ((o0 < b0 + bytes && b0 < o0 + bytes) || (o0 != a0 && o0 < a0 + bytes && a0 < o0 + bytes))
        return op.refuse("out overlaps an input (it may be exactly a, nothing else)");
    hipLaunchKernelGGL(merge_mirrored_poses_kernel, dim3(ew_grid((long long)rows * joints * 3)), dim3(256), 0, (hipStream_t)stream, a,
                       b_mirrored, perm, out, (long long)rows, joints);
    return op.done();
}

int r50_op_sequence_metrics(const float* fused, const float* gt, const float* spread, const int* offsets, const int* seq, const int* idx,
                            const int* group, int frames, int joints, int root, int n_groups, double* part, int n_blocks, void* stream) {
    const Op op{"r50_op_sequence_metrics"};
    if (!fused || !gt || !spread || !offsets || !seq || !idx || !group || !part) return op.refuse("null pointer");
    if (frames < 1 || joints < 1 || joints > 64 || root < 0 || root >= joints || n_groups < 1 || n_blocks < 1 ||
        (int64_t)n_blocks * n_groups > INT32_MAX / 8)
        return op.refuse("invalid arguments (need frames, n_groups, n_blocks >= 1, 1 <= joints <= 64 and 0 <= root < joints)");
    hipLaunchKernelGGL(sequence_metrics_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, fused, gt, spread, offsets, seq,
                       idx, group, frames, joints, root, n_groups, part);
    return op.done();
}

int r50_op_future_pose_loss_grad(const float* y_hat, const float* gt, int b, int t, int joints, float loss_scale, float* dy, float* loss2,
                                 void* stream) {
    const Op op{"r50_op_future_pose_loss_grad"};
    if (!y_hat || !gt || !dy || !loss2 || b < 1 || t < 2 || joints < 1 || (int64_t)b * t > INT64_MAX / 3 / joints)
        return op.refuse("invalid arguments (null pointer, b < 1, t < 2 or joints < 1)");
    hipLaunchKernelGGL(future_pose_loss_grad_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, y_hat, gt, (long long)b * t, t, joints,
                       loss_scale, dy, loss2);
    return op.done();
}

int r50_op_joint_pose_loss_grad(const float* y, const float* gt, int b, int t, int joints, float lambda_future, float loss_scale, float* dy,
                                float* out4, void* stream) {
    const Op op{"r50_op_joint_pose_loss_grad"};
    if (!y || !gt || !dy || !out4) return op.refuse("null pointer");
    if (b < 1 || t < 2 || joints < 1 || joints > 64 || (int64_t)b * t > INT32_MAX)
        return op.refuse("invalid arguments (need b >= 1, t >= 2 and 1 <= joints <= 64)");
    hipLaunchKernelGGL(joint_pose_loss_grad_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, y, gt, (long long)b * t, t, joints,
                       loss_scale, loss_scale * lambda_future, dy, out4);
    return op.done();
}

int r50_op_geo_pose_loss_grad(const float* y, const float* gt3d, const float* gt2d, const float* K, int b, int t, int s0, int joints,
                              const int* edges_host, int n_edges, float lambda_2d, float lambda_vel, float lambda_bone, float eps,
                              float term_scale, float loss_scale, float* dy, double* part, float* out8, void* stream) {
    const Op op{"r50_op_geo_pose_loss_grad"};
    if (!y || !gt3d || !gt2d || !K || !part || !out8) return op.refuse("null pointer (y, gt3d, gt2d, K, part and out8 are required; only dy may be NULL)");
    if (b < 1) return op.refuse("need b >= 1");
    if (s0 < 0 || s0 > 1) return op.refuse("need 0 <= s0 <= 1");
    if (t < 1 || t - s0 < 1) return op.refuse("need t - s0 >= 1");
    if (joints < 1 || joints > 64) return op.refuse("need 1 <= joints <= 64");
    if (n_edges < 0 || n_edges > GEO_MAX_EDGES) return op.refuse("need 0 <= n_edges <= 64");
    if (n_edges > 0 && !edges_host) return op.refuse("null pointer (edges_host with n_edges > 0)");
    if (!std::isfinite(lambda_2d) || !std::isfinite(lambda_vel) || !std::isfinite(lambda_bone) || lambda_2d < 0.f || lambda_vel < 0.f ||
        lambda_bone < 0.f)
        return op.refuse("the lambdas must be finite and >= 0");
    if (!(eps > 0.f) || !std::isfinite(eps)) return op.refuse("need eps > 0");
    if (lambda_vel != 0.f && t - s0 < 2) return op.refuse("need t - s0 >= 2 when lambda_vel != 0");
    if ((int64_t)t * joints > GEO_MAX_TJ) return op.refuse("t * joints exceeds 4608, the most one workgroup stages in LDS (T 256 at J 17 fits)");
    if ((int64_t)b * t * joints > INT32_MAX / 3) return op.refuse("b * t * joints * 3 exceeds the int range");
    GeoEdges ed;
    for (int q = 0; q < GEO_MAX_EDGES; ++q) ed.ab[q] = 0;
    for (int q = 0; q < n_edges; ++q) {
        const int ea = edges_host[2 * q], eb = edges_host[2 * q + 1];
        if (ea < 0 || ea >= joints || eb < 0 || eb >= joints) return op.refuse("every edge index must be in [0, joints)");
        ed.ab[q] = ea | (eb << 8);
    }
    const double nj = (double)b * (t - s0) * joints, nvj = (double)b * (t - s0 - 1) * joints, nb = (double)b * (t - s0) * n_edges;
    const float c2 = (float)(2.0 * (double)lambda_2d / (2.0 * nj));
    const float cv = nvj > 0.0 ? (float)(2.0 * (double)lambda_vel / (3.0 * nvj)) : 0.f;
    const float cb = nb > 0.0 ? (float)(2.0 * (double)lambda_bone / nb) : 0.f;
    const size_t lds = (size_t)t * joints * 24;
    static std::atomic<unsigned long long> lds_set{0};      // the kernel's dynamic-LDS ceiling is raised once per device, not per call
    int dev = 0;
    hipError_t ea = hipGetDevice(&dev);
    if (ea != hipSuccess) return op.done(ea);
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (!bit || !(lds_set.load() & bit)) {
        ea = hipFuncSetAttribute(reinterpret_cast<const void*>(geo_pose_loss_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 GEO_MAX_TJ * 24);
        if (ea != hipSuccess) return op.done(ea);
        lds_set.fetch_or(bit);
    }
    hipLaunchKernelGGL(geo_pose_loss_grad_kernel, dim3((unsigned)b), dim3(256), lds, (hipStream_t)stream, y, gt3d, gt2d, K, t, s0, joints, ed,
                       n_edges, (int)(lambda_2d != 0.f), (int)(lambda_vel != 0.f && nvj > 0.0), (int)(lambda_bone != 0.f && nb > 0.0),
                       (float)(3ll * (long long)nj), loss_scale * term_scale, c2, cv, cb, eps, dy, part);
    hipLaunchKernelGGL(geo_pose_sum_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, (const double*)part, b, nj, nvj, nb, lambda_2d,
                       lambda_vel, lambda_bone, out8);
    return op.done();
}

int r50_op_ar_latent_grad(const void* ar, const void* phi, const float* dphi_hat, int b, int t, int d, float lambda, float loss_scale,
                          void* dar, float* loss_lat, float* row_part, int et, void* stream) {
    const Op op{"r50_op_ar_latent_grad"};
    if (!ar || !phi || !dphi_hat || !dar || !loss_lat || !row_part) return op.refuse("null pointer");
    if (b < 1 || t < 2 || (int64_t)b * t > INT32_MAX) return op.refuse("need b >= 1, t >= 2 (b*t within int range)");
    if (d < 8 || d % 8) return op.refuse("d must be a positive multiple of 8");
    if (et != 0 && et != 1) return op.refuse("et must be 0 (bf16) or 1 (fp16)");
    if (int rc = op.aligned({{ar, "ar", 16}, {phi, "phi", 16}, {dphi_hat, "dphi_hat", 16}, {dar, "dar", 16}})) return rc;
    const long long rows = (long long)b * t;
    const double n_l = (double)b * (t - 1) * d;
    const float coef = (float)((double)lambda * 2.0 / n_l * (double)loss_scale);
    R50_ET_LAUNCH(et, ar_latent_grad_kernel, dim3((unsigned)rows), dim3(128), 0, stream, (const unsigned short*)ar, (const unsigned short*)phi,
                  dphi_hat, t, d, coef, (unsigned short*)dar, row_part);
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_part, rows, 1.0 / n_l, loss_lat);
    return op.done();
}

int r50_op_hal_latent_grad(const void* h, const void* phi, const float* dh_reg, int64_t rows, int d, float lambda, float loss_scale,
                           void* dh, float* loss_lat, float* row_part, int et, void* stream) {
    const Op op{"r50_op_hal_latent_grad"};
    if (!h || !phi || !dh_reg || !dh || !loss_lat || !row_part) return op.refuse("null pointer");
    if (rows < 1 || rows > INT32_MAX) return op.refuse("need 1 <= rows (within int range)");
    if (d < 8 || d % 8) return op.refuse("d must be a positive multiple of 8");
    if (et != 0 && et != 1) return op.refuse("et must be 0 (bf16) or 1 (fp16)");
    if (int rc = op.aligned({{h, "h", 16}, {phi, "phi", 16}, {dh_reg, "dh_reg", 16}, {dh, "dh", 16}})) return rc;
    const double n_l = (double)rows * d;
    const float coef = (float)((double)lambda * 2.0 / n_l * (double)loss_scale);
    R50_ET_LAUNCH(et, hal_latent_grad_kernel, dim3((unsigned)rows), dim3(128), 0, stream, (const unsigned short*)h, (const unsigned short*)phi,
                  dh_reg, d, coef, (unsigned short*)dh, row_part);
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_part, (long long)rows, 1.0 / n_l, loss_lat);
    return op.done();
}

// ---- temporal smoothing and constant bone lengths (include/r50_smooth.h, smooth_kernels.h) ----
static bool overlaps(const void* a, const void* b, long long bytes) {
    const char *a0 = (const char*)a, *b0 = (const char*)b;
    return a0 < b0 + bytes && b0 < a0 + bytes;
}
static const long long kSmoothMaxRows = INT32_MAX / (3 * SMOOTH_MAX_J);

// The edge list of the bone ops, checked: on success `ed` and `is_child` are filled, else the reason is returned.
static const char* check_bone_edges(const int* edges, int E, int J, BoneEdges& ed, unsigned long long& is_child) {
    if (E < 1 || E > J - 1) return "need 1 <= E <= J - 1";
    is_child = 0;
    for (int q = 0; q < SMOOTH_MAX_J; ++q) ed.parent[q] = ed.child[q] = 0;
    for (int q = 0; q < E; ++q) {
        const int pa = edges[2 * q], ch = edges[2 * q + 1];
        if (pa < 0 || pa >= J || ch < 0 || ch >= J) return "every edge index must be in [0, J)";
        if (pa == ch) return "an edge needs two different joints";
        if ((is_child >> ch) & 1ull) return "a joint may be the child of one edge only";
        is_child |= 1ull << ch;
        ed.parent[q] = (unsigned char)pa;
        ed.child[q] = (unsigned char)ch;
    }
    unsigned long long placed = 0;
    for (int q = 0; q < E; ++q) {
        const int pa = ed.parent[q];
        if (((is_child >> pa) & 1ull) && !((placed >> pa) & 1ull)) return "every edge must come after the edge that places its parent";
        placed |= 1ull << ed.child[q];
    }
    return nullptr;
}

int r50_op_fir_sequences(const float* x, const int* seg_start, const int* row_seg, int64_t F, int G, int J, const double* coef, int W,
                         float* out, int* short_rows, void* stream) {
    const Op op{"r50_op_fir_sequences"};
    if (!x || !seg_start || !row_seg || !coef || !out || !short_rows) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || G < 1 || G > F || J < 1 || J > SMOOTH_MAX_J)
        return op.refuse("invalid arguments (need 1 <= G <= F < 2^31 / 192 and 1 <= J <= 64)");
    if (W < 1 || W > SMOOTH_MAX_W || W % 2 == 0) return op.refuse("W must be odd and in [1, 63]");
    if (overlaps(x, out, F * 3 * J * (long long)sizeof(float))) return op.refuse("out overlaps x");
    hipLaunchKernelGGL(fir_sequences_kernel, dim3((unsigned)((F + FIR_ROWS - 1) / FIR_ROWS)), dim3(256), 0, (hipStream_t)stream, x, seg_start,
                       row_seg, (int)F, G, 3 * J, coef, W, out, short_rows);
    return op.done();
}

int r50_op_one_euro_sequences(const float* x, const int* seg_start, int64_t F, int G, int J, double rate, double min_cutoff, double beta,
                              double d_cutoff, float* out, void* stream) {
    const Op op{"r50_op_one_euro_sequences"};
    if (!x || !seg_start || !out) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || G < 1 || G > F || J < 1 || J > SMOOTH_MAX_J)
        return op.refuse("invalid arguments (need 1 <= G <= F < 2^31 / 192 and 1 <= J <= 64)");
    if (!(rate > 0.0 && min_cutoff > 0.0 && d_cutoff > 0.0 && beta >= 0.0) || !std::isfinite(rate) || !std::isfinite(min_cutoff) ||
        !std::isfinite(d_cutoff) || !std::isfinite(beta))
        return op.refuse("need finite rate, min_cutoff, d_cutoff > 0 and beta >= 0");
    if (overlaps(x, out, F * 3 * J * (long long)sizeof(float))) return op.refuse("out overlaps x");
    const int slabs = (3 * J + 63) / 64;
    hipLaunchKernelGGL(one_euro_sequences_kernel, dim3((unsigned)(((long long)G * slabs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x,
                       seg_start, G, 3 * J, slabs, rate, min_cutoff, beta, d_cutoff, out);
    return op.done();
}

int r50_op_bone_stats(const float* x, const int* seq_start, int64_t F, int S, int J, const int* edges, int E, double* stats, void* stream) {
    const Op op{"r50_op_bone_stats"};
    if (!x || !seq_start || !edges || !stats) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || S < 1 || S > F || J < 2 || J > SMOOTH_MAX_J)
        return op.refuse("invalid arguments (need 1 <= S <= F < 2^31 / 192 and 2 <= J <= 64)");
    BoneEdges ed;
    unsigned long long is_child;
    if (const char* why = check_bone_edges(edges, E, J, ed, is_child)) return op.refuse(std::string("edges: ") + why);
    hipLaunchKernelGGL(bone_stats_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, x, seq_start, 3 * J, ed, E, stats);
    return op.done();
}

int r50_op_bone_rebuild(const float* x, const int* row_seq, int64_t F, int S, int J, const int* edges, int E, const double* stats, float* out,
                        void* stream) {
    const Op op{"r50_op_bone_rebuild"};
    if (!x || !row_seq || !edges || !stats || !out) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || S < 1 || S > F || J < 2 || J > SMOOTH_MAX_J)
        return op.refuse("invalid arguments (need 1 <= S <= F < 2^31 / 192 and 2 <= J <= 64)");
    BoneEdges ed;
    unsigned long long is_child;
    if (const char* why = check_bone_edges(edges, E, J, ed, is_child)) return op.refuse(std::string("edges: ") + why);
    if (overlaps(x, out, F * 3 * J * (long long)sizeof(float))) return op.refuse("out overlaps x");
    const int rb = bone_rebuild_rows(J);
    hipLaunchKernelGGL(bone_rebuild_kernel, dim3((unsigned)((F + rb - 1) / rb)), dim3(64), bone_rebuild_lds(J), (hipStream_t)stream, x, row_seq,
                       (int)F, J, ed, E, is_child, stats, out);
    return op.done();
}

// ---- joint rotations on a rigid skeleton (include/r50_kinematics.h, kinematics_kernels.h) ----
// The host skeleton tables, checked: on success `sk` is filled, else the reason is returned.
static const char* check_kin_skeleton(int J, const int* edges, int E, const int* frames, int NF, const double* rest_dirs, const double* sign,
                                      KinSkeleton& sk) {
    if (E != J - 1) return "edges: need E == J - 1 (one root)";
    if (NF < 0 || NF > J) return "frames: need 0 <= NF <= J";
    std::memset(&sk, 0, sizeof(sk));
    unsigned long long is_child = 0;
    if (E > 0) {
        BoneEdges ed;
        if (const char* why = check_bone_edges(edges, E, J, ed, is_child)) return why;
        for (int q = 0; q < E; ++q) sk.parent[q] = ed.parent[q], sk.child[q] = ed.child[q];
    }
    int children[KIN_MAX_J] = {0};
    sk.root = -1;
    for (int j = 0; j < J; ++j) {
        sk.par_of[j] = 255;
        if (!((is_child >> j) & 1ull)) sk.root = j;                                 // E == J - 1 distinct children: exactly one
    }
    for (int q = 0; q < E; ++q) {
        sk.par_of[sk.child[q]] = sk.parent[q];
        if (++children[sk.parent[q]] == 1) sk.arg[sk.parent[q]] = sk.child[q];
    }
    for (int j = 0; j < J; ++j) sk.kind[j] = children[j] == 1 ? KIN_AIM : KIN_INHERIT;
    unsigned long long framed = 0;
    for (int q = 0; q < NF; ++q) {
        const int* f = frames + 5 * q;
        for (int k = 0; k < 5; ++k)
            if (f[k] < 0 || f[k] >= J) return "frames: every index must be in [0, J)";
        if (f[1] == f[2] || f[3] == f[4]) return "frames: a0 != a1 and b0 != b1 are needed";
        if ((framed >> f[0]) & 1ull) return "frames: a joint may be framed once only";
        framed |= 1ull << f[0];
        sk.kind[f[0]] = KIN_FRAMED;
        sk.arg[f[0]] = (unsigned char)q;
        for (int k = 0; k < 4; ++k) sk.fr[q][k] = (unsigned char)f[1 + k];
    }
    for (int k = 0; k < 3; ++k) {
        if (!(sign[k] == 1.0 || sign[k] == -1.0)) return "sign: every entry must be +1 or -1";
        sk.sign[k] = sign[k];
    }
    if (sign[0] * sign[1] * sign[2] != 1.0) return "sign: the product must be +1";
    for (int j = 0; j < J; ++j) {
        if (j == sk.root) continue;
        const double* v = rest_dirs + 3 * j;
        const double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        if (!(std::fabs(n2 - 1.0) <= 1e-12)) return "rest_dirs: a unit vector is needed for every joint but the root";
        for (int k = 0; k < 3; ++k) sk.dirs[j][k] = v[k];
    }
    return nullptr;
}

struct KinRange { const void* p; long long bytes; };
static bool kin_any_overlap(const KinRange* in, int n_in, const KinRange* out, int n_out) {
    for (int o = 0; o < n_out; ++o) {
        const char* o0 = (const char*)out[o].p;
        for (int i = 0; i < n_in + o; ++i) {                                       // every input, and every earlier output
            const KinRange& r = i < n_in ? in[i] : out[i - n_in];
            const char* r0 = (const char*)r.p;
            if (o0 < r0 + r.bytes && r0 < o0 + out[o].bytes) return true;
        }
    }
    return false;
}

int r50_op_rest_offsets(const float* x, const int* seq_start, int64_t F, int S, int J, const int* edges, int E, const int* frames, int NF,
                        const double* rest_dirs, const double* sign, double* rest, void* stream) {
    const Op op{"r50_op_rest_offsets"};
    if (!x || !seq_start || !rest_dirs || !sign || !rest || (!edges && E > 0) || (!frames && NF > 0)) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || S < 1 || S > F || J < 1 || J > KIN_MAX_J)
        return op.refuse("invalid arguments (need 1 <= S <= F < 2^31 / 192 and 1 <= J <= 64)");
    KinSkeleton sk;
    if (const char* why = check_kin_skeleton(J, edges, E, frames, NF, rest_dirs, sign, sk)) return op.refuse(std::string("") + why);
    const KinRange in[2] = {{x, F * 3 * J * (long long)sizeof(float)}, {seq_start, ((long long)S + 1) * (long long)sizeof(int)}};
    const KinRange out[1] = {{rest, (long long)S * 3 * J * (long long)sizeof(double)}};
    if (kin_any_overlap(in, 2, out, 1)) return op.refuse("rest overlaps an input");
    hipLaunchKernelGGL(rest_offsets_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, x, seq_start, J, sk, rest);
    return op.done();
}

int r50_op_pose_rotations(const float* x, const int* row_seq, int64_t F, int S, int J, const int* edges, int E, const int* frames, int NF,
                          const double* rest_dirs, const double* sign, const double* rest, float* quat, float* euler, float* rigid,
                          float* resid, int* flags, void* stream) {
    const Op op{"r50_op_pose_rotations"};
    if (!x || !row_seq || !rest_dirs || !sign || !rest || !quat || !euler || !rigid || !resid || !flags || (!edges && E > 0) ||
        (!frames && NF > 0))
        return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || S < 1 || S > F || J < 1 || J > KIN_MAX_J)
        return op.refuse("invalid arguments (need 1 <= S <= F < 2^31 / 192 and 1 <= J <= 64)");
    KinSkeleton sk;
    if (const char* why = check_kin_skeleton(J, edges, E, frames, NF, rest_dirs, sign, sk)) return op.refuse(std::string("") + why);
    if (int rc = op.aligned({{quat, "quat", 16}})) return rc;
    const long long fj = F * J * (long long)sizeof(float);
    const KinRange in[3] = {{x, 3 * fj}, {row_seq, F * (long long)sizeof(int)}, {rest, (long long)S * 3 * J * (long long)sizeof(double)}};
    const KinRange out[5] = {{quat, 4 * fj}, {euler, 3 * fj}, {rigid, 3 * fj}, {resid, F * (long long)sizeof(float)},
                             {flags, F * (long long)sizeof(int)}};
    if (kin_any_overlap(in, 3, out, 5)) return op.refuse("an output overlaps an input or another output");
    const size_t lds = pose_rot_lds(J);
    if (lds > 65536) return op.refuse("the LDS budget does not hold");
    const int rb = pose_rot_rows(J);
    hipLaunchKernelGGL(pose_rotations_kernel, dim3((unsigned)((F + rb - 1) / rb)), dim3(64), lds, (hipStream_t)stream, x, row_seq, (int)F, J,
                       sk, rest, quat, euler, rigid, resid, flags);
    return op.done();
}

// ---- a pose at any time stamp (include/r50_resample.h, resample_kernels.h, INTEGRATION.md section AB) ----
int r50_op_resample_sequences(const float* x, const int* idx, const int* seq_start, int64_t F, int S, int J, const double* out_time,
                              const int* out_seq, const int* out_left, int64_t G, int kind, int max_gap, float* y, int* flags,
                              void* stream) {
    const Op op{"r50_op_resample_sequences"};
    if (!x || !idx || !seq_start || !out_time || !out_seq || !out_left || !y || !flags) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || G < 1 || G > kSmoothMaxRows || S < 1 || S > F || J < 1 || J > RESAMPLE_MAX_J)
        return op.refuse("invalid arguments (need 1 <= S <= F < 2^31 / 192, 1 <= G < 2^31 / 192 and 1 <= J <= 64)");
    if (kind != R50_RESAMPLE_LINEAR && kind != R50_RESAMPLE_CUBIC) return op.refuse("kind must be 0 (linear) or 1 (cubic)");
    if (max_gap < 1) return op.refuse("max_gap must be >= 1");
    if ((uintptr_t)out_time & 7u) return op.refuse("out_time must be 8-byte aligned");
    const long long row = 3 * J * (long long)sizeof(float), word = (long long)sizeof(int);
    const KinRange in[6] = {{x, F * row}, {idx, F * word}, {seq_start, ((long long)S + 1) * word}, {out_time, G * (long long)sizeof(double)},
                            {out_seq, G * word}, {out_left, G * word}};
    const KinRange out[2] = {{y, G * row}, {flags, G * word}};
    if (kin_any_overlap(in, 6, out, 2)) return op.refuse("y or flags overlaps an input or the other output");
    const long long total = G * 3 * J;
    hipLaunchKernelGGL(resample_sequences_kernel, dim3((unsigned)((total + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK)), dim3(RESAMPLE_BLOCK), 0,
                       (hipStream_t)stream, x, idx, seq_start, 3 * J, out_time, out_seq, out_left, (int)G, kind, max_gap, y, flags);
    return op.done();
}

// ---- stratified cluster bootstrap of per-unit sums (include/r50_bootstrap.h, bootstrap_kernels.h, INTEGRATION.md section AC) ----
int r50_op_bootstrap_sums(const double* v, const int* stratum_start, int64_t U, int G, int M, int64_t r0, int64_t R, uint64_t seed,
                          int window, double* out, int* counts, void* stream) {
    const Op op{"r50_op_bootstrap_sums"};
    if (!v || !stratum_start || !out) return op.refuse("null pointer");
    if (U < 1 || G < 1 || M < 1 || R < 1 || G > U || U > R50_BOOTSTRAP_MAX_UNITS || M > R50_BOOTSTRAP_MAX_COLUMNS)
        return op.refuse("invalid arguments (need 1 <= G <= U <= 2^24, 1 <= M <= 4096 and R >= 1)");
    if (r0 < 0 || r0 > INT64_MAX - R) return op.refuse("need r0 >= 0 and r0 + R within int64");
    const long long limit = 1ll << 40;
    if (R >= limit || R > (limit - 1) / ((long long)G * M) || R > (limit - 1) / U)   // by division: the products may overflow
        return op.refuse("R * G * M and R * U must stay below 2^40");
    if (window < 1 || window > R50_BOOTSTRAP_MAX_WINDOW) return op.refuse("window must lie in [1, 32768]");
    if (((uintptr_t)v & 7u) || ((uintptr_t)out & 7u) || ((uintptr_t)counts & 3u))
        return op.refuse("v and out must be 8-byte aligned (counts 4-byte)");
    const KinRange in[2] = {{v, U * M * (long long)sizeof(double)}, {stratum_start, ((long long)G + 1) * (long long)sizeof(int)}};
    const KinRange outs[2] = {{out, R * G * M * (long long)sizeof(double)}, {counts, R * U * (long long)sizeof(int)}};
    if (kin_any_overlap(in, 2, outs, counts ? 2 : 1)) return op.refuse("out or counts overlaps an input or the other output");
    const long long grid_z = (R + BOOT_GRID_Y - 1) / BOOT_GRID_Y;
    if (grid_z > 65535) return op.refuse("R exceeds the launch grid (65535 * 65535 replicates)");
    const size_t lds = sizeof(int) * (size_t)std::min<long long>(window, U);
    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(bootstrap_sums_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return op.done(ea);
    hipLaunchKernelGGL(bootstrap_sums_kernel, dim3((unsigned)G, (unsigned)std::min<long long>(R, BOOT_GRID_Y), (unsigned)grid_z), dim3(BOOT_BLOCK),
                       lds, (hipStream_t)stream, v, stratum_start, (long long)U, G, M, (long long)r0, (long long)R, (uint32_t)seed,
                       (uint32_t)(seed >> 32), window, out, counts);
    return op.done();
}

// ---- 2D-guided refinement of stitched sequences (include/r50_refine.h, refine_kernels.h) ----
// The optional edge list of the fit ops: E == 0 means no bones (edges is not read); otherwise it is checked as the bone ops check theirs.
static const char* check_fit_edges(const int* edges, int E, int J, BoneEdges& ed) {
    for (int q = 0; q < SMOOTH_MAX_J; ++q) ed.parent[q] = ed.child[q] = 0;
    if (E == 0) return nullptr;
    if (!edges) return "edges is null with E > 0";
    unsigned long long is_child;
    return check_bone_edges(edges, E, J, ed, is_child);
}

int r50_op_pose_fit_sweeps(const float* x0, const float* rays, const float* conf, const int* seg_start, const int* row_seg, const int* row_seq,
                           int64_t F, int G, int S, int J, const int* edges, int E, const double* bone_len, double lambda_2d, double lambda_3d,
                           double lambda_acc, double lambda_bone, double omega, double z_min, int iters, double* workspace, float* out,
                           void* stream) {
    const Op op{"r50_op_pose_fit_sweeps"};
    if (!x0 || !rays || !seg_start || !row_seg || !row_seq || !workspace || !out) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || G < 1 || G > F || S < 1 || S > G || J < 1 || J > FIT_MAX_J)
        return op.refuse("invalid arguments (need 1 <= S <= G <= F < 2^31 / 192 and 1 <= J <= 64)");
    if (!(std::isfinite(lambda_3d) && lambda_3d > 0.0)) return op.refuse("lambda_3d must be finite and > 0 (it keeps H positive definite)");
    if (!(std::isfinite(lambda_2d) && lambda_2d >= 0.0 && std::isfinite(lambda_acc) && lambda_acc >= 0.0 && std::isfinite(lambda_bone) &&
          lambda_bone >= 0.0))
        return op.refuse("lambda_2d, lambda_acc and lambda_bone must be finite and >= 0");
    if (!(omega > 0.0 && omega <= 0.75)) return op.refuse("need 0 < omega <= 0.75");
    if (!(std::isfinite(z_min) && z_min > 0.0)) return op.refuse("z_min must be finite and > 0");
    if (iters < 0 || iters > 1000) return op.refuse("need 0 <= iters <= 1000");
    if (E < 0) return op.refuse("edges: need E >= 0");
    BoneEdges ed;
    if (const char* why = check_fit_edges(edges, E, J, ed)) return op.refuse(std::string("edges: ") + why);
    if (lambda_bone != 0.0 && (E < 1 || !bone_len)) return op.refuse("lambda_bone != 0 needs edges and bone_len");
    const long long fj = F * J * (long long)sizeof(float);
    const KinRange in[4] = {{x0, 3 * fj}, {rays, 2 * fj}, {conf ? (const void*)conf : (const void*)x0, conf ? fj : 0},
                            {bone_len && lambda_bone != 0.0 ? (const void*)bone_len : (const void*)x0,
                             bone_len && lambda_bone != 0.0 ? (long long)S * E * (long long)sizeof(double) : 0}};
    const KinRange outs[2] = {{workspace, 2 * F * 3 * J * (long long)sizeof(double)}, {out, 3 * fj}};
    if (kin_any_overlap(in, 4, outs, 2)) return op.refuse("out or workspace overlaps an input, or each other");
    if (pose_fit_lds(J) > 65536) return op.refuse("the LDS budget does not hold");
    hipStream_t st = (hipStream_t)stream;
    if (iters == 0) {
        return op.done(hipMemcpyAsync(out, x0, (size_t)(3 * fj), hipMemcpyDeviceToDevice, st));
    }
    FitAdjacency adj;
    std::memset(&adj, 0, sizeof(adj));
    int n = 0;
    for (int j = 0; j < J; ++j) {                                                  // per joint, its edges in edge-list order
        adj.start[j] = (unsigned char)n;
        for (int q = 0; q < E; ++q) {
            if (ed.parent[q] != j && ed.child[q] != j) continue;
            adj.edge[n] = (unsigned char)q;
            adj.other[n] = ed.parent[q] == j ? ed.child[q] : ed.parent[q];
            ++n;
        }
    }
    for (int j = J; j <= FIT_MAX_J; ++j) adj.start[j] = (unsigned char)n;
    const FitParams pr = {lambda_2d, lambda_3d, lambda_acc, lambda_bone, omega, z_min};
    double* buf[2] = {workspace, workspace + (size_t)F * 3 * J};
    const int f = (int)F;
    for (int k = 0; k < iters; ++k) {                                              // sweep k reads buf[(k - 1) & 1] and writes buf[k & 1]
        const double* src = k == 0 ? nullptr : buf[(k - 1) & 1];
        double* dst = buf[k & 1];
        const bool lastk = k == iters - 1;
        if (k == 0 && lastk) launch_fit_sweep<true, true>(x0, src, rays, conf, seg_start, row_seg, row_seq, f, J, adj, E, bone_len, pr, dst, out, st);
        else if (k == 0) launch_fit_sweep<true, false>(x0, src, rays, conf, seg_start, row_seg, row_seq, f, J, adj, E, bone_len, pr, dst, out, st);
        else if (lastk) launch_fit_sweep<false, true>(x0, src, rays, conf, seg_start, row_seg, row_seq, f, J, adj, E, bone_len, pr, dst, out, st);
        else launch_fit_sweep<false, false>(x0, src, rays, conf, seg_start, row_seg, row_seq, f, J, adj, E, bone_len, pr, dst, out, st);
    }
    return op.done();
}

int r50_op_pose_fit_energy(const float* x, const float* x0, const float* rays, const float* conf, const int* seq_start, const int* row_seg,
                           int64_t F, int S, int J, const int* edges, int E, const double* bone_len, double z_min, double* energy,
                           void* stream) {
    const Op op{"r50_op_pose_fit_energy"};
    if (!x || !x0 || !rays || !seq_start || !row_seg || !energy) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || S < 1 || S > F || J < 1 || J > FIT_MAX_J)
        return op.refuse("invalid arguments (need 1 <= S <= F < 2^31 / 192 and 1 <= J <= 64)");
    if (!(std::isfinite(z_min) && z_min > 0.0)) return op.refuse("z_min must be finite and > 0");
    if (E < 0) return op.refuse("edges: need E >= 0");
    BoneEdges ed;
    if (const char* why = check_fit_edges(edges, E, J, ed)) return op.refuse(std::string("edges: ") + why);
    if (bone_len && E < 1) return op.refuse("bone_len needs edges");
    const long long fj = F * J * (long long)sizeof(float);
    const KinRange in[2] = {{x, 3 * fj}, {x0, 3 * fj}};
    const KinRange outs[1] = {{energy, (long long)S * FIT_ENERGY_SLOTS * (long long)sizeof(double)}};
    if (kin_any_overlap(in, 2, outs, 1)) return op.refuse("energy overlaps an input");
    hipLaunchKernelGGL(pose_fit_energy_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, x, x0, rays, conf, seq_start, row_seg, J, ed,
                       E, bone_len, z_min, energy);
    return op.done();
}

// ---- the cameras of a take in one frame of reference, fused (include/r50_multiview.h, multiview_kernels.h) ----
int r50_op_view_rigid_fit(const float* y, const float* x, int64_t rows_y, int64_t rows_x, int J, const int* pair_start, const int* match,
                          int P, double* fit, void* stream) {
    const Op op{"r50_op_view_rigid_fit"};
    if (!y || !x || !pair_start || !match || !fit) return op.refuse("null pointer");
    if (rows_y < 1 || rows_y > kSmoothMaxRows || rows_x < 1 || rows_x > kSmoothMaxRows || J < 1 || J > VIEW_MAX_J || P < 1)
        return op.refuse("invalid arguments (need 1 <= rows_y, rows_x < 2^31 / 192, 1 <= J <= 64 and P >= 1)");
    hipLaunchKernelGGL(view_rigid_fit_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, y, x, J, pair_start, match, fit);
    return op.done();
}

int r50_op_view_fuse(const float* pose, int64_t F, int J, const int* peer_start, const int* peer_row, const int* peer_fit, const double* fit,
                     int P, int mode, float* fused, float* disagreement, void* stream) {
    const Op op{"r50_op_view_fuse"};
    if (!pose || !peer_start || !peer_row || !peer_fit || !fit || !fused || !disagreement) return op.refuse("null pointer");
    if (F < 1 || F > kSmoothMaxRows || J < 1 || J > VIEW_MAX_J || P < 0)
        return op.refuse("invalid arguments (need 1 <= F < 2^31 / 192, 1 <= J <= 64 and P >= 0)");
    if (mode < 0 || mode > 2) return op.refuse("mode must be 0 (mean), 1 (median) or 2 (others)");
    if (overlaps(pose, fused, F * 3 * J * (long long)sizeof(float))) return op.refuse("fused overlaps pose");
    hipLaunchKernelGGL(view_fuse_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pose, (int)F, J, peer_start,
                       peer_row, peer_fit, fit, mode, fused, disagreement);
    return op.done();
}

int r50_op_gn_relu_causal3_bwd(const void* dr, const void* x, int b, int t, int c, int groups, const float* gamma, const float* beta,
                               float eps, const void* add, void* dx, float* dgamma_part, float* dbeta_part, int et, void* stream) {
    const Op op{"r50_op_gn_relu_causal3_bwd"};
    if (int rc = op.aligned({{dr, "dr", 2}, {x, "x", 2}, {add, "add", 2}, {dx, "dx", 2}})) return rc;
    if (!dr || !x || !gamma || !beta || !dx || !dgamma_part || !dbeta_part || b < 1 || t < 1 || c < 1 || groups < 1 || c % groups ||
        c / groups > 256 || (et != 0 && et != 1))
        return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, gn_relu_causal3_bwd_kernel, dim3((unsigned)(b * groups)), dim3(256), 0, stream, (const unsigned short*)dr,
                  (const unsigned short*)x, gamma, beta, (const unsigned short*)add, (unsigned short*)dx, dgamma_part, dbeta_part, t, c,
                  groups, eps);
    return op.done();
}

int r50_op_gn_relu_causal3_tm_bwd(const void* dr, const void* x, int b, int t, int t0, int c, int groups, const float* gamma,
                                  const float* beta, float eps, const void* add, void* dx, float* dgamma_part, float* dbeta_part, int et,
                                  void* stream) {
    const Op op{"r50_op_gn_relu_causal3_tm_bwd"};
    if (int rc = op.aligned({{dr, "dr", 2}, {x, "x", 2},
                             {add, "add", 2}, {dx, "dx", 2}}))
        return rc;
    if (!dr || !x || !gamma || !beta || !dx || !dgamma_part || !dbeta_part) return op.refuse("null pointer");
    if (b < 1 || t < 1 || t0 < 0 || t0 >= t || c < 1 || groups < 1 || c % groups || c / groups > 256 || (et != 0 && et != 1) ||
        (int64_t)b * groups > INT32_MAX || (int64_t)t * (c / groups) > INT32_MAX)
        return op.refuse("invalid arguments (need b, t >= 1, 0 <= t0 < t, c % groups == 0, c / groups <= 256, et 0 or 1)");
    R50_ET_LAUNCH(et, gn_relu_causal3_tm_bwd_kernel, dim3((unsigned)(b * groups)), dim3(256), 0, stream, (const unsigned short*)dr,
                  (const unsigned short*)x, gamma, beta, (const unsigned short*)add, (unsigned short*)dx, dgamma_part, dbeta_part, b, t, t0,
                  c, groups, eps);
    return op.done();
}

int r50_op_rollout_pose_loss_grad(const float* pred, const float* gt, int b, int k, int t_gt, int i0, int joints, float loss_scale,
                                  float* dy, float* loss2, void* stream) {
    const Op op{"r50_op_rollout_pose_loss_grad"};
    if (!pred || !gt || !dy || !loss2) return op.refuse("null pointer");
    if (b < 1 || k < 1 || joints < 1 || i0 < 0 || (int64_t)i0 + k > t_gt || (int64_t)b * t_gt > INT32_MAX ||
        (int64_t)k * b * joints > INT64_MAX / 3)
        return op.refuse("invalid arguments (need b, k, joints >= 1 and 0 <= i0, i0 + k <= t_gt)");
    hipLaunchKernelGGL(rollout_pose_loss_grad_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, pred, gt, b, k, t_gt, i0, joints,
                       loss_scale, dy, loss2);
    return op.done();
}

int r50_op_rollout_latent_grad(const void* fut, const void* phi, int b, int k, int t_phi, int i0, int d, float lambda, float loss_scale,
                               float* dfut, float* loss_lat, float* row_part, int et, void* stream) {
    const Op op{"r50_op_rollout_latent_grad"};
    if (!fut || !phi || !dfut || !loss_lat || !row_part) return op.refuse("null pointer");
    if (b < 1 || k < 1 || i0 < 0 || (int64_t)i0 + k > t_phi || (int64_t)b * k > INT32_MAX || (int64_t)b * t_phi > INT32_MAX)
        return op.refuse("need b, k >= 1 and 0 <= i0, i0 + k <= t_phi");
    if (d < 8 || d % 8) return op.refuse("d must be a positive multiple of 8");
    if (et != 0 && et != 1) return op.refuse("et must be 0 (bf16) or 1 (fp16)");
    if (int rc = op.aligned({{fut, "fut", 16}, {phi, "phi", 16}, {dfut, "dfut", 16}})) return rc;
    const long long rows = (long long)b * k;
    const double n_l = (double)rows * d;
    const float coef = (float)((double)lambda * 2.0 / n_l * (double)loss_scale);
    R50_ET_LAUNCH(et, rollout_latent_grad_kernel, dim3((unsigned)rows), dim3(128), 0, stream, (const unsigned short*)fut, (const unsigned short*)phi,
                  b, t_phi, i0, d, coef, dfut, row_part);
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_part, rows, 1.0 / n_l, loss_lat);
    return op.done();
}

int r50_op_check_finite(const float* g, int64_t n, int* found, void* stream) {
    const Op op{"r50_op_check_finite"};
    if (!g || !found || n < 1) return op.refuse("invalid arguments");
    hipLaunchKernelGGL(check_finite_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, g, (long long)n, found);
    return op.done();
}

int r50_op_check_overflow16(const void* x, int64_t n, int* found, int et, void* stream) {
    const Op op{"r50_op_check_overflow16"};
    if (int rc = op.aligned({{x, "x", 2}})) return rc;
    if (!x || !found || n < 1 || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    R50_ET_LAUNCH(et, check_overflow16_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, (const unsigned short*)x, (long long)n, found);
    return op.done();
}

int r50_op_adamw(float* p, float* m, float* v, const float* g, void* p16, int64_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, const int* found_inf, int et, void* stream) {
    const Op op{"r50_op_adamw"};
    if (int rc = op.aligned({{p16, "p16", 2}})) return rc;
    if (!p || !m || !v || !g || !p16 || n < 1 || step < 1 || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    const double bc1 = 1.0 - std::pow((double)beta1, step), bc2 = 1.0 - std::pow((double)beta2, step);
    R50_ET_LAUNCH(et, adamw_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, p, m, v, g, (unsigned short*)p16, (long long)n, lr, beta1, beta2, eps,
                  weight_decay, (float)bc1, (float)std::sqrt(bc2), found_inf);
    return op.done();
}

// The schedule of grad_norm_part_kernel, from n alone: W = min(ceil(n / GRAD_NORM_GRANULE), GRAD_NORM_MAX_WG) workgroups, each a
// slice of ceil(n / W) elements rounded up to a multiple of 4.
static int grad_norm_workgroups(long long n) {
    return (int)std::min<long long>((n + GRAD_NORM_GRANULE - 1) / GRAD_NORM_GRANULE, GRAD_NORM_MAX_WG);
}

int r50_op_grad_norm(const float* g, int64_t n, float max_norm, double* part, int n_part, int* found, float* clip2, double* stats4,
                     void* stream) {
    const Op op{"r50_op_grad_norm"};
    if (!g || !part || !found || !clip2 || !stats4) return op.refuse("null pointer");
    if (n < 1 || n > (1ll << 40)) return op.refuse("need 1 <= n <= 2^40");
    if (max_norm != max_norm) return op.refuse("max_norm is nan");
    const int w = grad_norm_workgroups(n);
    if (n_part < w)
        return op.refuse("part holds " + std::to_string(n_part) + " doubles, n = " + std::to_string(n) + " needs " + std::to_string(w));
    if (int rc = op.aligned({{g, "g", 16}})) return rc;
    const long long slice = (((long long)n + w - 1) / w + 3) / 4 * 4;
    hipLaunchKernelGGL(grad_norm_part_kernel, dim3(w), dim3(256), 0, (hipStream_t)stream, g, (long long)n, slice, part);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, w, max_norm, found, clip2,
                       stats4);
    return op.done();
}

int r50_op_adamw_clip_ema(float* p, float* m, float* v, const float* g, void* p16, int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int step, const int* found_inf, const float* clip, float* ema, float ema_weight, int et,
                          void* stream) {
    const Op op{"r50_op_adamw_clip_ema"};
    if (int rc = op.aligned({{p16, "p16", 2}})) return rc;
    if (!p || !m || !v || !g || !p16 || n < 1 || step < 1 || (et != 0 && et != 1)) return op.refuse("invalid arguments");
    const double bc1 = 1.0 - std::pow((double)beta1, step), bc2 = 1.0 - std::pow((double)beta2, step);
    R50_ET_LAUNCH(et, adamw_clip_ema_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, p, m, v, g, (unsigned short*)p16, (long long)n, lr, beta1, beta2,
                  eps, weight_decay, (float)bc1, (float)std::sqrt(bc2), found_inf, clip, ema, ema_weight);
    return op.done();
}

int64_t r50_stem_scratch_bytes(int n) { return (int64_t)STEM_W_BYTES + (int64_t)n * STEM_HP * STEM_WP * 8; }

int r50_op_stem(const float* x, int n, const float* w_host, const float* bias_dev, void* scratch, void* y, void* stream) {
    const Op op{"r50_op_stem"};
    if (int rc = op.aligned({{bias_dev, "bias_f32_dev", 16}, {scratch, "scratch_dev", 16},
                             {y, "y_nhwc_bf16", 16}}))
        return rc;
    if (!x || !w_host || !bias_dev || !scratch || !y || n < 1) return op.refuse("invalid arguments");
    // stem_conv_kernel runs one workgroup per (image, 4 output rows): the grid is an int (every offset inside both kernels is 64-bit)
    if (Launch r; size_over(r, "workgroups n*28", (long long)n * (112 / STEM_ROWS_PER_WG), k2p31, "2^31")) return op.done(r);
    std::vector<uint16_t> pk;
    const int et = op_et();
    pack_stem(w_host, pk, et == 1 ? 2 : 0);
    hipStream_t s = (hipStream_t)stream;
    if (hipError_t e = hipMemcpyAsync(scratch, pk.data(), STEM_W_BYTES, hipMemcpyHostToDevice, s)) return op.done(e);
    if (hipError_t e = hipStreamSynchronize(s)) return op.done(e);   // pk is a host temporary
    char* xp = (char*)scratch + STEM_W_BYTES;
    if (int rc = op.done(launch_stem_pack(x, xp, n, s, et))) return rc;
    return op.done(launch_stem_conv(xp, scratch, bias_dev, y, n, s, et));
}

int r50_op_maxpool(const void* x, int n, int h, int w, int c, void* y, void* stream) {
    const Op op{"r50_op_maxpool"};
    if (int rc = op.aligned({{x, "x_nhwc_bf16", 16}, {y, "y_nhwc_bf16", 16}})) return rc;
    if (!x || !y || n < 1 || h < 1 || w < 1 || c < 8 || c % 8) return op.refuse("invalid arguments");
    // maxpool3x3s2_kernel counts and addresses in 64 bits (a grid-stride loop over at most 2^14 workgroups): the limit is the byte offset itself
    if ((__int128)n * h * w * c * 2 >= ((__int128)1 << 63)) return op.refuse("x bytes, n*h*w*c*2, must be < 2^63");
    return op.done(launch_maxpool(x, y, n, h, w, c, (hipStream_t)stream, op_et()));
}

int r50_op_avgpool(const void* x, int n, int hw, int c, float* y, void* stream) {
    const Op op{"r50_op_avgpool"};
    if (int rc = op.aligned({{x, "x_nhwc_bf16", 16}, {y, "y_f32", 16}})) return rc;
    if (!x || !y || n < 1 || hw < 1 || c < 8 || c % 8) return op.refuse("invalid arguments");
    // avgpool_kernel: one thread per (image, 8 channels), numbered in an int over a grid rounded up to 256 threads; the row offsets are 64-bit
    if (Launch r; size_over(r, "threads n*(c/8) + 255", (long long)n * (c / 8) + 255, k2p31, "2^31")) return op.done(r);
    if ((__int128)n * hw * c * 2 >= ((__int128)1 << 63)) return op.refuse("x bytes, n*hw*c*2, must be < 2^63");
    return op.done(launch_avgpool(x, y, n, hw, c, (hipStream_t)stream, op_et()));
}

// ---- forecast baselines (kernels.h: row_norm2_kernel, nn_search_kernel, nn_merge_kernel, baseline_forecasts_kernel) ----
constexpr int kNnMaxWgs = 512;           // workgroups whose lists the workspace holds (the grid is the CU budget, at most this)
static int nn_chunk_rows(int d) { return d <= 1024 ? 32 : 16; }

size_t r50_op_nn_search_workspace(int nq, int n, int k) {
    if (nq < 1 || n < 1 || k < 1 || k > NN_MAX_K) return 0;
    const long long chunks = ((long long)n + 15) / 16;                   // the smallest chunk any d uses
    const long long wgs = std::min<long long>(chunks, kNnMaxWgs);
    return (size_t)wgs * (size_t)std::min(nq, NN_MAX_Q) * (size_t)k * 8;
}

int r50_op_row_norm2(const void* x, int n, int d, int et, float* out, void* stream) {
    const Op op{"r50_op_row_norm2"};
    if (!x || !out) return op.refuse("null pointer");
    if (n < 1 || d < 8 || d % 8 != 0 || (et != 0 && et != 1)) return op.refuse("invalid arguments (need n >= 1, d a positive multiple of 8)");
    if (int rc = op.aligned({{x, "x", 16}})) return rc;
    R50_ET_LAUNCH(et, row_norm2_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, (const unsigned short*)x, n, d, out);
    return op.done();
}

int r50_op_nn_search(const void* q, int nq, const void* x, int n, int d, int et, const float* x_norm2, int k, int* idx_out, float* dist2_out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    const Op op{"r50_op_nn_search"};
    if (!q || !x || !x_norm2 || !idx_out || !dist2_out || !workspace) return op.refuse("null pointer");
    if (nq < 1 || n < 1 || n > (1 << 30) || k < 1 || k > NN_MAX_K || k > n || d < 32 || d > 2048 || d % 32 != 0 || (et != 0 && et != 1))
        return op.refuse("invalid arguments (need nq >= 1, 1 <= k <= 8, k <= n <= 2^30, d % 32 == 0 and 32 <= d <= 2048)");
    if (int rc = op.aligned({{q, "q", 16}, {x, "x", 16}, {workspace, "workspace", 4}})) return rc;
    if (workspace_bytes < r50_op_nn_search_workspace(nq, n, k)) return op.refuse("the workspace is smaller than r50_op_nn_search_workspace asks for");
    const int cus = num_cus();
    if (cus == 0) return op.hip_failed("the device could not be queried");
    const int ch = nn_chunk_rows(d);
    const int n_chunks = (n + ch - 1) / ch;
    const int grid = std::min(std::min(n_chunks, cus), kNnMaxWgs);
    hipStream_t s = (hipStream_t)stream;
    float* ws_score = (float*)workspace;
    for (int q0 = 0; q0 < nq; q0 += NN_MAX_Q) {                          // one walk of the database per 256 queries
        const int nql = std::min(nq - q0, NN_MAX_Q);
        int* ws_idx = (int*)(ws_score + (size_t)grid * nql * k);
        const size_t lds = (size_t)2 * ch * d * 2 + (size_t)((nql + 63) / 64 * 64) * k * 8;
        const unsigned short* ql = (const unsigned short*)q + (size_t)q0 * d;
        auto kern = ch == 32 ? R50_BY_ET(et, nn_search_kernel, 2) : R50_BY_ET(et, nn_search_kernel, 1);      // rows per block: 2 with 32-row chunks
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return op.done(e);
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NN_THREADS), lds, s, ql, nql, (const unsigned short*)x, n, d, x_norm2, k, ws_score, ws_idx);
        R50_ET_LAUNCH(et, nn_merge_kernel, dim3((unsigned)nql), dim3(64), 0, stream, (const float*)ws_score, (const int*)ws_idx, grid, nql, k, ql, d,
                      idx_out + (size_t)q0 * k, dist2_out + (size_t)q0 * k);
    }
    return op.done();
}

int r50_op_baseline_forecasts(const float* a1, const float* a0, const int* nn_row, const float* dbj, int64_t n_db, int b, int k, int t_db,
                              int joints, int root, int input_len, int pred_len, float* const_pose, float* const_vel, float* nn,
                              void* stream) {
    const Op op{"r50_op_baseline_forecasts"};
    if (!a1 || (const_vel && !a0) || (nn && (!nn_row || !dbj)) || (!const_pose && !const_vel && !nn))
        return op.refuse("null pointer (a1 always; a0 with const_vel; nn_row and dbj with nn; at least one output)");
    if (b < 1 || joints < 1 || joints > 64 || root < 0 || root >= joints || pred_len < 1 || input_len < 1 ||
        (int64_t)b * pred_len * joints > INT32_MAX / 3)
        return op.refuse("invalid arguments (need b, pred_len, input_len >= 1, 1 <= joints <= 64, 0 <= root < joints)");
    if (nn && (k < 1 || k > NN_MAX_K || n_db < 1 || t_db < 1 || (int64_t)input_len + pred_len > t_db || (int64_t)b * k > INT32_MAX))
        return op.refuse("invalid arguments (with nn: 1 <= k <= 8, n_db >= 1 and input_len + pred_len <= t_db)");
    hipLaunchKernelGGL(baseline_forecasts_kernel, dim3(ew_grid((long long)b * pred_len * joints * 3)), dim3(256), 0, (hipStream_t)stream, a1,
                       a0, nn_row, dbj, b, k, t_db, joints, root, input_len, pred_len, const_pose, const_vel, nn);
    return op.done();
}

}  // extern "C"
