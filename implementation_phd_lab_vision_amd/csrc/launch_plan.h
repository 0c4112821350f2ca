// Which launches one pass over the ResNet-50 [:-1] stack consists of, decided in one place and as data.
// plan_stack() reads the precision, the options, which packed weight buffers exist and the conv shapes, and returns the stem
// form, one BlockPlan per bottleneck block and where the stack stops; run_stack (r50_abi.hip) executes that and decides nothing.
// Plain C++ without HIP: tests/launch_plan_check.cpp enumerates every option combination on the host and checks the
// invariants the executor relies on.
#pragma once

#include <cstring>
#include <string>
#include <vector>

namespace launch_plan {

constexpr int kBf16 = 1, kFp32x = 2, kBf16w2 = 3, kFp16 = 4, kFp8 = 5;      // = R50_PREC_* of include/r50.h
inline bool is16(int p) { return p == kBf16 || p == kFp16; }
inline bool is16_or_fp8(int p) { return is16(p) || p == kFp8; }

struct ConvShape { int cin, cout, ks, stride, pad; };
struct ConvSpec { std::string conv_key, bn_key; ConvShape shape; };

constexpr int kStages[4][3] = {{64, 3, 1}, {128, 4, 2}, {256, 6, 2}, {512, 3, 2}};       // planes, blocks, stride of the first block
constexpr int kNumBlocks = 16;
constexpr int kNumConvs = 53;            // the stem + 3 per block + one downsample conv per stage
constexpr int kFp8FirstConv = 11;        // convs[1..10] = layer1 (4 + 3 + 3); fp8 mode quantises from layer2.0.conv1 on

inline std::string block_name(int si, int b) { return "layer" + std::to_string(si + 1) + "." + std::to_string(b); }

// every conv of the stack in execution order, convs[0] = stem; a stage's first block is conv1, conv2, conv3, downsample
inline std::vector<ConvSpec> conv_specs() {
    std::vector<ConvSpec> v;
    v.push_back({"conv1", "bn1", {3, 64, 7, 2, 3}});
    int inpl = 64;
    for (int si = 0; si < 4; ++si) {
        const int planes = kStages[si][0], blocks = kStages[si][1], stride = kStages[si][2];
        for (int b = 0; b < blocks; ++b) {
            const int s = (b == 0) ? stride : 1;
            const std::string p = block_name(si, b);
            v.push_back({p + ".conv1", p + ".bn1", {inpl, planes, 1, 1, 0}});
            v.push_back({p + ".conv2", p + ".bn2", {planes, planes, 3, s, 1}});
            v.push_back({p + ".conv3", p + ".bn3", {planes, planes * 4, 1, 1, 0}});
            if (b == 0) v.push_back({p + ".downsample.0", p + ".downsample.1", {inpl, planes * 4, 1, s, 0}});
            inpl = planes * 4;
        }
    }
    return v;
}

struct PlanInputs {
    int precision = kBf16;
    int fused_stem = 1, fuse_stem_c1 = 1, fuse_tail = 1, fuse_tail3 = 1, fuse_tail3_last = 1, fuse_ds_cat = 1, fuse_cat_chain = 1, sub_out = 1,
        fuse_block1 = 3, fuse_block2 = 1, inplace_out = 0, overlap_ds = 0, fuse_fp8_handover = 1, tile_override = 0, profile = 0;
    bool cat_w[4] = {}, tail3_wp[8] = {}, catchain_wp = false;      // which packed weight buffers exist
    bool fp8_scales_complete = false;
    const char* tap = nullptr;
    ConvShape convs[kNumConvs] = {};
};

enum class Stem { Split, Fused, FusedConv1, PackConv };               // FusedConv1: the fused kernel also computes layer1.0.conv1; Split / PackConv: + a maxpool launch
enum class Conv1 { Launch, Ready };                                   // Ready: written by the previous block's chained launch or by the stem
enum class Body { Conv2, Block1, Block1Ds, Block2 };                  // Conv2: conv2 launch, then a tail; the others: conv2 .. block output in one launch
enum class Tail { Conv3, Tail1, Tail2, Tail3, Tail3NoNext, Cat, CatChain };
enum class TapAt { None, Stem, Pool, T1, T2, Ds, Out };
enum class Stop { Avgpool, Tap, Fp8Part, Fp8TapRefused, UnknownTap };

struct BlockPlan {
    int si = 0, b = 0, li = 0;       // stage, block of the stage, index of the block's conv1 in convs
    int li_next = 0;                 // index of the next block's conv1 (kNumConvs behind the last block)
    Conv1 conv1 = Conv1::Launch;
    Body body = Body::Conv2;
    Tail tail = Tail::Conv3;         // Body::Conv2 only
    bool fuse_ds = false;            // Tail1: the downsample conv of the block input is computed in the tail kernel
    bool ds_separate = false;        // the downsample conv is a launch of its own on the main stream
    bool ds_side = false;            // ... on the side stream, beside conv1 -> conv2
    bool chain_next = false;         // this block's last launch also writes the next block's conv1 output
    bool inplace = false;            // the block output goes over the block input
    bool sub_out = false;            // Block1: only the even rows / columns of the block output are stored
    bool x_sub = false;              // CatChain: the block input is such a compact tensor
    bool handover = false;           // Conv3: fp8 mode, quantise layer1's output in this conv's epilogue
    TapAt tap = TapAt::None;         // the requested activation is available in this block, at this point
};

struct StackPlan {
    Stem stem = Stem::Fused;
    TapAt tap = TapAt::None;         // Stem / Pool: the stack stops there
    int n_blocks = 0;                // blocks that run (the last one up to its tap, if it has one)
    BlockPlan blocks[kNumBlocks];
    Stop stop = Stop::Avgpool;
};

// ---- shapes the fused kernels are written for -------------------------------------------------------------------------
inline bool is_3x3_body(const ConvShape& c2, int ch) { return c2.ks == 3 && c2.stride == 1 && c2.pad == 1 && c2.cin == ch && c2.cout == ch; }
inline bool is_1x1_s1(const ConvShape& c, int cin, int cout) { return c.ks == 1 && c.stride == 1 && c.cin == cin && c.cout == cout; }
inline bool is_layer1_body(const ConvShape& c1, const ConvShape& c2, const ConvShape& c3, int hh, int ww) {
    return hh == 56 && ww == 56 && c1.cout == 64 && is_3x3_body(c2, 64) && c3.ks == 1 && c3.cin == 64 && c3.cout == 256;
}
inline bool is_layer2_body(const ConvShape& c1, const ConvShape& c2, const ConvShape& c3, int hh, int ww) {
    return hh == 28 && ww == 28 && c1.cout == 128 && is_3x3_body(c2, 128) && c3.ks == 1 && c3.cin == 128 && c3.cout == 512;
}
// tails: conv3 of this block and conv1 of the next (both 1x1 stride 1: `chainable` below)
inline bool is_layer1_tail(const ConvShape& c3, const ConvShape& nx) { return c3.cin == 64 && c3.cout == 256 && nx.cin == 256 && (nx.cout == 64 || nx.cout == 128); }
inline bool is_layer2_tail(const ConvShape& c3, const ConvShape& nx) { return c3.cin == 128 && c3.cout == 512 && nx.cin == 512 && nx.cout == 128; }
inline bool is_layer3_tail(const ConvShape& c3) { return c3.cin == 256 && c3.cout == 1024; }
inline bool is_layer3_chain(const ConvShape& c3, const ConvShape& nx) { return is_layer3_tail(c3) && nx.cin == 1024 && nx.cout == 256; }

inline StackPlan plan_stack(const PlanInputs& in) {
    StackPlan plan;
    const bool split = in.precision == kFp32x;
    const bool tiles_auto = in.tile_override == 0;       // every fused form stands for launches with automatic tile choice
    const char* tap = in.tap;
    auto tap_is = [&](const char* name) { return tap && std::strcmp(tap, name) == 0; };
    auto tap_in = [&](int si, int b, const char* suffix) { return tap && block_name(si, b) + suffix == tap; };     // e.g. "layer2.0" + ".ds"

    // ---- stem ----
    bool have_t1 = false;        // the coming block's conv1 output already exists
    if (split) plan.stem = Stem::Split;
    else if (in.fused_stem && !tap_is("stem")) {
        const ConvShape& l1c1 = in.convs[1];
        have_t1 = in.fuse_stem_c1 && is16_or_fp8(in.precision) && tiles_auto && is_1x1_s1(l1c1, 64, 64);
        plan.stem = have_t1 ? Stem::FusedConv1 : Stem::Fused;
    } else plan.stem = Stem::PackConv;
    if (plan.stem != Stem::Fused && plan.stem != Stem::FusedConv1 && tap_is("stem")) { plan.tap = TapAt::Stem; plan.stop = Stop::Tap; return plan; }
    if (tap_is("pool")) { plan.tap = TapAt::Pool; plan.stop = Stop::Tap; return plan; }

    // ---- blocks ----
    int hh = 56, ww = 56, li = 1;
    for (int si = 0; si < 4; ++si) {
        const int blocks = kStages[si][1];
        if (si == 1 && in.precision == kFp8) {       // layer2-4 run on e4m3 tensors: run_fp8_part
            plan.stop = tap ? Stop::Fp8TapRefused : Stop::Fp8Part;
            break;
        }
        for (int b = 0; b < blocks; ++b) {
            BlockPlan& bp = plan.blocks[plan.n_blocks++];
            bp.si = si; bp.b = b; bp.li = li; bp.li_next = li + ((b == 0) ? 4 : 3);
            bp.conv1 = have_t1 ? Conv1::Ready : Conv1::Launch;
            have_t1 = false;
            const ConvShape &c1 = in.convs[li], &c2 = in.convs[li + 1], &c3 = in.convs[li + 2];
            const ConvShape* nx = (bp.li_next < kNumConvs) ? &in.convs[bp.li_next] : nullptr;
            const ConvShape* cdp = (b == 0) ? &in.convs[li + 3] : nullptr;
            const bool last = b == blocks - 1;
            const bool tap_ds = tap_in(si, b, ".ds");
            const int h2 = (hh + 2 * c2.pad - c2.ks) / c2.stride + 1, w2 = (ww + 2 * c2.pad - c2.ks) / c2.stride + 1;      // conv1 / conv3 are 1x1 stride 1
            const bool nx_is_fp8 = in.precision == kFp8 && bp.li_next >= kFp8FirstConv;       // the next conv1's weights are e4m3 bytes
            // a fused launch may stand for conv3 and the next conv1
            const bool chainable = nx && c3.ks == 1 && c3.stride == 1 && nx->ks == 1 && nx->stride == 1;
            const bool fuse_ok = !split && !nx_is_fp8 && is16_or_fp8(in.precision) && in.fuse_tail && tiles_auto && chainable;
            // layer2.0 / 3.0 / 4.0: conv3 + downsample + add + ReLU as ONE 1x1 conv over K = [t2 | block input at the block's stride] against
            // [W3 | Wd].  It takes precedence over the layer2 tail fusion in layer2.0 (whose identity would be that downsample tensor).
            const bool cat_ds = b == 0 && si >= 1 && !split && in.fuse_ds_cat && in.cat_w[si] && tiles_auto && cdp && cdp->ks == 1 && c3.ks == 1 && !tap_ds;
            const bool fuse3 = fuse_ok && in.fuse_tail3 && b > 0 && b < 8 && in.tail3_wp[b] && is_layer3_chain(c3, *nx);      // plain identity
            const bool fuse2 = fuse_ok && is_layer2_tail(c3, *nx);
            const bool fuse = !cat_ds && ((fuse_ok && is_layer1_tail(c3, *nx)) || fuse2 || fuse3);
            bp.fuse_ds = fuse && cdp && is_1x1_s1(*cdp, 64, 256) && !tap_ds;
            // The downsample branch only depends on the block input: on a side stream it runs beside conv1 -> conv2.  Not while
            // profiling (event brackets of two streams would interleave) and not when a tap is requested.
            bp.ds_side = b == 0 && in.overlap_ds && !in.profile && !tap && !bp.fuse_ds && !cat_ds;

            // ---- the body from conv2 on in one launch (same bits as the launches it replaces) ----
            const bool body_ok = in.fuse_tail && !split && !tap && tiles_auto;
            const bool nx64 = nx && nx->ks == 1 && nx->stride == 1 && nx->cin == 256 && (nx->cout == 64 || (nx->cout == 128 && in.fuse_block1 >= 2));
            if (in.fuse_block1 >= 3 && body_ok && si == 0 && b == 0 && cdp && nx && is16_or_fp8(in.precision) && is_layer1_body(c1, c2, c3, hh, ww) &&
                is_1x1_s1(*cdp, 64, 256) && is_1x1_s1(*nx, 256, 64) && !nx_is_fp8)
                bp.body = Body::Block1Ds;
            else if (in.fuse_block1 && body_ok && si == 0 && b > 0 && nx64 && (is16(in.precision) || (in.precision == kFp8 && nx->cout == 64)) &&
                     is_layer1_body(c1, c2, c3, hh, ww))
                bp.body = Body::Block1;
            else if (in.fuse_block2 && body_ok && si == 1 && b > 0 && !bp.ds_side && is16(in.precision) && is_layer2_body(c1, c2, c3, hh, ww))
                bp.body = Body::Block2;

            if (bp.body != Body::Conv2) {
                bp.fuse_ds = false;
                bp.chain_next = bp.body != Body::Block2 || (nx && is_1x1_s1(*nx, 512, 128));
            } else {
                if (tap_in(si, b, ".t1")) bp.tap = TapAt::T1;
                else if (tap_in(si, b, ".t2")) bp.tap = TapAt::T2;
                else {
                    bp.ds_separate = b == 0 && !bp.ds_side && !bp.fuse_ds && !cat_ds;
                    if (bp.ds_separate && tap_ds) bp.tap = TapAt::Ds;
                }
                const bool identity_is_input = !bp.ds_side && !bp.ds_separate;
                const bool fp8_last_of_layer1 = in.precision == kFp8 && si == 0 && last;
                // Plain-identity blocks may write the block output over the block input: every element of the identity is read by the
                // lane that produces the output element at the same address before that element is stored, and nobody else reads the
                // block input any more (conv1 ran earlier).  (The fp8 hand-over writes 1-byte elements.)
                bp.inplace = in.inplace_out && !split && b > 0 && identity_is_input && !cat_ds && !bp.fuse_ds && !fp8_last_of_layer1;
                if (fuse) { bp.tail = fuse3 ? Tail::Tail3 : fuse2 ? Tail::Tail2 : Tail::Tail1; bp.chain_next = true; }
                else if (cat_ds && in.fuse_cat_chain && in.catchain_wp && si == 1 && fuse_ok && !tap && h2 == 28 && w2 == 28 && hh == 56 && ww == 56 &&
                         is16(in.precision) && is_layer2_tail(c3, *nx) && cdp->cin == 256 && cdp->stride == 2) { bp.tail = Tail::CatChain; bp.chain_next = true; }
                else if (cat_ds) bp.tail = Tail::Cat;
                // layer3.5: conv3 + identity + ReLU through the pipelined tail kernel without a second GEMM (its next conv1, layer4.0's
                // 1024 -> 512, does not fit the chain)
                else if (si == 2 && last && b < 8 && in.tail3_wp[b] && in.fuse_tail3 && in.fuse_tail3_last && body_ok && is16(in.precision) &&
                         c3.ks == 1 && is_layer3_tail(c3) && identity_is_input) bp.tail = Tail::Tail3NoNext;
                else bp.handover = fp8_last_of_layer1 && in.fuse_fp8_handover && !tap && in.fp8_scales_complete;
                if (bp.tap == TapAt::None && tap_in(si, b, "")) bp.tap = TapAt::Out;
            }
            if (bp.tap != TapAt::None) { plan.stop = Stop::Tap; return plan; }
            have_t1 = bp.chain_next;
            hh = h2; ww = w2;
            li = bp.li_next;
        }
    }
    if (plan.stop == Stop::Avgpool && tap) plan.stop = Stop::UnknownTap;

    // layer1.2 stores only the even rows / columns of its output when the one reader that understands the compact tensor, the
    // chained layer2.0 tail, is the launch that follows: one condition, read by both blocks.
    for (int i = 0; i + 1 < plan.n_blocks; ++i) {
        BlockPlan &bp = plan.blocks[i], &next = plan.blocks[i + 1];
        const bool compact_fits = bp.body == Body::Block1 && bp.b == kStages[bp.si][1] - 1 && in.convs[bp.li_next].cout == 128;
        bp.sub_out = next.x_sub = in.sub_out && compact_fits && next.tail == Tail::CatChain;
    }
    return plan;
}

}  // namespace launch_plan
