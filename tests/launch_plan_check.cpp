// Exhaustive host-side check of csrc/launch_plan.h: plans the stack for every option combination and asserts what the executor
// (run_stack in r50_abi.hip) relies on.  No GPU: tests/test_launch_plan_cpu.py compiles this file with ASan + UBSan and runs it.
#include "../implementation_phd_lab_vision_amd/csrc/launch_plan.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

using namespace launch_plan;

static long long g_plans = 0, g_violations = 0;

static void describe(const PlanInputs& in, char* out, size_t cap) {
    std::snprintf(out, cap, "precision %d stem %d c1 %d tail %d tail3 %d last %d dscat %d chain %d sub %d b1 %d b2 %d inplace %d overlap %d handover %d "
                  "tile %d profile %d buffers %d scales %d tap %s", in.precision, in.fused_stem, in.fuse_stem_c1, in.fuse_tail, in.fuse_tail3,
                  in.fuse_tail3_last, in.fuse_ds_cat, in.fuse_cat_chain, in.sub_out, in.fuse_block1, in.fuse_block2, in.inplace_out, in.overlap_ds,
                  in.fuse_fp8_handover, in.tile_override, in.profile, (int)in.catchain_wp, (int)in.fp8_scales_complete, in.tap ? in.tap : "-");
}

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            char txt[512];                                                                                   \
            describe(in, txt, sizeof txt);                                                                   \
            if (++g_violations <= 20) std::fprintf(stderr, "line %d: %s\n  with %s\n", __LINE__, #cond, txt); \
        }                                                                                                    \
    } while (0)

struct Launches { int igemm = 0, conv1 = 0, maxpool = 0, avgpool = 0, stem_pack = 0, tail = 0, tail3 = 0, block2 = 0, catchain = 0; };

// launches of a whole forward (no tap), by the profile classes of r50_abi.hip
static Launches count_launches(const StackPlan& p) {
    Launches n;
    n.conv1 = 1;
    if (p.stem == Stem::PackConv) n.stem_pack = 1;
    if (p.stem == Stem::PackConv || p.stem == Stem::Split) n.maxpool = 1;
    for (int i = 0; i < p.n_blocks; ++i) {
        const BlockPlan& b = p.blocks[i];
        n.igemm += (b.conv1 == Conv1::Launch) + b.ds_side + b.ds_separate;
        if (b.body != Body::Conv2) { ++n.block2; continue; }
        ++n.igemm;       // conv2
        switch (b.tail) {
            case Tail::Conv3: case Tail::Cat: ++n.igemm; break;
            case Tail::Tail1: case Tail::Tail2: ++n.tail; break;
            case Tail::Tail3: case Tail::Tail3NoNext: ++n.tail3; break;
            case Tail::CatChain: ++n.catchain; break;
        }
    }
    if (p.stop == Stop::Avgpool) n.avgpool = 1;
    return n;
}

static void check_plan(const PlanInputs& in) {
    const StackPlan p = plan_stack(in);
    ++g_plans;
    const bool split = in.precision == kFp32x, fp8 = in.precision == kFp8;
    const bool pooled_stem = p.stem == Stem::Fused || p.stem == Stem::FusedConv1;
    CHECK(split == (p.stem == Stem::Split));
    CHECK(p.tap == TapAt::None || p.tap == TapAt::Pool || (p.tap == TapAt::Stem && !pooled_stem));
    CHECK(p.tap == TapAt::None || (p.n_blocks == 0 && p.stop == Stop::Tap));
    if (!in.tap) {
        CHECK(p.stop == (fp8 ? Stop::Fp8Part : Stop::Avgpool));
        CHECK(p.n_blocks == (fp8 ? kStages[0][1] : kNumBlocks));
    }
    int taps = p.tap != TapAt::None, li = 1;
    for (int i = 0; i < p.n_blocks; ++i) {
        const BlockPlan& b = p.blocks[i];
        const BlockPlan* next = i + 1 < p.n_blocks ? &p.blocks[i + 1] : nullptr;
        const int blocks = kStages[b.si][1];
        const bool last = b.b == blocks - 1, conv2 = b.body == Body::Conv2;
        const bool cat = conv2 && (b.tail == Tail::Cat || b.tail == Tail::CatChain);
        CHECK(b.li == li && b.li_next == li + (b.b == 0 ? 4 : 3) && b.li_next <= kNumConvs);
        li = b.li_next;
        // conv1 is "already there" exactly when the launch before this block wrote it
        const bool fed = i == 0 ? p.stem == Stem::FusedConv1 : p.blocks[i - 1].chain_next;
        CHECK((b.conv1 == Conv1::Ready) == fed);
        CHECK(!b.chain_next || b.li_next < kNumConvs);
        CHECK(b.chain_next == (conv2 ? (b.tail == Tail::Tail1 || b.tail == Tail::Tail2 || b.tail == Tail::Tail3 || b.tail == Tail::CatChain)
                                     : (b.body != Body::Block2 || b.b < blocks - 1)));
        // the compact layer1.2 output has exactly one writer / reader pair
        CHECK(!b.sub_out || (next && next->body == Body::Conv2 && next->tail == Tail::CatChain && b.body == Body::Block1 && !in.tap));
        CHECK((next ? next->x_sub : false) == b.sub_out);
        CHECK(i > 0 || !b.x_sub);
        CHECK(!b.x_sub || (conv2 && b.tail == Tail::CatChain));
        // ... and is written under the condition r50_abi.hip spelled out twice before the plan existed
        CHECK(b.sub_out == (in.sub_out && b.body == Body::Block1 && last && in.convs[b.li_next < kNumConvs ? b.li_next : 0].cout == 128 && in.fuse_ds_cat &&
                            in.cat_w[1] && in.fuse_cat_chain && in.catchain_wp && is16(in.precision)));
        // in place: a plain identity that is the block input, and no fused form that reads the input after the output is written
        const bool identity_is_input = !b.ds_side && !b.ds_separate;
        CHECK(b.inplace == (conv2 && in.inplace_out && !split && b.b > 0 && identity_is_input && !cat && !b.fuse_ds && !(fp8 && b.si == 0 && last)));
        CHECK(b.b > 0 || (b.ds_side + b.ds_separate + b.fuse_ds + cat + (b.body == Body::Block1Ds) == 1) || b.tap == TapAt::T1 || b.tap == TapAt::T2);
        CHECK(b.b == 0 || !(b.ds_side || b.ds_separate || b.fuse_ds || cat || b.body == Body::Block1Ds));
        CHECK(!b.ds_side || (conv2 && !b.fuse_ds && !cat && !in.profile && !in.tap && in.overlap_ds));
        CHECK(!b.fuse_ds || (conv2 && b.tail == Tail::Tail1));
        CHECK(!b.handover || (fp8 && b.si == 0 && last && conv2 && b.tail == Tail::Conv3 && in.fuse_fp8_handover && in.fp8_scales_complete && !in.tap));
        // every fused form stands for launches with automatic tiles, on 16-bit (layer1: or fp8-mode) tensors, and reads buffers that exist
        const bool fused = !conv2 || b.tail != Tail::Conv3;
        CHECK(!fused || (in.tile_override == 0 && !split));
        CHECK(conv2 || (!in.tap && in.fuse_tail && is16_or_fp8(in.precision)));
        CHECK(!(conv2 && (b.tail == Tail::Tail3 || b.tail == Tail::Tail3NoNext)) || (b.si == 2 && b.b > 0 && in.tail3_wp[b.b] && is16(in.precision)));
        CHECK(!(conv2 && b.tail == Tail::Tail3NoNext) || last);
        CHECK(!cat || in.cat_w[b.si]);
        CHECK(!(conv2 && b.tail == Tail::CatChain) || (in.catchain_wp && b.si == 1 && b.b == 0 && is16(in.precision)));
        CHECK((b.body == Body::Block1Ds) <= (b.si == 0 && b.b == 0) && (b.body == Body::Block1) <= (b.si == 0 && b.b > 0) && (b.body == Body::Block2) <= (b.si == 1 && b.b > 0));
        CHECK(b.tap == TapAt::None || (i == p.n_blocks - 1 && conv2 && p.stop == Stop::Tap));
        taps += b.tap != TapAt::None;
    }
    CHECK((p.stop == Stop::Tap) == (taps == 1) && taps <= 1);
}

// the twelve 0/1 options: every combination, or (few: the taps, whose names multiply everything by sixty) all off, all on, and each one alone off / on
template <typename F>
static void for_each_option_set(PlanInputs in, bool few, F&& f) {
    int* const bits[12] = {&in.fused_stem, &in.fuse_stem_c1, &in.fuse_tail, &in.fuse_tail3, &in.fuse_tail3_last, &in.fuse_ds_cat, &in.fuse_cat_chain,
                           &in.sub_out, &in.fuse_block2, &in.inplace_out, &in.overlap_ds, &in.fuse_fp8_handover};
    for (int mask = 0; mask < (1 << 12); ++mask) {
        const int ones = __builtin_popcount(mask);
        if (few && ones > 1 && ones < 11) continue;
        for (int i = 0; i < 12; ++i) *bits[i] = (mask >> i) & 1;
        f(in);
    }
}

static void set_buffers(PlanInputs& in, bool present) {
    for (bool& b : in.cat_w) b = present;
    for (bool& b : in.tail3_wp) b = present;
    in.cat_w[0] = false;                 // layer1.0 has no two-source form: r50_load_weights never packs it
    in.tail3_wp[0] = false;              // ... and layer3.0 no chained tail
    in.tail3_wp[6] = in.tail3_wp[7] = false;
    in.catchain_wp = present;
    in.fp8_scales_complete = present;
}

int main() {
    const std::vector<ConvSpec> specs = conv_specs();
    if ((int)specs.size() != kNumConvs) { std::fprintf(stderr, "conv_specs() has %zu entries, kNumConvs = %d\n", specs.size(), kNumConvs); return 1; }
    PlanInputs base;
    for (int i = 0; i < kNumConvs; ++i) base.convs[i] = specs[i].shape;

    // every tap name the spec table can produce, and a few it cannot
    std::vector<std::string> taps = {"stem", "pool"};
    for (int si = 0; si < 4; ++si)
        for (int b = 0; b < kStages[si][1]; ++b) {
            const std::string p = block_name(si, b);
            taps.insert(taps.end(), {p + ".t1", p + ".t2", p});
            if (b == 0) taps.push_back(p + ".ds");
        }
    const size_t n_real = taps.size();
    taps.insert(taps.end(), {"layer1.1.ds", "layer5.0", "layer1.3", "layer1.00", "avgpool", ""});

    const int precisions[] = {kBf16, kFp32x, kBf16w2, kFp16, kFp8};
    for (int precision : precisions)
        for (int present = 0; present < 2; ++present)
            for (int fb1 = 0; fb1 <= 3; ++fb1)
                for (int tile : {0, 2})
                    for (int profile = 0; profile < 2; ++profile) {
                        PlanInputs in = base;
                        in.precision = precision; in.fuse_block1 = fb1; in.tile_override = tile; in.profile = profile;
                        set_buffers(in, present != 0);
                        for_each_option_set(in, false, check_plan);                   // no tap: the whole cross product
                        if (tile || profile) continue;
                        for (size_t t = 0; t < taps.size(); ++t) {                    // taps: every name, at automatic tiles and without the profile
                            in.tap = taps[t].c_str();
                            for_each_option_set(in, true, [&](const PlanInputs& q) {
                                check_plan(q);
                                const PlanInputs& in = q;
                                const StackPlan p = plan_stack(q);
                                // a real name is hit at exactly one position (check_plan: at most one), or refused beyond layer1 in fp8 mode; others are unknown
                                const bool layer1 = t < 2 || taps[t].rfind("layer1.", 0) == 0;
                                if (t >= n_real) CHECK(p.stop == (precision == kFp8 ? Stop::Fp8TapRefused : Stop::UnknownTap));
                                else if (precision == kFp8 && !layer1) CHECK(p.stop == Stop::Fp8TapRefused);
                                else {
                                    CHECK(p.stop == Stop::Tap);
                                    std::string where = p.tap == TapAt::Stem ? "stem" : "pool";
                                    if (p.tap == TapAt::None && p.n_blocks > 0) {
                                        const BlockPlan& b = p.blocks[p.n_blocks - 1];
                                        where = block_name(b.si, b.b) + (b.tap == TapAt::T1 ? ".t1" : b.tap == TapAt::T2 ? ".t2" : b.tap == TapAt::Ds ? ".ds" : "");
                                    }
                                    CHECK(where == taps[t]);
                                }
                                for (int i = 0; i < p.n_blocks; ++i) CHECK(!p.blocks[i].sub_out);
                            });
                        }
                    }

    // The default bf16 plan against the launches per step bench.py reported for the default configuration: BENCH_r04.json,
    // parsed.kernels (batch 256, bf16): igemm 19, bneck_tail3 5, bneck_block2 6, bneck_catchain 1, conv1 1, avgpool 1 = 33 launches.
    {
        PlanInputs in = base;
        set_buffers(in, true);
        const Launches n = count_launches(plan_stack(in));
        CHECK(n.igemm == 19 && n.tail3 == 5 && n.block2 == 6 && n.catchain == 1 && n.conv1 == 1 && n.avgpool == 1);
        CHECK(n.tail == 0 && n.maxpool == 0 && n.stem_pack == 0);
        CHECK(n.igemm + n.tail + n.tail3 + n.block2 + n.catchain + n.conv1 + n.maxpool + n.stem_pack + n.avgpool == 33);
        // host time of one plan
        const int reps = 20000;
        long long sink = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) { in.inplace_out = i & 1; sink += plan_stack(in).n_blocks; }
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / reps;
        std::printf("plan_stack: %.0f ns per call (%lld)\n", ns, sink);
    }
    std::printf("plans checked: %lld, violations: %lld\n", g_plans, g_violations);
    return g_violations ? 1 : 0;
}
