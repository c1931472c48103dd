// kernel_variants_check -- rtc_scene_prep.h's kernel variants (render_variant, trace_variant, refine_variant, plan_supersampled,
// deep_variant) on hand-built plans, as a host program of its own: no device, no HIP call, so that it can run under the host sanitizers.
//
// (rtc_scene_prep.h wants rtc_kernel_core.h's types in front of it, so the compiler is hipcc; the sanitizers go to the host side)
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Iray_tracer_challenge_amd/csrc tools/kernel_variants_check.cpp -o tools/kernel_variants_check
//   tools/kernel_variants_check        (prints "kernel variants: ok"; exit status 1 and every difference otherwise)
//
// The renamings insert in front of a name's last character: a name that is not there (a world without objects has no scene
// kernel) must stay empty, and an option list that is not there must stay empty.
#include <cstdio>
#include <string>
#include <vector>

#include "rtc_kernel_core.h"
#include "rtc_scene_prep.h"

using namespace rtc;
typedef std::vector<std::string> Defs;

// rtc_internal.h's error reporting, which the library defines in rtc_host.cpp
namespace rtc {
rtc_status fail(rtc_status st, const char*, ...) { return st; }
}  // namespace rtc

static int g_failures = 0;
static std::string joined(const Defs& d) {
    std::string s;
    for (size_t i = 0; i < d.size(); i++) s += (i ? " " : "") + d[i];
    return s;
}
static void expect(const char* what, const KernelVariant& v, const Defs& defs, const std::string& family, const std::string& spec) {
    if (v.defs == defs && v.family_name == family && v.spec_name == spec) return;
    g_failures++;
    std::fprintf(stderr, "%s:\n  got  [%s] '%s' '%s'\n  want [%s] '%s' '%s'\n", what, joined(v.defs).c_str(), v.family_name.c_str(), v.spec_name.c_str(),
                 joined(defs).c_str(), family.c_str(), spec.c_str());
}

static void expect_kind(const char* what, const KernelVariant& v, JitKind kind, uint32_t k) {
    if (v.kind == kind && v.k == k) return;
    g_failures++;
    std::fprintf(stderr, "%s: kind %d factor %u, want %d and %u\n", what, (int)v.kind, v.k, (int)kind, k);
}
// deep_variant at depths 8, 9 and 33: stacks of 16, 16 and 64 levels; no -DRTC_SPEC_LDS_FRAMES=, -DRTC_SPEC_MAX_DEPTH= last, the
// rest (names, kind and factor too) as it was; without options an error and `deep` untouched
static void expect_deep(const char* what, const KernelVariant& v) {
    for (int depth : {8, 9, 33}) {
        KernelVariant deep;
        deep.spec_name = "untouched";
        const rtc_status st = deep_variant(v, depth, &deep);
        if (v.defs.empty()) {
            if (st != RTC_ERR_INVALID_ARG || deep.spec_name != "untouched" || !deep.defs.empty()) g_failures++, std::fprintf(stderr, "%s: deep_variant of no options\n", what);
            continue;
        }
        Defs want;
        for (const auto& d : v.defs)
            if (d.rfind("-DRTC_SPEC_LDS_FRAMES=", 0) != 0) want.push_back(d);
        want.push_back(std::string("-DRTC_SPEC_MAX_DEPTH=") + (depth == 33 ? "64" : "16"));
        if (st != RTC_OK) g_failures++, std::fprintf(stderr, "%s: deep_variant failed\n", what);
        expect(what, deep, want, v.family_name, v.spec_name);
        expect_kind(what, deep, v.kind, v.k);
    }
}

int main() {
    if (deep_stack_cap(-1) != 16 || deep_stack_cap(16) != 16 || deep_stack_cap(17) != 32 || deep_stack_cap(129) != RTC_MAX_DEPTH || deep_stack_cap(RTC_MAX_DEPTH) != RTC_MAX_DEPTH) {
        g_failures++;
        std::fprintf(stderr, "deep_stack_cap\n");
    }
    {  // a plan with every launch shape on
        ScenePlan p;
        p.spec_defs = {"-DRTC_SPEC_LIST=0x301", "-DRTC_SPEC_SHARE=1", "-DRTC_SPEC_BLOCKS_Y=1", "-DRTC_SPEC_RECT=1", "-DRTC_SPEC_ANY_REFL=1"};
        p.family_name = "render_kernel<4,simple>", p.spec_name = "render_kernel_spec[0x301;simple]";
        expect("render", render_variant(p), p.spec_defs, p.family_name, p.spec_name);
        expect_kind("render", render_variant(p), JitKind::RENDER, 1u);
        expect_kind("ss2", render_variant(p, 2u), JitKind::SS, 2u);
        expect_kind("trace", trace_variant(p), JitKind::TRACE, 1u);
        expect_kind("adaptive4", refine_variant(p, 4u), JitKind::ADAPTIVE, 4u);
        for (const KernelVariant& v : {render_variant(p), render_variant(p, 2u), trace_variant(p), refine_variant(p, 4u)}) expect_deep("deep", v);
        ScenePlan lds = p;  // ... and with the option a deep kernel drops, in the middle and twice
        lds.spec_defs.insert(lds.spec_defs.begin() + 2, "-DRTC_SPEC_LDS_FRAMES=5");
        lds.spec_defs.push_back("-DRTC_SPEC_LDS_FRAMES=5");
        for (const KernelVariant& v : {render_variant(lds), trace_variant(lds), refine_variant(lds, 2u)}) expect_deep("deep, LDS frames", v);
        expect("ss2", render_variant(p, 2u),
               {"-DRTC_SPEC_LIST=0x301", "-DRTC_SPEC_SHARE=1", "-DRTC_SPEC_BLOCKS_Y=0", "-DRTC_SPEC_RECT=0", "-DRTC_SPEC_ANY_REFL=1", "-DRTC_SPEC_SS=2"},
               "ss_render_kernel<4,simple;ss=2>", "ss_render_kernel_spec[0x301;simple;ss=2]");
        const Defs stream = {"-DRTC_SPEC_LIST=0x301", "-DRTC_SPEC_SHARE=0", "-DRTC_SPEC_BLOCKS_Y=0", "-DRTC_SPEC_RECT=0", "-DRTC_SPEC_ANY_REFL=1"};
        Defs want = stream;
        want.push_back("-DRTC_SPEC_TRACE=1");
        expect("trace", trace_variant(p), want, "trace_kernel<4,simple>", "trace_kernel_spec[0x301;simple]");
        want.back() = "-DRTC_SPEC_ADAPTIVE=4";
        expect("adaptive4", refine_variant(p, 4u), want, "adaptive_refine_kernel<4,simple;ss=4>", "adaptive_refine_kernel_spec[0x301;simple;ss=4]");
        // ... and what a supersampled context keeps of it
        p.scene_tile_mask.assign(12, 1), p.scene_rect[1] = 3u, p.scene_rect[3] = 4u;
        p.spec_blocks_y = p.spec_rect = p.spec_shares = p.wf_pays = true;
        plan_supersampled(&p, 4u);
        expect("plan_supersampled", render_variant(p),
               {"-DRTC_SPEC_LIST=0x301", "-DRTC_SPEC_SHARE=1", "-DRTC_SPEC_BLOCKS_Y=0", "-DRTC_SPEC_RECT=0", "-DRTC_SPEC_ANY_REFL=1", "-DRTC_SPEC_SS=4"},
               "ss_render_kernel<4,simple;ss=4>", "ss_render_kernel_spec[0x301;simple;ss=4]");
        expect_kind("plan_supersampled", render_variant(p), JitKind::SS, 4u);
        expect_deep("deep, plan_supersampled", render_variant(p));
        if (!p.scene_tile_mask.empty() || p.scene_rect[1] || p.scene_rect[3] || p.spec_blocks_y || p.spec_rect || p.wf_pays || !p.spec_shares) {
            g_failures++;
            std::fprintf(stderr, "plan_supersampled: the fine frame's tiles, rectangle or blocks were carried over\n");
        }
    }
    {  // a world without objects: no options, no scene kernel's name
        ScenePlan p;
        p.family_name = "render_kernel<4,simple>";
        expect("empty defs: ss4", render_variant(p, 4u), {}, "ss_render_kernel<4,simple;ss=4>", "");
        expect("empty defs: trace", trace_variant(p), {}, "trace_kernel<4,simple>", "");
        expect("empty defs: adaptive2", refine_variant(p, 2u), {}, "adaptive_refine_kernel<4,simple;ss=2>", "");
        for (const KernelVariant& v : {render_variant(p), render_variant(p, 4u), trace_variant(p), refine_variant(p, 2u)}) expect_deep("empty defs: deep", v);
        plan_supersampled(&p, 2u);
        expect("empty defs: plan_supersampled", render_variant(p), {}, "ss_render_kernel<4,simple;ss=2>", "");
    }
    {  // no names at all, options without a launch shape; and names that are one character or not a render kernel's
        ScenePlan p;
        p.spec_defs = {"-DRTC_SPEC_LIST=0x1"};
        expect("empty names: ss2", render_variant(p, 2u), {"-DRTC_SPEC_LIST=0x1", "-DRTC_SPEC_SS=2"}, "", "");
        expect("empty names: trace", trace_variant(p), {"-DRTC_SPEC_LIST=0x1", "-DRTC_SPEC_TRACE=1"}, "", "");
        expect("empty names: adaptive2", refine_variant(p, 2u), {"-DRTC_SPEC_LIST=0x1", "-DRTC_SPEC_ADAPTIVE=2"}, "", "");
        p.family_name = ">", p.spec_name = "wavefront[x]";
        expect("odd names: ss2", render_variant(p, 2u), {"-DRTC_SPEC_LIST=0x1", "-DRTC_SPEC_SS=2"}, "ss_;ss=2>", "ss_wavefront[x;ss=2]");
        expect("odd names: trace", trace_variant(p), {"-DRTC_SPEC_LIST=0x1", "-DRTC_SPEC_TRACE=1"}, ">", "wavefront[x]");
        expect("odd names: adaptive4", refine_variant(p, 4u), {"-DRTC_SPEC_LIST=0x1", "-DRTC_SPEC_ADAPTIVE=4"}, ";ss=4>", "wavefront[x;ss=4]");
        for (const KernelVariant& v : {render_variant(p), render_variant(p, 2u), trace_variant(p), refine_variant(p, 4u)}) expect_deep("odd names: deep", v);
    }
    if (g_failures) return 1;
    std::puts("kernel variants: ok");
    return 0;
}
