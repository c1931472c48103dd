// kernel_variants_check -- rtc_scene_prep.h's kernel variants (render_variant, trace_variant, refine_variant, plan_supersampled) on
// hand-built plans, as a host program of its own: no device, no HIP call, so that it can run under the host sanitizers.
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

int main() {
    {  // a plan with every launch shape on
        ScenePlan p;
        p.spec_defs = {"-DRTC_SPEC_LIST=0x301", "-DRTC_SPEC_SHARE=1", "-DRTC_SPEC_BLOCKS_Y=1", "-DRTC_SPEC_RECT=1", "-DRTC_SPEC_ANY_REFL=1"};
        p.family_name = "render_kernel<4,simple>", p.spec_name = "render_kernel_spec[0x301;simple]";
        expect("render", render_variant(p), p.spec_defs, p.family_name, p.spec_name);
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
    }
    if (g_failures) return 1;
    std::puts("kernel variants: ok");
    return 0;
}
