// rtc_jit.h -- the scene-kernel JIT's host side: which of the seven scene kernels a variant is (JitKind: entry point, the header
// beside the core, the argument block in the key), what a compile is made of (plan_jit: hiprtc's option list, the key text, the
// source hash and the cache file's name) and the disk cache's entries (read_cache_entry / publish_cache_entry: the only host code
// that reads files it did not write).  No device, no HIP header, nothing of rtc_kernel_core.h: rtc_device.hip's jit_get compiles,
// loads and remembers what is planned here; tests/test_jit_plan.py and tools/jit_check.cpp reach it without a GPU.
// The key's format is what keeps every disk cache and every profile keyed by rtc_ctx_kernel_id matched to its kernel: a change
// of a byte of it is a change of every id.
#ifndef RTC_JIT_H
#define RTC_JIT_H

#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rtc_internal.h"

namespace rtc {

inline uint64_t fnv1a(const std::string& s, uint64_t h = 1469598103934665603ull) { return fnv1a(s.data(), s.size(), h); }

// The six kernels a scene can have compiled for it: the frame's (rtc_kernel_core.h alone), the supersampled frame's, the ray
// streams', the adaptive refinement's (rtc_supersample.h / rtc_trace.h / rtc_adaptive.h beside the core), the lens frame's
// (rtc_lens.h, which includes rtc_supersample.h: two headers beside the core, and `beside` -- the text a hash folds in -- is the
// two texts one after the other, rtc_supersample.h first) and the lens frame's of the one-call seam (rtc_lens_seam.h, which
// includes rtc_lens.h: three headers, their texts in the same order -- rtc_supersample.h, rtc_lens.h, rtc_lens_seam.h).
// The seventh: the one-call seam's adaptive kernels (rtc_adaptive_seam.h, which includes rtc_adaptive.h: two headers, rtc_adaptive.h
// first) -- factor 2 or 4: the refinement of a part's share; factor 1: its halo pass.
enum class JitKind { RENDER, SS, TRACE, ADAPTIVE, LENS, LENS_SEAM, ADAPTIVE_SEAM };
struct JitKindFacts {
    const char *entry, *header, *program;  // entry point; the header beside the core ("": none); the program text handed to hiprtc
    const char *aot_prefix, *args_line;    // of the ahead-of-time id (SS, ADAPTIVE, LENS: the factor follows); of the key's argument-size line
    const char* header_below = "";         // the header that `header` includes beside the core ("": none)
    const char* header_below2 = "";        // ... and the one that one includes ("": none)
    const char* aot_suffix = "";           // of the ahead-of-time id, after the hash
};
inline const JitKindFacts& jit_kind_facts(JitKind kind) {
    static const JitKindFacts facts[7] = {
        {"render_kernel_spec", "", "#include \"rtc_kernel_core.h\"\n", "aot_", nullptr},
        {"ss_render_kernel_spec", "rtc_supersample.h", "#include \"rtc_supersample.h\"\n", "aot_ss", nullptr},
        {"trace_kernel_spec", "rtc_trace.h", "#include \"rtc_trace.h\"\n", "aot_trace_", "trace args "},
        {"adaptive_refine_kernel_spec", "rtc_adaptive.h", "#include \"rtc_adaptive.h\"\n", "aot_adaptive", "adaptive args "},
        {"lens_render_kernel_spec", "rtc_lens.h", "#include \"rtc_lens.h\"\n", "aot_lens", "lens args ", "rtc_supersample.h"},
        {"lens_render_kernel_spec", "rtc_lens_seam.h", "#include \"rtc_lens_seam.h\"\n", "aot_lens", "lens args ", "rtc_lens.h", "rtc_supersample.h", ".seam"},
        {"adaptive_seam_kernel_spec", "rtc_adaptive_seam.h", "#include \"rtc_adaptive_seam.h\"\n", "aot_adaptive_seam", "adaptive seam args ", "rtc_adaptive.h"}};
    return facts[(int)kind];
}
// (the plain kernels' names do not move: only the other four fold their headers' text into a hash)
inline uint64_t source_hash_of(JitKind kind, uint64_t h, const std::string& beside) { return kind == JitKind::RENDER ? h : fnv1a(beside, h); }

// Identifies the ahead-of-time kernels of this build by the source they were compiled from: "aot_<hash>", "aot_ss<k>_<hash>",
// "aot_trace_<hash>", "aot_adaptive<k>_<hash>", "aot_lens<k>_<hash>" -- and "aot_lens<k>_<hash>.seam", the one-call seam's lens
// kernel, whose hash is its own: it folds rtc_lens_seam.h in as well -- and "aot_adaptive_seam<k>_<hash>", the seam's adaptive kernels
// (k = 1: the halo pass), whose hash folds in rtc_adaptive.h and then rtc_adaptive_seam.h.
inline std::string aot_kernel_id(JitKind kind, uint32_t k, const std::string& core, const std::string& beside) {
    char hash[24];
    snprintf(hash, sizeof(hash), "%016llx", (unsigned long long)source_hash_of(kind, fnv1a(core), beside));
    const bool factor = kind == JitKind::SS || kind == JitKind::ADAPTIVE || kind == JitKind::LENS || kind == JitKind::LENS_SEAM || kind == JitKind::ADAPTIVE_SEAM;
    return jit_kind_facts(kind).aot_prefix + (factor ? std::to_string(k) + "_" : std::string()) + hash + jit_kind_facts(kind).aot_suffix;
}

// The sizes of the argument blocks, which the key carries (a kernel compiled for another layout must not be found).
struct JitArgSizes {
    size_t render, trace, adaptive;  // sizeof RenderArgs, TraceArgs, AdaptiveRefineArgs
    size_t lens = 0;                 // sizeof LensRenderArgs
    size_t adaptive_seam = 0;        // sizeof AdaptiveSeamArgs
};
// The key's text after the options: compiler version, ABI, the size of RenderArgs -- and of the kind's own argument block (its
// layout is its header's text, hashed as well).
inline std::string jit_key_tail(JitKind kind, int hiprtc_major, int hiprtc_minor, const JitArgSizes& sizes) {
    std::string t = "hiprtc " + std::to_string(hiprtc_major) + "." + std::to_string(hiprtc_minor) + " abi " + std::to_string(RTC_ABI_VERSION) + " args " +
                    std::to_string(sizes.render) + "\n";
    if (const char* line = jit_kind_facts(kind).args_line)
        t += line + std::to_string(kind == JitKind::TRACE ? sizes.trace : kind == JitKind::LENS || kind == JitKind::LENS_SEAM ? sizes.lens
                                   : kind == JitKind::ADAPTIVE_SEAM ? sizes.adaptive_seam : sizes.adaptive) + "\n";
    return t;
}

struct JitPlan {
    std::vector<std::string> opts;  // hiprtc's option list
    std::string key_text;           // every option, one per line, then jit_key_tail
    uint64_t source_hash = 0;       // of the core's text, key_text and (not RENDER) the header beside the core
    std::string cache_file;         // "spec_<16 hex of source_hash>.hsaco"
    const char* entry = nullptr;
};
// What one compile is made of.  `defs`: the variant's options, in order; `flags`: the development flags (RTC_AMD_JIT_FLAGS), space
// separated.  (Not in the key: WHICH libhiprtc this process holds.  A Python process that imported torch first compiles with the
// wheel's bundled compiler, the same script under rocprofv3 -- which puts /opt/rocm/lib first in LD_LIBRARY_PATH -- with the
// system's; both report one hiprtcVersion and emit different, equally valid code for these kernels (same images, same speed:
// profiles/r04_ab_compilers.txt).  Sharing the entry is what lets a profiled run measure the very code object a plain run
// compiled -- profiles/run_profile.sh compiles first, plainly -- and code_object_id says which binary it was.)
inline JitPlan plan_jit(const std::vector<std::string>& defs, JitKind kind, const std::string& flags, int hiprtc_major, int hiprtc_minor,
                        const JitArgSizes& sizes, const std::string& core, const std::string& beside) {
    JitPlan p;
    p.entry = jit_kind_facts(kind).entry;
    p.opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize"};
    p.opts.insert(p.opts.end(), defs.begin(), defs.end());
    // occupancy target of the specialised kernel: measured 4 -> 3.39, 5 -> 3.42, 6 -> 3.24, 7 -> 3.17, 8 -> 3.17 ms (C3) before
    // light-cone culling; with it (more state per shade point) 5 -> 0.98, 6 -> 0.97, 7 -> 0.95, 8 -> 1.02 ms (tools/ab_env.py over -DRTC_WAVES_PER_SIMD)
    bool waves_given = false;
    for (const auto& d : defs) waves_given = waves_given || d.rfind("-DRTC_WAVES_PER_SIMD=", 0) == 0;
    if (!waves_given) p.opts.push_back("-DRTC_WAVES_PER_SIMD=7");
    std::istringstream in(flags);
    for (std::string tok; in >> tok;) p.opts.push_back(tok);
    for (const auto& o : p.opts) p.key_text += o + "\n";
    p.key_text += jit_key_tail(kind, hiprtc_major, hiprtc_minor, sizes);
    p.source_hash = source_hash_of(kind, fnv1a(p.key_text, fnv1a(core)), beside);
    char name[64];
    snprintf(name, sizeof(name), "spec_%016llx.hsaco", (unsigned long long)p.source_hash);
    p.cache_file = name;
    return p;
}

// ---- the disk cache's entries ------------------------------------------------------------------------------------------
// An entry is its header {magic, size, checksum} + the code object.
struct CacheHeader {
    char magic[8];
    uint64_t size, checksum;
};
inline bool read_file(const std::string& path, std::string* out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::ostringstream ss;
    ss << f.rdbuf();
    *out = ss.str();
    return true;
}
// -> the code object of a whole entry.  A truncated or foreign file is ignored (the HIP runtime does not survive a damaged code
// object), and overwritten by the fresh compile.
inline bool read_cache_entry(const std::string& path, std::string* code) {
    if (!read_file(path, code) || code->size() <= sizeof(CacheHeader)) return false;
    CacheHeader h;
    std::memcpy(&h, code->data(), sizeof(h));
    code->erase(0, sizeof(h));
    return std::memcmp(h.magic, "RTCJIT1", 8) == 0 && h.size == code->size() && h.checksum == fnv1a(*code);
}
// Best effort: a read-only tree just means every process compiles for itself.  Only a completely written file is published (a
// short write -- disk full, quota -- would otherwise poison the cache for every later run): temporary file, then rename.
inline bool publish_cache_entry(const std::string& dir, const std::string& path, const std::string& code) {
    if (dir.empty() || !(::mkdir(dir.c_str(), 0777) == 0 || errno == EEXIST)) return false;
    const std::string tmp = path + "." + std::to_string((long)getpid());
    bool ok = false;
    {
        std::ofstream f(tmp, std::ios::binary);
        if (f) {
            const CacheHeader h = {{'R', 'T', 'C', 'J', 'I', 'T', '1', 0}, (uint64_t)code.size(), fnv1a(code)};
            f.write((const char*)&h, sizeof(h));
            f.write(code.data(), (std::streamsize)code.size());
            f.close();
            ok = f.good();
        }
    }
    ok = ok && std::rename(tmp.c_str(), path.c_str()) == 0;
    if (!ok) (void)::unlink(tmp.c_str());
    return ok;
}
// The id names the code object itself: "spec_<hash of source, options, compiler>.<checksum of the compiled code>".  The second
// half is there because one source does not always give one binary: a hiprtc compile inside a process started under rocprofv3
// came out different from the same compile in a plain process (LABNOTES "Round 4": 436 against 484 B of scratch per lane, 421 M
// against 387 M VALU instructions a C3 frame), and a profile must never be quoted for a binary it did not measure.
inline std::string code_object_id(const std::string& cache_file, const std::string& code) {
    char sum[16];
    snprintf(sum, sizeof(sum), ".%08x", (unsigned)(fnv1a(code) & 0xffffffffu));
    return cache_file.substr(0, cache_file.rfind(".hsaco")) + sum;
}

}  // namespace rtc

#endif
