// jit_check -- rtc_jit.h (the scene-kernel JIT's plan and its disk-cache entries) as a host program of its own: no device, no HIP
// header, so that the one piece of host code that reads files it did not write runs under the host sanitizers.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iray_tracer_challenge_amd/csrc
//       tools/jit_check.cpp -o tools/jit_check                                                     (one command)
//   tools/jit_check [scratch directory, default /tmp]     (prints "jit: ok"; exit status 1 and every difference otherwise)
//
// The cache-entry cases are those of tests/test_jit_plan.py: publish then read, every truncation, one flipped byte in each field,
// a size field of 2^63, a foreign file, a missing directory, a directory that is a regular file.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rtc_jit.h"

using namespace rtc;

// rtc_internal.h's error reporting, which the library defines in rtc_host.cpp
namespace rtc {
rtc_status fail(rtc_status st, const char*, ...) { return st; }
}  // namespace rtc

static int g_failures = 0;
static void expect(bool ok, const char* what) {
    if (ok) return;
    g_failures++;
    std::fprintf(stderr, "jit_check: %s\n", what);
}
static void write_file(const std::string& path, const std::string& bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write(bytes.data(), (std::streamsize)bytes.size());
}
static bool exists(const std::string& path) {
    struct stat st;
    return ::stat(path.c_str(), &st) == 0;
}

static void cache_entries(const std::string& scratch) {
    const std::string dir = scratch + "/jit_check." + std::to_string((long)getpid()), path = dir + "/spec_0123456789abcdef.hsaco";
    const std::string tmp = path + "." + std::to_string((long)getpid());
    std::string payload(5000, '\0');
    for (size_t i = 0; i < payload.size(); i++) payload[i] = (char)((i * 2654435761u) >> 13);
    std::string code;
    expect(!exists(dir) && publish_cache_entry(dir, path, payload), "a missing directory is created and the entry published");
    expect(read_cache_entry(path, &code) && code == payload, "publish then read returns the payload");
    expect(!exists(tmp), "no temporary file is left");
    std::string entry;
    expect(read_file(path, &entry) && entry.size() == sizeof(CacheHeader) + payload.size(), "an entry is its header and the code");
    const size_t H = sizeof(CacheHeader);
    for (size_t n : {(size_t)0, (size_t)1, H - 1, H, H + 1, entry.size() / 3, entry.size() - 1}) {
        write_file(path, entry.substr(0, n));
        expect(!read_cache_entry(path, &code), "a truncated entry is rejected");
    }
    for (size_t at : {(size_t)3, (size_t)9, (size_t)17, H + 1234}) {  // magic, size, checksum, payload
        std::string damaged = entry;
        damaged[at] ^= 0x10;
        write_file(path, damaged);
        expect(!read_cache_entry(path, &code), "one flipped byte is rejected");
    }
    {
        std::string huge = entry;
        const uint64_t size = 1ull << 63;
        std::memcpy(&huge[8], &size, 8);
        write_file(path, huge);
        expect(!read_cache_entry(path, &code), "a size field of 2^63 is rejected");
    }
    write_file(path, "\x7f" "ELF" + payload);
    expect(!read_cache_entry(path, &code), "a foreign file is rejected");
    expect(!read_cache_entry(dir + "/nothing.hsaco", &code), "a file that is not there is rejected");
    expect(!read_cache_entry(dir, &code), "a directory is rejected");
    write_file(path, entry);
    expect(read_cache_entry(path, &code) && code == payload, "the whole entry is read again");
    // a directory that is a regular file: nothing published, nothing left behind
    const std::string file_dir = dir + "/plain";
    write_file(file_dir, "x");
    expect(!publish_cache_entry(file_dir, file_dir + "/spec.hsaco", payload), "a directory that is a regular file publishes nothing");
    expect(!exists(file_dir + "/spec.hsaco") && !exists(file_dir + "/spec.hsaco." + std::to_string((long)getpid())), "... and leaves nothing");
    expect(!publish_cache_entry("", "/spec.hsaco", payload), "no directory: nothing published");
    expect(code_object_id("spec_0123456789abcdef.hsaco", "") == "spec_0123456789abcdef.739d0383", "the id of an empty code object");
    (void)::unlink(path.c_str()), (void)::unlink(file_dir.c_str()), (void)::rmdir(dir.c_str());
}

static void plans() {
    const JitArgSizes sizes = {312, 96, 104};
    const std::vector<std::string> fixed = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize"};
    auto with = [&](std::vector<std::string> more) {
        std::vector<std::string> v = fixed;
        v.insert(v.end(), more.begin(), more.end());
        return v;
    };
    const std::string core = "core text\n", beside = "beside text\n";
    for (const char* flags : {"", " ", "   \t  "}) {  // no options, no flags (or only spaces): the fixed options and the default occupancy
        const JitPlan p = plan_jit({}, JitKind::RENDER, flags, 7, 1, sizes, core, beside);
        expect(p.opts == with({"-DRTC_WAVES_PER_SIMD=7"}), "empty options: the fixed five and the default waves per SIMD");
        std::string key;
        for (const auto& o : p.opts) key += o + "\n";
        expect(p.key_text == key + "hiprtc 7.1 abi " + std::to_string(RTC_ABI_VERSION) + " args 312\n", "empty options: key text");
        expect(p.source_hash == fnv1a(p.key_text, fnv1a(core)), "a render kernel's hash leaves the header beside the core out");
        expect(std::string(p.entry) == "render_kernel_spec" && p.cache_file.size() == 27 && p.cache_file.rfind("spec_", 0) == 0, "entry and file name");
    }
    const std::string big = "-DRTC_SPEC_LIST=" + std::string(4096, '7');
    const JitPlan t = plan_jit({big, "-DRTC_WAVES_PER_SIMD=5", "-DRTC_SPEC_TRACE=1"}, JitKind::TRACE, " -DA=1  -mB ", 7, 1, sizes, core, beside);
    expect(t.opts == with({big, "-DRTC_WAVES_PER_SIMD=5", "-DRTC_SPEC_TRACE=1", "-DA=1", "-mB"}), "a 4 KB option, given waves, split flags");
    expect(t.key_text.size() > 4096 && t.key_text.rfind("args 312\ntrace args 96\n") == t.key_text.size() - 23, "a stream's key names TraceArgs");
    expect(t.source_hash == fnv1a(beside, fnv1a(t.key_text, fnv1a(core))) && std::string(t.entry) == "trace_kernel_spec", "a stream's hash and entry");
    const JitPlan a = plan_jit({"-DRTC_SPEC_ADAPTIVE=4"}, JitKind::ADAPTIVE, "", 7, 1, sizes, core, beside);
    expect(a.key_text.rfind("args 312\nadaptive args 104\n") == a.key_text.size() - 27, "a refinement's key names AdaptiveRefineArgs");
    const JitPlan s = plan_jit({"-DRTC_SPEC_SS=2"}, JitKind::SS, "", 7, 1, sizes, core, beside);
    expect(s.key_text.rfind("args 312\n") == s.key_text.size() - 9 && std::string(s.entry) == "ss_render_kernel_spec", "a supersampling kernel's key and entry");
    char want[64];
    snprintf(want, sizeof(want), "aot_%016llx", (unsigned long long)fnv1a(core));
    expect(aot_kernel_id(JitKind::RENDER, 1u, core, beside) == want, "aot id: render");
    snprintf(want, sizeof(want), "aot_ss4_%016llx", (unsigned long long)fnv1a(beside, fnv1a(core)));
    expect(aot_kernel_id(JitKind::SS, 4u, core, beside) == want, "aot id: ss4");
    snprintf(want, sizeof(want), "aot_trace_%016llx", (unsigned long long)fnv1a(beside, fnv1a(core)));
    expect(aot_kernel_id(JitKind::TRACE, 1u, core, beside) == want, "aot id: trace");
    snprintf(want, sizeof(want), "aot_adaptive2_%016llx", (unsigned long long)fnv1a(beside, fnv1a(core)));
    expect(aot_kernel_id(JitKind::ADAPTIVE, 2u, core, beside) == want, "aot id: adaptive2");
}

int main(int argc, char** argv) {
    cache_entries(argc > 1 ? argv[1] : "/tmp");
    plans();
    if (g_failures) return 1;
    std::puts("jit: ok");
    return 0;
}
