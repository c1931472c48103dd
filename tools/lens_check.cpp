// lens_check -- rtc_lens_rays and the lens's argument checks (rtc_host.cpp) as a host program of its own: no device, no HIP header,
// so that the host code which writes through caller pointers by rows and columns runs under the host sanitizers.
//
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       -Iray_tracer_challenge_amd/csrc tools/lens_check.cpp ray_tracer_challenge_amd/csrc/rtc_host.cpp -o tools/lens_check
//   tools/lens_check                                       (prints "lens: ok"; exit status 1 and every difference otherwise)
//
// Buffers are allocated to the byte (a row too many, a column too many is a heap overflow the sanitizer reports); every argument
// error must leave them untouched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rtc.h"

static int g_failures = 0;
static void expect(bool ok, const char* what) {
    if (ok) return;
    g_failures++;
    std::fprintf(stderr, "lens_check: %s (%s)\n", what, rtc_last_error());
}

int main() {
    const float from[4] = {-2.6f, 1.5f, -3.9f, 1.0f}, to[4] = {-0.6f, 1.0f, -0.8f, 1.0f}, up[4] = {0.0f, 1.0f, 0.0f, 0.0f};
    float view[16];
    rtc_view_transform(from, to, up, view);
    rtc_camera cam;
    expect(rtc_camera_new(26, 18, 1.0471976f, view, &cam) == RTC_OK, "rtc_camera_new");
    const rtc_lens lens = {0.35f, 4.25f, 7u};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t k : {2u, 4u}) {
        const uint32_t fw = k * cam.width, fh = k * cam.height;
        std::vector<float> whole_o((size_t)fw * fh * 4), whole_d((size_t)fw * fh * 4);
        expect(rtc_lens_rays(&cam, k, &lens, 0, fh, whole_o.data(), whole_d.data()) == RTC_OK, "the whole frame");
        for (size_t i = 0; i < whole_o.size(); i++) expect(std::isfinite(whole_o[i]) && std::isfinite(whole_d[i]), "a ray that is not finite");
        // rows of the frame, into buffers of exactly their size; either buffer alone; no rows at all
        for (uint32_t y0 : {0u, 5u, fh - 1u}) {
            const uint32_t n = y0 == 5u ? 7u : 1u;
            std::vector<float> o((size_t)n * fw * 4), d((size_t)n * fw * 4);
            expect(rtc_lens_rays(&cam, k, &lens, y0, n, o.data(), d.data()) == RTC_OK, "some rows");
            expect(std::memcmp(o.data(), whole_o.data() + (size_t)y0 * fw * 4, o.size() * sizeof(float)) == 0, "rows differ from the frame's (origins)");
            expect(std::memcmp(d.data(), whole_d.data() + (size_t)y0 * fw * 4, d.size() * sizeof(float)) == 0, "rows differ from the frame's (directions)");
            std::vector<float> only((size_t)n * fw * 4);
            expect(rtc_lens_rays(&cam, k, &lens, y0, n, nullptr, only.data()) == RTC_OK && only == d, "directions alone");
            expect(rtc_lens_rays(&cam, k, &lens, y0, n, only.data(), nullptr) == RTC_OK && only == o, "origins alone");
        }
        expect(rtc_lens_rays(&cam, k, &lens, fh, 0, nullptr, nullptr) == RTC_OK, "no rows");
        // argument errors write nothing: one float, which must stay what it is
        float canary_o = 42.0f, canary_d = 43.0f;
        expect(rtc_lens_rays(&cam, k, &lens, fh, 1, &canary_o, &canary_d) == RTC_ERR_INVALID_ARG, "a row beyond the frame");
        expect(rtc_lens_rays(&cam, k, &lens, 0xffffffffu, 2, &canary_o, &canary_d) == RTC_ERR_INVALID_ARG, "rows that wrap");
        expect(rtc_lens_rays(&cam, k, nullptr, 0, 1, &canary_o, &canary_d) == RTC_ERR_INVALID_ARG, "a null lens");
        expect(rtc_lens_rays(nullptr, k, &lens, 0, 1, &canary_o, &canary_d) == RTC_ERR_INVALID_ARG, "a null camera");
        for (float r : {-0.5f, -inf, inf, nan}) {
            const rtc_lens bad = {r, 1.0f, 0u};
            expect(rtc_lens_rays(&cam, k, &bad, 0, 1, &canary_o, &canary_d) == RTC_ERR_INVALID_ARG, "a bad aperture");
        }
        for (float f : {0.0f, -1.0f, inf, nan}) {
            const rtc_lens bad = {0.1f, f, 0u};
            expect(rtc_lens_rays(&cam, k, &bad, 0, 1, &canary_o, &canary_d) == RTC_ERR_INVALID_ARG, "a bad focal distance");
        }
        expect(canary_o == 42.0f && canary_d == 43.0f, "an argument error wrote through a pointer");
    }
    float canary = 1.0f;
    for (uint32_t k : {0u, 1u, 3u, 8u, 0xffffffffu})
        expect(rtc_lens_rays(&cam, k, &lens, 0, 1, &canary, &canary) == RTC_ERR_INVALID_ARG && canary == 1.0f, "a factor that is not 2 or 4");
    rtc_camera big = cam;
    big.width = big.height = 40000u;
    expect(rtc_lens_rays(&big, 4, &lens, 0, 1, &canary, &canary) == RTC_ERR_INVALID_ARG && canary == 1.0f, "a fine frame beyond 2^32 pixels");
    // an aperture of zero: every ray leaves the camera's origin
    std::vector<float> o((size_t)2 * cam.width * 4);
    const rtc_lens pinhole = {0.0f, 2.0f, 1u};
    expect(rtc_lens_rays(&cam, 2, &pinhole, 3, 1, o.data(), nullptr) == RTC_OK, "a pinhole");
    for (size_t i = 4; i < o.size(); i++) expect(o[i] == o[i % 4], "a pinhole's origins differ");
    if (g_failures) return 1;
    std::printf("lens: ok\n");
    return 0;
}
