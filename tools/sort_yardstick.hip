// A yardstick for the sort phase of ray reordering (development tool, not linked into the library): rocPRIM's
// radix_sort_pairs on a file of u32 keys (tools/time_reorder.py --keys-out), values 0 .. n - 1, 32 key bits.
// hipcc --offload-arch=gfx950 -O2 -o tools/sort_yardstick tools/sort_yardstick.hip && tools/sort_yardstick keys.u32
#include <hip/hip_runtime.h>

#include <cstring>  // (rocprim's texture_cache_iterator.hpp calls memset without it)

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#define TRY(expr)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s failed: %s\n", #expr, hipGetErrorString(e_));         \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s keys.u32 [rounds]\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / sizeof(uint32_t);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> keys(n), idx(n);
    if (std::fread(keys.data(), sizeof(uint32_t), n, f) != n) {
        std::fprintf(stderr, "%s: short read\n", argv[1]);
        return 2;
    }
    std::fclose(f);
    if (n == 0 || n > 0x7fffffffu) {
        std::fprintf(stderr, "%zu keys\n", n);
        return 2;
    }
    std::iota(idx.begin(), idx.end(), 0u);
    const int rounds = argc > 2 ? std::max(1, std::atoi(argv[2])) : 10;
    uint32_t *k_in, *k_out, *v_in, *v_out;
    TRY(hipMalloc((void**)&k_in, n * 4));
    TRY(hipMalloc((void**)&k_out, n * 4));
    TRY(hipMalloc((void**)&v_in, n * 4));
    TRY(hipMalloc((void**)&v_out, n * 4));
    TRY(hipMemcpy(k_in, keys.data(), n * 4, hipMemcpyHostToDevice));
    TRY(hipMemcpy(v_in, idx.data(), n * 4, hipMemcpyHostToDevice));
    size_t temp_bytes = 0;
    TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, k_in, k_out, v_in, v_out, n, 0, 32));
    void* temp = nullptr;
    TRY(hipMalloc(&temp, temp_bytes));
    hipEvent_t e0, e1;
    TRY(hipEventCreate(&e0));
    TRY(hipEventCreate(&e1));
    std::vector<float> ms(rounds);
    for (int r = -2; r < rounds; r++) {  // two untimed sorts first
        TRY(hipEventRecord(e0, nullptr));
        TRY(rocprim::radix_sort_pairs(temp, temp_bytes, k_in, k_out, v_in, v_out, n, 0, 32));
        TRY(hipEventRecord(e1, nullptr));
        TRY(hipEventSynchronize(e1));
        if (r >= 0) TRY(hipEventElapsedTime(&ms[r], e0, e1));
    }
    // the permutation is the stable one: checked against the host's
    std::vector<uint32_t> got(n);
    TRY(hipMemcpy(got.data(), v_out, n * 4, hipMemcpyDeviceToHost));
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    const bool same = got == idx;
    std::sort(ms.begin(), ms.end());
    std::printf("rocprim::radix_sort_pairs, %zu (key, index) pairs, %zu B of temporary storage: %.3f (%.3f .. %.3f) ms over %d sorts; stable order: %s\n", n,
                temp_bytes, ms[rounds / 2], ms.front(), ms.back(), rounds, same ? "yes" : "NO");
    return same ? 0 : 1;
}
