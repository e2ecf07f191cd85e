// Device yardstick for the inbox sort (tools/inbox_bench.py): the time of
// hipcub::DeviceRadixSort::SortPairs over D (u32 key, u32 value) pairs whose
// keys are uniform in [0, max_key] -- the subscriber-id distribution of the
// bench workloads -- sorting only the bits max_key needs, as the engine does.
// Stand-alone: nothing in libemqx_tm.so uses hipcub.
//
//   hipcc --offload-arch=gfx950 -O3 -o inbox_sort_ref tools/inbox_sort_ref.hip
//   ./inbox_sort_ref D max_key [reps]      -> one JSON line
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define OK(expr)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "%s at line %d: %s\n", #expr, __LINE__, hipGetErrorString(e_)); \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

__global__ void fill_keys(uint32_t* keys, uint32_t* vals, uint64_t n, uint64_t range, uint64_t seed) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);   // splitmix64
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    keys[i] = (uint32_t)(((z >> 32) * range) >> 32);        // uniform in [0, range)
    vals[i] = (uint32_t)i;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s D max_key [reps]\n", argv[0]);
        return 2;
    }
    const uint64_t n = strtoull(argv[1], nullptr, 10);
    const uint64_t max_key = std::min<uint64_t>(strtoull(argv[2], nullptr, 10), 0xFFFFFFFFull);
    const int reps = argc > 3 ? std::max(1, atoi(argv[3])) : 10;
    if (!n || n > 0xFFFFFFF0ull) {
        fprintf(stderr, "D out of range\n");
        return 2;
    }
    int bits = 0;
    while (bits < 32 && (max_key >> bits)) ++bits;
    bits = std::max(bits, 1);
    uint32_t *k0, *k1, *v0, *v1;
    OK(hipMalloc((void**)&k0, n * 4)); OK(hipMalloc((void**)&k1, n * 4));
    OK(hipMalloc((void**)&v0, n * 4)); OK(hipMalloc((void**)&v1, n * 4));
    size_t tmp_bytes = 0;
    OK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k0, k1, v0, v1, n, 0, bits));
    void* tmp;
    OK(hipMalloc(&tmp, std::max<size_t>(tmp_bytes, 16)));
    hipEvent_t a, b;
    OK(hipEventCreate(&a)); OK(hipEventCreate(&b));
    std::vector<float> ms;
    for (int r = 0; r < reps + 2; ++r) {   // two warm-up rounds
        fill_keys<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(k0, v0, n, max_key + 1, 77);
        OK(hipGetLastError());
        OK(hipEventRecord(a));
        OK(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, k0, k1, v0, v1, n, 0, bits));
        OK(hipEventRecord(b));
        OK(hipEventSynchronize(b));
        float t;
        OK(hipEventElapsedTime(&t, a, b));
        if (r >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"pairs\": %llu, \"max_key\": %llu, \"bits\": %d, \"reps\": %d, \"hipcub_sort_pairs_ms\": "
           "{\"min\": %.4f, \"median\": %.4f, \"max\": %.4f}}\n",
           (unsigned long long)n, (unsigned long long)max_key, bits, reps, ms.front(), ms[ms.size() / 2], ms.back());
    OK(hipFree(k0)); OK(hipFree(k1)); OK(hipFree(v0)); OK(hipFree(v1)); OK(hipFree(tmp));
    return 0;
}
