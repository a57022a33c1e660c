// check_text_digits.cpp -- the shared float32 formatter of the device text export (csrc/sph_text.hpp) against the host writer's
// sphexp::format_f32 (csrc/sph_export.hpp: std::to_chars) for every float32 bit pattern, on the CPU.
//
//   g++ -O2 -std=c++17 -pthread tools/check_text_digits.cpp -o check_text_digits && ./check_text_digits > profiles/text_digits_exhaustive.txt
//   ./check_text_digits STRIDE     every STRIDE-th pattern (e.g. a build with -fsanitize=address,undefined)
//
// Compares the characters, their number against text_f32_len, and checks that nothing is written past TEXT_F32_MAX.  Prints the number
// of differences (0 = the two agree everywhere) and exits 1 if there is one.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../sph_project_amd/csrc/sph_export.hpp"
#include "../sph_project_amd/csrc/sph_text.hpp"

int main(int argc, char **argv) {
    const uint64_t stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    if (stride < 1) { fprintf(stderr, "stride must be >= 1\n"); return 2; }
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    std::atomic<uint64_t> differences{0}, checked{0}, first_bad{~0ull};
    std::atomic<int> longest{0};
    const uint64_t total = 1ull << 32, per = (total + nthreads - 1) / nthreads;
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t] {
            uint64_t lo = t * per, hi = lo + per < total ? lo + per : total;
            lo = (lo + stride - 1) / stride * stride;
            uint64_t bad = 0, n = 0, fb = ~0ull;
            int lmax = 0;
            for (uint64_t b = lo; b < hi; b += stride) {
                const uint32_t bits = (uint32_t)b;
                float v;
                memcpy(&v, &bits, 4);
                char ref[64], got[TEXT_F32_MAX + 8];
                memset(got, '#', sizeof(got));
                const int nr = sphexp::format_f32(v, ref);
                const int ng = text_f32(bits, got);
                bool same = nr == ng && ng <= TEXT_F32_MAX && ng == text_f32_len(bits) && memcmp(ref, got, (size_t)nr) == 0;
                for (int k = ng < 0 ? 0 : ng; same && k < (int)sizeof(got); ++k) same = got[k] == '#';
                if (!same) { ++bad; if (fb == ~0ull) fb = b; }
                if (ng > lmax) lmax = ng;
                ++n;
            }
            differences += bad;
            checked += n;
            int cur = longest.load();
            while (lmax > cur && !longest.compare_exchange_weak(cur, lmax)) {}
            uint64_t f = first_bad.load();
            while (fb < f && !first_bad.compare_exchange_weak(f, fb)) {}
        });
    for (auto &th : pool) th.join();
    printf("float32 bit patterns checked: %llu (stride %llu, %u threads)\n", (unsigned long long)checked.load(), (unsigned long long)stride, nthreads);
    printf("reference: sphexp::format_f32 (std::to_chars, scientific, shortest round-trip)\n");
    printf("longest result: %d characters (TEXT_F32_MAX %d)\n", longest.load(), TEXT_F32_MAX);
    if (differences.load()) printf("first differing bit pattern: 0x%08llX\n", (unsigned long long)first_bad.load());
    printf("differences: %llu\n", (unsigned long long)differences.load());
    return differences.load() ? 1 : 0;
}
