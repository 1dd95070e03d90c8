// Exhaustive check of the absorption stage's exponential (computational_ray_tracer_amd/csrc/rt_medium.h
// medium_exp_neg) against its definition, (float)exp(-(double)x) with glibc, over EVERY float x in [0, 87): the range
// medium_transmittance feeds it (x >= 87 gives 0 without an exponential).  rtm::exp_tab's comment vouches for
// |x| <= 2.3 only; this is the check that it holds up to 87.  For each input the function either took the library call
// (near a float rounding midpoint: counted) or must return the same float as the library value.  Prints the counts; exit
// status 1 on any mismatch.
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread tools/verify_absorb.cpp -o /tmp/verify_absorb && /tmp/verify_absorb [stride]
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../computational_ray_tracer_amd/csrc/rt_medium.h"

static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

int main(int argc, char** argv) {
    uint32_t stride = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 1;
    if (stride < 1) stride = 1;
    const uint32_t end = f2u(rtmi::kMediumCut);  // bit patterns [0, end): +0 up to the float below 87
    int nt = (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    std::atomic<uint64_t> n{0}, fallback{0}, bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            uint64_t ln = 0, lf = 0, lb = 0;
            for (uint64_t i = (uint64_t)t * stride; i < end; i += (uint64_t)nt * stride) {
                const float x = u2f((uint32_t)i);
                int fb = 0;
                const float f = rtmi::medium_exp_neg(x, &fb);
                ++ln;
                lf += fb;
                lb += f2u(f) != f2u((float)std::exp(-(double)x));
            }
            n += ln; fallback += lf; bad += lb;
        });
    for (auto& t : th) t.join();
    std::printf("exp(-x): x in [0, %.9g) stride %u: %llu inputs, %llu near-midpoint (library), %llu mismatches\n",
                rtmi::kMediumCut, stride, (unsigned long long)n.load(), (unsigned long long)fallback.load(),
                (unsigned long long)bad.load());
    return bad ? 1 : 0;
}
