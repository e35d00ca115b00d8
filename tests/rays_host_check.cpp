// Host-only companion of tests/rays_cases.py: the device headers of the ray front end compiled for the CPU (with -ffp-contract=off, as the
// library), so that the numpy restatement can be held bit for bit against the very code the kernels run, without a GPU.  Writes to argv[1]:
//   int32 n_fma, n_lin, n_sc, then
//   float[n_fma][4]   (a, b, c, std::fmaf(a, b, c)): random bit patterns, near-cancelling sums, and constructed half-way cases -- a * b sits
//                     exactly on a float32 tie and c is a non-zero residual far below it, so float64(a * b + c) lands ON the tie;
//   float[n_lin]      linspace01(i, S), i = 0..S-1, for S = 1..300, 512, 768 (raygen_device.h);
//   float[n_sc][3]    (r, sin, cos) of sincos_pe_fast (sincos_cw.h) for |r| <= 65536: random, and around multiples of pi/4.
// Compiled and run by tests/test_rays_cases_host.py; prints one line and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// the hardware sin / cos path of sincos_cw.h is not under test here (and has no host form): stand-ins so that the header parses
#define __builtin_amdgcn_fractf(x) ((x) - std::floor(x))
#define __builtin_amdgcn_sinf(x) std::sin(6.283185307179586f * (x))
#define __builtin_amdgcn_cosf(x) std::cos(6.283185307179586f * (x))
#include "../uc_nerf_amd/csrc/raygen_device.h"
#include "../uc_nerf_amd/csrc/sincos_cw.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t next() {                                       // splitmix64, upper half
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static float uniform() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }      // [0, 1), 24 bits

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<float> fma, lin, sc;
    auto triple = [&](float a, float b, float c) {
        volatile float va = a, vb = b, vc = c;                 // (nothing folded at compile time)
        fma.push_back(a); fma.push_back(b); fma.push_back(c); fma.push_back(std::fmaf(va, vb, vc));
    };
    for (int i = 0; i < 400000; ++i) {                         // any finite bit patterns
        uint32_t u[3];
        for (auto& x : u) { do x = next(); while ((x & 0x7f800000u) == 0x7f800000u); }
        triple(from_bits(u[0]), from_bits(u[1]), from_bits(u[2]));
    }
    for (int i = 0; i < 400000; ++i) {                         // ordinary magnitudes, c close to -a b (the Cody-Waite steps are of this kind)
        const float a = (uniform() - 0.5f) * 64.f, b = (uniform() - 0.5f) * 64.f;
        const float c = -(a * b) * (1.0f + (uniform() - 0.5f) * from_bits(0x33800000u + ((next() % 12) << 23)));
        triple(a, b, c);
    }
    for (int i = 0; i < 200000; ++i) {                         // |c| of the product's size: the sum's rounding decides
        const float a = (uniform() - 0.5f) * 4.f, b = (uniform() - 0.5f) * 4.f;
        triple(a, b, (uniform() - 0.5f) * 16.f);
    }
    for (int i = 0; i < 200000; ++i) {                         // half-way cases: odd m1 m2 in [2^24, 2^25) is a 25-bit number, a tie of the 24-bit grid
        const uint32_t m1 = 4097 + 2 * (next() % 847), m2 = 4097 + 2 * (next() % 847);      // both odd, < 5791: m1 m2 < 2^25
        const int e = (int)(next() % 40) - 20;
        const float a = std::ldexp((float)m1, e), b = std::ldexp((float)m2, -12);
        float c = std::ldexp(1.0f + uniform(), e - 12 + 24 - 30 - (int)(next() % 30));     // far below the tie's last bit
        if (next() & 1) c = -c;
        if (next() & 1) triple(-a, b, c); else triple(a, b, c);
    }
    for (int S = 1; S <= 302; ++S) {
        const int s = S == 301 ? 512 : S == 302 ? 768 : S;
        for (int i = 0; i < s; ++i) lin.push_back(ucnerf::linspace01(i, s));
    }
    auto one = [&](float r) {
        if (!(std::fabs(r) <= ucnerf::SINCOS_FAST_MAX)) return;
        float s, c;
        ucnerf::sincos_pe_fast(r, &s, &c);
        sc.push_back(r); sc.push_back(s); sc.push_back(c);
    };
    for (int i = 0; i < 700000; ++i) one((uniform() - 0.5f) * 131072.f);
    for (int i = 0; i < 200000; ++i) one((uniform() - 0.5f) * 16.f);
    for (int k = -83442; k <= 83442; ++k) {                    // around every multiple of pi/4 in range
        const float r = (float)(k * 0.78539816339744831);
        one(r); one(std::nextafter(r, 1e30f)); one(std::nextafter(r, -1e30f));
    }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    const int32_t head[3] = {(int32_t)(fma.size() / 4), (int32_t)lin.size(), (int32_t)(sc.size() / 3)};
    std::fwrite(head, 4, 3, f);
    std::fwrite(fma.data(), 4, fma.size(), f);
    std::fwrite(lin.data(), 4, lin.size(), f);
    std::fwrite(sc.data(), 4, sc.size(), f);
    std::fclose(f);
    std::printf("rays host check ok: %d fmaf, %d linspace, %d sincos\n", head[0], head[1], head[2]);
    return 0;
}
