// Host-only check of ExactDiv (csrc/common.h): the multiply-high quotient the channel-last gather uses for idx / S equals the integer division for
// EVERY divisor 2..8192 at the multiples of the divisor and their neighbours spread over [0, 2^31 - 1], and d = 1 through div().
// Compiled and run by tests/test_gather_cases_host.py; prints one line and returns 0 when every quotient is right.
#include "../uc_nerf_amd/csrc/common.h"

#include <cstdio>

int main() {
    using ucnerf::ExactDiv;
    const unsigned top = 0x7fffffffu;
    unsigned long long checked = 0;
    auto check = [&](const ExactDiv& q, unsigned d, unsigned x, bool through_div) {
        const unsigned got = through_div ? q.div(x) : q.quot(x);
        ++checked;
        if (got == x / d) return true;
        std::printf("ExactDiv(%u): %u / %u = %u, got %u\n", d, x, d, x / d, got);
        return false;
    };
    for (unsigned d = 1; d <= 8192; ++d) {
        const ExactDiv q(d);
        const bool through_div = d == 1;                       // (quot() is for d >= 2: the kernels keep their own test for a divisor of 1)
        if (!check(q, d, 0, through_div) || !check(q, d, top, through_div)) return 1;
        const unsigned k_max = top / d;                        // largest k with k * d <= 2^31 - 1
        const unsigned steps = 400;
        for (unsigned i = 0; i <= steps; ++i) {
            // k spread over [1, k_max]: dense at the bottom (i^3 law), the top included
            const double t = (double)i / steps;
            unsigned k = 1 + (unsigned)((double)(k_max - 1) * t * t * t);
            if (i == steps || k > k_max) k = k_max;
            const unsigned long long kd = (unsigned long long)k * d;
            if (!check(q, d, (unsigned)(kd - 1), through_div) || !check(q, d, (unsigned)kd, through_div)) return 1;
            if (kd + 1 <= top && !check(q, d, (unsigned)(kd + 1), through_div)) return 1;
        }
    }
    std::printf("ExactDiv ok: %llu quotients, divisors 1..8192\n", checked);
    return 0;
}
