// Host check of csrc/knp_dispatch.hpp (tests/test_dispatch_host.py compiles and runs it, under ASan/UBSan where they link).
// One line per call, for the test to judge:
//   lanes LO HI n calls got clamp      with_lanes<LO, HI>(n, f): times f ran, the constant it received, clamp_lanes<LO, HI>(n)
//   flag b calls_true calls_false      with_flag(b, f)
//   either A B first calls got         with_either<A, B>(first, f), the three pairs the launchers use
#include <cstdio>

#include "knp_dispatch.hpp"

static_assert(clamp_lanes<2, 64>(8) == 8 && clamp_lanes<4, 32>(2) == 32 && clamp_lanes<2, 16>(16) == 16, "clamp_lanes is a constant expression");

template <int LO, int HI>
static void sweep() {
    for (int n = -2; n <= 130; ++n) {
        int calls = 0, got = 0;
        with_lanes<LO, HI>(n, [&](auto L) {
            static_assert(L() >= LO && L() <= HI, "only LO .. HI are instantiated");
            ++calls;
            got = L();
        });
        std::printf("lanes %d %d %d %d %d %d\n", LO, HI, n, calls, got, clamp_lanes<LO, HI>(n));
    }
}

template <int A, int B>
static void either(bool first) {
    int calls = 0, got = 0;
    with_either<A, B>(first, [&](auto V) { ++calls; got = V(); });
    std::printf("either %d %d %d %d %d\n", A, B, first ? 1 : 0, calls, got);
}

int main() {
    sweep<2, 16>();
    sweep<2, 32>();
    sweep<2, 64>();
    sweep<4, 32>();
    for (int b = 0; b < 2; ++b) {
        int t = 0, f = 0;
        with_flag(b != 0, [&](auto B) { if (B()) ++t; else ++f; });
        std::printf("flag %d %d %d\n", b, t, f);
        either<1, 2>(b != 0);
        either<2, 3>(b != 0);
        either<3, 8>(b != 0);
    }
    return 0;
}
