// dispatch_driver.cpp - rq::dispatch_bools (raptor_amd/csrc/rq_dispatch.hpp) under a plain host compiler: for each of the 16 values of
// four run-time bools the callable must be entered exactly once, with exactly those four values as compile-time constants, in the
// order they were given.  Driven by tests/test_capi_cpu.py; exit status 0 and "ok 16" on success.
#include <cstdio>

#include "rq_dispatch.hpp"

template <bool A, bool B, bool C, bool D>
struct Got { static constexpr int code = (A ? 1 : 0) | (B ? 2 : 0) | (C ? 4 : 0) | (D ? 8 : 0); };

int main() {
    int bad = 0;
    for (int want = 0; want < 16; ++want) {
        int calls = 0, got = -1;
        rq::dispatch_bools([&](auto a, auto b, auto c, auto d) {
            // template arguments: the values are constants of the arguments' TYPES, not run-time copies
            got = Got<decltype(a)::value, decltype(b)::value, decltype(c)::value, decltype(d)::value>::code;
            ++calls;
        }, (want & 1) != 0, (want & 2) != 0, (want & 4) != 0, (want & 8) != 0);
        if (calls != 1 || got != want) { std::printf("bools %d: %d call(s), constants %d\n", want, calls, got); ++bad; }
    }
    // the ends of the recursion: no bool at all, and one
    int none = 0, one = 0;
    rq::dispatch_bools([&] { ++none; });
    rq::dispatch_bools([&](auto a) { one += decltype(a)::value ? 1 : 100; }, true);
    rq::dispatch_bools([&](auto a) { one += decltype(a)::value ? 100 : 10; }, false);
    if (none != 1 || one != 11) { std::printf("edge cases: none %d, one %d\n", none, one); ++bad; }
    if (bad) return 1;
    std::printf("ok 16\n");
    return 0;
}
