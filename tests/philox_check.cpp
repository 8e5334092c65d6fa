// Stand-alone host check of csrc/vag_philox.h (the draws of the device sampler), built by tests/test_sampler_host.py with the system
// C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer.  Prints "ok <case>" per case that holds, "FAIL <case>" otherwise;
// the exit status is the number of failures.
#include <cstdint>
#include <cstdio>

#include "../vegasafterglow_amd/csrc/vag_philox.h"

static int failures = 0;

static void report(const char* name, bool ok) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) ++failures;
}

static bool vector_is(const uint32_t (&ctr)[4], const uint32_t (&key)[2], const uint32_t (&want)[4]) {
    uint32_t out[4];
    vag::philox4x32_10(ctr, key, out);
    return out[0] == want[0] && out[1] == want[1] && out[2] == want[2] && out[3] == want[3];
}

int main() {
    // the known-answer vectors of Random123 (kat_vectors: philox4x32 10)
    report("vector zeros", vector_is({0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}));
    report("vector ones", vector_is({0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
                                    {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}));
    report("vector pi", vector_is({0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
                                  {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}));
    {   // in place: out may be the counter
        uint32_t c[4] = {0, 0, 0, 0};
        const uint32_t k[2] = {0, 0};
        vag::philox4x32_10(c, k, c);
        report("vector in place", c[0] == 0x6627e8d5u && c[3] == 0x9b00dbd8u);
    }
    report("u53 zero", vag::u53(0, 0) == 0.0);
    const double top = vag::u53(0xffffffffu, 0xffffffffu);
    report("u53 top", top == 1.0 - 0x1p-53);
    report("partner top", vag::stretch_partner(0xffffffffu, 65) == 64);
    report("partner zero", vag::stretch_partner(0u, 65) == 0);
    report("stretch_z low", vag::stretch_z(2.0, 0.0) == 0.5);
    report("stretch_z high", vag::stretch_z(2.0, top) < 2.0);
    return failures;
}
