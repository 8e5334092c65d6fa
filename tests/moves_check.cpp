// Stand-alone host check of the inline functions of csrc/vag_moves.h (the move mix of the device sampler), built by
// tests/test_moves_host.py with the system C++ compiler and AddressSanitizer + UndefinedBehaviorSanitizer.  Prints "ok <case>" per
// case that holds, "FAIL <case>" otherwise; the exit status is the number of failures.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../vegasafterglow_amd/csrc/vag_moves.h"

static int failures = 0;

static void report(const char* name, bool ok) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) ++failures;
}

static const uint32_t WORDS[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu, 0x12345678u, 0x9e3779b9u, 0x55555555u, 0xaaaaaaabu};
static const int N_WORDS = (int)(sizeof(WORDS) / sizeof(WORDS[0]));

static bool pairs_hold(int nh) {
    bool ok = true;
    for (int i = 0; i < N_WORDS; ++i)
        for (int j = 0; j < N_WORDS; ++j) {
            const vag::MovePair p = vag::move_pair(WORDS[i], WORDS[j], nh);
            ok = ok && p.a >= 0 && p.a < nh && p.b >= 0 && p.b < nh && p.a != p.b;
        }
    return ok;
}

static bool triples_hold(int nh) {
    bool ok = true;
    for (int i = 0; i < N_WORDS; ++i)
        for (int j = 0; j < N_WORDS; ++j)
            for (int k = 0; k < N_WORDS; ++k) {
                const vag::MoveTriple t = vag::move_triple(WORDS[i], WORDS[j], WORDS[k], nh);
                const vag::MovePair p = vag::move_pair(WORDS[i], WORDS[j], nh);
                ok = ok && t.z == p.a && t.z1 == p.b && t.z2 >= 0 && t.z2 < nh && t.z2 != t.z && t.z2 != t.z1;
            }
    return ok;
}

// every index of the half is reached: the third of a triple covers what the first two leave
static bool triple_covers(int nh) {
    bool ok = true;
    for (int a = 0; a < nh && ok; ++a) {
        const uint32_t xa = (uint32_t)((((uint64_t)a << 32) + (uint64_t)nh - 1) / (uint64_t)nh);  // the first word that gives a
        if (vag::stretch_partner(xa, nh) != a) return false;
        for (int off = 0; off < nh - 1 && ok; ++off) {
            const uint32_t xb = (uint32_t)((((uint64_t)off << 32) + (uint64_t)nh - 2) / (uint64_t)(nh - 1));
            bool seen[65] = {false};
            for (int c = 0; c < nh - 2; ++c) {
                const uint32_t xc = (uint32_t)((((uint64_t)c << 32) + (uint64_t)nh - 3) / (uint64_t)(nh - 2));
                const vag::MoveTriple t = vag::move_triple(xa, xb, xc, nh);
                ok = ok && !seen[t.z2];
                seen[t.z2] = true;
            }
            const vag::MovePair p = vag::move_pair(xa, xb, nh);
            int n_seen = 0;
            for (int s = 0; s < nh; ++s) n_seen += seen[s];
            ok = ok && n_seen == nh - 2 && !seen[p.a] && !seen[p.b];
        }
    }
    return ok;
}

int main() {
    report("pairs nh=2", pairs_hold(2));
    report("pairs nh=3", pairs_hold(3));
    report("pairs nh=65", pairs_hold(65));
    report("triples nh=3", triples_hold(3));
    report("triples nh=65", triples_hold(65));
    report("triples cover nh=3", triple_covers(3));
    report("triples cover nh=65", triple_covers(65));
    {   // words 0 and 0xffffffff by hand
        const vag::MovePair lo = vag::move_pair(0u, 0u, 65), hi = vag::move_pair(0xffffffffu, 0xffffffffu, 65);
        report("pair ends", lo.a == 0 && lo.b == 1 && hi.a == 64 && hi.b == 63);  // (64 + 1 + 63) mod 65
        const vag::MoveTriple t0 = vag::move_triple(0u, 0u, 0u, 65), t1 = vag::move_triple(0xffffffffu, 0xffffffffu, 0xffffffffu, 65);
        report("triple ends", t0.z2 == 2 && t1.z2 == 62);
        const vag::MovePair two = vag::move_pair(0xffffffffu, 0xffffffffu, 2);
        report("pair nh=2 top", two.a == 1 && two.b == 0);
    }
    const double top = vag::u53(0xffffffffu, 0xffffffffu);
    {   // the choice at the weight boundaries
        using vag::move_choice;
        report("choice reference mix", move_choice(0.0, 0.0, 0.8, 0.2) == vag::MOVE_DE && move_choice(std::nextafter(0.8, 0.0), 0.0, 0.8, 0.2) == vag::MOVE_DE &&
                                           move_choice(0.8, 0.0, 0.8, 0.2) == vag::MOVE_SNOOKER && move_choice(top, 0.0, 0.8, 0.2) == vag::MOVE_SNOOKER);
        report("choice stretch only", move_choice(0.0, 1.0, 0.0, 0.0) == vag::MOVE_STRETCH && move_choice(top, 1.0, 0.0, 0.0) == vag::MOVE_STRETCH &&
                                          move_choice(top, 3.0, 0.0, 0.0) == vag::MOVE_STRETCH && move_choice(top, 1.0 + 0x1p-52, 0.0, 0.0) == vag::MOVE_STRETCH);
        report("choice no snooker", move_choice(top, 0.8, 0.2, 0.0) == vag::MOVE_DE && move_choice(top, 1.0, 2.0, 0.0) == vag::MOVE_DE &&
                                        move_choice(top, 1e-300, 1e300, 0.0) == vag::MOVE_DE);
        report("choice zero first", move_choice(0.0, 0.0, 0.0, 1.0) == vag::MOVE_SNOOKER && move_choice(0.0, 0.0, 1.0, 0.0) == vag::MOVE_DE);
        report("choice zero middle", move_choice(0.5, 0.5, 0.0, 0.5) == vag::MOVE_SNOOKER && move_choice(std::nextafter(0.5, 0.0), 0.5, 0.0, 0.5) == vag::MOVE_STRETCH);
        report("choice unnormalised", move_choice(0.79, 0.0, 8.0, 2.0) == vag::MOVE_DE && move_choice(0.81, 0.0, 8.0, 2.0) == vag::MOVE_SNOOKER);
        report("choice thirds", move_choice(0.0, 1.0, 1.0, 1.0) == vag::MOVE_STRETCH && move_choice(0.34, 1.0, 1.0, 1.0) == vag::MOVE_DE &&
                                    move_choice(top, 1.0, 1.0, 1.0) == vag::MOVE_SNOOKER);
    }
    {   // the uniform of the choice is the first two words of counter (0, step lo, step hi, 3)
        const uint32_t ctr[4] = {0u, 5u, 1u, 3u}, key[2] = {7u, 256u};
        uint32_t x[4];
        vag::philox4x32_10(ctr, key, x);
        report("choice uniform", vag::move_choice_uniform(7u, 256u, (1ull << 32) + 5ull) == vag::u53(x[0], x[1]));
    }
    {   // the quantised normal at the ends of u1
        const double n0 = vag::de_quantise(vag::de_normal(0.0, 0.25));
        report("normal u1 zero", n0 == 0.0 && vag::de_gamma(0.5, 1e-5, n0) == 0.5);
        const double raw = vag::de_normal(top, 0.0), n1 = vag::de_quantise(raw);
        report("normal u1 top", std::isfinite(raw) && std::fabs(raw - std::sqrt(106.0 * std::log(2.0))) < 1e-12 && std::fabs(n1 - raw) <= 0x1p-21 &&
                                    n1 * 0x1p20 == std::rint(n1 * 0x1p20) && n1 * 0x1p20 < 0x1p24);
        const double n2 = vag::de_quantise(vag::de_normal(top, 0.5));
        report("normal u1 top negative", n2 == -n1);
        report("quantise ties to even", vag::de_quantise(0x1p-21) == 0.0 && vag::de_quantise(3 * 0x1p-21) == 0x1p-19 && vag::de_quantise(-0x1p-21) == 0.0);
    }
    report("gamma0", vag::de_gamma0(2) == 1.19 && vag::de_gamma0(8) == 0.595 && std::fabs(vag::de_gamma0(3) * vag::de_gamma0(3) * 6.0 - 2.38 * 2.38) < 1e-14);
    return failures;
}
