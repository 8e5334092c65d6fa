// Host check of the quotient the split flux item forms from its reciprocal (flux_quot_adjust, vag_flux_limits.h): the boundary team
// steps its work items by AL / nk, AL = 64 * FLUX_SPLIT_A lanes, nk the window nodes of a row.  The kernel takes
// q = (int)((float)AL * rcp(nk)) from the hardware's approximate reciprocal (v_rcp_f32: one unit in the last place) and adjusts once
// each way.  Here: every nk of a lattice of up to 204 nodes, the reciprocal moved by up to four units in the last place either
// way; the estimate must stay within one of the quotient (what the adjustment assumes) and the adjusted value must be the quotient.
// Beyond that: every (a, n) up to 1024 with every estimate within one of the quotient.
#include <cmath>
#include <cstdio>

#include "../vegasafterglow_amd/csrc/vag_flux_limits.h"

int main() {
    constexpr int AL = vag::FLUX_SPLIT_A * 64;
    static_assert(AL == 384, "the team the issue was measured at");
    int fails = 0, cases = 0;
    for (int nk = 1; nk <= 204; ++nk) {
        const float r0 = 1.0f / (float)nk;
        for (int ulps = -4; ulps <= 4; ++ulps) {
            float r = r0;
            for (int s = 0; s < (ulps < 0 ? -ulps : ulps); ++s) r = std::nextafterf(r, ulps < 0 ? 0.0f : 2.0f);
            const int q = (int)((float)AL * r);
            const int want = AL / nk, got = vag::flux_quot_adjust(AL, nk, q);
            ++cases;
            if (q < want - 1 || q > want + 1 || got != want) {
                std::printf("FAIL nk=%d ulps=%d estimate=%d adjusted=%d want=%d\n", nk, ulps, q, got, want);
                ++fails;
            }
        }
    }
    for (int a = 1; a <= 1024; ++a)
        for (int n = 1; n <= 1024; ++n)
            for (int d = -1; d <= 1; ++d) {
                ++cases;
                if (vag::flux_quot_adjust(a, n, a / n + d) != a / n) {
                    if (fails < 20) std::printf("FAIL a=%d n=%d estimate=%d\n", a, n, a / n + d);
                    ++fails;
                }
            }
    std::printf("%s flux_quot_adjust: %d cases, %d failures\n", fails ? "FAIL" : "ok", cases, fails);
    return fails ? 1 : 0;
}
