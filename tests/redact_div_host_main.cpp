// Host build of csrc/ss_redact_div.h (tests/test_redact_cpu.py): proves the blur's multiply-shift divider exact — for every radius
// r in 1 .. SS_REDACT_MAX_RADIUS and every window sum in [0, 255 k^2], k = 2r + 1, ss_redact_mean equals (sum + k^2 / 2) / k^2 in
// plain integer division — and checks ss_redact_reflect against a step-by-step walk.  stdout: one line "ok <sums checked>" or the
// first disagreement; the exit code is 0 only when everything agrees.
#include <cstdio>

#include "../strongsort_yolo_amd/csrc/ss_redact_div.h"

static int walk(int i, int n)            // reflect-101 by walking: bounce between 0 and n - 1
{
    if (n == 1) return 0;
    int pos = 0, dir = 1;
    for (int s = i < 0 ? -i : i; s > 0; --s) {
        if (pos + dir < 0 || pos + dir >= n) dir = -dir;
        pos += dir;
    }
    return pos;                          // (symmetric about 0: index -i is index i)
}

int main()
{
    unsigned long long checked = 0;
    for (int r = 1; r <= SS_REDACT_MAX_RADIUS; ++r) {
        const uint32_t d = (uint32_t)((2 * r + 1) * (2 * r + 1)), m = ss_redact_div_magic(r);
        for (uint32_t sum = 0; sum <= 255u * d; ++sum, ++checked) {
            const uint32_t want = (sum + d / 2) / d, got = ss_redact_mean(sum, d, m);
            if (got != want) { printf("r %d sum %u: %u, not %u\n", r, sum, got, want); return 1; }
        }
    }
    for (int n = 1; n <= 9; ++n)
        for (int i = -80; i <= 80; ++i)
            if (ss_redact_reflect(i, n) != walk(i, n)) { printf("reflect(%d, %d) = %d, not %d\n", i, n, ss_redact_reflect(i, n), walk(i, n)); return 1; }
    printf("ok %llu\n", checked);
    return 0;
}
