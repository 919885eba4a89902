/* Stand-alone check of the row generator of `frirl_demo --evaluate` (host/demo_rows.h) under ASan / UBSan: every unit lies in [-1, 1),
 * row 0 of every agent is the agent's own start (all zeros), the rows are keyed by the GLOBAL row (agent e of a run with K rows per
 * agent = the rows e * K .. e * K + K - 1 of the recurrence), and two runs give the same bits. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "demo_rows.h"

int main(void)
{
    const int agents = 37, K = 5, ns = 4;
    const size_t n = (size_t)agents * K * ns;
    double *a = malloc(sizeof(double) * n), *b = malloc(sizeof(double) * n);
    double lo = 1.0, hi = -1.0, sum = 0.0;
    int e, j, k, bad = 0;
    if (!a || !b) return 1;
    frirl_demo_row_units(agents, K, ns, a);
    frirl_demo_row_units(agents, K, ns, b);
    if (memcmp(a, b, sizeof(double) * n) != 0) { fprintf(stderr, "demo_rows: two runs differ\n"); bad = 1; }
    for (e = 0; e < agents; e++)
        for (j = 0; j < K; j++)
            for (k = 0; k < ns; k++) {
                const double v = a[((size_t)e * K + j) * ns + k];
                if (j == 0 && v != 0.0) { fprintf(stderr, "demo_rows: row 0 of agent %d is not the agent's own start\n", e); bad = 1; }
                if (j > 0 && v != frirl_demo_row_unit((uint64_t)e * K + j, k)) { fprintf(stderr, "demo_rows: agent %d row %d is not keyed by the global row\n", e, j); bad = 1; }
                if (!(v >= -1.0 && v < 1.0)) { fprintf(stderr, "demo_rows: unit %g outside [-1, 1)\n", v); bad = 1; }
                if (j > 0) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; sum += v; }
            }
    if (!(lo < -0.9 && hi > 0.9 && sum / (agents * (K - 1) * ns) > -0.1 && sum / (agents * (K - 1) * ns) < 0.1)) {
        fprintf(stderr, "demo_rows: units do not cover [-1, 1): min %g max %g mean %g\n", lo, hi, sum / (agents * (K - 1) * ns));
        bad = 1;
    }
    if (frirl_demo_row_unit(0xFFFFFFFFFFFFFFFFull, 15) < -1.0 || frirl_demo_row_unit(0, 0) >= 1.0) bad = 1;      /* the keys' edges */
    free(a); free(b);
    if (!bad) printf("demo_rows: ok (min %.4f max %.4f)\n", lo, hi);
    return bad;
}
