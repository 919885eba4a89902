/*
 * demo_rows.h -- the start states of `frirl_demo --evaluate K`: a fixed integer recurrence keyed by the GLOBAL row e * K + j and the
 * state dimension (SplitMix64's output function on a Weyl sequence), not rand(): the same rows on every machine and for every sharding.
 */
#ifndef FRIRL_DEMO_ROWS_H
#define FRIRL_DEMO_ROWS_H

#include <stdint.h>

/* offset of state dimension k of global row `row` in units of spread * span: uniform in [-1, 1) */
static double frirl_demo_row_unit(uint64_t row, int k)
{
    uint64_t z = (row + 1u) * 0x9E3779B97F4A7C15ull + (uint64_t)(k + 1) * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;      /* 53 bits * 2^-52 - 1 */
}

/* units [agents][K][ns]; row 0 of every agent is all zeros: the agent's own start state */
static void frirl_demo_row_units(int agents, int K, int ns, double *units)
{
    int e, j, k;
    for (e = 0; e < agents; e++)
        for (j = 0; j < K; j++)
            for (k = 0; k < ns; k++)
                units[((size_t)e * K + j) * ns + k] = j == 0 ? 0.0 : frirl_demo_row_unit((uint64_t)e * (uint64_t)K + (uint64_t)j, k);
}

#endif
