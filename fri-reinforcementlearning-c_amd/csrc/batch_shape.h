// batch_shape.h -- host side: the lane shapes of the kernels whose workgroups each serve rows of ONE agent of a batch (the batched
// reductions, which see it through reduce_ws.h, and the batched roll-outs, rollout_batch.hip).
#pragma once
#include "shared_sweep.h"

// Lanes per row: G action slots (4 for up to 4 actions, else 8) times H rule slices.  The rounds run H = 8 while that keeps every
// row resident, the baseline replay (one row per agent) the widest group a wave holds.
static constexpr int RB_H = 8;              // rule slices of the shape the depth rule counts with

static int rb_group(int A) { return A <= 4 ? 4 : 8; }

// Resident workgroups per CU of the H = 8 roll-out kernels (one wave of a workgroup per SIMD, so = waves per SIMD), from their
// register counts: G = 4 needs 107 (nant 3) / 133 (nant 5) VGPRs -> 4 / 3 waves, G = 8 needs 235 / 255 -> 2 / 1.  The
// smaller of the two antecedent counts is taken; the 15.6 KB of LDS per workgroup would allow 10.
static int rb_wg_per_cu(int A) { return A <= 4 ? 3 : 1; }

static int rb_cus()
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) return n;
    (void)hipGetLastError();
    return 256;                              // no device visible: an MI355X is assumed
}

// rows the H = 8 shape keeps resident on the chip
static long rb_resident_rows(int A) { return (long)rb_cus() * rb_wg_per_cu(A) * (frirl::SH_BLOCK / (rb_group(A) * RB_H)); }

static size_t up16(size_t n) { return (n + 15) / 16 * 16; }

// rule slices of a round with `rows` rows in all: 8 while every row stays resident, else 4, else 1
static int rb_slices(long rows, int A)
{
    const long rows8 = rb_resident_rows(A);
    return rows <= rows8 ? 8 : (rows <= 2 * rows8 ? 4 : 1);
}
