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

// rule slices of a tiled batched roll-out of n rows on each of E agents (rollout_batch.hip's tiled form, the recorded and the
// point-keeping roll-out): rb_slices on the rows of the whole call; one row per agent: a full wave per row.  `forced` (an option's
// value, 0 = none) overrides it with 1 / 4 / 8, or 16 for up to 4 actions.
static int rb_rollout_slices(int E, int n, int A, int forced)
{
    if (forced == 1 || forced == 4 || forced == 8 || (forced == 16 && A <= 4)) return forced;
    return n == 1 ? FRIRL_WAVE / rb_group(A) : rb_slices((long)E * n, A);
}

// ---- argument checks of the entry points (no device is looked at) ----
// a caller's workspace: refused when NULL, not 16-byte aligned or smaller than `need`; query = the function that tells the size
static int check_workspace(const char *who, const void *workspace, size_t bytes, size_t need, const char *query)
{
    if (workspace && !(reinterpret_cast<uintptr_t>(workspace) & 15) && bytes >= need) return FRIRL_HIP_OK;
    frirl_host::set_error("%s: workspace %p / %zu bytes: needs %zu bytes, 16-byte aligned (%s)", who, workspace, bytes, need, query);
    return FRIRL_HIP_EINVAL;
}

// The agent of a roll-out in one of the demo environments (frirl_hip_rollout_batch, _record, _points), in the two places the entry
// points refuse it: first that it, its grids and the call's descriptor (desc: with the arrays it must name) are there, and, behind
// the descriptor's own refusals, its ranges, environment kind and grid lengths.
static int check_rollout_agent_null(const frirl_hip_agent *agent, bool desc, const char *who)
{
    if (agent && desc && agent->grid_values && agent->action_ve) return FRIRL_HIP_OK;
    frirl_host::set_error("%s: NULL argument", who);
    return FRIRL_HIP_EINVAL;
}

static int check_rollout_agent(const frirl_hip_tables *t, const frirl_hip_agent *agent, const char *who)
{
    if (agent->A < 1 || agent->A > FRIRL_HIP_MAX_ACTIONS || agent->max_steps < 0) {
        frirl_host::set_error("%s: A=%d / max_steps=%d out of range", who, agent->A, agent->max_steps);
        return FRIRL_HIP_EINVAL;
    }
    const int rc = frirl_host::check_demo_kind(t, agent, who);
    return rc ? rc : frirl_host::check_grid_len(t, agent, who);
}
