/*
 * demo_envs.c -- the three demo environments as host callbacks + their descriptors (part of libfrirl_dropin).
 *
 * Own driver for machines without the reference tree (the GPU box): it fills struct frirl_desc with the
 * hyper-parameters of the reference's examples (data from examples/<env>/<env>.c main()), installs host
 * callbacks implementing the same dynamics with libm trig, calls frirl_init / frirl_run (construct mode)
 * and dumps <env>.frirlrb.txt/.bin exactly like the reference's examples.  The reference's own,
 * unchanged example sources also compile and link against these headers and this library.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "frirl.h"
#include "frirl_types_def.h"
#include "frirl_app_helpers.h"
#include "frirl_demo.h"
#include "dropin_internal.h"
#include "frirl_hip.h"

#define PI 3.14159265358979323846264338327

static void generic_quantize(struct frirl_desc *fr, fri_float *s, int n, fri_float *q)
{
    int i;
    for (i = 0; i < n; i++) {
        int where = (int)round((s[i] + fabs(fr->statedims[i].values[0])) / fr->statedims[i].values_div);
        if (where < 0) where = 0;
        else if (where > fr->statedims[i].values_len - 1) where = fr->statedims[i].values_len - 1;
        q[i] = fr->statedims[i].values[where];
    }
}

/* mountain car */
static void mc_do_action(struct frirl_desc *fr, fri_float a, fri_float *s, int n, fri_float *ns)
{
    double v = (s[1] + (0.001 * a) + (-0.0025 * cos(3.0 * s[0]))) * 0.999, p;
    (void)fr; (void)n;
    if (v < -0.07) v = -0.07;
    if (v > 0.07) v = 0.07;
    p = s[0] + v;
    if (p <= -1.5) { p = -1.5; v = 0.0; }
    ns[0] = p; ns[1] = v;
}
static void mc_reward(struct frirl_desc *fr, fri_float *s, int n, struct frirl_reward_desc *rw)
{
    (void)fr; (void)n;
    rw->value = -10; rw->success = 0;
    if (s[0] >= 0.45) { rw->value = 1000; rw->success = 1; }
}

/* cart pole (sin and cos of the same angle through one sincos(), as gcc -O2 compiles the reference) */
static void cp_do_action(struct frirl_desc *fr, fri_float a, fri_float *s, int n, fri_float *ns)
{
    const double g = 9.8, mt = 1.0 + 0.1, mp = 0.1, len = 0.5, pml = mp * len, tau = 0.02, fourthirds = 4.0 / 3.0;
    const double force = a * 10.0;
    double sn, cs, temp, thacc, xacc;
    (void)fr; (void)n;
    sincos(s[2], &sn, &cs);
    temp = (force + pml * s[3] * s[3] * sn) / mt;
    thacc = (g * sn - cs * temp) / (len * (fourthirds - mp * cs * cs / mt));
    xacc = temp - pml * thacc * cs / mt;
    ns[0] = s[0] + tau * s[1];
    ns[1] = s[1] + tau * xacc;
    ns[2] = s[2] + tau * s[3];
    ns[3] = s[3] + tau * thacc;
}
static void cp_reward(struct frirl_desc *fr, fri_float *s, int n, struct frirl_reward_desc *rw)
{
    const double lim = PI / 4;
    (void)fr; (void)n;
    if (s[0] < -4.0 || s[0] > 4.0 || s[2] < (-1 * lim) || s[2] > lim) { rw->value = -10000 - 50 * fabs(s[0]) - 100 * fabs(s[2]); rw->success = 1; }
    else { rw->value = 10 - 1000 * s[2] * s[2] - 5 * fabs(s[0]) - 10 * s[3]; rw->success = 0; }
}
static void cp_quantize(struct frirl_desc *fr, fri_float *s, int n, fri_float *q)
{
    const double d12 = PI / 15, d3 = PI / 60;
    double q0 = s[0], q1 = round(s[1]), q2 = floor(s[2] / d3) * d3, q3 = s[3];
    (void)fr; (void)n;
    if (q0 < 0) q0 = -1;
    if (q0 > 0) q0 = 1;
    if (q1 < -1) q1 = -1;
    if (q1 > 1) q1 = 1;
    if (q2 > d12) q2 = d12;
    if (q2 < (-1 * d12)) q2 = -1 * d12;
    if (q3 < 0) q3 = -1;
    if (q3 > 0) q3 = 1;
    q[0] = q0; q[1] = q1; q[2] = q2; q[3] = q3;
}

/* acrobot */
static void ab_do_action(struct frirl_desc *fr, fri_float torque, fri_float *s, int n, fri_float *ns)
{
    const double vmax1 = 4 * PI, vmax2 = 9 * PI, m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8, dt = 0.05;
    const double l1sq = l1 * l1, lc1sq = lc1 * lc1, lc2sq = lc2 * lc2;
    double t1 = s[0], t2 = s[1], t1d = s[2], t2d = s[3];
    double c2, s2, d1, d2, phi1, phi2, acc1, acc2;
    int i;
    (void)fr; (void)n;
    sincos(t2, &s2, &c2);
    d1 = m1 * lc1sq + m2 * (l1sq + lc2sq + 2 * l1 * lc2 * c2) + I1 + I2;
    d2 = m2 * (lc2sq + l1 * lc2 * c2) + I2;
    phi2 = m2 * lc2 * g * cos(t1 + t2 - PI / 2);
    phi1 = -m2 * l1 * lc2 * t2d * s2 * (t2d - 2 * t1d) + (m1 * lc1 + m2 * l1) * g * cos(t1 - (PI / 2)) + phi2;
    acc2 = (torque + phi1 * (d2 / d1) - m2 * l1 * lc2 * t1d * t1d * s2 - phi2);
    acc2 = acc2 / (m2 * lc2sq + I2 - (d2 * d2 / d1));
    acc1 = -(d2 * acc2 + phi1) / d1;
    for (i = 0; i < 4; i++) {
        t1d = t1d + acc1 * dt;
        if (t1d < -vmax1) t1d = -vmax1;
        if (t1d > vmax1) t1d = vmax1;
        t1 = t1 + t1d * dt;
        t2d = t2d + acc2 * dt;
        if (t2d < -vmax2) t2d = -vmax2;
        if (t2d > vmax2) t2d = vmax2;
        t2 = t2 + t2d * dt;
    }
    if (t1 < -PI) t1 = -PI;
    if (t1 > PI) t1 = PI;
    if (t2 < -PI) t2 = -PI;
    if (t2 > PI) t2 = PI;
    ns[0] = t1; ns[1] = t2; ns[2] = t1d; ns[3] = t2d;
}
static void ab_reward(struct frirl_desc *fr, fri_float *s, int n, struct frirl_reward_desc *rw)
{
    const double y1 = 0.0 - cos(s[0]);
    const double y2 = y1 - cos(s[1]);
    (void)fr; (void)n;
    rw->value = -10; rw->success = 0;
    if (y2 >= 0.0 + 1.0) { rw->value = 1000; rw->success = 1; }
}

static void set_dim(struct frirl_dimension_desc *d, int n, const double *vals, double *store, double vdiv, double steep, double def, int U, double udiv)
{
    memset(d, 0, sizeof *d);
    d->values_len = n; d->values = store; d->values_div = vdiv; d->values_steep = steep; d->values_def = def;
    d->universe_len = U; d->universe_div = udiv;
    d->universe = malloc(sizeof(double) * U);
    if (vals) memcpy(store, vals, sizeof(double) * n); else frirl_gen_fixres_arr(store, n, vdiv);
    frirl_gen_fixres_arr(d->universe, U, udiv);
}

/* fills `fr` (already holding frirl_desc_default or parsed options) for one of the three demos; the
 * dimension descriptors and value arrays are heap-allocated and released by frirl_demo_release(). */
int frirl_demo_setup(struct frirl_desc *fr, const char *env)
{
    struct frirl_dimension_desc *sd = calloc(4, sizeof *sd);
    double (*v)[32] = calloc(5, sizeof *v);
    if (!sd || !v) return -1;
    fr->skip_rules = 1;
    if (!strcmp(env, "mountaincar")) {
        static const double v0[] = {-1.5, -1.295, -1.09, -0.885, -0.68, -0.475, -0.27, -0.065, 0.14, 0.345};
        static const double v1[] = {-0.07, -0.042, -0.014, 0.014, 0.042, 0.07};
        fr->reward_good_above = -5000.0; fr->alpha = 0.5; fr->gamma = 1.0; fr->epsilon = 0.01;
        fr->qdiff_pos_boundary = 1.0; fr->qdiff_neg_boundary = -4.0; fr->qdiff_final_tolerance = 500.0;
        fr->do_action_func = mc_do_action; fr->get_reward_func = mc_reward; fr->quant_obs_func = generic_quantize;
        set_dim(&sd[0], 10, v0, v[0], 0.205, 1.0, -0.5, 41, 0.1);
        set_dim(&sd[1], 6, v1, v[1], 0.028, 1.0, 0.0, 41, 0.005);
        fr->statedims_len = 2;
        set_dim(&fr->actiondim, 3, NULL, v[4], 1.0, 0.0, 0.0, 41, 0.1);
    } else if (!strcmp(env, "cartpole")) {
        static const double v2[] = {-0.2094, -0.1571, -0.1047, -0.0524, 0.0, 0.0524, 0.1047, 0.1571, 0.2094};
        static const double va[] = {-1.0, -0.9, -0.8, -0.7, -0.6, -0.5, -0.3999999999999999, -0.29999999999999992, -0.19999999999999995,
                                    -0.09999999999999998, 0.0, +0.09999999999999998, +0.19999999999999995, +0.29999999999999992,
                                    +0.3999999999999999, +0.5, +0.6, +0.7, +0.8, +0.9, +1.0};
        fr->reward_good_above = 0.0; fr->alpha = 0.3; fr->gamma = 1.0; fr->epsilon = 0.001;
        fr->qdiff_pos_boundary = 1.0; fr->qdiff_neg_boundary = -200.0; fr->qdiff_final_tolerance = 250.0;
        fr->do_action_func = cp_do_action; fr->get_reward_func = cp_reward; fr->quant_obs_func = cp_quantize;
        set_dim(&sd[0], 2, NULL, v[0], 2.0, 1.0, 1.0, 1001, 0.016);
        set_dim(&sd[1], 3, NULL, v[1], 1.0, 1.0, 0.0, 1001, 0.032);
        set_dim(&sd[2], 9, v2, v[2], 0.0524, 21.485917317405871, 0.0, 1001, 0.0031415926535897933);
        set_dim(&sd[3], 2, NULL, v[3], 2.0, 1.0, 0.0, 1001, 0.016);
        fr->statedims_len = 4;
        set_dim(&fr->actiondim, 21, va, v[4], 0.1, 0.0, 0.0, 1001, 0.008);
    } else if (!strcmp(env, "acrobot")) {
        static const double v0[] = {-1.570796326794897, -0.785398163397448, 0, 0.785398163397448, 1.570796326794897};
        fr->reward_good_above = 0.0; fr->alpha = 0.5; fr->gamma = 1.0; fr->epsilon = 0.001;
        fr->qdiff_pos_boundary = 1.0; fr->qdiff_neg_boundary = -200.0; fr->qdiff_final_tolerance = 50.0;
        fr->do_action_func = ab_do_action; fr->get_reward_func = ab_reward; fr->quant_obs_func = generic_quantize;
        set_dim(&sd[0], 5, v0, v[0], 0.785398163397448, 1.0, 0.0, 41, 0.1);
        set_dim(&sd[1], 5, v0, v[1], 0.785398163397448, 1.0, 0.0, 41, 0.1);
        set_dim(&sd[2], 3, NULL, v[2], 0.785398163397448, 1.0, 0.0, 41, 0.05);
        set_dim(&sd[3], 3, NULL, v[3], 0.785398163397448, 1.0, 0.0, 41, 0.05);
        fr->statedims_len = 4;
        set_dim(&fr->actiondim, 3, NULL, v[4], 1.0, 0.0, 0.0, 41, 0.1);
    } else {
        free(sd); free(v); fprintf(stderr, "unknown env %s (mountaincar|cartpole|acrobot)\n", env);
        return -1;
    }
    fr->statedims = sd;
    fr->construct_rb = 1;                 /* construct mode (the reference's mountaincar ships reduce-only) */
    fr->reduce_rb = 0;
    return 0;
}

void frirl_demo_release(struct frirl_desc *fr)
{
    int i;
    double *store = fr->statedims ? fr->statedims[0].values : NULL;
    for (i = 0; i < fr->statedims_len; i++) free(fr->statedims[i].universe);
    free(fr->actiondim.universe);
    free(store);
    free(fr->statedims);
    fr->statedims = NULL;
}

/* Tables of an agent from a flat description of its dimensions (any environment; needs no GPU): dimension k < nstates is a
 * state, k = nstates the action.  Universes as the demos' setup builds them (frirl_gen_fixres_arr over U points of step
 * universe_div[k]), VE rows by frirl_init_ve from the grid values / steepness (the action row's steepness is derived from
 * A, frirl_init_ve.c:91-92), VE value of every action as frirl_init.c:156-158.
 *   values_len [nstates+1], values [nstates+1][FRIRL_HIP_MAX_GRID] (row k: its first values_len[k] entries), values_steep,
 *   universe_div [nstates+1]  ->  u, ve [nstates+1][U], action_ve [values_len[nstates]].  0, or -1 on a bad argument. */
int frirl_describe_tables(int nstates, int U, const int *values_len, const double *values, const double *values_steep,
                          const double *universe_div, double *u, double *ve, double *action_ve)
{
    struct frirl_desc fr = frirl_desc_default;
    struct frirl_dimension_desc sd[FRIRL_HIP_MAX_NANT];
    int k, j;
    if (nstates < 1 || nstates >= FRIRL_HIP_MAX_NANT || U < 2 || !values_len || !values || !values_steep || !universe_div || !u || !ve || !action_ve) return -1;
    for (k = 0; k <= nstates; k++)
        if (values_len[k] < 1 || values_len[k] > FRIRL_HIP_MAX_GRID || !(universe_div[k] > 0.0)) return -1;
    if (values_len[nstates] > FRIRL_HIP_MAX_ACTIONS) return -1;
    for (k = 0; k <= nstates; k++) {
        struct frirl_dimension_desc *d = (k < nstates) ? &sd[k] : &fr.actiondim;
        memset(d, 0, sizeof *d);
        d->values_len = values_len[k]; d->values = (fri_float *)(values + (size_t)k * FRIRL_HIP_MAX_GRID); d->values_steep = values_steep[k];
        d->universe_len = U; d->universe_div = universe_div[k];
        frirl_gen_fixres_arr(u + (size_t)k * U, U, universe_div[k]);                     /* set_dim */
    }
    fr.statedims = sd; fr.statedims_len = nstates; fr.numofantecedents = nstates + 1;
    if (frirl_init_ve(&fr, ve, u, U) != 0) return -1;
    {
        const double *ua = u + (size_t)nstates * U, *vea = ve + (size_t)nstates * U;
        const double udiv = (ua[U - 1] - ua[0]) / (U - 1);
        for (j = 0; j < values_len[nstates]; j++) action_ve[j] = vea[five_dropin_snap(ua, U - 1, fr.actiondim.values[j], udiv)];
    }
    return 0;
}

/* Flat description of a demo for bindings (bench.py, tests): the demo's setup, then frirl_describe_tables.  Needs no GPU. */
int frirl_demo_describe(const char *env, int *nstates, int *U, int *A, double *u, double *ve, double *grid, int *grid_len,
                        double *grid_div, double *values_def, double *action_ve, double *hparams, int *max_steps)
{
    struct frirl_desc fr = frirl_desc_default;
    int k, j, n, usize, rc = 0;
    if (frirl_demo_setup(&fr, env) != 0) return -1;
    n = fr.statedims_len + 1;
    usize = fr.statedims[0].universe_len;
    *nstates = fr.statedims_len; *U = usize; *A = fr.actiondim.values_len; *max_steps = fr.max_steps;
    if (u && ve) {
        double steep[FRIRL_HIP_MAX_NANT], udiv[FRIRL_HIP_MAX_NANT];
        for (k = 0; k < n; k++) {
            const struct frirl_dimension_desc *d = (k < fr.statedims_len) ? &fr.statedims[k] : &fr.actiondim;
            grid_len[k] = d->values_len; grid_div[k] = d->values_div; values_def[k] = d->values_def;
            steep[k] = d->values_steep; udiv[k] = d->universe_div;
            for (j = 0; j < d->values_len; j++) grid[k * FRIRL_HIP_MAX_GRID + j] = d->values[j];
        }
        rc = frirl_describe_tables(fr.statedims_len, usize, grid_len, grid, steep, udiv, u, ve, action_ve);
        hparams[0] = fr.alpha; hparams[1] = fr.gamma; hparams[2] = fr.qdiff_pos_boundary; hparams[3] = fr.qdiff_neg_boundary;
        hparams[4] = fr.rule_weight_considered_significant_for_update; hparams[5] = fr.skip_rules; hparams[6] = fr.reward_good_above;
        hparams[7] = fr.qdiff_final_tolerance;
    }
    frirl_demo_release(&fr);
    return rc;
}

/* E agents of a demo, batched on the device: the C-level counterpart of the reference's many-agent run modes
 * (frirl_agent.c:294-467) without rule-base merging.  The environment's step() runs on the device with the portable
 * trig (include/frirl_hip.h), so the learned rule bases equal the host demo's up to the trig's last-bit differences. */
int frirl_demo_batch_run(const char *env, int agents, int max_episodes, const char *out_txt, int verbose)
{
    return frirl_demo_batch_run_reduce(env, agents, max_episodes, 0, out_txt, verbose);
}

int frirl_demo_batch_run_reduce(const char *env, int agents, int max_episodes, int reduce_strategy, const char *out_txt, int verbose)
{
    return frirl_demo_batch_run_ex(env, agents, max_episodes, reduce_strategy, NULL, NULL, out_txt, verbose);
}

/* host tables + agent descriptor of a demo for frirl_hip_batch_create / frirl_hip_multi_create; release with demo_desc_free */
struct demo_desc_mem { double *u, *ve, *grid, *action_ve, *rant0, *rconc0; };

static int demo_desc_build(const char *env, int agents, frirl_hip_batch_desc *d, struct demo_desc_mem *mm, int *nant_out)
{
    int ns, U, A, max_steps, nant, k, j, R0;
    int grid_len[FRIRL_HIP_MAX_NANT];
    double grid_div[FRIRL_HIP_MAX_NANT], values_def[FRIRL_HIP_MAX_NANT], hp[8];
    memset(mm, 0, sizeof *mm);
    if (frirl_demo_describe(env, &ns, &U, &A, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &max_steps) != 0) return -1;
    nant = ns + 1;
    mm->u = malloc(sizeof(double) * nant * U); mm->ve = malloc(sizeof(double) * nant * U);
    mm->grid = calloc((size_t)FRIRL_HIP_MAX_NANT * FRIRL_HIP_MAX_GRID, sizeof(double)); mm->action_ve = calloc(FRIRL_HIP_MAX_ACTIONS, sizeof(double));
    if (!mm->u || !mm->ve || !mm->grid || !mm->action_ve) return -1;
    if (frirl_demo_describe(env, &ns, &U, &A, mm->u, mm->ve, mm->grid, grid_len, grid_div, values_def, mm->action_ve, hp, &max_steps) != 0) return -1;
    R0 = 1 << nant;
    mm->rant0 = malloc(sizeof(double) * R0 * nant); mm->rconc0 = calloc(R0, sizeof(double));
    if (!mm->rant0 || !mm->rconc0) return -1;
    for (k = 0; k < nant; k++) {                               /* frirl_init_rb.c:99-126 */
        double mn = mm->grid[k * FRIRL_HIP_MAX_GRID], mx = mn;
        const unsigned int divider = (unsigned int)R0 >> (k + 1);
        for (j = 0; j < grid_len[k]; j++) { const double v = mm->grid[k * FRIRL_HIP_MAX_GRID + j]; if (v > mx) mx = v; if (v < mn) mn = v; }
        for (j = 0; j < R0; j++) mm->rant0[j * nant + k] = (((j / divider) % 2) == 0) ? mn : mx;
    }
    memset(d, 0, sizeof *d);
    d->nant = nant; d->U = U; d->E = agents; d->maxR = 1024; d->u = mm->u; d->ve = mm->ve; d->R0 = R0; d->rant0 = mm->rant0; d->rconc0 = mm->rconc0;
    d->agent.alpha = hp[0]; d->agent.gamma = hp[1]; d->agent.qdiff_pos_boundary = hp[2]; d->agent.qdiff_neg_boundary = hp[3];
    d->agent.weight_significant = hp[4]; d->agent.skip_rules = (int32_t)hp[5]; d->agent.reward_good_above = hp[6]; d->agent.qdiff_final_tolerance = hp[7];
    d->agent.p = 0; d->agent.A = A; d->agent.max_steps = max_steps; d->agent.no_random = 1;
    d->agent.env_kind = !strcmp(env, "mountaincar") ? FRIRL_HIP_ENV_MOUNTAINCAR : (!strcmp(env, "cartpole") ? FRIRL_HIP_ENV_CARTPOLE : FRIRL_HIP_ENV_ACROBOT);
    for (k = 0; k < nant; k++) { d->agent.grid_len[k] = grid_len[k]; d->agent.grid_div[k] = grid_div[k]; d->agent.values_def[k] = values_def[k]; }
    d->agent.grid_values = mm->grid; d->agent.action_ve = mm->action_ve;
    *nant_out = nant;
    return 0;
}

static void demo_desc_free(struct demo_desc_mem *mm)
{
    free(mm->u); free(mm->ve); free(mm->grid); free(mm->action_ve); free(mm->rant0); free(mm->rconc0);
}

static int dump_rule_base_txt(const char *out_txt, int nant, int R, const double *rant, const double *rconc)
{
    int j, k;
    FILE *fp = fopen(out_txt, "w");
    if (!fp) return -1;
    for (j = 0; j < R; j++) {
        for (k = 0; k < nant; k++) fprintf(fp, "%.18f ", rant[j * nant + k]);
        fprintf(fp, "%.18f \n", rconc[j]);
    }
    fclose(fp);
    return 0;
}

/* `agents` agents of a demo sharded over `gpus` visible devices (0 = all): frirl_hip_multi_* -- one batch and one host thread
 * per device, the per-episode report all-reduced with RCCL.  Prints the job's report; out_txt (or NULL) receives the rule base of
 * the agent with global id 0.  Returns the number of converged agents, or -1. */
int frirl_demo_multi_run(const char *env, int agents, int gpus, int max_episodes, const char *out_txt, int verbose)
{
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_multi *m;
    frirl_hip_batch_stats_t st;
    int nant = 0, episodes = 0, rc, g;
    int32_t ng = 0, ver = 0;
    int64_t start[64], count[64];
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    m = frirl_hip_multi_create(&d, agents, gpus);
    if (!m) five_dropin_fatal("frirl_demo_multi_run(create)", FRIRL_HIP_ENODEV);
    rc = frirl_hip_multi_train(m, max_episodes, &episodes);
    if (rc) five_dropin_fatal("frirl_demo_multi_run(train)", rc);
    rc = frirl_hip_multi_stats(m, &st);
    if (rc) five_dropin_fatal("frirl_demo_multi_run(stats)", rc);
    frirl_hip_multi_info(m, &ng, &ver, NULL, NULL);
    if (ng <= 64) frirl_hip_multi_info(m, &ng, &ver, start, count);
    if (verbose) {
        printf("multi %s: gpus %d (RCCL %d) agents %lld episodes %d converged %lld env-steps %lld mean-rules %.3f mean-reward %.6f (min %.6f max %.6f)\n", env,
               (int)ng, (int)ver, (long long)st.agents, episodes, (long long)st.converged, (long long)st.total_env_steps, st.rules_sum / st.agents,
               st.reward_sum / st.agents, st.reward_min, st.reward_max);
        for (g = 0; g < ng && ng <= 64; g++) printf("multi %s: device %d runs agents [%lld, %lld)\n", env, g, (long long)start[g], (long long)(start[g] + count[g]));
    }
    if (st.full_agents > 0)
        fprintf(stderr, "Warning: %lld of %lld rule bases are at their capacity of %d rules: further rule insertions were refused\n",
                (long long)st.full_agents, (long long)st.agents, (int)d.maxR);
    if (out_txt) {
        int32_t R = 0;
        double *rant = malloc(sizeof(double) * 1024 * nant), *rconc = malloc(sizeof(double) * 1024);
        if (!rant || !rconc || frirl_hip_multi_get_rulebase(m, 0, &R, rant, rconc) != 0 || dump_rule_base_txt(out_txt, nant, R, rant, rconc) != 0) {
            fprintf(stderr, "frirl_demo_multi_run: cannot dump rule base\n");
            return -1;
        }
        free(rant); free(rconc);
    }
    frirl_hip_multi_destroy(m);
    demo_desc_free(&mm);
    return (int)st.converged;
}

/* The reference's many-agent mode WITH the rule-base exchange (frirl_omp_run, frirl_agent.c:294-385 + :424-462) on one GPU: `agents`
 * agents start from different states (gen_def_states), learn in chunks of FRIRL_AGENT_EPCHUNK - 1 = 9 episodes and merge their rule
 * bases after every chunk (frirl_hip_batch_train_merged).  out_txt = the master's (agent 0's) rule base.  Returns the number of merge
 * rounds, or -1. */
int frirl_demo_merged_run(const char *env, int agents, int max_episodes, const char *out_txt, int verbose)
{
    int nant = 0, episodes = 0, rounds = 0, rc;
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_batch *b;
    frirl_hip_batch_stats_t st;
    double *start;
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    start = malloc(sizeof(double) * (size_t)agents * (nant - 1));
    if (!start || frirl_hip_gen_def_states(d.rant0, d.R0, nant, agents, d.agent.values_def, start) != 0) return -1;
    d.start_states = start;
    b = frirl_hip_batch_create(&d);
    if (!b) five_dropin_fatal("frirl_demo_merged_run(create)", FRIRL_HIP_ENODEV);
    rc = frirl_hip_batch_train_merged(b, max_episodes, 10, &episodes, &rounds);
    if (rc) five_dropin_fatal("frirl_demo_merged_run(train)", rc);
    rc = frirl_hip_batch_stats(b, &st);
    if (rc) five_dropin_fatal("frirl_demo_merged_run(stats)", rc);
    if (verbose)
        printf("merged %s: agents %lld episodes %d merge-rounds %d converged %lld env-steps %lld mean-rules %.3f mean-reward %.6f\n", env, (long long)st.agents,
               episodes, rounds, (long long)st.converged, (long long)st.total_env_steps, st.rules_sum / st.agents, st.reward_sum / st.agents);
    if (st.full_agents > 0)
        fprintf(stderr, "Warning: %lld of %lld rule bases are at their capacity of %d rules: further rule insertions were refused\n",
                (long long)st.full_agents, (long long)st.agents, (int)d.maxR);
    if (out_txt) {
        int32_t R = 0;
        double *rant = malloc(sizeof(double) * 1024 * nant), *rconc = malloc(sizeof(double) * 1024);
        if (!rant || !rconc || frirl_hip_batch_get_rulebase(b, 0, &R, rant, rconc) != 0 || dump_rule_base_txt(out_txt, nant, R, rant, rconc) != 0) return -1;
        free(rant); free(rconc);
    }
    frirl_hip_batch_destroy(b);
    demo_desc_free(&mm);
    free(start);
    return rounds;
}

/* The same over `gpus` devices (0 = all): frirl_hip_multi_train_merged -- the master's rule list is broadcast to every device, the devices
 * send their agents' rule lists to device 0 (RCCL), the master takes them over in global agent order.  Returns the merge rounds, or -1. */
int frirl_demo_multi_merged_run(const char *env, int agents, int gpus, int max_episodes, const char *out_txt, int verbose)
{
    int nant = 0, episodes = 0, rounds = 0, rc;
    int32_t ng = 0, ver = 0;
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_multi *m;
    frirl_hip_batch_stats_t st;
    double *start;
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    start = malloc(sizeof(double) * (size_t)agents * (nant - 1));
    if (!start || frirl_hip_gen_def_states(d.rant0, d.R0, nant, agents, d.agent.values_def, start) != 0) return -1;
    d.start_states = start;
    m = frirl_hip_multi_create(&d, agents, gpus);
    if (!m) five_dropin_fatal("frirl_demo_multi_merged_run(create)", FRIRL_HIP_ENODEV);
    rc = frirl_hip_multi_train_merged(m, max_episodes, 10, &episodes, &rounds);
    if (rc) five_dropin_fatal("frirl_demo_multi_merged_run(train)", rc);
    rc = frirl_hip_multi_stats(m, &st);
    if (rc) five_dropin_fatal("frirl_demo_multi_merged_run(stats)", rc);
    frirl_hip_multi_info(m, &ng, &ver, NULL, NULL);
    if (verbose)
        printf("merged %s: gpus %d (RCCL %d) agents %lld episodes %d merge-rounds %d converged %lld env-steps %lld mean-rules %.3f mean-reward %.6f\n", env,
               (int)ng, (int)ver, (long long)st.agents, episodes, rounds, (long long)st.converged, (long long)st.total_env_steps, st.rules_sum / st.agents,
               st.reward_sum / st.agents);
    if (st.full_agents > 0)
        fprintf(stderr, "Warning: %lld of %lld rule bases are at their capacity of %d rules: further rule insertions were refused\n",
                (long long)st.full_agents, (long long)st.agents, (int)d.maxR);
    if (out_txt) {
        int32_t R = 0;
        double *rant = malloc(sizeof(double) * 1024 * nant), *rconc = malloc(sizeof(double) * 1024);
        if (!rant || !rconc || frirl_hip_multi_get_rulebase(m, 0, &R, rant, rconc) != 0 || dump_rule_base_txt(out_txt, nant, R, rant, rconc) != 0) return -1;
        free(rant); free(rconc);
    }
    frirl_hip_multi_destroy(m);
    demo_desc_free(&mm);
    free(start);
    return rounds;
}

/* start states [agents][K][ns] of K rows per agent: row 0 = agent.values_def, row j >= 1 = values_def[k] + spread * units[e][j][k] *
 * (largest - smallest grid value of dimension k), clipped to the grid (frirl_demo.h: frirl_demo_batch_run_evaluate) */
static void demo_row_starts(const frirl_hip_batch_desc *d, const struct demo_desc_mem *mm, int agents, int K, int ns, double spread, const double *units,
                            double *start)
{
    int e, j, k;
    for (k = 0; k < ns; k++) {
        const double *g = mm->grid + (size_t)k * FRIRL_HIP_MAX_GRID;
        double lo = g[0], hi = g[0];
        for (j = 0; j < d->agent.grid_len[k]; j++) { if (g[j] < lo) lo = g[j]; if (g[j] > hi) hi = g[j]; }
        for (e = 0; e < agents; e++)
            for (j = 0; j < K; j++) {
                const size_t i = ((size_t)e * K + j) * ns + k;
                double v = d->agent.values_def[k] + spread * units[i] * (hi - lo);
                if (j == 0) v = d->agent.values_def[k];             /* the agent's own start state */
                start[i] = v < lo ? lo : (v > hi ? hi : v);
            }
    }
}

static int demo_batch_run(const char *env, int agents, int max_episodes, int reduce_strategy, int reduce_all, const char *load_bin,
                          const char *save_bin, const char *out_txt, int starts, double spread, const double *units, int map, int verbose);

int frirl_demo_batch_run_evaluate_teach(const char *env, int agents, int max_episodes, const char *load_bin, const char *save_bin, int K, double spread,
                                        const double *units, int teach_episodes, int teach_passes, int verbose)
{
    int nant = 0, ns, episodes = 0, rc, e, stage;
    int32_t best = 0;
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_batch *b;
    frirl_hip_rollout_score *sc;
    double *start;
    long long rows = 0, succ = 0, steps = 0;
    double rsum = 0.0, rmin = 0.0, rmax = 0.0;
    if (K < 1 || !units || !(spread >= 0.0) || teach_episodes < 0 || demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    ns = nant - 1;
    sc = malloc(sizeof *sc * (size_t)agents);
    start = malloc(sizeof(double) * (size_t)agents * (size_t)K * (size_t)ns);
    if (!sc || !start) return -1;
    demo_row_starts(&d, &mm, agents, K, ns, spread, units, start);
    b = frirl_hip_batch_create(&d);
    if (!b) five_dropin_fatal("frirl_demo_batch_run_evaluate(create)", FRIRL_HIP_ENODEV);
    if (load_bin) {
        int32_t nrec = 0;
        rc = frirl_hip_batch_load_rulebases(b, load_bin, &nrec);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_evaluate(load)", rc);
        if (verbose) printf("evaluate %s: loaded %d rule base record(s) from %s\n", env, (int)nrec, load_bin);
    } else {
        rc = frirl_hip_batch_train(b, max_episodes, &episodes);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_evaluate(train)", rc);
    }
    if (save_bin) {
        rc = frirl_hip_batch_save_rulebases(b, save_bin);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_evaluate(save)", rc);
    }
    for (stage = 0; stage < (teach_episodes > 0 ? 2 : 1); stage++) {
        if (stage == 1) {               /* the best agent shows every other agent teach_episodes greedy episodes */
            frirl_hip_teach_result tr;
            rc = frirl_hip_batch_teach(b, best, teach_episodes, NULL, teach_passes, NULL, &tr);
            if (rc) five_dropin_fatal("frirl_demo_batch_run_evaluate(teach)", rc);
            if (verbose)
                printf("taught: teacher %d episodes_recorded %d successes %d records %d students %d refused %d records_replayed %lld\n", (int)tr.teacher,
                       (int)tr.episodes_recorded, (int)tr.successes, (int)tr.records, (int)tr.students, (int)tr.refused, (long long)tr.records_replayed);
            rows = succ = steps = 0;
            rsum = rmin = rmax = 0.0;
        }
        rc = frirl_hip_batch_evaluate(b, K, start, sc, &best);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_evaluate(evaluate)", rc);
        for (e = 0; e < agents; e++) {
            if (sc[e].rows > 0 && (rows == 0 || sc[e].reward_min < rmin)) rmin = sc[e].reward_min;
            if (sc[e].rows > 0 && (rows == 0 || sc[e].reward_max > rmax)) rmax = sc[e].reward_max;
            rows += sc[e].rows; succ += sc[e].successes; steps += sc[e].steps_sum; rsum += sc[e].reward_sum;
        }
        if (verbose) {
            printf("evaluate %s: agents %d rows %lld successful %.4f mean-steps %.3f mean-reward %.6f (min %.6f max %.6f) spread %.3f\n", env, agents, rows,
                   rows ? (double)succ / rows : 0.0, rows ? (double)steps / rows : 0.0, rows ? rsum / rows : 0.0, rmin, rmax, spread);
            printf("evaluate %s: best agent %d: %d of %d rows successful, reward-sum %.6f, steps %lld\n", env, (int)best, (int)sc[best].successes,
                   (int)sc[best].rows, sc[best].reward_sum, (long long)sc[best].steps_sum);
        }
    }
    frirl_hip_batch_destroy(b);
    demo_desc_free(&mm);
    free(sc); free(start);
    return (int)best;
}

int frirl_demo_batch_run_evaluate(const char *env, int agents, int max_episodes, const char *load_bin, const char *save_bin, int K, double spread,
                                  const double *units, int verbose)
{
    return frirl_demo_batch_run_evaluate_teach(env, agents, max_episodes, load_bin, save_bin, K, spread, units, 0, 1, verbose);
}

int frirl_demo_batch_run_ex(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                            const char *out_txt, int verbose)
{
    return demo_batch_run(env, agents, max_episodes, reduce_strategy, 0, load_bin, save_bin, out_txt, 0, 0.0, NULL, 0, verbose);
}

int frirl_demo_batch_run_reduce_all(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                                    const char *out_txt, int verbose)
{
    return demo_batch_run(env, agents, max_episodes, reduce_strategy, 1, load_bin, save_bin, out_txt, 0, 0.0, NULL, 0, verbose);
}

int frirl_demo_batch_run_reduce_all_starts(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                                           const char *out_txt, int K, double spread, const double *units, int verbose)
{
    if (K < 1 || K > FRIRL_HIP_REDUCE_MAX_STARTS || !units || !(spread >= 0.0) || (reduce_strategy != 1 && reduce_strategy != 2)) return -1;
    return demo_batch_run(env, agents, max_episodes, reduce_strategy, 1, load_bin, save_bin, out_txt, K, spread, units, 0, verbose);
}

int frirl_demo_batch_run_reduce_all_map(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                                        const char *out_txt, int K, double spread, const double *units, int only_successful, int verbose)
{
    if (K < 1 || K > FRIRL_HIP_REDUCE_MAX_STARTS || !units || !(spread >= 0.0) || (reduce_strategy != 1 && reduce_strategy != 2)) return -1;
    return demo_batch_run(env, agents, max_episodes, reduce_strategy, 1, load_bin, save_bin, out_txt, K, spread, units, only_successful ? 1 : 2, verbose);
}

/* starts >= 1: the reduction of every agent validates each removal against `starts` start states per agent (demo_row_starts);
 * map != 0: on the policy map at the points the greedy policy visits from them instead (1 = of the successful starts, 2 = of all) */
static int demo_batch_run(const char *env, int agents, int max_episodes, int reduce_strategy, int reduce_all, const char *load_bin,
                          const char *save_bin, const char *out_txt, int starts, double spread, const double *units, int map, int verbose)
{
    int nant = 0, episodes = 0, rc;
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_batch *b;
    frirl_hip_batch_stats_t st;
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    d.agent.evaluate = load_bin ? 1 : 0;          /* loaded rule bases are replayed greedily, not trained (frirl_test_run.c:66-70) */
    b = frirl_hip_batch_create(&d);
    if (!b) five_dropin_fatal("frirl_demo_batch_run(create)", FRIRL_HIP_ENODEV);
    if (load_bin) {
        int32_t nrec = 0;
        rc = frirl_hip_batch_load_rulebases(b, load_bin, &nrec);
        if (rc) five_dropin_fatal("frirl_demo_batch_run(load)", rc);
        if (verbose) printf("batch %s: loaded %d rule base record(s) from %s\n", env, (int)nrec, load_bin);
        rc = frirl_hip_batch_episode(b);          /* one greedy episode per agent */
        episodes = 1;
    } else {
        rc = frirl_hip_batch_train(b, max_episodes, &episodes);
    }
    if (rc) five_dropin_fatal("frirl_demo_batch_run(train)", rc);
    rc = frirl_hip_batch_stats(b, &st);
    if (rc) five_dropin_fatal("frirl_demo_batch_run(stats)", rc);
    if (verbose)
        printf("batch %s: agents %lld episodes %d converged %lld env-steps %lld mean-rules %.3f mean-reward %.6f (min %.6f max %.6f)\n", env,
               (long long)st.agents, episodes, (long long)st.converged, (long long)st.total_env_steps, st.rules_sum / st.agents,
               st.reward_sum / st.agents, st.reward_min, st.reward_max);
    if (st.full_agents > 0)      /* the reference never checks the capacity (FIVE_add_rule writes past it); here the append is refused and reported */
        fprintf(stderr, "Warning: %lld of %lld rule bases are at their capacity of %d rules: further rule insertions were refused\n",
                (long long)st.full_agents, (long long)st.agents, (int)d.maxR);
    if (save_bin) {                               /* all agents' rule bases, before any reduction */
        rc = frirl_hip_batch_save_rulebases(b, save_bin);
        if (rc) five_dropin_fatal("frirl_demo_batch_run(save)", rc);
    }
    if ((reduce_strategy == 1 || reduce_strategy == 2) && reduce_all && map && starts >= 1) {      /* validated on the policy map */
        const size_t rows = (size_t)agents * (size_t)starts;
        double *start = malloc(sizeof(double) * rows * (size_t)(nant - 1));
        frirl_hip_reduce_map_totals tot;
        if (!start) five_dropin_fatal("frirl_demo_batch_run(reduce all map)", FRIRL_HIP_ELAUNCH);
        demo_row_starts(&d, &mm, agents, starts, nant - 1, spread, units, start);
        rc = frirl_hip_batch_reduce_all_map(b, reduce_strategy, starts, start, map == 1, 0, NULL, &tot);
        free(start);
        if (rc) five_dropin_fatal("frirl_demo_batch_run(reduce all map)", rc);
        if (verbose)
            printf("reduced-map: batch %s: %d of %d agents reduced, %lld -> %lld rules (strategy %d, %d starts, %s), points %lld, overflow %d, without points %d\n",
                   env, (int)tot.agents_reduced, agents, (long long)tot.rules_before, (long long)tot.rules_after, reduce_strategy, starts,
                   map == 1 ? "successful starts" : "all starts", (long long)tot.points, (int)tot.agents_overflow, (int)tot.agents_without_points);
    } else if ((reduce_strategy == 1 || reduce_strategy == 2) && reduce_all) {      /* every agent's rule base in one batched run */
        frirl_hip_reduce_result *rr = malloc(sizeof *rr * (size_t)agents);
        long long before = 0, after = 0, rollouts = 0;
        int32_t reduced = 0, rounds = 0;
        int e;
        long long used = 0;
        if (rr && starts >= 1) {                  /* starts whose baseline episode is not good are left out (drop_bad_starts = 1) */
            const size_t rows = (size_t)agents * (size_t)starts;
            double *start = malloc(sizeof(double) * rows * (size_t)(nant - 1));
            frirl_hip_reduce_start_result *ps = malloc(sizeof *ps * rows);
            size_t i;
            if (!start || !ps) five_dropin_fatal("frirl_demo_batch_run(reduce all)", FRIRL_HIP_ELAUNCH);
            demo_row_starts(&d, &mm, agents, starts, nant - 1, spread, units, start);
            rc = frirl_hip_batch_reduce_all_starts(b, reduce_strategy, 0.0, 0, starts, start, 1, rr, ps, &reduced);
            for (i = 0; rc == 0 && i < rows; i++) used += ps[i].used;
            free(start); free(ps);
        } else
            rc = rr ? frirl_hip_batch_reduce_all(b, reduce_strategy, 0.0, 0, rr, &reduced) : FRIRL_HIP_ELAUNCH;
        if (rc) five_dropin_fatal("frirl_demo_batch_run(reduce all)", rc);
        for (e = 0; e < agents; e++) {
            before += rr[e].rules_before; after += rr[e].rules_after; rollouts += rr[e].rollouts;
            if (rr[e].rounds > rounds) rounds = rr[e].rounds;
        }
        if (verbose && starts > 1)                /* one start state: the agent's own, the line of the run without start states */
            printf("batch %s: %d of %d agents reduced, %lld -> %lld rules (strategy %d, %d rounds, %lld replays), starts used %lld of %lld\n", env,
                   (int)reduced, agents, before, after, reduce_strategy, (int)rounds, rollouts, used, (long long)agents * starts);
        else if (verbose)
            printf("batch %s: %d of %d agents reduced, %lld -> %lld rules (strategy %d, %d rounds, %lld replays)\n", env, (int)reduced, agents, before,
                   after, reduce_strategy, (int)rounds, rollouts);
        free(rr);
    } else if (reduce_strategy == 1 || reduce_strategy == 2) {
        frirl_hip_reduce_result rr;
        rc = frirl_hip_batch_reduce(b, 0, reduce_strategy, 0.0, 0, &rr);
        if (rc) five_dropin_fatal("frirl_demo_batch_run(reduce)", rc);
        if (verbose)
            printf("batch %s: agent 0 reduced %d -> %d rules (strategy %d, %d launches, %d replays, episode of %d steps, reward %.6f)\n", env,
                   rr.rules_before, rr.rules_after, reduce_strategy, rr.rounds, rr.rollouts, rr.steps_incremental, rr.reward);
    }
    if (out_txt) {
        int32_t R = 0;
        double *rant = malloc(sizeof(double) * 1024 * nant), *rconc = malloc(sizeof(double) * 1024);
        if (!rant || !rconc || frirl_hip_batch_get_rulebase(b, 0, &R, rant, rconc) != 0 || dump_rule_base_txt(out_txt, nant, R, rant, rconc) != 0) {
            fprintf(stderr, "frirl_demo_batch_run: cannot dump rule base\n");
            return -1;
        }
        free(rant); free(rconc);
    }
    frirl_hip_batch_destroy(b);
    demo_desc_free(&mm);
    return (int)st.converged;
}

/* ---- a hyper-parameter sweep in one run: frirl_demo --agents N --hparams FILE ---------------------------------------------------------
 * FILE: one set per line, `alpha gamma qdiff_pos qdiff_neg weight_thr skip_rules`; `#` starts a comment; blank lines are skipped.
 * *sets = malloc'ed [*nsets][6]; err receives "line N: why" for the first malformed line, or why the file is unusable. */
int frirl_demo_parse_hparams(const char *path, double **sets, int *nsets, char *err, size_t err_len)
{
    char line[512];
    int lineno = 0, n = 0, cap = 0;
    double *out = NULL;
    FILE *fp = fopen(path, "r");
    *sets = NULL; *nsets = 0;
    if (!fp) { snprintf(err, err_len, "cannot open %s", path); return -1; }
    while (fgets(line, sizeof line, fp)) {
        double v[6];
        char tail[2], *hash = strchr(line, '#');
        int got, k;
        lineno++;
        if (!strchr(line, '\n') && !feof(fp)) { snprintf(err, err_len, "line %d: longer than %d characters", lineno, (int)sizeof line - 2); free(out); fclose(fp); return -1; }
        if (hash) *hash = '\0';
        if (line[strspn(line, " \t\r\n")] == '\0') continue;
        got = sscanf(line, "%lf %lf %lf %lf %lf %lf %1s", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], tail);
        if (got != 6) { snprintf(err, err_len, "line %d: expected 6 values (alpha gamma qdiff_pos qdiff_neg weight_thr skip_rules), found %s", lineno, got > 6 ? "more" : "fewer"); free(out); fclose(fp); return -1; }
        for (k = 0; k < 6; k++) if (!(v[k] - v[k] == 0.0)) { snprintf(err, err_len, "line %d: value %d is not finite", lineno, k + 1); free(out); fclose(fp); return -1; }
        if (v[2] < v[3]) { snprintf(err, err_len, "line %d: qdiff_pos %g < qdiff_neg %g", lineno, v[2], v[3]); free(out); fclose(fp); return -1; }
        if (v[4] < 0.0) { snprintf(err, err_len, "line %d: weight_thr %g is negative", lineno, v[4]); free(out); fclose(fp); return -1; }
        if (v[5] != 0.0 && v[5] != 1.0) { snprintf(err, err_len, "line %d: skip_rules %g is neither 0 nor 1", lineno, v[5]); free(out); fclose(fp); return -1; }
        if (n == cap) {
            double *grown = realloc(out, sizeof(double) * 6 * (size_t)(cap = cap ? 2 * cap : 16));
            if (!grown) { snprintf(err, err_len, "out of memory"); free(out); fclose(fp); return -1; }
            out = grown;
        }
        memcpy(out + 6 * (size_t)n++, v, sizeof v);
    }
    fclose(fp);
    if (n == 0) { snprintf(err, err_len, "%s holds no hyper-parameter set", path); free(out); return -1; }
    *sets = out; *nsets = n;
    return 0;
}

/* `agents` agents of a demo in one persistent-learner run, agent e under set e mod nsets (sets HOST [nsets][6], the columns of
 * frirl_demo_parse_hparams): frirl_hip_batch_set_hparams + frirl_hip_batch_train, then one line per set from
 * frirl_hip_batch_agent_report.  Returns the number of converged agents, or -1. */
int frirl_demo_batch_run_hparams(const char *env, int agents, int max_episodes, const double *sets, int nsets, int verbose)
{
    int nant = 0, episodes = 0, rc, e, s, k, total = 0;
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_batch *b;
    frirl_hip_hparam_rows rows;
    double *col = malloc(sizeof(double) * 5 * (size_t)agents), *reward = malloc(sizeof(double) * (size_t)agents);
    int32_t *skip = malloc(sizeof(int32_t) * 4 * (size_t)agents), *conv = skip + agents, *eps = conv + agents, *rules = eps + agents;
    if (!col || !reward || !skip || nsets < 1) return -1;
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    for (e = 0; e < agents; e++) {
        for (k = 0; k < 5; k++) col[(size_t)k * agents + e] = sets[6 * (size_t)(e % nsets) + k];
        skip[e] = (int32_t)sets[6 * (size_t)(e % nsets) + 5];
    }
    rows.alpha = col; rows.gamma = col + agents; rows.qdiff_pos_boundary = col + 2 * (size_t)agents; rows.qdiff_neg_boundary = col + 3 * (size_t)agents;
    rows.weight_significant = col + 4 * (size_t)agents; rows.skip_rules = skip;
    b = frirl_hip_batch_create(&d);
    if (!b) five_dropin_fatal("frirl_demo_batch_run_hparams(create)", FRIRL_HIP_ENODEV);
    rc = frirl_hip_batch_set_hparams(b, &rows);
    if (rc) five_dropin_fatal("frirl_demo_batch_run_hparams(set)", rc);
    rc = frirl_hip_batch_train(b, max_episodes, &episodes);
    if (rc) five_dropin_fatal("frirl_demo_batch_run_hparams(train)", rc);
    rc = frirl_hip_batch_agent_report(b, conv, eps, rules, NULL, reward);
    if (rc) five_dropin_fatal("frirl_demo_batch_run_hparams(report)", rc);
    for (s = 0; s < nsets && s < agents; s++) {
        long long n = 0, nconv = 0, ep_sum = 0, rule_sum = 0;
        int ep_max = 0;
        double rew_sum = 0.0;
        for (e = s; e < agents; e += nsets) {
            n++; nconv += conv[e] != 0; ep_sum += eps[e]; rule_sum += rules[e]; rew_sum += reward[e];
            if (eps[e] > ep_max) ep_max = eps[e];
        }
        total += (int)nconv;
        if (verbose)
            printf("hparams %s: set %d agents %lld converged %lld mean-episodes %.3f max-episodes %d mean-rules %.3f mean-reward %.6f\n", env, s, n, nconv,
                   (double)ep_sum / n, ep_max, (double)rule_sum / n, rew_sum / n);
    }
    frirl_hip_batch_destroy(b);
    demo_desc_free(&mm);
    free(col); free(reward); free(skip);
    return total;
}

/* ---- an exploration sweep in one run: frirl_demo --agents N --explore FILE [--hparams FILE] [--seed S] ---------------------------------
 * FILE: one `epsilon horizon` pair per line; `#` starts a comment; blank lines are skipped.  *eps = malloc'ed [*n], *horizon =
 * malloc'ed [*n]; err receives "line N: why" for the first malformed line, or why the file is unusable. */
int frirl_demo_parse_explore(const char *path, double **eps, int **horizon, int *n_out, char *err, size_t err_len)
{
    char line[512];
    int lineno = 0, n = 0, cap = 0;
    double *oe = NULL;
    int *oh = NULL;
    FILE *fp = fopen(path, "r");
    *eps = NULL; *horizon = NULL; *n_out = 0;
    if (!fp) { snprintf(err, err_len, "cannot open %s", path); return -1; }
    while (fgets(line, sizeof line, fp)) {
        double e, h;
        char tail[2], *hash = strchr(line, '#');
        int got;
        lineno++;
        if (!strchr(line, '\n') && !feof(fp)) { snprintf(err, err_len, "line %d: longer than %d characters", lineno, (int)sizeof line - 2); goto bad; }
        if (hash) *hash = '\0';
        if (line[strspn(line, " \t\r\n")] == '\0') continue;
        got = sscanf(line, "%lf %lf %1s", &e, &h, tail);
        if (got != 2) { snprintf(err, err_len, "line %d: expected 2 values (epsilon horizon), found %s", lineno, got > 2 ? "more" : "fewer"); goto bad; }
        if (!(e >= 0.0 && e <= 1.0)) { snprintf(err, err_len, "line %d: epsilon %g is not in [0, 1]", lineno, e); goto bad; }
        if (!(h >= 0.0 && h <= 1073741824.0) || h != (double)(int)h) { snprintf(err, err_len, "line %d: horizon %g is not a whole number in 0..2^30", lineno, h); goto bad; }
        if (n == cap) {
            double *ge;
            int *gh;
            cap = cap ? 2 * cap : 16;
            ge = realloc(oe, sizeof(double) * (size_t)cap);
            if (ge) oe = ge;
            gh = realloc(oh, sizeof(int) * (size_t)cap);
            if (gh) oh = gh;
            if (!ge || !gh) { snprintf(err, err_len, "out of memory"); goto bad; }
        }
        oe[n] = e; oh[n] = (int)h; n++;
    }
    fclose(fp);
    if (n == 0) { snprintf(err, err_len, "%s holds no epsilon / horizon pair", path); free(oe); free(oh); return -1; }
    *eps = oe; *horizon = oh; *n_out = n;
    return 0;
bad:
    free(oe); free(oh); fclose(fp);
    return -1;
}

/* `agents` agents of a demo in one persistent-learner run, agent e exploring under pair e mod n (eps, horizon: HOST [n], the columns
 * of frirl_demo_parse_explore) on the stream of `seed`, global ids id_base .. id_base + agents - 1, and -- sets != NULL -- learning under
 * hyper-parameter set e mod nsets: frirl_hip_batch_set_exploration (+ _set_hparams) + frirl_hip_batch_train, then one line per pair
 * (and per set) from frirl_hip_batch_agent_report.  Returns the number of converged agents, or -1. */
int frirl_demo_batch_run_explore(const char *env, int agents, int max_episodes, const double *eps, const int *horizon, int n, unsigned long long seed,
                                 unsigned long long id_base, const double *sets, int nsets, int verbose)
{
    int nant = 0, episodes = 0, rc, e, s, k, total = 0, pass;
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_batch *b;
    frirl_hip_hparam_rows rows;
    frirl_hip_explore_rows ex;
    double *col = malloc(sizeof(double) * 6 * (size_t)agents), *reward = malloc(sizeof(double) * (size_t)agents), *xe = col + 5 * (size_t)agents;
    int32_t *skip = malloc(sizeof(int32_t) * 5 * (size_t)agents), *conv = skip + agents, *eps_run = conv + agents, *rules = eps_run + agents, *xh = rules + agents;
    if (!col || !reward || !skip || n < 1 || (sets && nsets < 1)) return -1;
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    d.agent.seed = seed; d.agent.env_id_base = id_base;
    for (e = 0; e < agents; e++) { xe[e] = eps[e % n]; xh[e] = horizon[e % n]; }
    memset(&ex, 0, sizeof ex);
    ex.epsilon = xe; ex.horizon = xh;
    b = frirl_hip_batch_create(&d);
    if (!b) five_dropin_fatal("frirl_demo_batch_run_explore(create)", FRIRL_HIP_ENODEV);
    if (sets) {
        for (e = 0; e < agents; e++) {
            for (k = 0; k < 5; k++) col[(size_t)k * agents + e] = sets[6 * (size_t)(e % nsets) + k];
            skip[e] = (int32_t)sets[6 * (size_t)(e % nsets) + 5];
        }
        rows.alpha = col; rows.gamma = col + agents; rows.qdiff_pos_boundary = col + 2 * (size_t)agents; rows.qdiff_neg_boundary = col + 3 * (size_t)agents;
        rows.weight_significant = col + 4 * (size_t)agents; rows.skip_rules = skip;
        rc = frirl_hip_batch_set_hparams(b, &rows);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_explore(hparams)", rc);
    }
    rc = frirl_hip_batch_set_exploration(b, &ex);
    if (rc) five_dropin_fatal("frirl_demo_batch_run_explore(set)", rc);
    rc = frirl_hip_batch_train(b, max_episodes, &episodes);
    if (rc) five_dropin_fatal("frirl_demo_batch_run_explore(train)", rc);
    rc = frirl_hip_batch_agent_report(b, conv, eps_run, rules, NULL, reward);
    if (rc) five_dropin_fatal("frirl_demo_batch_run_explore(report)", rc);
    for (pass = 0; pass < (sets ? 2 : 1); pass++) {                /* the agents grouped by exploration line, then by hyper-parameter set */
        const int groups = pass ? nsets : n;
        for (s = 0; s < groups && s < agents; s++) {
            long long cnt = 0, nconv = 0, ep_sum = 0, rule_sum = 0;
            int ep_max = 0;
            double rew_sum = 0.0;
            for (e = s; e < agents; e += groups) {
                cnt++; nconv += conv[e] != 0; ep_sum += eps_run[e]; rule_sum += rules[e]; rew_sum += reward[e];
                if (eps_run[e] > ep_max) ep_max = eps_run[e];
            }
            if (!pass) total += (int)nconv;
            if (verbose)
                printf("%s %s: %s %d agents %lld converged %lld mean-episodes %.3f max-episodes %d mean-rules %.3f mean-reward %.6f\n", pass ? "hparams" : "explore", env,
                       pass ? "set" : "line", s, cnt, nconv, (double)ep_sum / cnt, ep_max, (double)rule_sum / cnt, rew_sum / cnt);
        }
    }
    frirl_hip_batch_destroy(b);
    demo_desc_free(&mm);
    free(col); free(reward); free(skip);
    return total;
}

/* ---- a TD target per agent: frirl_demo --agents N [--explore FILE] --target sarsa|q  or  --target-rows FILE ------------------------------
 * FILE: one 0 (SARSA) or 1 (Q) per line; `#` starts a comment; blank lines are skipped.  *target = malloc'ed [*n]; err receives
 * "line N: why" for the first malformed line, or why the file is unusable. */
int frirl_demo_parse_target(const char *path, unsigned char **target, int *n_out, char *err, size_t err_len)
{
    char line[512];
    int lineno = 0, n = 0, cap = 0;
    unsigned char *ot = NULL;
    FILE *fp = fopen(path, "r");
    *target = NULL; *n_out = 0;
    if (!fp) { snprintf(err, err_len, "cannot open %s", path); return -1; }
    while (fgets(line, sizeof line, fp)) {
        double v;
        char tail[2], *hash = strchr(line, '#');
        int got;
        lineno++;
        if (!strchr(line, '\n') && !feof(fp)) { snprintf(err, err_len, "line %d: longer than %d characters", lineno, (int)sizeof line - 2); goto bad; }
        if (hash) *hash = '\0';
        if (line[strspn(line, " \t\r\n")] == '\0') continue;
        got = sscanf(line, "%lf %1s", &v, tail);
        if (got != 1) { snprintf(err, err_len, "line %d: expected 1 value (target), found %s", lineno, got > 1 ? "more" : "fewer"); goto bad; }
        if (!(v == 0.0 || v == 1.0)) { snprintf(err, err_len, "line %d: target %g is neither 0 (SARSA) nor 1 (Q)", lineno, v); goto bad; }
        if (n == cap) {
            unsigned char *gt;
            cap = cap ? 2 * cap : 16;
            gt = realloc(ot, (size_t)cap);
            if (!gt) { snprintf(err, err_len, "out of memory"); goto bad; }
            ot = gt;
        }
        ot[n++] = (unsigned char)v;
    }
    fclose(fp);
    if (n == 0) { snprintf(err, err_len, "%s holds no target", path); free(ot); return -1; }
    *target = ot; *n_out = n;
    return 0;
bad:
    free(ot); fclose(fp);
    return -1;
}

/* The run behind frirl_demo_batch_run_target and frirl_demo_batch_run_expected (`who`: the one that calls, for fatal errors).  `agents`
 * agents of a demo in one persistent-learner run, every agent under its byte of ONE per-agent column -- with_expected == 0: the TD target
 * target[e mod nt] (HOST [nt], the column of frirl_demo_parse_target; NULL: target_all for every agent), set with
 * frirl_hip_batch_set_target; with_expected != 0: the expected-SARSA flag expected[e mod nf] (frirl_demo_parse_expected; NULL:
 * expected_all), set with frirl_hip_batch_set_expected -- and, eps != NULL, exploring under pair e mod nx as in
 * frirl_demo_batch_run_explore.  Then frirl_hip_batch_train, the `batch ENV:` report line with the choice at its end and, with eps, one
 * `explore ENV: line s ...` line per pair.  Returns the converged agents, or -1. */
static int demo_batch_run_td(const char *who, const char *env, int agents, int max_episodes, const double *eps, const int *horizon, int nx, unsigned long long seed,
                             unsigned long long id_base, const unsigned char *target, int nt, int target_all, int with_expected, const unsigned char *expected,
                             int nf, int expected_all, int verbose)
{
    int nant = 0, episodes = 0, rc, e, s, nset = 0;      /* nset: agents whose byte is 1 (target Q / expected) */
    char where[96];
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_batch *b;
    frirl_hip_batch_stats_t st;
    double *xe = malloc(sizeof(double) * 2 * (size_t)agents), *reward = xe ? xe + agents : NULL;
    int32_t *xh = malloc(sizeof(int32_t) * 4 * (size_t)agents), *conv = xh ? xh + agents : NULL, *eps_run = xh ? conv + agents : NULL, *rules = xh ? eps_run + agents : NULL;
    uint8_t *col = malloc((size_t)(agents > 0 ? agents : 1));
    if (!xe || !xh || !col || agents < 1 || (eps && nx < 1) || (target && nt < 1) || (expected && nf < 1)) return -1;
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    if (eps) { d.agent.seed = seed; d.agent.env_id_base = id_base; }
    b = frirl_hip_batch_create(&d);
    if (!b) { snprintf(where, sizeof where, "%s(create)", who); five_dropin_fatal(where, FRIRL_HIP_ENODEV); }
    if (eps) {
        frirl_hip_explore_rows ex;
        for (e = 0; e < agents; e++) { xe[e] = eps[e % nx]; xh[e] = horizon[e % nx]; }
        memset(&ex, 0, sizeof ex);
        ex.epsilon = xe; ex.horizon = xh;
        rc = frirl_hip_batch_set_exploration(b, &ex);
        if (rc) { snprintf(where, sizeof where, "%s(explore)", who); five_dropin_fatal(where, rc); }
    }
    if (with_expected) {
        for (e = 0; e < agents; e++) { col[e] = expected ? expected[e % nf] : (uint8_t)expected_all; nset += col[e] != 0; }
        rc = frirl_hip_batch_set_expected(b, expected ? col : NULL, expected ? 0 : expected_all);
        if (rc) { snprintf(where, sizeof where, "%s(set)", who); five_dropin_fatal(where, rc); }
    } else {
        for (e = 0; e < agents; e++) { col[e] = target ? target[e % nt] : (uint8_t)target_all; nset += col[e] == FRIRL_HIP_TARGET_Q; }
        rc = frirl_hip_batch_set_target(b, target ? col : NULL, target ? FRIRL_HIP_TARGET_SARSA : target_all);
        if (rc) { snprintf(where, sizeof where, "%s(set)", who); five_dropin_fatal(where, rc); }
    }
    rc = frirl_hip_batch_train(b, max_episodes, &episodes);
    if (rc) { snprintf(where, sizeof where, "%s(train)", who); five_dropin_fatal(where, rc); }
    rc = frirl_hip_batch_stats(b, &st);
    if (rc) { snprintf(where, sizeof where, "%s(stats)", who); five_dropin_fatal(where, rc); }
    if (verbose) {
        printf("batch %s: agents %lld episodes %d converged %lld env-steps %lld mean-rules %.3f mean-reward %.6f (min %.6f max %.6f) %s ", env,
               (long long)st.agents, episodes, (long long)st.converged, (long long)st.total_env_steps, st.rules_sum / st.agents,
               st.reward_sum / st.agents, st.reward_min, st.reward_max, with_expected ? "expected" : "target");
        if (with_expected && expected) printf("rows (%d of %d agents expected)\n", nset, agents);
        else if (with_expected) printf("%s\n", expected_all ? "all" : "none");
        else if (target) printf("rows (%d of %d agents q)\n", nset, agents);
        else printf("%s\n", target_all == FRIRL_HIP_TARGET_Q ? "q" : "sarsa");
    }
    if (eps && verbose) {
        rc = frirl_hip_batch_agent_report(b, conv, eps_run, rules, NULL, reward);
        if (rc) { snprintf(where, sizeof where, "%s(report)", who); five_dropin_fatal(where, rc); }
        for (s = 0; s < nx && s < agents; s++) {
            long long cnt = 0, nconv = 0, ep_sum = 0, rule_sum = 0;
            int ep_max = 0;
            double rew_sum = 0.0;
            for (e = s; e < agents; e += nx) {
                cnt++; nconv += conv[e] != 0; ep_sum += eps_run[e]; rule_sum += rules[e]; rew_sum += reward[e];
                if (eps_run[e] > ep_max) ep_max = eps_run[e];
            }
            printf("explore %s: line %d agents %lld converged %lld mean-episodes %.3f max-episodes %d mean-rules %.3f mean-reward %.6f\n", env, s, cnt, nconv,
                   (double)ep_sum / cnt, ep_max, (double)rule_sum / cnt, rew_sum / cnt);
        }
    }
    frirl_hip_batch_destroy(b);
    demo_desc_free(&mm);
    free(xe); free(xh); free(col);
    return (int)st.converged;
}

int frirl_demo_batch_run_target(const char *env, int agents, int max_episodes, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                unsigned long long id_base, const unsigned char *target, int nt, int target_all, int verbose)
{
    return demo_batch_run_td("frirl_demo_batch_run_target", env, agents, max_episodes, eps, horizon, nx, seed, id_base, target, nt, target_all, 0, NULL, 0, 0, verbose);
}

/* ---- expected SARSA per agent: frirl_demo --agents N [--explore FILE] --expected  or  --expected-rows FILE -------------------------------
 * FILE: one 0 or 1 per line; `#` starts a comment; blank lines are skipped.  *expected = malloc'ed [*n]; err receives "line N: why"
 * for the first malformed line, or why the file is unusable. */
int frirl_demo_parse_expected(const char *path, unsigned char **expected, int *n_out, char *err, size_t err_len)
{
    char line[512];
    int lineno = 0, n = 0, cap = 0;
    unsigned char *ot = NULL;
    FILE *fp = fopen(path, "r");
    *expected = NULL; *n_out = 0;
    if (!fp) { snprintf(err, err_len, "cannot open %s", path); return -1; }
    while (fgets(line, sizeof line, fp)) {
        double v;
        char tail[2], *hash = strchr(line, '#');
        int got;
        lineno++;
        if (!strchr(line, '\n') && !feof(fp)) { snprintf(err, err_len, "line %d: longer than %d characters", lineno, (int)sizeof line - 2); goto bad; }
        if (hash) *hash = '\0';
        if (line[strspn(line, " \t\r\n")] == '\0') continue;
        got = sscanf(line, "%lf %1s", &v, tail);
        if (got != 1) { snprintf(err, err_len, "line %d: expected 1 value (expected), found %s", lineno, got > 1 ? "more" : "fewer"); goto bad; }
        if (!(v == 0.0 || v == 1.0)) { snprintf(err, err_len, "line %d: expected %g is neither 0 nor 1", lineno, v); goto bad; }
        if (n == cap) {
            unsigned char *gt;
            cap = cap ? 2 * cap : 16;
            gt = realloc(ot, (size_t)cap);
            if (!gt) { snprintf(err, err_len, "out of memory"); goto bad; }
            ot = gt;
        }
        ot[n++] = (unsigned char)v;
    }
    fclose(fp);
    if (n == 0) { snprintf(err, err_len, "%s holds no flag", path); free(ot); return -1; }
    *expected = ot; *n_out = n;
    return 0;
bad:
    free(ot); fclose(fp);
    return -1;
}

/* frirl_demo_batch_run_target with frirl_hip_batch_set_expected in place of _set_target: agent e learns towards the expectation where
 * expected[e mod nf] is 1 (NULL: expected_all for every agent); the `batch ENV:` line ends in the choice. */
int frirl_demo_batch_run_expected(const char *env, int agents, int max_episodes, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                  unsigned long long id_base, const unsigned char *expected, int nf, int expected_all, int verbose)
{
    return demo_batch_run_td("frirl_demo_batch_run_expected", env, agents, max_episodes, eps, horizon, nx, seed, id_base, NULL, 0, 0, 1, expected, nf, expected_all, verbose);
}

/* ---- selection inside a population: frirl_demo --agents N --select G --select-episodes M --select-parents P --select-replace K ----------
 * G generations of frirl_hip_batch_train(M + 1) followed by frirl_hip_batch_select (every agent evaluated from `rows` start states, as
 * --evaluate maps them; the `replace` worst become copies of the `parents` best, with `inherit` also of their rows), one `select ENV:
 * generation g ...` line each; then training goes on to max_episodes and the report line follows.  sets / eps + horizon: the sweeps of
 * frirl_demo_batch_run_hparams / _explore, or NULL.  Returns the number of converged agents, or -1.
 * With spec != NULL (frirl_demo_batch_run_evolve) the selection is frirl_hip_batch_evolve_step and the line ends in ` perturbed K`. */
static int demo_batch_run_select(const char *env, int agents, int max_episodes, int generations, int gen_episodes, int parents, int replace, int inherit,
                                 int rows, double spread, const double *units, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                 unsigned long long id_base, const double *sets, int nsets, const frirl_hip_perturb_spec *spec, int verbose)
{
    int nant = 0, ns, episodes = 0, rc, e, k, g;
    frirl_hip_batch_desc d;
    struct demo_desc_mem mm;
    frirl_hip_batch *b;
    frirl_hip_batch_stats_t st;
    frirl_hip_rollout_score *sc;
    double *col, *start;
    int32_t *skip, *xh;
    if (agents < 1 || generations < 1 || gen_episodes < 1 || rows < 1 || !units || !(spread >= 0.0) || (eps && nx < 1) || (sets && nsets < 1)) return -1;
    if (demo_desc_build(env, agents, &d, &mm, &nant) != 0) return -1;
    ns = nant - 1;
    if (eps) { d.agent.seed = seed; d.agent.env_id_base = id_base; }
    sc = malloc(sizeof *sc * (size_t)agents);
    col = malloc(sizeof(double) * 6 * (size_t)agents);
    skip = malloc(sizeof(int32_t) * 2 * (size_t)agents);
    start = malloc(sizeof(double) * (size_t)agents * (size_t)rows * (size_t)ns);
    if (!sc || !col || !skip || !start) return -1;
    xh = skip + agents;
    demo_row_starts(&d, &mm, agents, rows, ns, spread, units, start);
    b = frirl_hip_batch_create(&d);
    if (!b) five_dropin_fatal("frirl_demo_batch_run_select(create)", FRIRL_HIP_ENODEV);
    if (sets) {
        frirl_hip_hparam_rows hp;
        for (e = 0; e < agents; e++) {
            for (k = 0; k < 5; k++) col[(size_t)k * agents + e] = sets[6 * (size_t)(e % nsets) + k];
            skip[e] = (int32_t)sets[6 * (size_t)(e % nsets) + 5];
        }
        hp.alpha = col; hp.gamma = col + agents; hp.qdiff_pos_boundary = col + 2 * (size_t)agents; hp.qdiff_neg_boundary = col + 3 * (size_t)agents;
        hp.weight_significant = col + 4 * (size_t)agents; hp.skip_rules = skip;
        rc = frirl_hip_batch_set_hparams(b, &hp);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_select(hparams)", rc);
    }
    if (eps) {
        frirl_hip_explore_rows ex;
        double *xe = col + 5 * (size_t)agents;
        for (e = 0; e < agents; e++) { xe[e] = eps[e % nx]; xh[e] = horizon[e % nx]; }
        memset(&ex, 0, sizeof ex);
        ex.epsilon = xe; ex.horizon = xh;
        rc = frirl_hip_batch_set_exploration(b, &ex);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_select(explore)", rc);
    }
    for (g = 0; g < generations; g++) {
        frirl_hip_select_result res;
        rc = frirl_hip_batch_train(b, gen_episodes + 1, &episodes);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_select(train)", rc);
        if (spec) {
            frirl_hip_evolve_result ev;
            int32_t successes = 0;
            double reward = 0.0;
            rc = frirl_hip_batch_evolve_step(b, rows, start, parents, replace, inherit, spec, &ev);
            if (rc == 0) rc = frirl_hip_batch_evolve_best_score(b, &successes, &reward);
            if (rc) five_dropin_fatal("frirl_demo_batch_run_evolve(evolve step)", rc);
            if (verbose)
                printf("select %s: generation %d best %d successes %d reward %.6f replaced %d rules_copied %lld perturbed %d\n", env, g, (int)ev.best, (int)successes,
                       reward, (int)ev.replaced, (long long)ev.rules_copied, (int)ev.perturbed);
            continue;
        }
        rc = frirl_hip_batch_select(b, rows, start, parents, replace, inherit, sc, NULL, &res);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_select(select)", rc);
        if (verbose)
            printf("select %s: generation %d best %d successes %d reward %.6f replaced %d rules_copied %lld\n", env, g, (int)res.best, (int)sc[res.best].successes,
                   sc[res.best].reward_sum, (int)res.replaced, (long long)res.rules_copied);
    }
    rc = frirl_hip_batch_stats(b, &st);
    if (rc) five_dropin_fatal("frirl_demo_batch_run_select(stats)", rc);
    if (max_episodes - (int)st.episodes_max > 1) {
        rc = frirl_hip_batch_train(b, max_episodes - (int)st.episodes_max, &episodes);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_select(train on)", rc);
        rc = frirl_hip_batch_stats(b, &st);
        if (rc) five_dropin_fatal("frirl_demo_batch_run_select(stats)", rc);
    }
    if (verbose)                    /* the report line of frirl_demo --agents N; episodes = the most any agent ran */
        printf("batch %s: agents %lld episodes %d converged %lld env-steps %lld mean-rules %.3f mean-reward %.6f (min %.6f max %.6f)\n", env,
               (long long)st.agents, (int)st.episodes_max, (long long)st.converged, (long long)st.total_env_steps, st.rules_sum / st.agents,
               st.reward_sum / st.agents, st.reward_min, st.reward_max);
    frirl_hip_batch_destroy(b);
    demo_desc_free(&mm);
    free(sc); free(col); free(skip); free(start);
    return (int)st.converged;
}

int frirl_demo_batch_run_select(const char *env, int agents, int max_episodes, int generations, int gen_episodes, int parents, int replace, int inherit,
                                int rows, double spread, const double *units, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                unsigned long long id_base, const double *sets, int nsets, int verbose)
{
    return demo_batch_run_select(env, agents, max_episodes, generations, gen_episodes, parents, replace, inherit, rows, spread, units, eps, horizon, nx, seed, id_base,
                                 sets, nsets, NULL, verbose);
}

/* ---- population-based training: frirl_demo ... --select G ... --select-perturb / --select-flip / --select-seed ------------------------ */
static void demo_perturb_spec(const struct frirl_demo_perturb *p, frirl_hip_perturb_spec *spec)
{
    memset(spec, 0, sizeof *spec);
    spec->columns = p->columns;
    spec->seed = p->seed;
    memcpy(spec->down, p->down, sizeof spec->down); memcpy(spec->up, p->up, sizeof spec->up);
    memcpy(spec->lo, p->lo, sizeof spec->lo); memcpy(spec->hi, p->hi, sizeof spec->hi);
    memcpy(spec->flip, p->flip, sizeof spec->flip);
}

int frirl_demo_perturb_column(const char *name)
{
    int c;
    for (c = 0; name && c < 8; c++)
        if (!strcmp(name, frirl_hip_perturb_column_name(c))) return c;
    return -1;
}

int frirl_demo_perturb_check(const struct frirl_demo_perturb *p, int have_hparams, int have_explore, char *err, size_t err_len)
{
    frirl_hip_perturb_spec spec;
    int c;
    if (!p || !err || err_len < 1) return -1;
    demo_perturb_spec(p, &spec);
    if (frirl_hip_perturb_spec_check(&spec) != 0) { snprintf(err, err_len, "%s", frirl_hip_last_error()); return -1; }
    for (c = 0; c < 8; c++) {
        const int with_hparams = c <= FRIRL_HIP_PERTURB_WEIGHT_SIGNIFICANT || c == FRIRL_HIP_PERTURB_SKIP_RULES;
        const int with_explore = c == FRIRL_HIP_PERTURB_EPSILON || c == FRIRL_HIP_PERTURB_HORIZON;
        if (!(p->columns >> c & 1)) continue;
        if (with_hparams ? have_hparams : with_explore ? have_explore : 0) continue;
        snprintf(err, err_len, "column %s is perturbed but the run does not set it: %s", frirl_hip_perturb_column_name(c),
                 with_hparams ? "give --hparams FILE" : with_explore ? "give --explore FILE" : "--select goes with neither --target nor --expected");
        return -1;
    }
    return 0;
}

int frirl_demo_batch_run_evolve(const char *env, int agents, int max_episodes, int generations, int gen_episodes, int parents, int replace, int inherit,
                                int rows, double spread, const double *units, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                unsigned long long id_base, const double *sets, int nsets, const struct frirl_demo_perturb *perturb, int verbose)
{
    frirl_hip_perturb_spec spec;
    if (!perturb) return -1;
    demo_perturb_spec(perturb, &spec);
    return demo_batch_run_select(env, agents, max_episodes, generations, gen_episodes, parents, replace, inherit, rows, spread, units, eps, horizon, nx, seed, id_base,
                                 sets, nsets, &spec, verbose);
}
