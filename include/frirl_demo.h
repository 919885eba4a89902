/*
 * frirl_demo.h -- the three demo environments of the reference (examples/mountaincar, cartpole, acrobot)
 * packaged in the drop-in library: descriptors + host callbacks, so that drivers and bindings on machines
 * without the reference tree can run them.  Additive API (not in the reference).
 */
#ifndef FRIRL_DEMO_H
#define FRIRL_DEMO_H

#include "frirl_types.h"

int frirl_demo_setup(struct frirl_desc *fr, const char *env);     /* "mountaincar" | "cartpole" | "acrobot" */
void frirl_demo_release(struct frirl_desc *fr);
/* flat description for bindings; u/ve [ (nstates+1) * U ], grid [ (nstates+1) * 64 ]; pass u = ve = NULL to query sizes */
/* tables of ANY environment from its dimensions (state dims 0..nstates-1, the action dim nstates): universes, VE rows
 * (frirl_init_ve) and the actions' VE values (frirl_init.c:156-158); values [nstates+1][64].  frirl_demo_describe = a demo's
 * setup + this.  0, or -1 on a bad argument. */
int frirl_describe_tables(int nstates, int U, const int *values_len, const double *values, const double *values_steep,
                          const double *universe_div, double *u, double *ve, double *action_ve);
int frirl_demo_describe(const char *env, int *nstates, int *U, int *A, double *u, double *ve, double *grid, int *grid_len,
                        double *grid_div, double *values_def, double *action_ve, double *hparams, int *max_steps);

/* Many independent agents of one demo on the GPU (frirl_hip_batch_*): every agent starts from the 2^nant corner
 * rule base and learns until its rule base is complete (at most max_episodes-1 episodes).  Prints one summary line;
 * when out_txt != NULL the rule base of agent 0 is written there in the reference's text format.
 * Returns the number of converged agents, or -1 on error. */
int frirl_demo_batch_run(const char *env, int agents, int max_episodes, const char *out_txt, int verbose);
/* the same, followed by the rule-base reduction (strategy 1 | 2, frirl_sequential_run.c:170-350) of agent 0's rule base on the
 * GPU (frirl_hip_batch_reduce); out_txt then holds the REDUCED rule base.  reduce_strategy 0 = frirl_demo_batch_run. */
int frirl_demo_batch_run_reduce(const char *env, int agents, int max_episodes, int reduce_strategy, const char *out_txt, int verbose);
/* the same; load_bin != NULL: instead of learning, every agent gets a rule base from that .frirlrb.bin file (written by the
 * reference, by the drop-in library or by frirl_hip_batch_save_rulebases) and replays one greedy episode on it
 * (frirl_test_run), then the optional reduction */
int frirl_demo_batch_run_ex(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                            const char *out_txt, int verbose);   /* save_bin != NULL: all agents' rule bases (before the reduction) go there */
/* the same, but the reduction covers EVERY agent's rule base in one batched run (frirl_hip_batch_reduce_all) instead of agent 0's
 * alone; prints one summary line: agents reduced, rules before -> after summed over the agents, rounds, replays */
int frirl_demo_batch_run_reduce_all(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                                    const char *out_txt, int verbose);
/* the same with every removal validated against K start states per agent (frirl_hip_batch_reduce_all_starts, drop_bad_starts = 1): the
 * rows of frirl_demo_batch_run_evaluate (row 0 = agent.values_def; units HOST [agents][K][nstates]), 1 <= K <= 256.  For K > 1 the
 * summary line also says how many of the agents * K start states were used; K == 1 prints the line of frirl_demo_batch_run_reduce_all */
int frirl_demo_batch_run_reduce_all_starts(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                                           const char *out_txt, int K, double spread, const double *units, int verbose);
/* the same rows, but every removal validated on the POLICY MAP at the points the agent's greedy policy visits from them
 * (frirl_hip_batch_reduce_all_map, cap 512): only_successful != 0 = the points of the starts whose episode succeeds.  Prints one
 * "reduced-map:" line with the totals */
int frirl_demo_batch_run_reduce_all_map(const char *env, int agents, int max_episodes, int reduce_strategy, const char *load_bin, const char *save_bin,
                                        const char *out_txt, int K, double spread, const double *units, int only_successful, int verbose);
/* Population evaluation: the agents learn (or, load_bin != NULL, load their rule bases), then EVERY agent is rolled out greedily on its
 * own rule base from K start states (frirl_hip_batch_evaluate): row 0 = agent.values_def, row j >= 1 = values_def[k] + spread *
 * units[e][j][k] * (largest - smallest grid value of dimension k), clipped to the grid; units HOST [agents][K][nstates] in -1..1.
 * Prints one summary line (agents, rows, share of successful rows, mean steps, mean / min / max reward) and the best agent.
 * Returns the best agent's index, or -1 on error. */
int frirl_demo_batch_run_evaluate(const char *env, int agents, int max_episodes, const char *load_bin, const char *save_bin, int K, double spread,
                                  const double *units, int verbose);
/* The same, then -- teach_episodes >= 1 -- the best agent teaches every other agent teach_episodes greedy episodes in teach_passes
 * passes (frirl_hip_batch_teach), one `taught:` line with the fields of frirl_hip_teach_result is printed, and the evaluation runs and
 * prints again.  teach_episodes == 0 is frirl_demo_batch_run_evaluate.  Returns the best agent of the last evaluation, or -1. */
int frirl_demo_batch_run_evaluate_teach(const char *env, int agents, int max_episodes, const char *load_bin, const char *save_bin, int K, double spread,
                                        const double *units, int teach_episodes, int teach_passes, int verbose);

/* A hyper-parameter sweep in one run (frirl_demo --agents N --hparams FILE).  frirl_demo_parse_hparams reads FILE: one set per line as
 * `alpha gamma qdiff_pos qdiff_neg weight_thr skip_rules`, `#` starts a comment, blank lines are skipped; *sets = malloc'ed
 * [*nsets][6] (the caller frees it).  -1 with err = "line N: why" for the first malformed line (not six numbers, a value that is not
 * finite, qdiff_pos < qdiff_neg, weight_thr < 0, skip_rules not 0 / 1), or why the file cannot be used (unreadable, no set in it).
 * No device is touched.
 * frirl_demo_batch_run_hparams: agent e learns under set e mod nsets (frirl_hip_batch_set_hparams, frirl_hip_batch_train: the
 * persistent learner), then one line per set: set index, agents, converged, mean and max episodes, mean rules, mean reward of the
 * last episode (frirl_hip_batch_agent_report).  Returns the number of converged agents, or -1. */
int frirl_demo_parse_hparams(const char *path, double **sets, int *nsets, char *err, size_t err_len);
int frirl_demo_batch_run_hparams(const char *env, int agents, int max_episodes, const double *sets, int nsets, int verbose);

/* An exploration sweep in one run (frirl_demo --agents N --explore FILE [--hparams FILE] [--seed S]).  frirl_demo_parse_explore
 * reads FILE: one `epsilon horizon` pair per line (frirl_hip_explore_rows: the agent's exploration rate and the number of episodes
 * over which it falls linearly to zero, 0 = constant), `#` starts a comment, blank lines are skipped; *eps and *horizon = malloc'ed
 * [*n] (the caller frees them).  -1 with err = "line N: why" for the first malformed line (not two numbers, epsilon outside [0, 1],
 * a horizon that is negative, fractional or above 2^30), or why the file cannot be used.  No device is touched.
 * frirl_demo_batch_run_explore: agent e (global id id_base + e, stream seed `seed`) explores under pair e mod n and, with sets != NULL, learns
 * under hyper-parameter set e mod nsets ([nsets][6], frirl_demo_parse_hparams; NULL: the demo's own values) -- one run of the
 * persistent learner (frirl_hip_batch_set_exploration, frirl_hip_batch_train), then one `explore ENV: line s ...` line per pair in
 * the format of the `hparams` lines, followed by those when sets are given.  Returns the number of converged agents, or -1. */
int frirl_demo_parse_explore(const char *path, double **eps, int **horizon, int *n, char *err, size_t err_len);
int frirl_demo_batch_run_explore(const char *env, int agents, int max_episodes, const double *eps, const int *horizon, int n, unsigned long long seed,
                                 unsigned long long id_base, const double *sets, int nsets, int verbose);

/* Selection inside a population (frirl_demo --agents N --select G --select-episodes M --select-parents P --select-replace K
 * [--select-inherit] [--evaluate n] [--hparams FILE] [--explore FILE]): G generations of frirl_hip_batch_train(M + 1) followed by
 * frirl_hip_batch_select -- every agent evaluated from `rows` start states (units / spread as frirl_demo_batch_run_evaluate maps them), the
 * `replace` worst replaced by copies of the `parents` best, with inherit != 0 also of their rows -- and one line per generation,
 *     select ENV: generation g best B successes S reward R replaced K rules_copied C
 * then training goes on to max_episodes and the `batch ENV: ...` report line of frirl_demo --agents N follows.  sets ([nsets][6]) and
 * eps / horizon ([nx]): the sweeps of frirl_demo_batch_run_hparams / _explore, or NULL.  Returns the number of converged agents, or -1. */
int frirl_demo_batch_run_select(const char *env, int agents, int max_episodes, int generations, int gen_episodes, int parents, int replace, int inherit,
                                int rows, double spread, const double *units, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                unsigned long long id_base, const double *sets, int nsets, int verbose);

/* Population-based training (frirl_demo ... --select G ... [--select-perturb col:down:up:lo:hi]... [--select-flip col:p]...
 * [--select-seed S]): the run of frirl_demo_batch_run_select with every generation's selection through frirl_hip_batch_evolve_step,
 * the clones' rows perturbed as frirl_hip_perturb_rows defines it; the generation line ends in ` perturbed K`.  struct
 * frirl_demo_perturb holds the fields of frirl_hip_perturb_spec for a host that does not include frirl_hip.h.
 * frirl_demo_perturb_column: the column index of a name (alpha, gamma, weight_significant, epsilon, horizon, skip_rules, target,
 * expected), or -1.  frirl_demo_perturb_check: 0, or -1 with err = why the values are refused (frirl_hip_perturb_spec_check) or which
 * column the run does not set (alpha, gamma, weight_significant, skip_rules come with --hparams, epsilon and horizon with --explore;
 * a --select run sets neither target nor expected).  No device is touched by either. */
struct frirl_demo_perturb {
    unsigned columns;               /* bit c = column c is perturbed */
    int given;                      /* one of the three flags was given */
    unsigned long long seed;
    double down[5], up[5], lo[5], hi[5], flip[3];
};
int frirl_demo_perturb_column(const char *name);
int frirl_demo_perturb_check(const struct frirl_demo_perturb *p, int have_hparams, int have_explore, char *err, size_t err_len);
int frirl_demo_batch_run_evolve(const char *env, int agents, int max_episodes, int generations, int gen_episodes, int parents, int replace, int inherit,
                                int rows, double spread, const double *units, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                unsigned long long id_base, const double *sets, int nsets, const struct frirl_demo_perturb *perturb, int verbose);

/* A TD target per agent in one run (frirl_demo --agents N [--explore FILE] --target sarsa|q, or --target-rows FILE).
 * frirl_demo_parse_target reads FILE: one 0 (FRIRL_HIP_TARGET_SARSA) or 1 (FRIRL_HIP_TARGET_Q) per line, `#` starts a comment, blank
 * lines are skipped; *target = malloc'ed [*n] (the caller frees it).  -1 with err = "line N: why" for the first malformed line (not one
 * number, a value other than 0 or 1), or why the file cannot be used.  No device is touched.
 * frirl_demo_batch_run_target: agent e learns towards target[e mod nt] (NULL: target_all for every agent) and, with eps != NULL,
 * explores under pair e mod nx on the stream of `seed` and id_base as in frirl_demo_batch_run_explore -- one run of the persistent
 * learner (frirl_hip_batch_set_target, frirl_hip_batch_train), then the `batch ENV: ...` report line ending in `target sarsa`, `target q`
 * or `target rows (K of N agents q)`, followed with eps by the `explore ENV: line s ...` lines.  Returns the converged agents, or -1. */
int frirl_demo_parse_target(const char *path, unsigned char **target, int *n, char *err, size_t err_len);
int frirl_demo_batch_run_target(const char *env, int agents, int max_episodes, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                unsigned long long id_base, const unsigned char *target, int nt, int target_all, int verbose);

/* Expected SARSA per agent in one run (frirl_demo --agents N [--explore FILE] --expected, or --expected-rows FILE).
 * frirl_demo_parse_expected reads FILE: one 0 or 1 per line, `#` starts a comment, blank lines are skipped; *expected = malloc'ed [*n]
 * (the caller frees it).  -1 with err = "line N: why" for the first malformed line (not one number, a value other than 0 or 1), or why
 * the file cannot be used.  No device is touched.
 * frirl_demo_batch_run_expected: frirl_demo_batch_run_target with frirl_hip_batch_set_expected in place of _set_target -- agent e learns
 * towards the expectation under its own pick where expected[e mod nf] is 1 (NULL: expected_all for every agent); the `batch ENV: ...`
 * report line ends in `expected all`, `expected none` or `expected rows (K of N agents expected)`.  Returns the converged agents, or -1. */
int frirl_demo_parse_expected(const char *path, unsigned char **expected, int *n, char *err, size_t err_len);
int frirl_demo_batch_run_expected(const char *env, int agents, int max_episodes, const double *eps, const int *horizon, int nx, unsigned long long seed,
                                  unsigned long long id_base, const unsigned char *expected, int nf, int expected_all, int verbose);

/* `agents` agents over `gpus` devices of this node (0 = every visible device) through frirl_hip_multi_* (one batch + host thread per
 * device, per-episode report all-reduced with RCCL); out_txt = rule base of global agent 0.  Returns the converged agents or -1. */
/* many agents WITH the reference's rule-base exchange (frirl_omp_run: chunks of 9 episodes, merge_rb in both directions after each,
 * start states from gen_def_states) on one GPU; out_txt = the master's rule base.  Returns the number of merge rounds, or -1. */
int frirl_demo_merged_run(const char *env, int agents, int max_episodes, const char *out_txt, int verbose);
/* the same with the agents sharded over `gpus` devices (0 = all) and the rule-base exchange over RCCL (frirl_hip_multi_train_merged) */
int frirl_demo_multi_merged_run(const char *env, int agents, int gpus, int max_episodes, const char *out_txt, int verbose);
int frirl_demo_multi_run(const char *env, int agents, int gpus, int max_episodes, const char *out_txt, int verbose);

#endif
