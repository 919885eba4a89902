/*
 * demo.c -- the three demo applications driven through the drop-in C API (one binary, --env NAME).
 *
 * Own driver for machines without the reference tree (the GPU box): frirl_demo_setup() (demo_envs.c) fills
 * struct frirl_desc with the hyper-parameters of the reference's examples and host callbacks implementing
 * the same dynamics with libm trig; then frirl_init / frirl_run (construct mode) and the <env>.frirlrb.txt/.bin
 * dumps, exactly the sequence of the reference's examples.  The reference's own, unchanged example
 * sources also compile and link against these headers and this library.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "frirl.h"
#include "frirl_types_def.h"
#include "frirl_app_helpers.h"
#include "frirl_demo.h"
#include "demo_rows.h"

static int usage(const char *what)
{
    fprintf(stderr, "usage error: %s\n"
                    "usage: frirl_demo --env NAME --agents N [--load f.bin] [--save f.bin] --evaluate K [--spread F] [--teach-best M [--teach-passes P]]   (K >= 1 rows per agent, 0 <= F <= 1, M >= 1 episodes, 1 <= P <= 1024)\n"
                    "       frirl_demo --env NAME --agents N --reduce S --reduce-all --reduce-starts K [--spread F]   (S = 1 | 2, 1 <= K <= 256 start states per agent, 0 <= F <= 1)\n"
                    "       frirl_demo --env NAME --agents N --reduce S --reduce-all --reduce-map K [--spread F] [--reduce-map-all]   (removals validated on the policy map at the points visited from K start states; --reduce-map-all: of every start, not the successful ones alone)\n"
                    "       frirl_demo --env NAME --agents N --hparams FILE [--max-episodes M]   (a sweep in one run: FILE holds one set per line, `alpha gamma qdiff_pos qdiff_neg weight_thr skip_rules`, # comments; agent e takes line e mod L)\n"
                    "       frirl_demo --env NAME --agents N --explore FILE [--hparams FILE] [--seed S] [--id-base B] [--max-episodes M]   (an exploration sweep in one run: FILE holds one `epsilon horizon` pair per line, epsilon falling linearly to zero over `horizon` episodes, 0 = constant; agent e takes line e mod L; S seeds the exploration stream, agent e draws under the global id B + e)\n"
                    "       frirl_demo --env NAME --agents N [--hparams FILE] [--explore FILE] --select G --select-episodes M --select-parents P --select-replace K [--select-inherit] [--evaluate n] [--spread F]   (G generations of M episodes; after each, every agent is evaluated from n start states, default 1, and the K worst become copies of the P best, with --select-inherit also of their rows)\n"
                    "         with --select: [--select-perturb col:down:up:lo:hi]... [--select-flip col:p]... [--select-seed S]   (population-based training: a clone's row value is multiplied by down or up, a coin flip per agent, generation and column, and clamped to [lo, hi]; col = alpha | gamma | weight_significant | skip_rules with --hparams, epsilon | horizon with --explore; a 0 / 1 column flips with probability p)\n"
                    "       frirl_demo --env NAME --agents N [--explore FILE [--seed S] [--id-base B]] --target sarsa|q | --target-rows FILE [--max-episodes M]   (the TD target: every agent learns towards Q(s',a') of the action it takes, sarsa, or towards Q(s',g) of the greedy action, q; FILE holds one 0 (sarsa) or 1 (q) per line, agent e takes line e mod L)\n"
                    "       frirl_demo --env NAME --agents N [--explore FILE [--seed S] [--id-base B]] --expected | --expected-rows FILE [--max-episodes M]   (expected SARSA: a flagged agent learns towards the expectation of Q(s',.) under its own epsilon-greedy pick; FILE holds one 0 or 1 per line, agent e takes line e mod L)\n", what);
    return 2;
}

int main(int argc, char **argv)
{
    struct frirl_desc fr = frirl_desc_default;
    const char *env = "mountaincar";
    char name[128];
    int i, max_episodes = 0, fargc = 0, reduce = 0, agents = 0, gpus = -1, merge = 0, reduce_all = 0;
    const char *load_bin = NULL, *save_bin = NULL;
    int evaluate = -1;              /* --evaluate K: greedy roll-outs of every agent from K start states, -1 = not asked for */
    double spread = 0.15;           /* --spread F: rows 1 .. K-1 start at values_def +- F * span */
    int teach_best = 0;             /* --teach-best M: after the evaluation the best agent teaches every other agent M greedy episodes, 0 = not asked for */
    int teach_passes = 1;           /* --teach-passes P: passes over the teacher's log */
    int reduce_starts = 0;          /* --reduce-starts K: with --reduce-all, every removal is validated against K start states per agent, 0 = not asked for */
    int reduce_map = 0;             /* --reduce-map K: with --reduce-all, every removal is validated on the policy map at the points visited from K start states, 0 = not asked for */
    int reduce_map_all = 0;         /* --reduce-map-all: the points of every start, not of the successful ones alone */
    const char *hparams = NULL;     /* --hparams FILE: with --agents, agent e learns under the hyper-parameter set on line e mod L of FILE */
    const char *explore = NULL;     /* --explore FILE: with --agents, agent e explores under the `epsilon horizon` pair on line e mod L of FILE */
    unsigned long long seed = 0;    /* --seed S: seed of the exploration stream (with --explore) */
    unsigned long long id_base = 0; /* --id-base B: global id of agent 0 on that stream (frirl_hip_agent.env_id_base; with --explore) */
    int stream_given = 0;           /* --seed or --id-base was given */
    int target_all = -1;            /* --target sarsa|q: every agent's TD target (FRIRL_HIP_TARGET_*), -1 = not asked for */
    const char *target_rows = NULL; /* --target-rows FILE: with --agents, agent e learns towards the target on line e mod L of FILE */
    int expected_all = 0;           /* --expected: every agent learns towards the expectation under its own pick (expected SARSA) */
    const char *expected_rows = NULL; /* --expected-rows FILE: with --agents, agent e is flagged by the 0 / 1 on line e mod L of FILE */
    int select_gen = 0;             /* --select G: generations of train + frirl_hip_batch_select, 0 = not asked for */
    int select_episodes = 0, select_parents = 0, select_replace = -1, select_inherit = 0;
    struct frirl_demo_perturb perturb;  /* --select-perturb col:down:up:lo:hi, --select-flip col:p, --select-seed S: the clones' rows are perturbed */
    char *fargv[16];
    memset(&perturb, 0, sizeof perturb);
    fargv[fargc++] = argv[0];
    for (i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--env") && i + 1 < argc) env = argv[++i];
        else if (!strcmp(argv[i], "--max-episodes") && i + 1 < argc) max_episodes = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--agents") && i + 1 < argc) agents = atoi(argv[++i]);      /* batched: N independent agents on the GPU */
        else if (!strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = atoi(argv[++i]);          /* with --agents: shard over G devices (0 = all), RCCL report */
        else if (!strcmp(argv[i], "--merge")) merge = 1;                                       /* with --agents: the agents exchange rule bases (frirl_omp_run) */
        else if (!strcmp(argv[i], "--load") && i + 1 < argc) load_bin = argv[++i];             /* batched: start from a .frirlrb.bin file */
        else if (!strcmp(argv[i], "--save") && i + 1 < argc) save_bin = argv[++i];             /* batched: all agents' rule bases to one .bin */
        else if (!strcmp(argv[i], "--reduce") && i + 1 < argc) reduce = atoi(argv[++i]);   /* construct, then reduce with strategy 1|2 */
        else if (!strcmp(argv[i], "--reduce-all")) reduce_all = 1;                              /* with --agents and --reduce: every agent's rule base, not agent 0's alone */
        else if (!strcmp(argv[i], "--evaluate") && i + 1 < argc) { evaluate = atoi(argv[++i]); if (evaluate < 1) return usage("--evaluate needs K >= 1"); }
        else if (!strcmp(argv[i], "--reduce-starts") && i + 1 < argc) { reduce_starts = atoi(argv[++i]); if (reduce_starts < 1 || reduce_starts > 256) return usage("--reduce-starts needs 1 <= K <= 256"); }
        else if (!strcmp(argv[i], "--reduce-map") && i + 1 < argc) { reduce_map = atoi(argv[++i]); if (reduce_map < 1 || reduce_map > 256) return usage("--reduce-map needs 1 <= K <= 256"); }
        else if (!strcmp(argv[i], "--reduce-map-all")) reduce_map_all = 1;
        else if (!strcmp(argv[i], "--hparams") && i + 1 < argc) hparams = argv[++i];
        else if (!strcmp(argv[i], "--explore") && i + 1 < argc) explore = argv[++i];
        else if (!strcmp(argv[i], "--target") && i + 1 < argc) { const char *v = argv[++i]; target_all = !strcmp(v, "sarsa") ? 0 : !strcmp(v, "q") ? 1 : -1; if (target_all < 0) return usage("--target needs sarsa or q"); }
        else if (!strcmp(argv[i], "--target-rows") && i + 1 < argc) target_rows = argv[++i];
        else if (!strcmp(argv[i], "--expected")) expected_all = 1;
        else if (!strcmp(argv[i], "--expected-rows") && i + 1 < argc) expected_rows = argv[++i];
        else if (!strcmp(argv[i], "--seed") && i + 1 < argc) { char *end; seed = strtoull(argv[++i], &end, 10); stream_given = 1; if (*end || end == argv[i]) return usage("--seed needs a whole number S >= 0"); }
        else if (!strcmp(argv[i], "--id-base") && i + 1 < argc) { char *end; id_base = strtoull(argv[++i], &end, 10); stream_given = 1; if (*end || end == argv[i]) return usage("--id-base needs a whole number B >= 0"); }
        else if (!strcmp(argv[i], "--spread") && i + 1 < argc) { spread = atof(argv[++i]); if (!(spread >= 0.0 && spread <= 1.0)) return usage("--spread needs 0 <= F <= 1"); }
        else if (!strcmp(argv[i], "--teach-best") && i + 1 < argc) { teach_best = atoi(argv[++i]); if (teach_best < 1) return usage("--teach-best needs M >= 1"); }
        else if (!strcmp(argv[i], "--teach-passes") && i + 1 < argc) { teach_passes = atoi(argv[++i]); if (teach_passes < 1 || teach_passes > 1024) return usage("--teach-passes needs 1 <= P <= 1024"); }
        else if (!strcmp(argv[i], "--select") && i + 1 < argc) { select_gen = atoi(argv[++i]); if (select_gen < 1) return usage("--select needs G >= 1 generations"); }
        else if (!strcmp(argv[i], "--select-episodes") && i + 1 < argc) { select_episodes = atoi(argv[++i]); if (select_episodes < 1) return usage("--select-episodes needs M >= 1"); }
        else if (!strcmp(argv[i], "--select-parents") && i + 1 < argc) { select_parents = atoi(argv[++i]); if (select_parents < 1) return usage("--select-parents needs P >= 1"); }
        else if (!strcmp(argv[i], "--select-replace") && i + 1 < argc) { select_replace = atoi(argv[++i]); if (select_replace < 0) return usage("--select-replace needs K >= 0"); }
        else if (!strcmp(argv[i], "--select-inherit")) select_inherit = 1;
        else if (!strcmp(argv[i], "--select-perturb") && i + 1 < argc) {
            char col[32];
            double v[4];
            int used = 0, c;
            const char *arg = argv[++i];
            if (sscanf(arg, "%31[^:]:%lf:%lf:%lf:%lf%n", col, &v[0], &v[1], &v[2], &v[3], &used) != 5 || arg[used] || (c = frirl_demo_perturb_column(col)) < 0 || c > 4)
                return usage("--select-perturb needs col:down:up:lo:hi with col one of alpha, gamma, weight_significant, epsilon, horizon");
            perturb.columns |= 1u << c;
            perturb.down[c] = v[0]; perturb.up[c] = v[1]; perturb.lo[c] = v[2]; perturb.hi[c] = v[3];
        }
        else if (!strcmp(argv[i], "--select-flip") && i + 1 < argc) {
            char col[32];
            double p;
            int used = 0, c;
            const char *arg = argv[++i];
            if (sscanf(arg, "%31[^:]:%lf%n", col, &p, &used) != 2 || arg[used] || (c = frirl_demo_perturb_column(col)) < 5)
                return usage("--select-flip needs col:p with col one of skip_rules, target, expected");
            perturb.columns |= 1u << c;
            perturb.flip[c - 5] = p;
        }
        else if (!strcmp(argv[i], "--select-seed") && i + 1 < argc) { char *end; perturb.seed = strtoull(argv[++i], &end, 10); perturb.given = 1; if (*end || end == argv[i]) return usage("--select-seed needs a whole number S >= 0"); }
        else if (fargc < 15) fargv[fargc++] = argv[i];
    }
    if (perturb.columns) perturb.given = 1;
    if (perturb.given && select_gen < 1) return usage("--select-perturb / --select-flip / --select-seed go with --select G");
    if (expected_all || expected_rows) {        /* expected SARSA per agent; --explore goes with it */
        const char *opt = expected_rows ? "--expected-rows" : "--expected";
        double *eps = NULL;
        int *horizon = NULL, nx = 0, nf = 0, rc;
        unsigned char *xf = NULL;
        char err[256], msg[256];
        if (expected_all && expected_rows) return usage("--expected and --expected-rows exclude each other");
        if (merge || gpus >= 0 || teach_best > 0) { snprintf(msg, sizeof msg, "%s does not go with --merge, --gpus or --teach-best: the rule-base exchange, frirl_hip_multi_* and the replay of a teacher's log take no expected SARSA", opt); return usage(msg); }
        if (agents < 1 || reduce || evaluate > 0 || load_bin || save_bin || hparams || select_gen > 0 || target_all >= 0 || target_rows) { snprintf(msg, sizeof msg, "%s goes with --agents N alone, or with --explore FILE (one device, trained from scratch)", opt); return usage(msg); }
        if (stream_given && !explore) return usage("--seed and --id-base go with --explore FILE");
        frirl_parse_cmdline(&fr, fargc, fargv);
        if (expected_rows && frirl_demo_parse_expected(expected_rows, &xf, &nf, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --expected-rows %s: %s\n", expected_rows, err);
            return 2;
        }
        if (explore && frirl_demo_parse_explore(explore, &eps, &horizon, &nx, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --explore %s: %s\n", explore, err);
            free(xf);
            return 2;
        }
        rc = frirl_demo_batch_run_expected(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, eps, horizon, nx, seed, id_base, xf, nf, expected_all, 1);
        free(xf); free(eps); free(horizon);
        return rc >= 0 ? 0 : 3;
    }
    if (target_all >= 0 || target_rows) {       /* a TD target per agent; --explore goes with it */
        const char *opt = target_rows ? "--target-rows" : "--target";
        double *eps = NULL;
        int *horizon = NULL, nx = 0, nt = 0, rc;
        unsigned char *tq = NULL;
        char err[256], msg[256];
        if (target_all >= 0 && target_rows) return usage("--target and --target-rows exclude each other");
        if (merge || gpus >= 0 || teach_best > 0) { snprintf(msg, sizeof msg, "%s does not go with --merge, --gpus or --teach-best: the rule-base exchange, frirl_hip_multi_* and the replay of a teacher's log take no TD target", opt); return usage(msg); }
        if (agents < 1 || reduce || evaluate > 0 || load_bin || save_bin || hparams || select_gen > 0) { snprintf(msg, sizeof msg, "%s goes with --agents N alone, or with --explore FILE (one device, trained from scratch)", opt); return usage(msg); }
        if (stream_given && !explore) return usage("--seed and --id-base go with --explore FILE");
        frirl_parse_cmdline(&fr, fargc, fargv);
        if (target_rows && frirl_demo_parse_target(target_rows, &tq, &nt, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --target-rows %s: %s\n", target_rows, err);
            return 2;
        }
        if (explore && frirl_demo_parse_explore(explore, &eps, &horizon, &nx, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --explore %s: %s\n", explore, err);
            free(tq);
            return 2;
        }
        rc = frirl_demo_batch_run_target(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, eps, horizon, nx, seed, id_base, tq, nt, target_all > 0, 1);
        free(tq); free(eps); free(horizon);
        return rc >= 0 ? 0 : 3;
    }
    if (select_gen > 0) {           /* generations of train + select; --evaluate n, --hparams and --explore go with it */
        double *sets = NULL, *eps = NULL, *units;
        int *horizon = NULL, nsets = 0, nx = 0, ns = 0, U = 0, A = 0, ms = 0, rc, rows = evaluate > 0 ? evaluate : 1;
        char err[256];
        if (merge) return usage("--select does not go with --merge: selection replaces rule bases, the exchange merges them");
        if (gpus >= 0) return usage("--select does not go with --gpus: selection across devices is not built");
        if (teach_best > 0) return usage("--select does not go with --teach-best: a clone takes the rule base over, it is not taught");
        if (agents < 1 || reduce || load_bin || save_bin) return usage("--select goes with --agents N (one device, trained from scratch, no --reduce)");
        if (select_episodes < 1 || select_parents < 1 || select_replace < 0) return usage("--select needs --select-episodes M, --select-parents P and --select-replace K");
        if (select_parents + select_replace > agents) return usage("--select-parents P + --select-replace K exceeds --agents N: a parent would be replaced");
        if (stream_given && !explore) return usage("--seed and --id-base go with --explore FILE");
        if (perturb.given && frirl_demo_perturb_check(&perturb, hparams != NULL, explore != NULL, err, sizeof err) != 0) return usage(err);
        frirl_parse_cmdline(&fr, fargc, fargv);
        if (frirl_demo_describe(env, &ns, &U, &A, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &ms) != 0) return 2;
        if (hparams && frirl_demo_parse_hparams(hparams, &sets, &nsets, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --hparams %s: %s\n", hparams, err);
            return 2;
        }
        if (explore && frirl_demo_parse_explore(explore, &eps, &horizon, &nx, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --explore %s: %s\n", explore, err);
            free(sets);
            return 2;
        }
        units = malloc(sizeof(double) * (size_t)agents * (size_t)rows * (size_t)ns);
        if (!units) return 1;
        frirl_demo_row_units(agents, rows, ns, units);
        if (perturb.given)
            rc = frirl_demo_batch_run_evolve(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, select_gen, select_episodes, select_parents, select_replace,
                                             select_inherit, rows, spread, units, eps, horizon, nx, seed, id_base, sets, nsets, &perturb, 1);
        else
            rc = frirl_demo_batch_run_select(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, select_gen, select_episodes, select_parents, select_replace,
                                             select_inherit, rows, spread, units, eps, horizon, nx, seed, id_base, sets, nsets, 1);
        free(units); free(sets); free(eps); free(horizon);
        return rc >= 0 ? 0 : 3;
    }
    if (select_episodes || select_parents || select_replace >= 0 || select_inherit) return usage("--select-episodes / -parents / -replace / -inherit go with --select G");
    if (evaluate > 0 && (agents < 1 || merge || gpus >= 0 || reduce)) return usage("--evaluate goes with --agents N (one device, no --merge / --reduce)");
    if (teach_best > 0 && evaluate < 1) return usage("--teach-best goes with --evaluate K");
    if (reduce_starts > 0 && (agents < 1 || !reduce_all || (reduce != 1 && reduce != 2) || merge || gpus >= 0))
        return usage("--reduce-starts goes with --agents N --reduce S --reduce-all (one device, no --merge)");
    if (reduce_map > 0 && reduce_starts > 0) return usage("--reduce-map and --reduce-starts exclude each other");
    if (reduce_map > 0 && (agents < 1 || !reduce_all || (reduce != 1 && reduce != 2) || merge || gpus >= 0))
        return usage("--reduce-map goes with --agents N --reduce S --reduce-all (one device, no --merge)");
    if (reduce_map_all && reduce_map < 1) return usage("--reduce-map-all goes with --reduce-map K");
    if (hparams && (merge || teach_best > 0)) return usage("--hparams does not go with --merge or --teach-best: the rule-base exchange and the replay of a teacher's log do not honour per-agent hyper-parameters");
    if (hparams && (agents < 1 || gpus >= 0 || reduce || evaluate > 0 || load_bin || save_bin)) return usage("--hparams goes with --agents N alone (one device, trained from scratch)");
    if (explore && (merge || teach_best > 0)) return usage("--explore does not go with --merge or --teach-best: the rule-base exchange and the replay of a teacher's log do not honour per-agent exploration");
    if (explore && (agents < 1 || gpus >= 0 || reduce || evaluate > 0 || load_bin || save_bin)) return usage("--explore goes with --agents N alone, or with --hparams FILE (one device, trained from scratch)");
    if (stream_given && !explore) return usage("--seed and --id-base go with --explore FILE");
    frirl_parse_cmdline(&fr, fargc, fargv);
    if (explore) {                  /* an exploration sweep (with --hparams: crossed with a hyper-parameter sweep): one persistent-learner run */
        double *sets = NULL, *eps = NULL;
        int *horizon = NULL, nsets = 0, n = 0, rc;
        char err[256];
        if (frirl_demo_parse_explore(explore, &eps, &horizon, &n, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --explore %s: %s\n", explore, err);
            return 2;
        }
        if (hparams && frirl_demo_parse_hparams(hparams, &sets, &nsets, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --hparams %s: %s\n", hparams, err);
            free(eps); free(horizon);
            return 2;
        }
        rc = frirl_demo_batch_run_explore(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, eps, horizon, n, seed, id_base, sets, nsets, 1);
        free(sets); free(eps); free(horizon);
        return rc >= 0 ? 0 : 3;
    }
    if (hparams) {                  /* a sweep: one persistent-learner run, one report line per set */
        double *sets = NULL;
        int nsets = 0, rc;
        char err[256];
        if (frirl_demo_parse_hparams(hparams, &sets, &nsets, err, sizeof err) != 0) {
            fprintf(stderr, "frirl_demo: --hparams %s: %s\n", hparams, err);
            return 2;
        }
        rc = frirl_demo_batch_run_hparams(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, sets, nsets, 1);
        free(sets);
        return rc >= 0 ? 0 : 3;
    }
    if (evaluate > 0) {             /* train (or --load), then every agent rolled out from K start states */
        int ns = 0, U = 0, A = 0, ms = 0, rc;
        double *units;
        if (frirl_demo_describe(env, &ns, &U, &A, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &ms) != 0) return 2;
        units = malloc(sizeof(double) * (size_t)agents * (size_t)evaluate * (size_t)ns);
        if (!units) return 1;
        frirl_demo_row_units(agents, evaluate, ns, units);
        if (teach_best > 0)
            rc = frirl_demo_batch_run_evaluate_teach(env, agents, load_bin ? 2 : (max_episodes > 0 ? max_episodes : fr.max_episodes), load_bin, save_bin, evaluate,
                                                     spread, units, teach_best, teach_passes, 1);
        else
            rc = frirl_demo_batch_run_evaluate(env, agents, load_bin ? 2 : (max_episodes > 0 ? max_episodes : fr.max_episodes), load_bin, save_bin, evaluate, spread,
                                               units, 1);
        free(units);
        return rc >= 0 ? 0 : 3;
    }
    if (agents > 0 && merge && gpus >= 0) {       /* rule-base exchange across devices */
        snprintf(name, sizeof name, "%s.multi.merged.frirlrb.txt", env);
        return frirl_demo_multi_merged_run(env, agents, gpus, max_episodes > 0 ? max_episodes : fr.max_episodes, name, 1) >= 0 ? 0 : 3;
    }
    if (agents > 0 && merge) {
        snprintf(name, sizeof name, "%s.merged.frirlrb.txt", env);
        return frirl_demo_merged_run(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, name, 1) >= 0 ? 0 : 3;
    }
    if (agents > 0 && gpus >= 0) {
        snprintf(name, sizeof name, "%s.multi.frirlrb.txt", env);
        return frirl_demo_multi_run(env, agents, gpus, max_episodes > 0 ? max_episodes : fr.max_episodes, name, 1) == agents ? 0 : 3;
    }
    if (agents > 0) {
        snprintf(name, sizeof name, "%s.batch.frirlrb.txt", env);
        if (reduce == 1 || reduce == 2) snprintf(name, sizeof name, "%s.batch.reduced%d.frirlrb.txt", env, reduce);
        if (reduce_map > 0) {       /* the rows --reduce-starts K would use */
            int ns = 0, U = 0, A = 0, ms = 0, rc;
            double *units;
            if (frirl_demo_describe(env, &ns, &U, &A, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &ms) != 0) return 2;
            units = malloc(sizeof(double) * (size_t)agents * (size_t)reduce_map * (size_t)ns);
            if (!units) return 1;
            frirl_demo_row_units(agents, reduce_map, ns, units);
            snprintf(name, sizeof name, "%s.batch.reducedmap%d.frirlrb.txt", env, reduce);
            rc = frirl_demo_batch_run_reduce_all_map(env, agents, load_bin ? 2 : (max_episodes > 0 ? max_episodes : fr.max_episodes), reduce, load_bin,
                                                     save_bin, name, reduce_map, spread, units, !reduce_map_all, 1);
            free(units);
            return rc >= 0 ? 0 : 3;
        }
        if (reduce_starts > 0) {    /* rows as --evaluate K --spread F maps them; row 0 = the agent's own start state */
            int ns = 0, U = 0, A = 0, ms = 0, rc;
            double *units;
            if (frirl_demo_describe(env, &ns, &U, &A, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &ms) != 0) return 2;
            units = malloc(sizeof(double) * (size_t)agents * (size_t)reduce_starts * (size_t)ns);
            if (!units) return 1;
            frirl_demo_row_units(agents, reduce_starts, ns, units);
            rc = frirl_demo_batch_run_reduce_all_starts(env, agents, load_bin ? 2 : (max_episodes > 0 ? max_episodes : fr.max_episodes), reduce, load_bin,
                                                        save_bin, name, reduce_starts, spread, units, 1);
            free(units);
            return rc >= 0 ? 0 : 3;
        }
        if (reduce_all && (reduce == 1 || reduce == 2))
            return frirl_demo_batch_run_reduce_all(env, agents, load_bin ? 2 : (max_episodes > 0 ? max_episodes : fr.max_episodes), reduce, load_bin, save_bin,
                                                   name, 1) >= 0 ? 0 : 3;
        if (load_bin) return frirl_demo_batch_run_ex(env, agents, 2, reduce, load_bin, save_bin, name, 1) >= 0 ? 0 : 3;
        return frirl_demo_batch_run_ex(env, agents, max_episodes > 0 ? max_episodes : fr.max_episodes, reduce, NULL, save_bin, name, 1) == agents ? 0 : 3;
    }
    if (frirl_demo_setup(&fr, env) != 0) return 2;
    if (max_episodes > 0) fr.max_episodes = max_episodes;
    if (frirl_init(&fr) != 0) { fprintf(stderr, "frirl_init failed\n"); return 1; }
    frirl_run(&fr, 1);
    if (reduce == 1 || reduce == 2) {          /* the reference runs this phase from a saved .bin (mountaincar.c:240-242); same code path */
        snprintf(name, sizeof name, "%s.frirlrb.txt", env);
        frirl_save_rb_to_text_file(&fr, name);
        fr.construct_rb = 0; fr.reduce_rb = 1; fr.reduction_strategy = (unsigned char)reduce;
        frirl_sequential_run(&fr);
        snprintf(name, sizeof name, "%s.reduced%d.frirlrb.txt", env, reduce);
        frirl_save_rb_to_text_file(&fr, name);
        printf("demo %s: reduced to %d rules (strategy %d)\n", env, fr.fiverb->numofrules, reduce);
        frirl_deinit(&fr);
        frirl_demo_release(&fr);
        return 0;
    }
    snprintf(name, sizeof name, "%s.frirlrb.bin", env);
    frirl_save_rb_to_bin_file(&fr, name);
    snprintf(name, sizeof name, "%s.frirlrb.txt", env);
    frirl_save_rb_to_text_file(&fr, name);
    printf("demo %s: episodes %u steps(last) %d rules %d converged %d\n", env, fr.episode_num, fr.reward.ep_total_steps, fr.fiverb->numofrules, fr.epended);
    frirl_deinit(&fr);
    frirl_demo_release(&fr);
    return 0;
}
