"""Plain-Python restatement of the exploration contract of include/frirl_hip.h (struct frirl_hip_agent: seed, env_id_base, epsilon,
no_random; frirl_hip_agent_begin / _observe, frirl_hip_policy_begin / _observe): the reference for every epsilon-greedy test.

The stream is counter-based: a pick has no state, only keys.
  * global environment id = agent.env_id_base + row of the batch; it enters the key shifted left by 32 bits in 64-bit arithmetic,
    so its high 32 bits drop out: streams repeat with a period of 2^32 global ids
  * episode: learning entry points count the episodes an environment has started (the first one is 1); roll-outs on a shared,
    finished rule base use episode 0
  * step: 0 for the first action of an episode, ep_steps + 1 for the action chosen after a step that found ep_steps steps done
  * draw: 0 decides whether to explore, 1 chooses the action
The mixing function is the SplitMix64 output function (Steele, Lea, Flood: "Fast splittable pseudorandom number generators",
OOPSLA 2014; the public-domain splitmix64.c of Vigna), whose published outputs for seed 0 anchor known_answers() below.

Python integers masked to 64 bits; the unit is the top 53 bits times 2^-53, exact in a float."""
import math

M64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15          # SplitMix64's increment: multiplies the (id, episode) key
STEP_GAMMA = 0xD1B54A32D192ED03            # multiplies the (step, draw) key


def mix64(z):
    """SplitMix64's output function of a 64-bit word."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def word(seed, gid, episode, step, draw):
    """The 64-bit output for one key tuple."""
    stream = ((gid << 32) | episode) & M64
    counter = ((step << 8) | draw) & M64
    return mix64(seed + GOLDEN_GAMMA * stream + STEP_GAMMA * counter)


def unit(seed, gid, episode, step, draw):
    """Uniform number of [0, 1) with 53 bits."""
    return (word(seed, gid, episode, step, draw) >> 11) * 2.0 ** -53


def c_round(x):
    """C round() of a finite x >= 0: to nearest, halves away from zero (x - floor(x) is exact)."""
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f


def explores(epsilon, no_random, seed, gid, episode, step):
    """True when the pick at these keys takes the random branch."""
    return not (no_random == 1 or epsilon == 0 or unit(seed, gid, episode, step, 0) > epsilon)


def random_action(A, seed, gid, episode, step):
    """(action of the random branch, whether the clamp turned A into A - 1)."""
    a = c_round(unit(seed, gid, episode, step, 1) * A)
    return (A - 1, True) if a > A - 1 else (a, False)


def pick(greedy, A, epsilon, no_random, seed, gid, episode, step):
    """frirl_e_greedy_selection on the counter-based stream: the greedy action, or round(u * A) clamped to A - 1."""
    if not explores(epsilon, no_random, seed, gid, episode, step):
        return greedy
    return random_action(A, seed, gid, episode, step)[0]


def known_answers():
    """(keys, word) pairs that do not come from this project: with seed 0, id 0, step 0 and draw 0 the mixed word is
    GOLDEN_GAMMA * episode, i.e. the state of a SplitMix64 generator seeded with 0 after `episode` calls, so the words are its
    published first and second outputs."""
    return [((0, 0, 1, 0, 0), 0xE220A8397B1DCDAF), ((0, 0, 2, 0, 0), 0x6E789E6AA1B965F4)]
