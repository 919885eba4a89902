// rule_usage.h -- the arrays of one rule-usage call (frirl_hip_rule_usage, rule_usage.hip), carved out of one workspace:
// what the first launch (lane = point) hands the second (lane = rule).  No kernel is defined here.
#pragma once
#include "reduce_map_ws.h"

namespace frirl {

constexpr int RU_BLOCK = 256;            // rules per workgroup of the second launch
constexpr int RU_TILE = 128;             // points staged in LDS per step of the second launch

struct RuleUsageWs {
    double *qve;                  // [E][n][nant-1] the VE points of the agents' points
    double *wsum;                 // [E][n] S: the Shepard weight sum of the greedy action (map_conclusions' sw)
    int32_t *astar;               // [E][n] the greedy action, as frirl_hip_policy_map's best (-1: the point does not exist)
    int32_t *hit;                 // [E][n] the first rule at distance 0 from (point, greedy action), -1 = none
};

}  // namespace frirl

static size_t rule_usage_layout(char *base, size_t E, size_t n, int nant, frirl::RuleUsageWs *ws)
{
    frirl::RuleUsageWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += up16(bytes); return p; };
    w.qve = reinterpret_cast<double *>(take(sizeof(double) * E * n * (size_t)(nant - 1)));
    w.wsum = reinterpret_cast<double *>(take(sizeof(double) * E * n));
    w.astar = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * n));
    w.hit = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * E * n));
    if (ws) *ws = w;
    return off;
}
