// five_rule_distance.hip -- batched rule-distance scan + first exact hit.
//
// Replaces reference src/five/five_rule_distance.c:63-295 (AVX2 kernels K1 :82-100 and K2
// :160-236): the reference writes per-dimension squared differences to a 64 B/rule scratch and
// re-reads them; here the two passes are fused in registers, so the only HBM traffic is the
// compulsory one: the antecedents once (+ 8 B written when the distances are materialised).
//
// HBM-bound stream with no reuse => no MFMA, no LDS tiling of the rule data.  What decides the rate is the ORDER in
// which the chip walks memory (profiles/r02_rule_distance_order.md): a traffic-only kernel with the same loads and
// stores reaches 0.59-0.70 of the 8 TB/s peak when concurrently running workgroups belong to different environments
// (thousands of scattered 4 KiB streams: round 1's grid = (environment, chunk)) and 0.74-0.80 when they sweep the
// chunks of a few consecutive environments together (compact DRAM windows).  So:
//   work item = (environment e, chunk c) of `chunk` consecutive rules, numbered item = e * cpe + c  (c fastest);
//   every lane loads two rules per column and instruction (16 B of f64 / 4 B of u16 indices): a wave instruction reads
//   1 KiB / 256 contiguous bytes and stores 1 KiB of contiguous distances; wider per-lane index loads (8 / 16 B) leave
//   the stores only half / quarter dense and measured 0.42 / 0.19.
// Five kernels, the same arithmetic on the same doubles (bit-identical results):
//   rule_distance_kernel          f64 VE columns (the reference's layout); one workgroup per item, hardware dispatch
//                                 order = item order;
//   rule_distance_idx_kernel      16-bit universe-index mirror, VE values gathered from an LDS copy of the tables;
//                                 one workgroup per item -- for SMALL tables (<= 4 KiB: the copy is refilled by every
//                                 workgroup from L2, cheaper than anything persistent: 0.73-0.79 moved);
//   rule_distance_idx_persist     LARGE tables (cartpole 40 KB, cfg5 125 KB): persistent workgroups fill the table ONCE
//                                 and take items from an in-order counter, four consecutive items per atomic (one per
//                                 item serialises on the atomic: 0.37), so the resident workgroups still advance as one
//                                 compact window (static striding lets them drift apart: 0.65); the next item's
//                                 indices and scalars are fetched before the current item is computed; the observation
//                                 VE values of every environment are computed once by observe_reset_kernel (which also
//                                 resets the hit words and the counter): no barrier, no LDS write and no dependent
//                                 global chain per item.  0.74-0.79 moved at cfg3 (round 1: 0.55), 0.69 at cfg5 (0.56).
//   rule_distance_pk_kernel       PACKED index mirror (pidx: 6-bit fields, five per 32-bit word; five_hip_rule_distance_packed)
//                                 for small tables with U <= 64: the idx kernel's items and stores, 4 B of indices per rule
//                                 for nant <= 5 instead of 2 * nant -- at cfg4 12 B moved per evaluation instead of 18.
//                                 Shipped form (SQ, option rd_sqdiff): what does not depend on the rule is done once per
//                                 workgroup -- an LDS table of the squared differences (q_k - ve[k][i])^2 replaces the VE
//                                 copy, so a rule costs NANT LDS reads + NANT - 1 adds, and when every entry of that table is
//                                 0 or in [2^-767, 2^1000] (one workgroup-uniform flag) the square root skips __dsqrt_rn's
//                                 rescale and special-case steps (sqrt_unscaled); otherwise __dsqrt_rn.  The same operations
//                                 on the same doubles in the same order: bit-identical.  cfg4: 27 % fewer VALU instructions,
//                                 1.18 -> 1.12 ms (profiles/r05_cfg4_sqdiff.md).
//                                 With a caller's workspace (five_hip_rule_distance_packed_ws, option rd_prepass, PRE) the tables,
//                                 the flags and the hit reset are done once per call by sq_tables_kernel (in place of the memset),
//                                 the scan's prologue is a copy, the workgroups of an environment share an XCD (one L2 fetches the
//                                 table) and items are 2048 rules: 1.124 -> 1.087 ms (profiles/r06_cfg4_prepass.md).
//                                 Floor: reads (~7 TB/s) and the 16-B write stream (5.5-5.9 TB/s) share HBM's one data bus, so their
//                                 times ADD (0.30 + 0.73...0.78 ms at cfg4); what is left above that sum is issue work and the
//                                 shape of the window the resident workgroups touch, not a lack of overlap.
//   rule_distance_cd_kernel       CODED copy (five_hip_rule_distance_coded_ws, option rd_coded, what Problem.rule_distance calls where it
//                                 applies): 3 bytes of indices per rule.  A rule's indices are ranks in per-dimension dictionaries,
//                                 two dimensions per field, at most 24 bits in all (cfg4: 11 + 11 + 2); the copy is lane-tiled, so a lane
//                                 makes three aligned 8-byte loads per 2048-rule item where the packed scan makes four, and the tables
//                                 of sq_tables_kernel<DIGIT> are laid out by rank: the scan is the pre-pass form of the packed one with
//                                 another decode -- bit-identical.  cfg4: FETCH 2.17 -> 1.63 GB, 1.052-1.053 -> 1.017-1.020 ms
//                                 (profiles/r10_cfg4_coded.md).  The decode works in byte offsets (5-6 instructions per pair field), 0
//                                 leaves the short square root through one v_max_f64 and the exact hits are found off the common path:
//                                 59 vector instructions per rule pair where there were 81, SQ_INSTS_VALU 3.99e8 -> 2.80e8 per launch,
//                                 34 VGPRs (profiles/r11_cfg4_scan_valu.md).
// First exact hit: per-lane minimum index -> wave butterfly -> (LDS ->) one integer atomicMin per workgroup / item
// (deterministic; only taken when a hit exists).  The coded scan looks for the index only in a wave that saw a zero (see there).
// "rd_*" / "no_uidx" options (frirl_hip_set_option) are experiment hooks (tools/ab_rd.py); unset, the shipped configuration runs.
#include <stdlib.h>

#include <type_traits>

#include "device_common.h"

namespace frirl {

// item -> (environment, first rule): chunk index fastest (shipped) or environment fastest (round-1 order, A/B only)
__device__ __forceinline__ void item_to_env_chunk(unsigned item, int cpe, int E, bool env_fastest, int &e, int &c)
{
    if (env_fastest) { c = (int)(item / (unsigned)E); e = (int)(item - (unsigned)c * (unsigned)E); }
    else { e = (int)(item / (unsigned)cpe); c = (int)(item - (unsigned)e * (unsigned)cpe); }
}

template <int NANT, bool WRITE, int UNROLL, int NT>
__global__ __launch_bounds__(FRIRL_BLOCK) void rule_distance_kernel(
    const double *__restrict__ u, const double *__restrict__ ve, int U, const double *__restrict__ rb,
    const int32_t *__restrict__ nrules, int maxR, const double *__restrict__ x, double *__restrict__ dists,
    uint32_t *__restrict__ hit, int rules_per_block, int cpe, int E, int env_fastest)
{
    int e, c;
    item_to_env_chunk(blockIdx.x, cpe, E, env_fastest != 0, e, c);
    const int R = nrules[e];
    const int r0 = c * rules_per_block;
    if (r0 >= R) return;   // uniform for the workgroup
    int r_end = r0 + rules_per_block;
    if (r_end > R) r_end = R;

    __shared__ double q_s[NANT];
    __shared__ unsigned red_s[FRIRL_WAVES_PER_BLOCK];
    if (threadIdx.x < NANT) q_s[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, x[(size_t)e * NANT + threadIdx.x]);
    __syncthreads();
    double q[NANT];
#pragma unroll
    for (int k = 0; k < NANT; k++) q[k] = q_s[k];

    const double *__restrict__ base = rb + (size_t)e * (NANT + 1) * maxR;
    double *__restrict__ out = WRITE ? dists + (size_t)e * maxR : nullptr;
    unsigned best = FRIRL_HIP_NO_HIT;
    constexpr int STEP = FRIRL_BLOCK * 2;

    for (int r = r0 + 2 * (int)threadIdx.x; r < r_end; r += STEP * UNROLL) {
        double2 v[UNROLL][NANT];
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {
#pragma unroll
                for (int k = 0; k < NANT; k++) {
                    const double2 *src = reinterpret_cast<const double2 *>(base + (size_t)k * maxR + rr);
                    if (NT == 1 || NT == 2) { v[j][k].x = __builtin_nontemporal_load(&src->x); v[j][k].y = __builtin_nontemporal_load(&src->y); }
                    else v[j][k] = *src;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {
                // dimension-ordered sum of squares, separate mul / add (five_rule_distance.c:88-90,171-208)
                double d0 = q[0] - v[j][0].x, d1 = q[0] - v[j][0].y;
                double a0 = d0 * d0, a1 = d1 * d1;
#pragma unroll
                for (int k = 1; k < NANT; k++) {
                    d0 = q[k] - v[j][k].x;
                    d1 = q[k] - v[j][k].y;
                    const double s0 = d0 * d0, s1 = d1 * d1;
                    a0 = a0 + s0;
                    a1 = a1 + s1;
                }
                double2 d;
                d.x = __dsqrt_rn(a0);   // IEEE sqrt (vsqrtpd, five_rule_distance.c:211)
                d.y = __dsqrt_rn(a1);
                if (WRITE) {                                              // rows are even-sized: rr+1 < maxR
                    if (NT == 1 || NT == 3) { __builtin_nontemporal_store(d.x, out + rr); __builtin_nontemporal_store(d.y, out + rr + 1); }
                    else *reinterpret_cast<double2 *>(out + rr) = d;
                }
                // first exact hit among valid rules (five_rule_distance.c:215-217,241-262)
                if (d.y == 0.0 && rr + 1 < R) best = min(best, (unsigned)(rr + 1));
                if (d.x == 0.0) best = min(best, (unsigned)rr);
            }
        }
    }
    best = block_min_u32(best, red_s);
    if (threadIdx.x == 0 && best != FRIRL_HIP_NO_HIT) atomicMin(&hit[e], best);
}

// Distances of two adjacent rules from their packed 16-bit universe indices (w[k] = rule r | rule r+1 << 16) and the
// LDS copy of the VE tables: the same subtract / multiply / add sequence as above on the same doubles.
template <int NANT>
__device__ __forceinline__ double2 idx_pair_distance(const uint32_t (&w)[NANT], const double (&q)[NANT], const double *__restrict__ tab_s, int U)
{
    double2 t = lds_table_pair(tab_s, w[0]);                  // one v_mad_u32_u16 per index (device_common.h)
    double d0 = q[0] - t.x, d1 = q[0] - t.y;
    double a0 = d0 * d0, a1 = d1 * d1;
#pragma unroll
    for (int k = 1; k < NANT; k++) {
        t = lds_table_pair(tab_s + k * U, w[k]);
        d0 = q[k] - t.x;
        d1 = q[k] - t.y;
        const double s0 = d0 * d0, s1 = d1 * d1;
        a0 = a0 + s0;
        a1 = a1 + s1;
    }
    double2 d;
    d.x = __dsqrt_rn(a0);
    d.y = __dsqrt_rn(a1);
    return d;
}

// Compressed-antecedent form, small tables: one workgroup per item, the table copy refilled per workgroup (<= 4 KiB from L2).
template <int NANT, bool WRITE, int UNROLL, int BLOCK = FRIRL_BLOCK>
__global__ __launch_bounds__(BLOCK) void rule_distance_idx_kernel(
    const double *__restrict__ u, const double *__restrict__ ve, int U, const uint16_t *__restrict__ uidx,
    const int32_t *__restrict__ nrules, int maxR, const double *__restrict__ x, double *__restrict__ dists,
    uint32_t *__restrict__ hit, int rules_per_block, int cpe, int E, int env_fastest)
{
    extern __shared__ double tab_s[];            // [NANT][U] vague environments
    int e, c;
    item_to_env_chunk(blockIdx.x, cpe, E, env_fastest != 0, e, c);
    const int R = nrules[e];
    const int r0 = c * rules_per_block;
    if (r0 >= R) return;
    int r_end = r0 + rules_per_block;
    if (r_end > R) r_end = R;

    __shared__ double q_s[NANT];
    __shared__ unsigned red_s[BLOCK / FRIRL_WAVE];
    for (int i = threadIdx.x; i < NANT * U; i += BLOCK) tab_s[i] = ve[i];
    if (threadIdx.x < NANT) q_s[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, x[(size_t)e * NANT + threadIdx.x]);
    __syncthreads();
    double q[NANT];
#pragma unroll
    for (int k = 0; k < NANT; k++) q[k] = q_s[k];

    const uint16_t *__restrict__ base = uidx + (size_t)e * NANT * maxR;
    double *__restrict__ out = WRITE ? dists + (size_t)e * maxR : nullptr;
    unsigned best = FRIRL_HIP_NO_HIT;
    constexpr int STEP = BLOCK * 2;

    for (int r = r0 + 2 * (int)threadIdx.x; r < r_end; r += STEP * UNROLL) {
        uint32_t w[UNROLL][NANT];
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {
#pragma unroll
                for (int k = 0; k < NANT; k++) w[j][k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(base + (size_t)k * maxR + rr));
            }
        }
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {
                const double2 d = idx_pair_distance<NANT>(w[j], q, tab_s, U);
                if (WRITE) { __builtin_nontemporal_store(d.x, out + rr); __builtin_nontemporal_store(d.y, out + rr + 1); }
                if (d.y == 0.0 && rr + 1 < R) best = min(best, (unsigned)(rr + 1));
                if (d.x == 0.0) best = min(best, (unsigned)rr);
            }
        }
    }
    best = wave_min_u32(best);
    if ((threadIdx.x & (FRIRL_WAVE - 1)) == 0) red_s[threadIdx.x / FRIRL_WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = red_s[0];
        for (int w = 1; w < BLOCK / FRIRL_WAVE; w++) m = red_s[w] < m ? red_s[w] : m;
        if (m != FRIRL_HIP_NO_HIT) atomicMin(&hit[e], m);
    }
}

// Packed-antecedent form (pidx mirror, five_hip_rule_distance_packed): the universe indices of a rule as BITS-bit fields of
// W = Packed<BITS>::words(NANT) 32-bit words, pidx[e][w][r] -- 4 B per rule for nant <= 5 at BITS 6 instead of 2 * nant.  Small
// tables only (one workgroup per item, the table refilled per workgroup), laid out in LDS with a row stride of 2^BITS entries:
// a field becomes its table entry's byte offset with one shift and one mask, and the row offset is the LDS read's immediate.
// Same item order, two adjacent rules per lane (one 8 B load per word and column set: 512 contiguous bytes per wave), the
// same 16 B distance stores, the same subtract / multiply / add sequence as the kernels above (bit-identical results).
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
static constexpr int RD_XCDS = 8;                // MI355X: workgroups are dealt round-robin over 8 XCDs, each with an L2 of its own

template <int BITS>
__device__ __forceinline__ double pk_table_entry(const double *__restrict__ tab_k, uint32_t w, int sh)
{
    constexpr uint32_t FM = ((1u << BITS) - 1u) << 3;
    const uint32_t off = (sh >= 3 ? (w >> (sh - 3)) : (w << (3 - sh))) & FM;     // 8 * index
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(tab_k) + off);
}

template <int NANT, int BITS>
__device__ __forceinline__ double2 pk_pair_distance(const u32x2_t (&w)[Packed<BITS>::words(NANT)], const double (&q)[NANT],
                                                    const double *__restrict__ tab_s)
{
    constexpr int FPW = Packed<BITS>::FPW, TS = 1 << BITS;
    double d0 = q[0] - pk_table_entry<BITS>(tab_s, w[0].x, 0), d1 = q[0] - pk_table_entry<BITS>(tab_s, w[0].y, 0);
    double a0 = d0 * d0, a1 = d1 * d1;
#pragma unroll
    for (int k = 1; k < NANT; k++) {
        const int sh = BITS * (k % FPW);
        d0 = q[k] - pk_table_entry<BITS>(tab_s + k * TS, w[k / FPW].x, sh);
        d1 = q[k] - pk_table_entry<BITS>(tab_s + k * TS, w[k / FPW].y, sh);
        const double s0 = d0 * d0, s1 = d1 * d1;
        a0 = a0 + s0;
        a1 = a1 + s1;
    }
    double2 d;
    d.x = __dsqrt_rn(a0);
    d.y = __dsqrt_rn(a1);
    return d;
}

// __dsqrt_rn's gfx950 expansion for an input it does not rescale (x >= 2^-767, finite): v_rsq_f64, the same two multiplies and
// seven Newton FMAs in the same order, and 0 passed through (one v_max_f64).  For such x the result has the bits of __dsqrt_rn(x); below 2^-767,
// at +inf or for NaN / negative x it does not (the full expansion rescales tiny inputs and passes +inf through).
__device__ __forceinline__ double sqrt_unscaled(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    const double s0 = x * y;
    const double h0 = y * 0.5;
    const double r0 = __builtin_fma(-h0, s0, 0.5);
    const double h1 = __builtin_fma(h0, r0, h0);
    const double s1 = __builtin_fma(s0, r0, s0);
    const double d0 = __builtin_fma(-s1, s1, x);
    const double s2 = __builtin_fma(d0, h1, s1);
    const double d1 = __builtin_fma(-s2, s2, x);
    const double r = __builtin_fma(d1, h1, s2);
    return __builtin_fmax(r, 0.0);               // x = +0: rsq = +inf, r = 0 * inf = NaN, and the maximum of a quiet NaN and +0 is +0; x > 0: r > 0
}

// Bounds on one squared difference under which every sum of at most FRIRL_HIP_MAX_NANT of them is exactly 0 or a finite value
// >= 2^-767 (a sum of non-negative terms is at least its largest term; 16 * 2^1000 stays finite): sqrt_unscaled is then exact.
__device__ __forceinline__ bool sq_in_unscaled_range(double s)
{
    return s == 0.0 || (s >= 0x1p-767 && s <= 0x1p1000);       // false for NaN
}

// Rule-independent half of the packed scan (rd_sqdiff, shipped): the workgroup's squared differences sq_s[k][i] = (q_k - t)^2,
// t = the table's VE value i (0.0 on the padding entries i >= U, as above), in LDS; a rule then costs NANT LDS reads and NANT - 1
// ordered adds -- the same subtract, multiply and dimension-ordered adds on the same doubles as pk_pair_distance.  The square
// root is sqrt_unscaled when every entry of the workgroup's table is in range (one flag per workgroup: __syncthreads_or), else
// __dsqrt_rn: bit-identical either way.
template <int NANT, int BITS, bool FAST>
__device__ __forceinline__ void pk_pair_sq(const u32x2_t (&w)[Packed<BITS>::words(NANT)], const double *__restrict__ sq_s, double2 &d,
                                           bool &z0, bool &z1)
{
    constexpr int FPW = Packed<BITS>::FPW, TS = 1 << BITS;
    double a0 = pk_table_entry<BITS>(sq_s, w[0].x, 0), a1 = pk_table_entry<BITS>(sq_s, w[0].y, 0);
#pragma unroll
    for (int k = 1; k < NANT; k++) {
        const int sh = BITS * (k % FPW);
        a0 = a0 + pk_table_entry<BITS>(sq_s + k * TS, w[k / FPW].x, sh);
        a1 = a1 + pk_table_entry<BITS>(sq_s + k * TS, w[k / FPW].y, sh);
    }
    if (FAST) {
        d.x = sqrt_unscaled(a0);
        d.y = sqrt_unscaled(a1);
        z0 = a0 == 0.0;                          // sqrt(a) == 0 exactly when a == 0: the select above and the hit test share it
        z1 = a1 == 0.0;
    } else {
        d.x = __dsqrt_rn(a0);
        d.y = __dsqrt_rn(a1);
        z0 = d.x == 0.0;
        z1 = d.y == 0.0;
    }
}

// One environment's squared-difference table (above) from its snapped observations q_s, by BLOCK threads numbered tid (sq_s: LDS in
// the scan, the environment's rows of the workspace in sq_tables_kernel); returns true when every entry is in the range of
// sqrt_unscaled.  Shared by rule_distance_pk_kernel, sq_tables_kernel and the probe five_hip_rule_distance_sq_guard.
template <int NANT, int BITS, int BLOCK>
__device__ __forceinline__ bool fill_sq_table(const double *q_s, double *sq_s, const double (&tv)[(NANT * (1 << BITS) + BLOCK - 1) / BLOCK], int tid)
{
    constexpr int TS = 1 << BITS, N = NANT * TS;
    bool ok = true;
#pragma unroll
    for (int m = 0; m < (N + BLOCK - 1) / BLOCK; m++) {
        const int i = tid + m * BLOCK;
        if (N % BLOCK == 0 || i < N) {
            const double d = q_s[i >> BITS] - tv[m];
            const double s = d * d;
            sq_s[i] = s;
            ok = ok && sq_in_unscaled_range(s);
        }
    }
    return ok;
}

// tv[m] = the table value of entry tid + m * BLOCK of fill_sq_table (loaded before the observations are known)
template <int NANT, int BITS, int BLOCK>
__device__ __forceinline__ void load_sq_sources(const double *__restrict__ ve, int U, double (&tv)[(NANT * (1 << BITS) + BLOCK - 1) / BLOCK], int tid)
{
    constexpr int TS = 1 << BITS, N = NANT * TS;
#pragma unroll
    for (int m = 0; m < (N + BLOCK - 1) / BLOCK; m++) {
        const int i = tid + m * BLOCK;
        const int k = i >> BITS, j = i & (TS - 1);
        tv[m] = (i < N && j < U) ? ve[k * U + j] : 0.0;
    }
}

// Per-call pre-pass of the packed scan (option rd_prepass, five_hip_rule_distance_packed_ws): what the workgroups of an environment
// would each redo in their prologue, done once -- one wave per environment, with the device functions of that prologue (same bits):
//   sqtab[e][k][i] = (q_k - ve[k][i])^2, q_k = observe_ve(x[e][k]) (0.0 table values on the padding entries i >= U),
//   fastv[e] = 1 when every entry is in the range of sqrt_unscaled, else 0,   hit[e] = "none" (in place of the memset).
// DIGIT (the coded scan, rule_distance_cd_kernel): entry j of row k is the table value of universe index dict[k][j] -- the j-th index of
// the rule bases' dictionary of dimension k, 0xFF beyond its length -- so sqtab[e][k][j] = (q_k - ve[k][dict[k][j]])^2, with the same 0.0
// table value wherever the index is not below U.  Row stride, flag and hit reset are unchanged.
template <int NANT, int BITS, bool DIGIT = false>
__global__ __launch_bounds__(FRIRL_BLOCK) void sq_tables_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U, int E,
                                                              const double *__restrict__ x, double *__restrict__ sqtab,
                                                              uint32_t *__restrict__ fastv, uint32_t *__restrict__ hit,
                                                              const uint8_t *__restrict__ dict = nullptr)
{
    constexpr int TS = 1 << BITS, N = NANT * TS;
    __shared__ double q_s[FRIRL_WAVES_PER_BLOCK][NANT];
    const int lane = threadIdx.x & (FRIRL_WAVE - 1), wave = threadIdx.x / FRIRL_WAVE;
    const int e = blockIdx.x * FRIRL_WAVES_PER_BLOCK + wave;
    const bool live = e < E;                     // uniform for the wave; every wave reaches the barrier
    double tv[(N + FRIRL_WAVE - 1) / FRIRL_WAVE];
    if constexpr (DIGIT) {
#pragma unroll
        for (int m = 0; m < (N + FRIRL_WAVE - 1) / FRIRL_WAVE; m++) {
            const int i = lane + m * FRIRL_WAVE;
            const int k = i >> BITS;
            const int idx = i < N ? (int)dict[i] : U;                    // dict[NANT][2^BITS]
            tv[m] = idx < U ? ve[k * U + idx] : 0.0;
        }
    } else {
        load_sq_sources<NANT, BITS, FRIRL_WAVE>(ve, U, tv, lane);
    }
    if (live && lane < NANT) q_s[wave][lane] = observe_ve(u, ve, U, lane, x[(size_t)e * NANT + lane]);
    __syncthreads();
    if (!live) return;
    const bool ok = fill_sq_table<NANT, BITS, FRIRL_WAVE>(q_s[wave], sqtab + (size_t)e * N, tv, lane);
    const bool fast = __all(ok);
    if (lane == 0) {
        fastv[e] = fast ? 1u : 0u;
        hit[e] = FRIRL_HIP_NO_HIT;
    }
}

// SQ = false: the kernel as it was before the squared-difference tables (option rd_sqdiff = 0, A/B only).
// qv != nullptr: the snapped observations qv[e][k] of observe_reset_kernel (option rd_qpass) instead of observe_ve in the prologue.
// PRE (with SQ; option rd_prepass, shipped where the caller gives a workspace): the prologue is a copy -- the environment's table
// sqtab[e] of sq_tables_kernel goes to LDS with plain loads (its sibling workgroups read the same 2^BITS * NANT doubles) and the
// flag fastv[e] is one scalar load: no u / ve / x, no division, one barrier.  Sweep, stores and hit reduction are those of SQ.
// env_fastest: 0 = chunk fastest (PRE: within groups of RD_XCDS environments, see below), 1 = environment fastest, 2 = PRE with the
// plain chunk-fastest order (A/B).
template <int NANT, bool WRITE, int UNROLL, int BITS, bool SQ, bool PRE = false>
__global__ __launch_bounds__(FRIRL_BLOCK) void rule_distance_pk_kernel(
    const double *__restrict__ u, const double *__restrict__ ve, int U, const uint32_t *__restrict__ pidx,
    const int32_t *__restrict__ nrules, int maxR, const double *__restrict__ x, const double *__restrict__ qv, double *__restrict__ dists,
    uint32_t *__restrict__ hit, int rules_per_block, int cpe, int E, int env_fastest, const double *__restrict__ sqtab = nullptr,
    const uint32_t *__restrict__ fastv = nullptr)
{
    static_assert(SQ || !PRE, "the pre-pass serves the squared-difference form");
    constexpr int W = Packed<BITS>::words(NANT), TS = 1 << BITS;
    __shared__ __attribute__((aligned(16))) double tab_s[NANT * TS];      // [NANT][2^BITS] vague environments (static: row offsets are immediates)
    __shared__ double q_s[NANT];
    __shared__ unsigned red_s[FRIRL_WAVES_PER_BLOCK];
    int e, c;
    if (PRE && env_fastest == 0) {
        // The workgroups of an environment on ONE XCD, so that its table is fetched into one L2 and not into eight: workgroups b and
        // b + RD_XCDS share an XCD, so RD_XCDS consecutive environments take the RD_XCDS * cpe workgroups of a group, environment =
        // workgroup index mod RD_XCDS, chunks ascending.  The grid is rounded up to whole groups: e >= E leaves at once.
        const unsigned grp = blockIdx.x / (unsigned)(RD_XCDS * cpe), j = blockIdx.x - grp * (unsigned)(RD_XCDS * cpe);
        e = (int)(grp * RD_XCDS + j % RD_XCDS);
        c = (int)(j / RD_XCDS);
        if (e >= E) return;
    } else {
        item_to_env_chunk(blockIdx.x, cpe, E, env_fastest == 1, e, c);
    }
    const int R = nrules[e];
    const int r0 = c * rules_per_block;
    if (r0 >= R) return;
    int r_end = r0 + rules_per_block;
    if (r_end > R) r_end = R;

    const uint32_t *__restrict__ base = pidx + (size_t)e * W * maxR;
    constexpr int STEP = FRIRL_BLOCK * 2;
    u32x2_t w[UNROLL][W];
    auto load = [&](int r) {
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {                    // rr even and maxR even: the pair is 8-byte aligned and inside the row
#pragma unroll
                for (int k = 0; k < W; k++) w[j][k] = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t *>(base + (size_t)k * maxR + rr));
            }
        }
    };
    int r = r0 + 2 * (int)threadIdx.x;
    load(r);                                     // the first sweep's indices are in flight while the table is filled and x is snapped
    double *__restrict__ out = WRITE ? dists + (size_t)e * maxR : nullptr;
    unsigned best = FRIRL_HIP_NO_HIT;

    if constexpr (SQ) {
        double *sq_s = tab_s;                    // [NANT][2^BITS] squared differences
        bool fast;                               // uniform
        if constexpr (PRE) {
            constexpr int N2 = NANT * TS / 2;    // 16 B per lane; sqtab + e * NANT * TS is 16-byte aligned (TS even, workspace checked)
            const double2 *__restrict__ src = reinterpret_cast<const double2 *>(sqtab + (size_t)e * (NANT * TS));
            for (int i = threadIdx.x; i < N2; i += FRIRL_BLOCK) reinterpret_cast<double2 *>(sq_s)[i] = src[i];
            fast = fastv[e] != 0u;
            __syncthreads();
        } else {
            double tv[(NANT * TS + FRIRL_BLOCK - 1) / FRIRL_BLOCK];
            load_sq_sources<NANT, BITS, FRIRL_BLOCK>(ve, U, tv, (int)threadIdx.x);
            if (threadIdx.x < NANT)
                q_s[threadIdx.x] = qv ? qv[(size_t)e * NANT + threadIdx.x] : observe_ve(u, ve, U, threadIdx.x, x[(size_t)e * NANT + threadIdx.x]);
            __syncthreads();
            fast = !__syncthreads_or(!fill_sq_table<NANT, BITS, FRIRL_BLOCK>(q_s, sq_s, tv, (int)threadIdx.x));
        }
        auto sweep = [&](auto fast_tag) {
            constexpr bool FAST = decltype(fast_tag)::value;
            for (; r < r_end; r += STEP * UNROLL) {
                if (r != r0 + 2 * (int)threadIdx.x) load(r);
#pragma unroll
                for (int j = 0; j < UNROLL; j++) {
                    const int rr = r + j * STEP;
                    if (rr < r_end) {
                        double2 d;
                        bool z0, z1;
                        pk_pair_sq<NANT, BITS, FAST>(w[j], sq_s, d, z0, z1);
                        if (WRITE) { __builtin_nontemporal_store(d.x, out + rr); __builtin_nontemporal_store(d.y, out + rr + 1); }
                        if (z1 && rr + 1 < R) best = min(best, (unsigned)(rr + 1));
                        if (z0) best = min(best, (unsigned)rr);
                    }
                }
            }
        };
        if (fast) sweep(std::true_type{});
        else sweep(std::false_type{});
        best = wave_min_u32(best);
        if ((threadIdx.x & (FRIRL_WAVE - 1)) == 0) red_s[threadIdx.x / FRIRL_WAVE] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned m = red_s[0];
            for (int v = 1; v < FRIRL_WAVES_PER_BLOCK; v++) m = red_s[v] < m ? red_s[v] : m;
            if (m != FRIRL_HIP_NO_HIT) atomicMin(&hit[e], m);
        }
        return;
    }

    for (int i = threadIdx.x; i < NANT * TS; i += FRIRL_BLOCK) {
        const int k = i >> BITS, j = i & (TS - 1);
        tab_s[i] = j < U ? ve[k * U + j] : 0.0;  // padding: what the odd last rule's unused column may point at
    }
    if (threadIdx.x < NANT) q_s[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, x[(size_t)e * NANT + threadIdx.x]);
    __syncthreads();
    double q[NANT];
#pragma unroll
    for (int k = 0; k < NANT; k++) q[k] = q_s[k];

    for (; r < r_end; r += STEP * UNROLL) {
        if (r != r0 + 2 * (int)threadIdx.x) load(r);
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {
                const double2 d = pk_pair_distance<NANT, BITS>(w[j], q, tab_s);
                if (WRITE) { __builtin_nontemporal_store(d.x, out + rr); __builtin_nontemporal_store(d.y, out + rr + 1); }
                if (d.y == 0.0 && rr + 1 < R) best = min(best, (unsigned)(rr + 1));
                if (d.x == 0.0) best = min(best, (unsigned)rr);
            }
        }
    }
    best = wave_min_u32(best);
    if ((threadIdx.x & (FRIRL_WAVE - 1)) == 0) red_s[threadIdx.x / FRIRL_WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = red_s[0];
        for (int v = 1; v < FRIRL_WAVES_PER_BLOCK; v++) m = red_s[v] < m ? red_s[v] : m;
        if (m != FRIRL_HIP_NO_HIT) atomicMin(&hit[e], m);
    }
}

// pidx[e][w][r] from uidx[e][k][r] for every one of the maxR columns (fields masked to BITS bits, unused high bits zero).
template <int BITS>
__global__ __launch_bounds__(FRIRL_BLOCK) void pack_indices_kernel(const uint16_t *__restrict__ uidx, int nant, int maxR, long total,
                                                                   uint32_t *__restrict__ pidx)
{
    constexpr int FPW = Packed<BITS>::FPW;
    const int W = (nant + FPW - 1) / FPW;
    for (long i = (long)blockIdx.x * FRIRL_BLOCK + threadIdx.x; i < total; i += (long)gridDim.x * FRIRL_BLOCK) {
        const long e = i / maxR;
        const long r = i - e * maxR;
        const uint16_t *__restrict__ src = uidx + (size_t)e * nant * maxR + r;
        uint32_t *__restrict__ dst = pidx + (size_t)e * W * maxR + r;
        for (int w = 0; w < W; w++) {
            uint32_t v = 0u;
            for (int f = 0; f < FPW && w * FPW + f < nant; f++)
                v |= ((uint32_t)src[(size_t)(w * FPW + f) * maxR] & ((1u << BITS) - 1u)) << (BITS * f);
            dst[(size_t)w * maxR] = v;
        }
    }
}

// Prologue of the persistent form: qv[e][k] = ve[k][snap(x[e][k])] (five_rule_distance.c:75,80) for every environment,
// hit[e] = "none", item counter = 0.
__global__ void observe_reset_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U, int nant, int E, const double *__restrict__ x,
                                     double *__restrict__ qv, uint32_t *__restrict__ hit, unsigned *__restrict__ counter)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *counter = 0u;
    if (i >= E * nant) return;
    const int e = i / nant, k = i - e * nant;
    qv[i] = observe_ve(u, ve, U, k, x[i]);
    if (k == 0) hit[e] = FRIRL_HIP_NO_HIT;
}

// Compressed-antecedent form, large tables: persistent workgroups (see the header of this file).  `counter` hands out
// batches of KB consecutive items in order; every workgroup leaves when the counter passes the last batch.
template <int NANT, bool WRITE, int UNROLL, int BLOCK, int KB>
__global__ __launch_bounds__(BLOCK) void rule_distance_idx_persist_kernel(
    const double *__restrict__ ve, int U, const uint16_t *__restrict__ uidx, const int32_t *__restrict__ nrules, int maxR,
    const double *__restrict__ qv, double *__restrict__ dists, uint32_t *__restrict__ hit, int cpe, int nitems, unsigned *__restrict__ counter)
{
    extern __shared__ double tab_s[];            // [NANT][U] vague environments
    __shared__ int batch_s[2];
    constexpr int STEP = BLOCK * 2, CH = STEP * UNROLL;
    const int nbatches = (nitems + KB - 1) / KB;
    uint32_t w[UNROLL][NANT];                    // indices of the NEXT item (in flight while the current one is computed)
    double qn[NANT];
    int en = 0, cn = 0, Rn = 0;
    auto load_item = [&](int it) {
        en = it / cpe; cn = it - en * cpe;
        Rn = nrules[en];
        const uint16_t *__restrict__ base = uidx + (size_t)en * NANT * maxR;
        const int r = cn * CH + 2 * (int)threadIdx.x;
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < Rn) {
#pragma unroll
                for (int k = 0; k < NANT; k++) w[j][k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(base + (size_t)k * maxR + rr));
            }
        }
#pragma unroll
        for (int k = 0; k < NANT; k++) qn[k] = qv[(size_t)en * NANT + k];      // uniform: scalar loads
    };
    int slot = 0, sub = 0;
    if (threadIdx.x == 0) batch_s[0] = (int)atomicAdd(counter, 1u);
    __syncthreads();
    int batch = batch_s[0];
    int item = batch < nbatches ? batch * KB : nitems;
    if (item < nitems) load_item(item);          // first loads are in flight while the table is filled
    for (int i = threadIdx.x; i < NANT * U; i += BLOCK) tab_s[i] = ve[i];
    __syncthreads();
    while (item < nitems) {                      // uniform for the workgroup: every wave sees the same item sequence
        const int e = en, c = cn, R = Rn;
        uint32_t cw[UNROLL][NANT];
        double q[NANT];
#pragma unroll
        for (int j = 0; j < UNROLL; j++)
#pragma unroll
            for (int k = 0; k < NANT; k++) cw[j][k] = w[j][k];
#pragma unroll
        for (int k = 0; k < NANT; k++) q[k] = qn[k];
        int nxt;
        sub++;
        if (sub < KB && item + 1 < nitems) nxt = item + 1;
        else {                                   // next batch; the double-buffered slot needs one barrier per fetch
            sub = 0;
            slot ^= 1;
            if (threadIdx.x == 0) batch_s[slot] = (int)atomicAdd(counter, 1u);
            __syncthreads();
            batch = batch_s[slot];
            nxt = batch < nbatches ? batch * KB : nitems;
        }
        if (nxt < nitems) load_item(nxt);
        double *__restrict__ out = WRITE ? dists + (size_t)e * maxR : nullptr;
        const int r = c * CH + 2 * (int)threadIdx.x;
        unsigned best = FRIRL_HIP_NO_HIT;
#pragma unroll
        for (int j = 0; j < UNROLL; j++) {
            const int rr = r + j * STEP;
            if (rr < R) {
                const double2 d = idx_pair_distance<NANT>(cw[j], q, tab_s, U);
                if (WRITE) { __builtin_nontemporal_store(d.x, out + rr); __builtin_nontemporal_store(d.y, out + rr + 1); }
                if (d.y == 0.0 && rr + 1 < R) best = min(best, (unsigned)(rr + 1));
                if (d.x == 0.0) best = min(best, (unsigned)rr);
            }
        }
        if (best != FRIRL_HIP_NO_HIT) atomicMin(&hit[e], best);      // rare; integer min: order-independent
        item = nxt;
    }
}

struct RdTune { int unroll, chunk, nt; };
static RdTune rd_tune()
{
    const frirl_host::Options &o = frirl_host::opts();     // read once from the environment / frirl_hip_set_option, not per launch
    RdTune t;
    t.unroll = o.rd_unroll;          // 0 = shipped default
    t.chunk = o.rd_chunk;            // 0 = shipped default
    t.nt = o.rd_nt;                  // -1 = shipped default (non-temporal loads and stores)
    return t;
}

struct RdGrid { unsigned items; int rules_per_block, cpe, env_fastest; };

template <int NANT, int UNROLL, int NT>
static void launch_variant(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const double *x, double *ruledists, uint32_t *hit,
                           hipStream_t s, const RdGrid &g)
{
    if (ruledists)
        hipLaunchKernelGGL((rule_distance_kernel<NANT, true, UNROLL, NT>), dim3(g.items), dim3(FRIRL_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules,
                           b->maxR, x, ruledists, hit, g.rules_per_block, g.cpe, b->E, g.env_fastest);
    else
        hipLaunchKernelGGL((rule_distance_kernel<NANT, false, UNROLL, NT>), dim3(g.items), dim3(FRIRL_BLOCK), 0, s, t->u, t->ve, t->U, b->rb, b->nrules,
                           b->maxR, x, ruledists, hit, g.rules_per_block, g.cpe, b->E, g.env_fastest);
}

// one workgroup per item; chunk = multiple of one 512-rule sweep of the workgroup
static bool make_grid(const frirl_hip_rulebases *b, int rules_per_block, RdGrid &g)
{
    rules_per_block = ((rules_per_block + 2 * FRIRL_BLOCK - 1) / (2 * FRIRL_BLOCK)) * (2 * FRIRL_BLOCK);
    const long cpe = ((long)b->maxR + rules_per_block - 1) / rules_per_block;
    const long items = cpe * (long)b->E;
    if (items > 0x7FFFFFFFL) return false;
    g.items = (unsigned)items; g.rules_per_block = rules_per_block; g.cpe = (int)cpe; g.env_fastest = frirl_host::opts().rd_order == 1;
    return true;
}

static int device_cus()
{
    static thread_local int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t p;
        cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
    }
    return cus;
}

// Persistent form: scratch = [counter | qv[E][NANT]] taken from the stream's memory pool (stream-ordered: concurrent calls on
// other streams never share it) and returned to it right after the launch.
template <int NANT, int UNROLL, int BLOCK, int KB>
static int launch_persist(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const double *x, double *ruledists, uint32_t *hit, hipStream_t s,
                          size_t tab_bytes, int wg_per_cu)
{
    using namespace frirl_host;
    constexpr int CH = BLOCK * 2 * UNROLL;
    const long cpe = ((long)b->maxR + CH - 1) / CH;
    const long nitems = cpe * (long)b->E;
    if (nitems > 0x7FFFFFF0L) { set_error("five_hip_rule_distance: %ld work items exceed the 31-bit item index", nitems); return FRIRL_HIP_EINVAL; }
    const long nbatches = (nitems + KB - 1) / KB;
    long grid = (long)device_cus() * wg_per_cu;
    if (grid > nbatches) grid = nbatches;
    const size_t qv_off = 256, bytes = qv_off + sizeof(double) * (size_t)b->E * NANT;
    void *scratch = nullptr;
    hipError_t e1 = hipMallocAsync(&scratch, bytes, s);
    if (e1 != hipSuccess) { (void)hipGetLastError(); set_error("five_hip_rule_distance: hipMallocAsync(%zu B) failed: %s", bytes, hipGetErrorString(e1)); return FRIRL_HIP_ELAUNCH; }
    unsigned *counter = static_cast<unsigned *>(scratch);
    double *qv = reinterpret_cast<double *>(static_cast<char *>(scratch) + qv_off);
    const int nq = b->E * NANT;
    hipLaunchKernelGGL(observe_reset_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, t->u, t->ve, t->U, NANT, b->E, x, qv, hit, counter);
    if (ruledists) {
        auto k = rule_distance_idx_persist_kernel<NANT, true, UNROLL, BLOCK, KB>;
        e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes);
        if (e1 == hipSuccess) hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(BLOCK), tab_bytes, s, t->ve, t->U, b->uidx, b->nrules, b->maxR, qv, ruledists, hit, (int)cpe, (int)nitems, counter);
    } else {
        auto k = rule_distance_idx_persist_kernel<NANT, false, UNROLL, BLOCK, KB>;
        e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes);
        if (e1 == hipSuccess) hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(BLOCK), tab_bytes, s, t->ve, t->U, b->uidx, b->nrules, b->maxR, qv, ruledists, hit, (int)cpe, (int)nitems, counter);
    }
    const hipError_t e2 = hipFreeAsync(scratch, s);
    if (e1 != hipSuccess) { set_error("five_hip_rule_distance: cannot reserve %zu B of LDS: %s", tab_bytes, hipGetErrorString(e1)); return FRIRL_HIP_ELAUNCH; }
    if (e2 != hipSuccess) { set_error("five_hip_rule_distance: hipFreeAsync failed: %s", hipGetErrorString(e2)); return FRIRL_HIP_ELAUNCH; }
    return check_launch("five_hip_rule_distance(uidx, persistent)");
}

// Shipped configuration (A/B-measured on MI355X, tools/ab_rd.py, tools/exp/rd_bench.hip; profiles/r01_rule_distance_tuning.md,
// profiles/r02_rule_distance_order.md): non-temporal loads AND stores (pure stream, nothing is re-read: +5..8 %), 8 independent
// column sets per lane for nant <= 5 (all loads issued before the first use), 4 for nant <= 8, 2 above.
template <int NANT>
struct RdConfig {
    static constexpr int UNROLL = (NANT <= 5) ? 8 : (NANT <= 8 ? 4 : 2);
};

// tables up to this size use one workgroup per item with a per-workgroup table copy; larger ones the persistent form
static constexpr size_t RD_SMALL_TABLE_BYTES = 4 * 1024;

template <int NANT>
static int launch_nant(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const double *x, double *ruledists,
                       uint32_t *hit, hipStream_t s)
{
    using namespace frirl_host;
    constexpr int UNROLL = RdConfig<NANT>::UNROLL;
    const size_t tab_bytes = sizeof(double) * NANT * (size_t)t->U;
    const RdTune tn = rd_tune();
    const bool idx = b->uidx && t->U <= 65536 && tab_bytes <= 150 * 1024 && !opts().no_uidx;
    const int persist = opts().rd_persist;       // -1 = by table size
    if (idx && (persist == 1 || (persist != 0 && tab_bytes > RD_SMALL_TABLE_BYTES))) {
        // 2 workgroups of 512 threads per CU while two table copies fit beside each other (<= 64 KiB each), else one of 1024
        if (tab_bytes <= 64 * 1024) return launch_persist<NANT, (NANT <= 8 ? 2 : 1), 512, 4>(t, b, x, ruledists, hit, s, tab_bytes, 2);
        return launch_persist<NANT, 1, 1024, 4>(t, b, x, ruledists, hit, s, tab_bytes, 1);
    }
    if (hipMemsetAsync(hit, 0xFF, sizeof(uint32_t) * (size_t)b->E, s) != hipSuccess) return check_launch("five_hip_rule_distance(memset)");
    RdGrid g;
    if (idx) {
        if (tab_bytes > 64 * 1024) { set_error("five_hip_rule_distance: option rd_persist=0 needs VE tables <= 64 KiB"); return FRIRL_HIP_EINVAL; }
        // chunk = ONE sweep of the workgroup (256 threads x 2 rules x UI column sets = 2048 rules for nant <= 8): smaller items keep
        // the window of concurrently streamed memory compact
        constexpr int UI = (NANT <= 8) ? 4 : 2;
        const int un = (NANT <= 5 && tn.unroll) ? tn.unroll : UI;      // tuning hook (experiments only)
        if (!make_grid(b, tn.chunk > 0 ? tn.chunk : 2 * FRIRL_BLOCK * UI, g)) { set_error("five_hip_rule_distance: too many work items"); return FRIRL_HIP_EINVAL; }
        hipError_t e1 = hipSuccess;
#define VI(U_)                                                                                                                               \
    do {                                                                                                                                     \
        if (ruledists) {                                                                                                                     \
            auto k = rule_distance_idx_kernel<NANT, true, U_>;                                                                               \
            if (tab_bytes > 48 * 1024) e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes); \
            if (e1 == hipSuccess) hipLaunchKernelGGL(k, dim3(g.items), dim3(FRIRL_BLOCK), tab_bytes, s, t->u, t->ve, t->U, b->uidx, b->nrules, b->maxR, x, ruledists, hit, g.rules_per_block, g.cpe, b->E, g.env_fastest); \
        } else {                                                                                                                             \
            auto k = rule_distance_idx_kernel<NANT, false, U_>;                                                                              \
            if (tab_bytes > 48 * 1024) e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes); \
            if (e1 == hipSuccess) hipLaunchKernelGGL(k, dim3(g.items), dim3(FRIRL_BLOCK), tab_bytes, s, t->u, t->ve, t->U, b->uidx, b->nrules, b->maxR, x, ruledists, hit, g.rules_per_block, g.cpe, b->E, g.env_fastest); \
        }                                                                                                                                    \
    } while (0)
        if (NANT <= 5 && un == 8) VI(8);
        else if (NANT <= 5 && un == 2) VI(2);
        else if (NANT <= 5 && un == 1) VI(1);
        else VI(UI);
#undef VI
        if (e1 != hipSuccess) { set_error("five_hip_rule_distance: cannot reserve %zu B of LDS: %s", tab_bytes, hipGetErrorString(e1)); return FRIRL_HIP_ELAUNCH; }
        return check_launch("five_hip_rule_distance(uidx)");
    }
    // f64 columns: 1024-rule items for small rule bases, 2048 above (A/B at cfg2: 1024 -> 6.53 TB/s, 2048 -> 6.10, 4096 -> 5.93;
    // at cfg4: 1024 -> 5.61, 2048 -> 6.20, 4096 -> 6.00, 8192 -> 5.96; tools/ab_rd.py with AB_F64=1)
    if (!make_grid(b, tn.chunk > 0 ? tn.chunk : (b->maxR <= 16384 + 512 ? 1024 : 2048), g)) { set_error("five_hip_rule_distance: too many work items"); return FRIRL_HIP_EINVAL; }
    if (NANT <= 5 && (tn.unroll || tn.nt >= 0)) {      // tuning hooks (experiments only)
        const int un = tn.unroll ? tn.unroll : UNROLL;
        const int nt = tn.nt >= 0 ? tn.nt : 1;
#define V(U_, N_) launch_variant<NANT, U_, N_>(t, b, x, ruledists, hit, s, g)
        if (nt == 1) { if (un == 1) V(1, 1); else if (un == 2) V(2, 1); else if (un == 8) V(8, 1); else V(4, 1); }
        else if (nt == 2) { if (un == 1) V(1, 2); else if (un == 2) V(2, 2); else if (un == 8) V(8, 2); else V(4, 2); }
        else if (nt == 3) { if (un == 1) V(1, 3); else if (un == 2) V(2, 3); else if (un == 8) V(8, 3); else V(4, 3); }
        else { if (un == 1) V(1, 0); else if (un == 2) V(2, 0); else if (un == 8) V(8, 0); else V(4, 0); }
#undef V
    } else {
        launch_variant<NANT, UNROLL, 1>(t, b, x, ruledists, hit, s, g);
    }
    return check_launch("five_hip_rule_distance");
}

// Packed form: BITS = 6 (U <= 64), small tables.  chunk = ONE sweep of the workgroup (256 threads x 2 rules x UNROLL column sets).
// Squared-difference form (rd_sqdiff, profiles/r05_cfg4_sqdiff.md), cfg4 / cfg2 medians of 5-7 x 20 launches: unroll 8 with 4096-rule
// items 1.116-1.119 / 0.138-0.142 ms (rd_sqdiff=0: 1.177-1.181 / 0.138-0.139); unroll 4 with 2048-rule items 1.174 / 0.147, with 4096
// 1.179 / 0.144; unroll 8 with 8192-rule items 1.163 / 0.203.  The observation pre-pass (rd_qpass=1: observe_reset_kernel in place of
// the memset) measured 1.138 / 0.142 and is off (rd_prepass supersedes it: it is an A/B hook of the rd_prepass = 0 path only).  It runs at 82 VGPRs (5 waves per SIMD); capping the kernel at 6 or 7 waves per SIMD
// (amdgpu_waves_per_eu) measured 1.132 / 1.145 ms at cfg4.
// 8 column sets per lane (4096-rule items) for nant <= 5: tools/ab_rd.py, cfg4 / cfg2, medians of 5 x 20 launches on one box --
// unroll 8: 1.175 / 0.135 ms, 4: 1.263 / 0.145, 2: 1.517 / 0.178; unroll 8 with 8192-rule items 1.180 / 0.204, with 16384 1.234;
// unroll 4 with 4096-rule items 1.202 / 0.139, with 8192 1.212 (the 16-bit mirror: 1.585 / 0.149).
static constexpr int RD_PK_BITS = 6;

static int packed_words(int nant, int U)
{
    if (nant < 1 || nant > FRIRL_HIP_MAX_NANT || U < 2 || U > (1 << RD_PK_BITS)) return 0;
    if (sizeof(double) * nant * (size_t)U > RD_SMALL_TABLE_BYTES) return 0;
    return Packed<RD_PK_BITS>::words(nant);
}

template <int NANT>
struct RdPkConfig {
    static constexpr int UNROLL = NANT <= 5 ? 8 : 4;
    // with the pre-pass (rd_prepass) the prologue is a copy and 2048-rule items win: 52 VGPRs (8 waves per SIMD) instead of 80 (6).
    // cfg4 / cfg2, medians of 7 x 20 launches on one box (profiles/r06_cfg4_prepass.md): per-workgroup tables 1.077 / 0.139 ms;
    // pre-pass with unroll 8 1.074 / 0.142, unroll 4 1.053 / 0.138, unroll 4 with 4096-rule items 1.101 / 0.148, unroll 2 1.095 / 0.140,
    // unroll 2 with 2048-rule items 1.074 / 0.139, unroll 1 1.401 / 0.182; unroll 8 WITHOUT the XCD grouping of the items 1.143 / 0.143.
    static constexpr int UNROLL_PRE = 4;
};

// Workspace of the pre-pass form: [sqtab[E][NANT][2^BITS] f64 | fastv[E] u32], 16-byte aligned, owned by the caller.
static size_t packed_ws_bytes(int nant, int U, long E)
{
    if (!packed_words(nant, U) || E < 1) return 0;
    return (sizeof(double) * (size_t)nant * (1u << RD_PK_BITS) + sizeof(uint32_t)) * (size_t)E;
}

template <int NANT, int UN, bool SQ>
static void launch_pk(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint32_t *pidx, const double *x, const double *qv,
                      double *ruledists, uint32_t *hit, hipStream_t s, const RdGrid &g)
{
    if (ruledists)
        hipLaunchKernelGGL((rule_distance_pk_kernel<NANT, true, UN, RD_PK_BITS, SQ>), dim3(g.items), dim3(FRIRL_BLOCK), 0, s, t->u, t->ve, t->U, pidx,
                           b->nrules, b->maxR, x, qv, ruledists, hit, g.rules_per_block, g.cpe, b->E, g.env_fastest);
    else
        hipLaunchKernelGGL((rule_distance_pk_kernel<NANT, false, UN, RD_PK_BITS, SQ>), dim3(g.items), dim3(FRIRL_BLOCK), 0, s, t->u, t->ve, t->U, pidx,
                           b->nrules, b->maxR, x, qv, ruledists, hit, g.rules_per_block, g.cpe, b->E, g.env_fastest);
}

template <int NANT, int UN>
static void launch_pk_form(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint32_t *pidx, const double *x, const double *qv,
                           double *ruledists, uint32_t *hit, hipStream_t s, const RdGrid &g, bool sq)
{
    if (sq) launch_pk<NANT, UN, true>(t, b, pidx, x, qv, ruledists, hit, s, g);
    else launch_pk<NANT, UN, false>(t, b, pidx, x, nullptr, ruledists, hit, s, g);
}

// Pre-pass form: sq_tables_kernel (tables, flags, hit reset) + the scan whose prologue copies its environment's table.
template <int NANT, int UN>
static void launch_pk_pre(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint32_t *pidx, const double *x, double *ruledists,
                          uint32_t *hit, void *ws, hipStream_t s, const RdGrid &g)
{
    double *sqtab = static_cast<double *>(ws);
    uint32_t *fastv = reinterpret_cast<uint32_t *>(sqtab + (size_t)b->E * NANT * (1 << RD_PK_BITS));
    const int order = frirl_host::opts().rd_order;                          // 0: environments grouped by XCD (grid of whole groups)
    const unsigned items = order == 0 ? (unsigned)g.cpe * (unsigned)((b->E + RD_XCDS - 1) / RD_XCDS * RD_XCDS) : g.items;
    hipLaunchKernelGGL((sq_tables_kernel<NANT, RD_PK_BITS>), dim3((unsigned)((b->E + FRIRL_WAVES_PER_BLOCK - 1) / FRIRL_WAVES_PER_BLOCK)), dim3(FRIRL_BLOCK),
                       0, s, t->u, t->ve, t->U, b->E, x, sqtab, fastv, hit);
    if (ruledists)
        hipLaunchKernelGGL((rule_distance_pk_kernel<NANT, true, UN, RD_PK_BITS, true, true>), dim3(items), dim3(FRIRL_BLOCK), 0, s, t->u, t->ve, t->U, pidx,
                           b->nrules, b->maxR, x, nullptr, ruledists, hit, g.rules_per_block, g.cpe, b->E, order, sqtab, fastv);
    else
        hipLaunchKernelGGL((rule_distance_pk_kernel<NANT, false, UN, RD_PK_BITS, true, true>), dim3(items), dim3(FRIRL_BLOCK), 0, s, t->u, t->ve, t->U, pidx,
                           b->nrules, b->maxR, x, nullptr, ruledists, hit, g.rules_per_block, g.cpe, b->E, order, sqtab, fastv);
}

// ws: the caller's workspace (five_hip_rule_distance_packed_ws, already checked) or nullptr (five_hip_rule_distance_packed)
template <int NANT>
static int launch_packed(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint32_t *pidx, const double *x,
                         double *ruledists, uint32_t *hit, void *ws, hipStream_t s)
{
    using namespace frirl_host;
    const RdTune tn = rd_tune();
    const bool sq = opts().rd_sqdiff != 0;
    const bool pre = ws && sq && opts().rd_prepass != 0;
    const int UP = pre ? RdPkConfig<NANT>::UNROLL_PRE : RdPkConfig<NANT>::UNROLL;
    const int un = (NANT <= 5 && tn.unroll) ? tn.unroll : UP;              // tuning hook (experiments only)
    const bool qpass = sq && !pre && opts().rd_qpass == 1;
    RdGrid g;
    if (!make_grid(b, tn.chunk > 0 ? tn.chunk : 2 * FRIRL_BLOCK * un, g)) { set_error("five_hip_rule_distance_packed: too many work items"); return FRIRL_HIP_EINVAL; }
    if (pre) {
        if ((long)g.cpe * ((long)b->E + RD_XCDS) > 0x7FFFFFFFL) { set_error("five_hip_rule_distance_packed_ws: too many work items"); return FRIRL_HIP_EINVAL; }
        if constexpr (NANT <= 5) {
            if (un == 8) launch_pk_pre<NANT, 8>(t, b, pidx, x, ruledists, hit, ws, s, g);
            else if (un == 2) launch_pk_pre<NANT, 2>(t, b, pidx, x, ruledists, hit, ws, s, g);
            else if (un == 1) launch_pk_pre<NANT, 1>(t, b, pidx, x, ruledists, hit, ws, s, g);
            else launch_pk_pre<NANT, 4>(t, b, pidx, x, ruledists, hit, ws, s, g);
        } else {
            launch_pk_pre<NANT, RdPkConfig<NANT>::UNROLL_PRE>(t, b, pidx, x, ruledists, hit, ws, s, g);
        }
        return check_launch("five_hip_rule_distance_packed_ws");
    }
    void *scratch = nullptr;
    const double *qv = nullptr;
    if (qpass) {
        // [counter | qv[E][NANT]] from the stream's pool, as in launch_persist; observe_reset_kernel also resets the hit words
        const size_t qv_off = 256, bytes = qv_off + sizeof(double) * (size_t)b->E * NANT;
        const hipError_t e1 = hipMallocAsync(&scratch, bytes, s);
        if (e1 != hipSuccess) { (void)hipGetLastError(); set_error("five_hip_rule_distance_packed: hipMallocAsync(%zu B) failed: %s", bytes, hipGetErrorString(e1)); return FRIRL_HIP_ELAUNCH; }
        double *q = reinterpret_cast<double *>(static_cast<char *>(scratch) + qv_off);
        const int nq = b->E * NANT;
        hipLaunchKernelGGL(observe_reset_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, t->u, t->ve, t->U, NANT, b->E, x, q, hit, static_cast<unsigned *>(scratch));
        qv = q;
    } else if (hipMemsetAsync(hit, 0xFF, sizeof(uint32_t) * (size_t)b->E, s) != hipSuccess) {
        return check_launch("five_hip_rule_distance_packed(memset)");
    }
    if constexpr (NANT <= 5) {
        if (un == 4) launch_pk_form<NANT, 4>(t, b, pidx, x, qv, ruledists, hit, s, g, sq);
        else if (un == 2) launch_pk_form<NANT, 2>(t, b, pidx, x, qv, ruledists, hit, s, g, sq);
        else if (un == 1) launch_pk_form<NANT, 1>(t, b, pidx, x, qv, ruledists, hit, s, g, sq);
        else launch_pk_form<NANT, RdPkConfig<NANT>::UNROLL>(t, b, pidx, x, qv, ruledists, hit, s, g, sq);
    } else {
        launch_pk_form<NANT, RdPkConfig<NANT>::UNROLL>(t, b, pidx, x, qv, ruledists, hit, s, g, sq);
    }
    if (scratch && hipFreeAsync(scratch, s) != hipSuccess) { set_error("five_hip_rule_distance_packed: hipFreeAsync failed"); return FRIRL_HIP_ELAUNCH; }
    return check_launch("five_hip_rule_distance_packed");
}

// ---- Coded form (five_hip_rule_distance_coded_ws, option rd_coded): 3 bytes of indices per rule -------------------------------------
// A rule's indices as ONE code of at most 24 bits.  Every dimension k has a dictionary (the sorted distinct 6-bit indices its column
// holds, d_k of them) and a rule's digit j_k is the rank of its index in it.  Dimensions are paired in order: field f holds
// v = j_b * d_a + j_a (a = 2f, b = 2f + 1) in ceil(log2(d_a * d_b)) bits, an odd last dimension j_a alone; fields lie low to high.  The
// scan never sees the dictionaries: sq_tables_kernel<DIGIT> lays the squared differences out by digit, so a digit is a table offset
// exactly as a 6-bit field is in rule_distance_pk_kernel.  Decode of a pair field: j_b = (v * M) >> 18 with M = ceil(2^18 / d_a) -- one
// 24-bit multiply, exact for v < 4096 and d_a <= 64 (tests/test_rd_codes_host.py proves it exhaustively) -- and j_a = v - j_b * d_a.
// Layout (lane-tiled): a tile is one item of the pre-pass scan, RD_CD_TILE = 2048 consecutive rules of one environment; thread t owns
// rules 2t + p + 512 j (p < 2, j < 4) as there, its eight codes (code 2j + p at byte 3 (2j + p)) form one 24-byte little-endian string,
// and piece m (8 bytes) of that string lies at tile + 2048 m + 8 t: three aligned 8-byte loads per lane and item, 512 contiguous bytes
// per wave instruction -- the load shape of the packed scan with three loads where it has four.  codes[e][tile][3][256][8] bytes,
// ceil(maxR / 2048) tiles per environment.
static constexpr int RD_CD_TILE = 2 * FRIRL_BLOCK * 4;           // rules per tile
static constexpr int RD_CD_TILE_BYTES = 3 * RD_CD_TILE;
static constexpr int RD_CD_MAX_NANT = 5, RD_CD_FIELDS = (RD_CD_MAX_NANT + 1) / 2;

struct CodeParams {                              // uniform kernel arguments
    uint32_t shift[RD_CD_FIELDS], mask[RD_CD_FIELDS], da[RD_CD_FIELDS], magic[RD_CD_FIELDS];
};

static int ceil_log2(uint32_t n)
{
    int b = 0;
    while ((1u << b) < n) b++;
    return b;
}

// field parameters from the dictionary lengths; false when the coded form does not apply (a field over 12 bits, a code over 24)
static bool code_params(int nant, const int32_t *d, CodeParams &cp)
{
    if (nant < 1 || nant > RD_CD_MAX_NANT || !d) return false;
    int total = 0;
    for (int f = 0; f < RD_CD_FIELDS; f++) cp.shift[f] = cp.mask[f] = 0u, cp.da[f] = 1u, cp.magic[f] = 1u << 18;
    for (int k = 0; k < nant; k += 2) {
        const int f = k / 2;
        if (d[k] < 1 || d[k] > 64 || (k + 1 < nant && (d[k + 1] < 1 || d[k + 1] > 64))) return false;
        const uint32_t da = (uint32_t)d[k], db = k + 1 < nant ? (uint32_t)d[k + 1] : 1u;
        const int bits = ceil_log2(da * db);
        if (bits > 12) return false;
        cp.shift[f] = (uint32_t)total;
        cp.mask[f] = (1u << bits) - 1u;
        cp.da[f] = da;
        cp.magic[f] = ((1u << 18) + da - 1u) / da;
        total += bits;
    }
    return total <= 24;
}

static size_t coded_bytes(int nant, int U, long E, long maxR, const int32_t *d)
{
    CodeParams cp;
    if (!packed_words(nant, U) || E < 1 || maxR < 2 || !code_params(nant, d, cp)) return 0;
    return (size_t)E * (size_t)((maxR + RD_CD_TILE - 1) / RD_CD_TILE) * RD_CD_TILE_BYTES;
}

// codes from uidx: one thread per (tile, thread slot), writing its 24-byte string as three 8-byte pieces.  rank[k][i] = rank of the
// 6-bit index i in the dictionary of dimension k.  Columns at or beyond nrules[e] rounded up to the next even index get code 0 (the
// odd last rule's partner column is coded like a rule: the scans write its distance).
__global__ __launch_bounds__(FRIRL_BLOCK) void pack_codes_kernel(const uint16_t *__restrict__ uidx, const int32_t *__restrict__ nrules, int nant, int maxR,
                                                                 int tpe, long ntiles, const uint8_t *__restrict__ rank, CodeParams cp,
                                                                 uint8_t *__restrict__ codes)
{
    const int t = threadIdx.x;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long e = tile / tpe;
        const int c = (int)(tile - e * tpe);
        const int R = nrules[e];
        const int Rp = min(R + (R & 1), maxR);
        const uint16_t *__restrict__ src = uidx + (size_t)e * nant * maxR;
        uint32_t code[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int r = c * RD_CD_TILE + 2 * t + (i & 1) + 2 * FRIRL_BLOCK * (i >> 1);
            uint32_t v = 0u;
            if (r < Rp) {
                for (int k = 0; k < nant; k += 2) {
                    const uint32_t ja = rank[k * 64 + (src[(size_t)k * maxR + r] & 63u)];
                    const uint32_t jb = k + 1 < nant ? rank[(k + 1) * 64 + (src[(size_t)(k + 1) * maxR + r] & 63u)] : 0u;
                    v |= (jb * cp.da[k / 2] + ja) << cp.shift[k / 2];
                }
            }
            code[i] = v & 0xFFFFFFu;
        }
        u32x2_t *__restrict__ dst = reinterpret_cast<u32x2_t *>(codes + (size_t)tile * RD_CD_TILE_BYTES + 8 * t);
        u32x2_t p0, p1, p2;
        p0.x = code[0] | code[1] << 24;  p0.y = code[1] >> 8 | code[2] << 16;
        p1.x = code[2] >> 16 | code[3] << 8;  p1.y = code[4] | code[5] << 24;
        p2.x = code[5] >> 8 | code[6] << 16;  p2.y = code[6] >> 16 | code[7] << 8;
        dst[0] = p0;
        dst[RD_CD_TILE / 8] = p1;                // + 2048 bytes
        dst[2 * (RD_CD_TILE / 8)] = p2;
    }
}

// What the scan derives from CodeParams once per wave (scalar registers): the decode of a pair field works in BYTE offsets.  The codes
// are unpacked to bit 3 (code8 = code << 3, rubbish below bit 3 and above bit 27), so that for a field at `shift`
//   v8  = (code8 >> shift) & (mask << 3)                   8 v: v < 2^bits <= 4096, v8 < 2^15           (field 0: shift = 0, the mask alone)
//   jb8 = ((v8 * magic) >> 18) & RD_CD_Q8                  8 (v / d_a): v8 * magic = 8 (v * magic), so the shift by 18 leaves 8 j_b + three
//                                                          bits of the fraction, which the mask drops; v_mul_u32_u24: v8 < 2^15 < 2^24,
//                                                          magic <= 2^18 < 2^24, and v8 * magic < 2^32: 2^bits < 2 d_a d_b, so the product is
//                                                          below 16 d_a d_b (2^18 / d_a + 1) <= 2^28 + 2^16
//   ja8 = v8 - jb8 * d_a                                   8 (v mod d_a): one v_mad_i32_i24 with -d_a: jb8 < 2^10, |-d_a| <= 64, no overflow
// all exact for every v below 2^bits (tests/test_rd_decode_host.py; v / d_a < 2 d_b <= 128 there, which RD_CD_Q8 holds); the pack kernel
// writes v < d_a d_b only.  A single field is its shift and mask.
static constexpr uint32_t RD_CD_Q8 = 127u << 3;
struct CodeScan {
    uint32_t shift[RD_CD_FIELDS], mask8[RD_CD_FIELDS], magic[RD_CD_FIELDS];
    int32_t negda[RD_CD_FIELDS];
    __device__ __forceinline__ explicit CodeScan(const CodeParams &cp)
    {
#pragma unroll
        for (int f = 0; f < RD_CD_FIELDS; f++) shift[f] = cp.shift[f], mask8[f] = (cp.mask[f] & 0xFFFu) << 3, magic[f] = cp.magic[f], negda[f] = -(int32_t)cp.da[f];
    }
};

__device__ __forceinline__ double cd_table_entry(const double *__restrict__ tab_k, uint32_t off8)
{
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(tab_k) + off8);
}

// the sum of a rule's NANT squared differences, dimensions ascending, from its code at bit 3 (other bits are ignored: every field is masked)
template <int NANT>
__device__ __forceinline__ double cd_rule_sq(uint32_t code8, const double *__restrict__ sq_s, const CodeScan &cs)
{
    constexpr int TS = 64;
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < NANT; k += 2) {
        const int f = k / 2;
        const uint32_t v8 = (f == 0 ? code8 : code8 >> cs.shift[f]) & cs.mask8[f];       // code_params: shift[0] = 0
        if (k + 1 < NANT) {
            const uint32_t jb8 = (__umul24(v8, cs.magic[f]) >> 18) & RD_CD_Q8;
            const uint32_t ja8 = (uint32_t)(__mul24((int)jb8, cs.negda[f]) + (int)v8);
            const double sa = cd_table_entry(sq_s + k * TS, ja8);
            const double sb = cd_table_entry(sq_s + (k + 1) * TS, jb8);
            a = k == 0 ? sa : a + sa;
            a = a + sb;
        } else {
            const double sa = cd_table_entry(sq_s + k * TS, v8);
            a = k == 0 ? sa : a + sa;
        }
    }
    return a;
}

// blockIdx.x / d for the scan's grid: d = RD_XCDS * cpe >= 8 and fewer than 2^31 workgroups.  With l = ceil(log2 d) and
// mul = ceil(2^(31 + l) / d) (d > 2^(l - 1): mul < 2^32), n / d = (n * mul) >> (31 + l) for every n < 2^31: the error of the product,
// n * (mul * d - 2^(31 + l)) / d < 2^31 * d / d, stays below the 2^(31 + l) / d that one step of the quotient's fraction is worth.
struct GroupDiv { uint32_t mul, shift; };        // quotient = __umulhi(n, mul) >> shift
static GroupDiv group_div(uint32_t d)
{
    const int l = ceil_log2(d);
    GroupDiv g;
    g.mul = (uint32_t)(((1ull << (31 + l)) + d - 1) / d);
    g.shift = (uint32_t)(l - 1);
    return g;
}

// The coded scan: the pre-pass form of rule_distance_pk_kernel (items of 2048 rules grouped by XCD, four column sets per lane, the table
// copy, the same adds, square roots and stores) reading three 8-byte pieces of codes per lane and item.
// First exact hit, off the common path: the sweep only keeps the lane's minimum of the HIGH WORDS of the squared sums (FAST) or distances
// (one v_min3_u32 per pair: +0 has a zero high word, a NaN has not), and the wave leaves unless one of its lanes saw a zero high word.
// Such a wave (a handful per launch; a subnormal sum would bring it here too, and find nothing) decodes its codes again, takes the lowest zero rule per lane under the bounds of the sweep (the partner column of an odd last rule is
// swept, and may bring the wave here, but is no rule), reduces over the wave and issues one atomicMin: no LDS, no second barrier.
template <int NANT, bool WRITE>
__global__ __launch_bounds__(FRIRL_BLOCK) void rule_distance_cd_kernel(const uint8_t *__restrict__ codes, const int32_t *__restrict__ nrules, int maxR,
                                                                     double *__restrict__ dists, uint32_t *__restrict__ hit, int cpe, int E,
                                                                     const double *__restrict__ sqtab, const uint32_t *__restrict__ fastv, CodeParams cp,
                                                                     GroupDiv gd)
{
    constexpr int TS = 64, STEP = FRIRL_BLOCK * 2;
    __shared__ __attribute__((aligned(16))) double sq_s[NANT * TS];
    const unsigned grp = __umulhi(blockIdx.x, gd.mul) >> gd.shift, gj = blockIdx.x - grp * (unsigned)(RD_XCDS * cpe);
    const int e = (int)(grp * RD_XCDS + gj % RD_XCDS);
    const int c = (int)(gj / RD_XCDS);
    if (e >= E) return;
    const int R = nrules[e];
    const int r0 = c * RD_CD_TILE;
    if (r0 >= R) return;
    int r_end = r0 + RD_CD_TILE;
    if (r_end > R) r_end = R;

    const int r = r0 + 2 * (int)threadIdx.x;
    const bool any = r < r_end;                  // the lane's first pair is its lowest: without it the lane has no rule in this tile
    u32x2_t w[3];
    if (any) {                                   // the whole tile exists (codes are allocated in whole tiles): aligned, in bounds
        const uint8_t *__restrict__ src = codes + ((size_t)e * cpe + c) * RD_CD_TILE_BYTES + 8 * threadIdx.x;
#pragma unroll
        for (int m = 0; m < 3; m++) w[m] = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t *>(src + m * RD_CD_TILE));
    }
    constexpr int N2 = NANT * TS / 2;
    const double2 *__restrict__ tsrc = reinterpret_cast<const double2 *>(sqtab + (size_t)e * (NANT * TS));
    for (int i = threadIdx.x; i < N2; i += FRIRL_BLOCK) reinterpret_cast<double2 *>(sq_s)[i] = tsrc[i];
    const bool fast = fastv[e] != 0u;
    const CodeScan cs(cp);
    __syncthreads();

    double *__restrict__ out = WRITE ? dists + (size_t)e * maxR : nullptr;
    uint32_t code[8];                            // at bit 3
    uint32_t lo = ~0u;                           // minimum high word of what the lane's hit test compares with 0.0
    auto sweep = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {
                const double a0 = cd_rule_sq<NANT>(code[2 * j], sq_s, cs), a1 = cd_rule_sq<NANT>(code[2 * j + 1], sq_s, cs);
                double2 d;
                if (FAST) {
                    d.x = sqrt_unscaled(a0);
                    d.y = sqrt_unscaled(a1);
                    lo = min(lo, min((uint32_t)__double2hiint(a0), (uint32_t)__double2hiint(a1)));     // sqrt(a) == 0 exactly when a == 0
                } else {
                    d.x = __dsqrt_rn(a0);
                    d.y = __dsqrt_rn(a1);
                    lo = min(lo, min((uint32_t)__double2hiint(d.x), (uint32_t)__double2hiint(d.y)));
                }
                if (WRITE) { __builtin_nontemporal_store(d.x, out + rr); __builtin_nontemporal_store(d.y, out + rr + 1); }
            }
        }
    };
    auto first_hit = [&](auto fast_tag) -> unsigned {
        constexpr bool FAST = decltype(fast_tag)::value;
        unsigned best = FRIRL_HIP_NO_HIT;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int rr = r + j * STEP;
            if (rr < r_end) {
                const double a0 = cd_rule_sq<NANT>(code[2 * j], sq_s, cs), a1 = cd_rule_sq<NANT>(code[2 * j + 1], sq_s, cs);
                const bool z0 = FAST ? a0 == 0.0 : __dsqrt_rn(a0) == 0.0, z1 = FAST ? a1 == 0.0 : __dsqrt_rn(a1) == 0.0;
                if (z1 && rr + 1 < R) best = min(best, (unsigned)(rr + 1));
                if (z0) best = min(best, (unsigned)rr);
            }
        }
        return best;
    };
    if (any) {
        code[0] = w[0].x << 3;
        code[1] = __builtin_amdgcn_alignbit(w[0].y, w[0].x, 21);
        code[2] = __builtin_amdgcn_alignbit(w[1].x, w[0].y, 13);
        code[3] = w[1].x >> 5;
        code[4] = w[1].y << 3;
        code[5] = __builtin_amdgcn_alignbit(w[2].x, w[1].y, 21);
        code[6] = __builtin_amdgcn_alignbit(w[2].y, w[2].x, 13);
        code[7] = w[2].y >> 5;
        if (fast) sweep(std::true_type{});
        else sweep(std::false_type{});
    }
    if (!__any(lo == 0u)) return;                // uniform for the wave
    unsigned best = FRIRL_HIP_NO_HIT;
    if (any) best = fast ? first_hit(std::true_type{}) : first_hit(std::false_type{});
    best = wave_min_u32(best);                   // every lane of the wave is here
    if ((threadIdx.x & (FRIRL_WAVE - 1)) == 0 && best != FRIRL_HIP_NO_HIT) atomicMin(&hit[e], best);
}

template <int NANT>
static int launch_coded(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint8_t *codes, const uint8_t *dict, const CodeParams &cp,
                        const double *x, double *ruledists, uint32_t *hit, void *ws, hipStream_t s)
{
    using namespace frirl_host;
    const long cpe = ((long)b->maxR + RD_CD_TILE - 1) / RD_CD_TILE;
    if (cpe * ((long)b->E + RD_XCDS) > 0x7FFFFFFFL) { set_error("five_hip_rule_distance_coded_ws: too many work items"); return FRIRL_HIP_EINVAL; }
    double *sqtab = static_cast<double *>(ws);
    uint32_t *fastv = reinterpret_cast<uint32_t *>(sqtab + (size_t)b->E * NANT * (1 << RD_PK_BITS));
    const unsigned items = (unsigned)cpe * (unsigned)((b->E + RD_XCDS - 1) / RD_XCDS * RD_XCDS);
    const GroupDiv gd = group_div((uint32_t)(RD_XCDS * cpe));
    hipLaunchKernelGGL((sq_tables_kernel<NANT, RD_PK_BITS, true>), dim3((unsigned)((b->E + FRIRL_WAVES_PER_BLOCK - 1) / FRIRL_WAVES_PER_BLOCK)), dim3(FRIRL_BLOCK),
                       0, s, t->u, t->ve, t->U, b->E, x, sqtab, fastv, hit, dict);
    if (ruledists)
        hipLaunchKernelGGL((rule_distance_cd_kernel<NANT, true>), dim3(items), dim3(FRIRL_BLOCK), 0, s, codes, b->nrules, b->maxR, ruledists, hit, (int)cpe,
                           b->E, sqtab, fastv, cp, gd);
    else
        hipLaunchKernelGGL((rule_distance_cd_kernel<NANT, false>), dim3(items), dim3(FRIRL_BLOCK), 0, s, codes, b->nrules, b->maxR, ruledists, hit, (int)cpe,
                           b->E, sqtab, fastv, cp, gd);
    return check_launch("five_hip_rule_distance_coded_ws");
}

// Probes for the tests (five_hip_sqrt_unscaled_check, five_hip_rule_distance_sq_guard): the device functions the packed scan uses.
__global__ void sqrt_unscaled_check_kernel(const double *__restrict__ a, double *__restrict__ fast, double *__restrict__ ref, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fast[i] = sqrt_unscaled(a[i]);
    ref[i] = __dsqrt_rn(a[i]);
}

template <int NANT>
__global__ __launch_bounds__(FRIRL_BLOCK) void sq_guard_kernel(const double *__restrict__ u, const double *__restrict__ ve, int U,
                                                             const double *__restrict__ x, int32_t *__restrict__ ok)
{
    constexpr int TS = 1 << RD_PK_BITS;
    __shared__ double sq_s[NANT * TS];
    __shared__ double q_s[NANT];
    const int e = blockIdx.x;
    double tv[(NANT * TS + FRIRL_BLOCK - 1) / FRIRL_BLOCK];
    load_sq_sources<NANT, RD_PK_BITS, FRIRL_BLOCK>(ve, U, tv, (int)threadIdx.x);
    if (threadIdx.x < NANT) q_s[threadIdx.x] = observe_ve(u, ve, U, threadIdx.x, x[(size_t)e * NANT + threadIdx.x]);
    __syncthreads();
    const bool fast = !__syncthreads_or(!fill_sq_table<NANT, RD_PK_BITS, FRIRL_BLOCK>(q_s, sq_s, tv, (int)threadIdx.x));
    if (threadIdx.x == 0) ok[e] = fast ? 1 : 0;
}

}  // namespace frirl

extern "C" int five_hip_rule_distance_uses_uidx(int32_t nant, int32_t U)
{
    return nant >= 1 && nant <= FRIRL_HIP_MAX_NANT && U <= 65536 && sizeof(double) * nant * (size_t)U <= 150 * 1024 && !frirl_host::opts().no_uidx;
}

extern "C" int five_hip_rule_distance(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const double *x,
                                      double *ruledists, uint32_t *hit, void *stream)
{
    using namespace frirl_host;
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!x || !hit) { set_error("five_hip_rule_distance: NULL x/hit"); return FRIRL_HIP_EINVAL; }
    if (ruledists && (reinterpret_cast<uintptr_t>(ruledists) & 15)) { set_error("five_hip_rule_distance: ruledists must be 16-byte aligned"); return FRIRL_HIP_EINVAL; }
    if ((rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);

    switch (t->nant) {
#define FRIRL_CASE(N) case N: return frirl::launch_nant<N>(t, b, x, ruledists, hit, s);
        FRIRL_CASE(1) FRIRL_CASE(2) FRIRL_CASE(3) FRIRL_CASE(4) FRIRL_CASE(5) FRIRL_CASE(6) FRIRL_CASE(7) FRIRL_CASE(8)
        FRIRL_CASE(9) FRIRL_CASE(10) FRIRL_CASE(11) FRIRL_CASE(12) FRIRL_CASE(13) FRIRL_CASE(14) FRIRL_CASE(15) FRIRL_CASE(16)
#undef FRIRL_CASE
    }
    set_error("five_hip_rule_distance: unsupported nant=%d", t->nant);
    return FRIRL_HIP_EINVAL;
}

extern "C" int five_hip_rule_distance_packed_words(int32_t nant, int32_t U)
{
    return frirl::packed_words(nant, U);
}

extern "C" int frirl_hip_pack_indices(const frirl_hip_tables *t, const frirl_hip_rulebases *b, uint32_t *pidx, void *stream)
{
    using namespace frirl_host;
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!b->uidx || !pidx) { set_error("frirl_hip_pack_indices: NULL uidx/pidx"); return FRIRL_HIP_EINVAL; }
    if (!frirl::packed_words(t->nant, t->U)) { set_error("frirl_hip_pack_indices: nant=%d U=%d is not served by the packed form", t->nant, t->U); return FRIRL_HIP_EINVAL; }
    if ((rc = check_device())) return rc;
    const long total = (long)b->E * b->maxR;
    long grid = (total + FRIRL_BLOCK - 1) / FRIRL_BLOCK;
    if (grid > (long)frirl::device_cus() * 32) grid = (long)frirl::device_cus() * 32;
    hipLaunchKernelGGL(frirl::pack_indices_kernel<frirl::RD_PK_BITS>, dim3((unsigned)grid), dim3(FRIRL_BLOCK), 0, as_stream(stream), b->uidx, t->nant,
                       b->maxR, total, pidx);
    return check_launch("frirl_hip_pack_indices");
}

extern "C" int five_hip_sqrt_unscaled_check(const double *a, double *fast, double *ref, int64_t n, void *stream)
{
    using namespace frirl_host;
    if (n < 0 || (n && (!a || !fast || !ref))) { set_error("five_hip_sqrt_unscaled_check: bad arguments"); return FRIRL_HIP_EINVAL; }
    int rc = check_device();
    if (rc) return rc;
    if (n) hipLaunchKernelGGL(frirl::sqrt_unscaled_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), a, fast, ref, (long)n);
    return check_launch("five_hip_sqrt_unscaled_check");
}

extern "C" int five_hip_rule_distance_sq_guard(const frirl_hip_tables *t, int32_t E, const double *x, int32_t *ok, void *stream)
{
    using namespace frirl_host;
    int rc = check_tables(t);
    if (rc) return rc;
    if (!frirl::packed_words(t->nant, t->U)) { set_error("five_hip_rule_distance_sq_guard: nant=%d U=%d is not served by the packed form", t->nant, t->U); return FRIRL_HIP_EINVAL; }
    if (E < 0 || (E && (!x || !ok))) { set_error("five_hip_rule_distance_sq_guard: bad arguments"); return FRIRL_HIP_EINVAL; }
    if ((rc = check_device())) return rc;
    if (!E) return 0;
    switch (t->nant) {
#define FRIRL_CASE(N) case N: hipLaunchKernelGGL(frirl::sq_guard_kernel<N>, dim3((unsigned)E), dim3(FRIRL_BLOCK), 0, as_stream(stream), t->u, t->ve, t->U, x, ok); break;
        FRIRL_CASE(1) FRIRL_CASE(2) FRIRL_CASE(3) FRIRL_CASE(4) FRIRL_CASE(5) FRIRL_CASE(6) FRIRL_CASE(7) FRIRL_CASE(8)
        FRIRL_CASE(9) FRIRL_CASE(10) FRIRL_CASE(11) FRIRL_CASE(12) FRIRL_CASE(13) FRIRL_CASE(14) FRIRL_CASE(15) FRIRL_CASE(16)
#undef FRIRL_CASE
    }
    return check_launch("five_hip_rule_distance_sq_guard");
}

static int rule_distance_packed(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint32_t *pidx, const double *x,
                                double *ruledists, uint32_t *hit, void *ws, void *stream)
{
    using namespace frirl_host;
    int rc;
    // shapes the packed form does not serve, and the A/B / test switches: the scan of five_hip_rule_distance (16-bit mirror or f64 columns)
    const Options &o = opts();
    if (!frirl::packed_words(t->nant, t->U) || !o.rd_packed || o.no_uidx || o.rd_persist == 1)
        return five_hip_rule_distance(t, b, x, ruledists, hit, stream);
    if (!pidx || !x || !hit) { set_error("five_hip_rule_distance_packed: NULL pidx/x/hit"); return FRIRL_HIP_EINVAL; }
    if (reinterpret_cast<uintptr_t>(pidx) & 7) { set_error("five_hip_rule_distance_packed: pidx must be 8-byte aligned"); return FRIRL_HIP_EINVAL; }
    if (ruledists && (reinterpret_cast<uintptr_t>(ruledists) & 15)) { set_error("five_hip_rule_distance_packed: ruledists must be 16-byte aligned"); return FRIRL_HIP_EINVAL; }
    if ((rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);

    switch (t->nant) {
#define FRIRL_CASE(N) case N: return frirl::launch_packed<N>(t, b, pidx, x, ruledists, hit, ws, s);
        FRIRL_CASE(1) FRIRL_CASE(2) FRIRL_CASE(3) FRIRL_CASE(4) FRIRL_CASE(5) FRIRL_CASE(6) FRIRL_CASE(7) FRIRL_CASE(8)
        FRIRL_CASE(9) FRIRL_CASE(10) FRIRL_CASE(11) FRIRL_CASE(12) FRIRL_CASE(13) FRIRL_CASE(14) FRIRL_CASE(15) FRIRL_CASE(16)
#undef FRIRL_CASE
    }
    set_error("five_hip_rule_distance_packed: unsupported nant=%d", t->nant);
    return FRIRL_HIP_EINVAL;
}

extern "C" int five_hip_rule_distance_packed(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint32_t *pidx, const double *x,
                                             double *ruledists, uint32_t *hit, void *stream)
{
    const int rc = frirl_host::check_rulebases(t, b);
    return rc ? rc : rule_distance_packed(t, b, pidx, x, ruledists, hit, nullptr, stream);
}

extern "C" size_t five_hip_rule_distance_packed_workspace_bytes(int32_t nant, int32_t U, int32_t E)
{
    return frirl::packed_ws_bytes(nant, U, E);
}

extern "C" int five_hip_rule_distance_packed_ws(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint32_t *pidx, const double *x,
                                                double *ruledists, uint32_t *hit, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frirl_host;
    const int rc = check_rulebases(t, b);
    if (rc) return rc;
    const size_t need = frirl::packed_ws_bytes(t->nant, t->U, b->E);      // 0: a shape the packed form does not serve (no workspace)
    if (need) {
        if (!workspace || workspace_bytes < need) {
            set_error("five_hip_rule_distance_packed_ws: workspace of %zu B at %p, nant=%d U=%d E=%d needs %zu B "
                      "(five_hip_rule_distance_packed_workspace_bytes)", workspace_bytes, workspace, t->nant, t->U, b->E, need);
            return FRIRL_HIP_EINVAL;
        }
        if (reinterpret_cast<uintptr_t>(workspace) & 15) { set_error("five_hip_rule_distance_packed_ws: workspace must be 16-byte aligned"); return FRIRL_HIP_EINVAL; }
    }
    return rule_distance_packed(t, b, pidx, x, ruledists, hit, need ? workspace : nullptr, stream);
}

extern "C" size_t five_hip_rule_distance_coded_bytes(int32_t nant, int32_t U, int32_t E, int32_t maxR, const int32_t *d)
{
    return frirl::coded_bytes(nant, U, E, maxR, d);
}

extern "C" int frirl_hip_pack_codes(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint8_t *rank, const int32_t *d, uint8_t *codes,
                                    void *stream)
{
    using namespace frirl_host;
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    if (!b->uidx || !rank || !codes) { set_error("frirl_hip_pack_codes: NULL uidx/rank/codes"); return FRIRL_HIP_EINVAL; }
    frirl::CodeParams cp;
    if (!frirl::coded_bytes(t->nant, t->U, b->E, b->maxR, d) || !frirl::code_params(t->nant, d, cp)) {
        set_error("frirl_hip_pack_codes: nant=%d U=%d with these dictionary lengths is not served by the coded form", t->nant, t->U);
        return FRIRL_HIP_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(codes) & 7) { set_error("frirl_hip_pack_codes: codes must be 8-byte aligned"); return FRIRL_HIP_EINVAL; }
    if ((rc = check_device())) return rc;
    const int tpe = (b->maxR + frirl::RD_CD_TILE - 1) / frirl::RD_CD_TILE;
    const long ntiles = (long)b->E * tpe;
    long grid = ntiles;
    if (grid > (long)frirl::device_cus() * 32) grid = (long)frirl::device_cus() * 32;
    hipLaunchKernelGGL(frirl::pack_codes_kernel, dim3((unsigned)grid), dim3(FRIRL_BLOCK), 0, as_stream(stream), b->uidx, b->nrules, t->nant, b->maxR, tpe,
                       ntiles, rank, cp, codes);
    return check_launch("frirl_hip_pack_codes");
}

extern "C" int five_hip_rule_distance_coded_ws(const frirl_hip_tables *t, const frirl_hip_rulebases *b, const uint8_t *codes, const uint8_t *dict,
                                               const int32_t *d, const uint32_t *pidx, const double *x, double *ruledists, uint32_t *hit,
                                               void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frirl_host;
    int rc = check_rulebases(t, b);
    if (rc) return rc;
    // the A/B hooks keep selecting the kernels they select without the coded form: any of them set, the 4-byte route runs
    const Options &o = opts();
    const bool plain = !o.rd_coded || !o.rd_packed || !o.rd_sqdiff || !o.rd_prepass || o.rd_persist == 1 || o.no_uidx || o.rd_order != 0 ||
                       (o.rd_unroll != 0 && o.rd_unroll != 4) || (o.rd_chunk != 0 && o.rd_chunk != frirl::RD_CD_TILE);
    frirl::CodeParams cp;
    if (plain || !frirl::coded_bytes(t->nant, t->U, b->E, b->maxR, d) || !frirl::code_params(t->nant, d, cp))
        return five_hip_rule_distance_packed_ws(t, b, pidx, x, ruledists, hit, workspace, workspace_bytes, stream);
    const size_t need = frirl::packed_ws_bytes(t->nant, t->U, b->E);
    if (!workspace || workspace_bytes < need) {
        set_error("five_hip_rule_distance_coded_ws: workspace of %zu B at %p, nant=%d U=%d E=%d needs %zu B "
                  "(five_hip_rule_distance_packed_workspace_bytes)", workspace_bytes, workspace, t->nant, t->U, b->E, need);
        return FRIRL_HIP_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 15) { set_error("five_hip_rule_distance_coded_ws: workspace must be 16-byte aligned"); return FRIRL_HIP_EINVAL; }
    if (!codes || !dict || !x || !hit) { set_error("five_hip_rule_distance_coded_ws: NULL codes/dict/x/hit"); return FRIRL_HIP_EINVAL; }
    if (reinterpret_cast<uintptr_t>(codes) & 7) { set_error("five_hip_rule_distance_coded_ws: codes must be 8-byte aligned"); return FRIRL_HIP_EINVAL; }
    if (ruledists && (reinterpret_cast<uintptr_t>(ruledists) & 15)) { set_error("five_hip_rule_distance_coded_ws: ruledists must be 16-byte aligned"); return FRIRL_HIP_EINVAL; }
    if ((rc = check_device())) return rc;
    hipStream_t s = as_stream(stream);
    switch (t->nant) {
#define FRIRL_CASE(N) case N: return frirl::launch_coded<N>(t, b, codes, dict, cp, x, ruledists, hit, workspace, s);
        FRIRL_CASE(1) FRIRL_CASE(2) FRIRL_CASE(3) FRIRL_CASE(4) FRIRL_CASE(5)
#undef FRIRL_CASE
    }
    set_error("five_hip_rule_distance_coded_ws: unsupported nant=%d", t->nant);
    return FRIRL_HIP_EINVAL;
}
