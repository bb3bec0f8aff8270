// Ranked Boolean queries in one call (ansx_topk_bool_batch_dev): per query the k ids with the largest scores among the
// ids of ALL of its lists (or of ANY of them), less the ids of its excluded lists; DESIGN.md section 3n.  gfx950 only.
//
// Under ALL a group runs as one of ansx_intersect_batch_dev (ansx_intersect_batch.h) with a u32 score beside every
// candidate:
//   k_isectb_gather   as it is: every query's driver ids -> the first candidates.
//   k_topkb_match     k_isectb_match carrying a score: the same launch shape, ballots and tile counts.  Round 0 first
//                     seeds every candidate -- of queries without a list in this round too: a candidate stays a member
//                     only where it is the first of its run of equal ids inside its query's segment, and its score
//                     starts as the saturating sum of sat32(driver's weight * payload) over that run.  In every round in
//                     which its query has a list it takes the lower bound t's position p in the list, member = found
//                     and equal, and adds sat32(weight * payload[p']) for every p' >= p with list[p'] == t.
//                     Two forms (ANSX_TOPK_BOOL_FORM): "search", the parent's whole-list lower bound; the default,
//                     where a tile inside one query first bounds -- two threads, bx_lower / bx_upper --
//                     the part [lo, hi) of the round's list its first and last candidate can meet, and every thread
//                     searches only there.  A tile that spans queries searches whole lists.
//   k_dr_scan<u64, false>, k_isect_compact (once for the ids, once more with the scores as its `cand`: the same
//   ballots), k_isectb_bounds   as they are.
// Behind the rounds, where the group excludes something: bool_exclude_step (ansx_bool.h) and the second k_isect_compact.
// Under ANY a group runs as one of ansx_topk_batch_dev (ansx_topk.h) up to k_topk_scores, then the same exclusion step
// over the heads.  Either way:
//   k_topkb_check     a surviving candidate whose score is 0xFFFFFFFF lowers the overflow word to its query (atomicMin).
//                     A saturating add keeps a score equal to 0xFFFFFFFF exactly when the 64-bit sum reaches 2^32 - 1.
//   k_topk_hist / k_topk_pick x 8, k_topk_gather, k_topk_sort   as they are, over (ids, scores, bounds).
// No workgroup waits for another.  k_topkb_check returns at once when the scan's flag word names a list; the host
// enqueues no round of k_topkb_match before the decode's and the scan's flag words have come back clean.
//
// Memory safety for ANY content of the containers and payloads.  Every index comes from the host as in
// ansx_intersect_batch.h: G's src + count and the tables' at + n lie inside the buffer of ids isb_plan laid out from
// the checked headers, and the buffer of payloads has the same layout and size, so a payload is read at the index an
// id of the same list is, or could be, read at.  seg is the table's dst or k_isectb_bounds' output, 0 <= seg[j] <=
// seg[j + 1] <= nc.  The seeding reads candidates [seg[q], seg[q + 1]) of its own query only -- i - 1 only where
// i > seg[q], and the run's end stops at seg[q + 1] -- and the payloads G[q].src + (e - G[q].dst) with e inside that
// segment, which in round 0 is the driver's span.  bx_lower / bx_upper return a value inside [lo, hi] of their
// arguments; the bounded part is clamped to lo <= hi <= L.n, and the walk over equal ids stops at L.n.  Payload VALUES
// are only multiplied and added; ids only compared.  A thread writes score i < nc of its own candidate, word i / 64 of
// the ballots and its own tile's count.  k_topkb_check reads heads below min(*total, n) and bounds at j <= Q.
#pragma once

#include "ansx_bool.h"
#include "ansx_topk.h"

#define ANSX_TOPKB_FORM_DEFAULT 0u  // a tile inside one query searches the part of the list it can meet
#define ANSX_TOPKB_FORM_SEARCH 1u   // the whole list, always

// Round `round` over the nc > 0 candidates; k_isectb_match's launch shape.  pay: the group's payloads, laid out as ids
// (null: every payload is 1); score[i]: candidate i's score, written in round 0 and added to afterwards; G / wd: every
// query's driver and its weight (read in round 0); rw: the weight of every entry of rt.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topkb_match(const u32* __restrict__ ids, const u32* __restrict__ pay,
    const u32* __restrict__ cand, u32* __restrict__ score, u32 nc, const u32* __restrict__ seg, u32 Q,
    const ansx_isb_query* __restrict__ G, const u32* __restrict__ wd, const u32* __restrict__ rt_off,
    const ansx_isb_list* __restrict__ rt, const u32* __restrict__ rw, u32 round, u32 form, u64* __restrict__ ballots,
    u64* __restrict__ counts)
{
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    __shared__ u32 qb[2];
    __shared__ u64 rng[2];
    const u32 tid = threadIdx.x;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    const u64 last = (i0 + ANSX_ISECT_TILE < nc ? i0 + ANSX_ISECT_TILE : nc) - 1;  // (the grid: i0 < nc)
    if (tid == 0) {  // the queries of the tile's first and last candidate
        qb[0] = isb_query_of(seg, 0, Q - 1, (u32)i0);
        qb[1] = isb_query_of(seg, qb[0], Q - 1, (u32)last);
    }
    __syncthreads();
    const u32 q0 = qb[0], q1 = qb[1];
    // inside one query that has a list in this round: the part of the list the tile can meet (the workgroup's decision)
    bool bounded = false;
    u64 blo = 0, bhi = 0;
    if (form != ANSX_TOPKB_FORM_SEARCH && q0 == q1) {
        const u32 e = rt_off[q0] + round;
        if (e >= rt_off[q0] && e < rt_off[q0 + 1]) {
            const ansx_isb_list L = rt[e];
            const u32* __restrict__ list = ids + L.at;
            if (tid == 0) rng[0] = bx_lower(list, 0, L.n, cand[i0]);
            if (tid == 64) rng[1] = bx_upper(list, 0, L.n, cand[last]);
            __syncthreads();
            blo = rng[0], bhi = rng[1];
            bhi = bhi < blo ? blo : bhi;  // (blo <= L.n and bhi <= L.n: bx_lower, bx_upper)
            bounded = true;
        }
    }
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = i0 + k * ANSX_ISECT_NT + tid;
        bool member = false;
        if (i < nc) {
            const u32 q = isb_query_of(seg, q0, q1, (u32)i);  // (no step while the tile lies inside one query)
            const u32 t = cand[i];
            u32 sc = 0;
            member = true;
            if (round == 0) {  // the seed: the first of its run of equal ids takes the run's postings
                const u32 s0 = seg[q], s1 = seg[q + 1];
                member = i == s0 || cand[i - 1] != t;
                if (member) {
                    const u32 w = wd[q];
                    const u32* __restrict__ pv = pay ? pay + G[q].src : nullptr;
                    const u64 d0 = G[q].dst;
                    for (u64 e = i; e < s1 && cand[e] == t; e++) sc = topk_sat_add(sc, pv ? topk_sat32(w, pv[e - d0]) : w);
                }
            } else {
                sc = score[i];
            }
            const u32 e = rt_off[q] + round;
            if (member && e >= rt_off[q] && e < rt_off[q + 1]) {  // (else no list in this round: passed through)
                const ansx_isb_list L = rt[e];
                const u32* __restrict__ list = ids + L.at;
                const u64 hi = bounded ? bhi : L.n;
                u64 p = bx_lower(list, bounded ? blo : 0, hi, t);  // the first p with list[p] >= t
                member = p < hi && list[p] == t;
                if (member) {
                    const u32 w = rw[e];
                    const u32* __restrict__ pv = pay ? pay + L.at : nullptr;
                    for (; p < L.n && list[p] == t; p++) sc = topk_sat_add(sc, pv ? topk_sat32(w, pv[p]) : w);
                }
            }
            if (member) score[i] = sc;
        }
        isect_ballot(member, i - (tid & 63u), nc, k * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    isect_tile_count(wcnt, counts);
}

// A workgroup per ANSX_ISECT_TILE candidates h < min(*total, n) (total null: n), score[h] beside them, query j's in
// [hseg[j], hseg[j + 1]): a score of 0xFFFFFFFF -> oflow[0] = min(oflow[0], its query).
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topkb_check(const u32* __restrict__ score, const u32* __restrict__ hseg, u32 Q,
    const u64* __restrict__ total, u32 n, u32* __restrict__ oflow, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    const u64 tot = qt_limit(total, n);
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u64 h = qt_elem(i0, q, threadIdx.x);
        if (h < tot && score[h] == 0xFFFFFFFFu) atomicMin(oflow, isb_query_of(hseg, 0, Q - 1, (u32)h));
    }
}
