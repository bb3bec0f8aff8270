// Ranked queries with required, optional and excluded terms and a minimum-should-match (ansx_topk_query_batch_dev): per
// query the k ids with the largest scores among the ids of ALL required lists that have at least m entries in the
// optional lists and occur in no excluded list; DESIGN.md section 3p.  gfx950 only.
//
// A query with a required term (kind R) runs as one of ansx_topk_bool_batch_dev under ALL (ansx_topk_bool.h) over its
// REQUIRED terms -- k_isectb_gather, the rounds of k_topkb_match, which leave every candidate once with the score of its
// required postings -- and then ONE step over what is left, however many optional lists the queries have:
//   k_topkq_should    k_bool_exclude's launch shape and its two regimes.  Candidate i of query j is looked up in every
//                     list of ot[ot_off[j] .. ot_off[j + 1]) (the host's table, ansx_plan.h); on a hit at p it takes
//                     every posting p' = p, p + 1, ... with list[p'] == t: the score grows by sat32(ow[e] * payload[p'])
//                     (topk_sat_add) and the match count by one.  No early exit: every list is looked at.  The score is
//                     written back in place; the ballot bit is "matches >= msm[j]".
//                     A tile inside one query walks the query's lists as a workgroup: two threads take the lower bound of
//                     the tile's first candidate and the upper bound of its last, the only ids [lo, hi) the tile can
//                     meet -- a candidate's whole run of equal ids lies inside it.  An empty range skips the list; one
//                     of at most ANSX_BOOL_STAGE ints goes to LDS and is searched there ("staged", and the default
//                     rule); a longer one is searched in global memory inside [lo, hi) ("search": always).  The
//                     payloads are read from global memory at the postings that hit.
//                     A tile that spans queries -- many small ones -- has no barrier: per candidate its query, then the
//                     whole-list lower bound over each of its lists.
//                     Ends as k_bool_exclude does; with a device total, a tile at or beyond it leaves as a whole
//                     workgroup with zero ballot words and a zero count.
//   k_dr_scan<u64, false>, k_isect_compact (ids, then scores), k_isectb_bounds   as they are.
// A query without a required term (kind O) runs as one of ansx_topk_batch_dev up to k_topk_scores; where a query of the
// group has a threshold of 2 or more:
//   k_topkq_atleast   per head h of query j: the entries equal to it = end - idx[h], end the next head's position or the
//                     end of the query's span (k_union_counts' formula); the ballot bit is "entries >= msm[j]".
// and the same scan, compaction (heads, then scores) and bounds.  Either way the exclusion step (ansx_bool.h),
// k_topkb_check and the select follow as in ansx_topk_bool.h.
// No workgroup waits for another.  Every thread returns at once when the scan's flag word names a list.
//
// Memory safety for ANY content of the containers and payloads.  Every at / n comes from the host's plan (isb_plan: at + n
// inside the buffer of ids it laid out from the checked headers; the buffer of payloads has the same layout and size, so
// a payload is read at an index an id of the same list is read at; ot_off ascends to the entries of ot, and ow has an
// entry per entry of ot), seg from k_isectb_bounds (0 <= seg[j] <= seg[j + 1] <= n), msm has Q entries, the total is
// clamped to n.  bx_lower and bx_upper return a value in [lo, hi] of their arguments and read list[mid] with
// lo <= mid < hi only; the range of a list is clamped to lo <= hi <= L.n whatever the candidates' order.  The staged
// part is hi - lo <= ANSX_BOOL_STAGE ints read from [lo, hi); the search in LDS and the walk over equal ids stay below
// that length, and the payload of staged posting p is read at lo + p < hi.  The walk in global memory stops at hi
// (bounded) or L.n (whole list).  Payload VALUES are only multiplied and added, ids only compared; the match count
// saturates.  Every loop halves an interval, counts to a table bound or walks to the end of a range.  Writes: score i
// of the thread's own candidate i < min(total, n), word i / 64 of the ballots for i < n, and the tile's own count.
// k_topkq_atleast reads heads below min(*total, n), idx[h + 1] only where h + 1 is a head of the same query below the
// total, and bounds at j <= Q; its writes are the ballots' and the count.
#pragma once

#include "ansx_topk_bool.h"

#define ANSX_TOPKQ_FORM_DEFAULT 0u
#define ANSX_TOPKQ_FORM_SEARCH 1u  // never stages
#define ANSX_TOPKQ_FORM_STAGED 2u  // stages whenever the range fits (today the default rule)

// The postings p, p + 1, ... < end of `list` equal to t: their saturated products with w into sc, their number into
// cnt.  pv: the list's payloads, or null (every payload is 1).  base: where list[0] stands in pv.
template <class P> ANSX_D void topkq_take(P list, const u32* __restrict__ pv, u64 base, u64 p, u64 end, u32 t, u32 w, u32& sc, u32& cnt)
{
    for (; p < end && list[p] == t; p++) {
        sc = topk_sat_add(sc, pv ? topk_sat32(w, pv[base + p]) : w);
        cnt += cnt != 0xFFFFFFFFu;
    }
}

// cand[0, n): the candidates, those of query j in [seg[j], seg[j + 1]), score[i] beside them; total: null, or the
// device's count of them (clamped to n).  The grid covers n > 0.  pay: the group's payloads, laid out as ids (null:
// every payload is 1); ow: the weight of every entry of ot; msm: every query's threshold.  form: ANSX_TOPKQ_FORM_*.
// (total: no caller gives one today -- should_step runs in front of the exclusion step, behind a round whose count the host
// has seen -- so the path "a tile at or beyond the total" is k_bool_exclude's code, unreached and untested here)
// (amdgpu_waves_per_eu: without it the compiler takes 65 VGPRs, one over what 8 waves a SIMD allow -- the stage's 16 KiB
// leave a CU its 8 workgroups; with it 54, no scratch, no spill, and the kernel 7 to 10 % faster: DESIGN.md section 3p)
__global__ __launch_bounds__(ANSX_ISECT_NT) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_topkq_should(
    const u32* __restrict__ ids, const u32* __restrict__ pay,
    const u32* __restrict__ cand, u32* __restrict__ score, u32 n, const u64* __restrict__ total, const u32* __restrict__ seg, u32 Q,
    const u32* __restrict__ ot_off, const ansx_isb_list* __restrict__ ot, const u32* __restrict__ ow, const u32* __restrict__ msm,
    u32 form, u64* __restrict__ ballots, u64* __restrict__ counts, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;  // (the scan is through: every thread may read it itself)
    __shared__ u32 stage[ANSX_BOOL_STAGE];
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    __shared__ u32 qb[2];
    __shared__ u64 rng[2][2];
    const u32 tid = threadIdx.x;
    const u32 nc = total ? (total[0] < n ? (u32)total[0] : n) : n;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (i0 >= nc) {  // (the whole workgroup; i0 < n: the grid)
        if (tid < ANSX_ISECT_WORDS && i0 + 64ull * tid < n) ballots[(i0 >> 6) + tid] = 0ull;
        if (tid == 0) counts[blockIdx.x] = 0ull;
        return;
    }
    const u64 last = (i0 + ANSX_ISECT_TILE < nc ? i0 + ANSX_ISECT_TILE : nc) - 1;
    if (tid == 0) {  // the queries of the tile's first and last candidate
        qb[0] = isb_query_of(seg, 0, Q - 1, (u32)i0);
        qb[1] = isb_query_of(seg, qb[0], Q - 1, (u32)last);
    }
    __syncthreads();
    const u32 q0 = qb[0], q1 = qb[1];
    u32 t[ANSX_ISECT_CPT], sc[ANSX_ISECT_CPT], cnt[ANSX_ISECT_CPT];
    bool live[ANSX_ISECT_CPT], pass[ANSX_ISECT_CPT];
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = i0 + k * ANSX_ISECT_NT + tid;
        live[k] = i < nc;
        t[k] = live[k] ? cand[i] : 0u;
        sc[k] = live[k] ? score[i] : 0u;
        cnt[k] = 0u, pass[k] = false;
    }
    if (q0 == q1) {  // inside one query: its lists one after the other, as a workgroup
        const u32 tf = cand[i0], tl = cand[last];
        const u32 e0 = ot_off[q0], e1 = ot_off[q0 + 1];
        for (u32 e = e0; e < e1; e++) {
            const ansx_isb_list L = ot[e];
            const u32* __restrict__ list = ids + L.at;
            const u32* __restrict__ pv = pay ? pay + L.at : nullptr;
            const u32 w = ow[e];
            u64* r = rng[(e - e0) & 1u];  // (two pairs in turn: a pair is written again two barriers after its readers)
            if (tid == 0) r[0] = bx_lower(list, 0, L.n, tf);
            if (tid == 64) r[1] = bx_upper(list, 0, L.n, tl);
            __syncthreads();  // (and every search in `stage` for the list before is through)
            const u64 lo = r[0];
            u64 hi = r[1];
            hi = hi < lo ? lo : hi;  // (lo <= L.n and hi <= L.n: bx_lower, bx_upper)
            if (lo == hi) continue;
            const u64 len = hi - lo;
            if (form != ANSX_TOPKQ_FORM_SEARCH && len <= ANSX_BOOL_STAGE) {
                const u32 ms = (u32)len;
                for (u32 j = tid; j < ms; j += ANSX_ISECT_NT) stage[j] = list[lo + j];
                __syncthreads();
#pragma unroll
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
                    if (live[k]) {
                        const u64 p = bx_lower((const u32*)stage, 0, ms, t[k]);
                        topkq_take((const u32*)stage, pv, lo, p, ms, t[k], w, sc[k], cnt[k]);
                    }
            } else {
#pragma unroll
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
                    if (live[k]) {
                        const u64 p = bx_lower(list, lo, hi, t[k]);
                        topkq_take(list, pv, 0, p, hi, t[k], w, sc[k], cnt[k]);
                    }
            }
        }
        const u32 m = msm[q0];
#pragma unroll
        for (u32 k = 0; k < ANSX_ISECT_CPT; k++) pass[k] = live[k] && cnt[k] >= m;
    } else {  // spanning queries: no barrier
#pragma unroll
        for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
            if (live[k]) {
                const u32 q = isb_query_of(seg, q0, q1, (u32)(i0 + k * ANSX_ISECT_NT + tid));
                const u32 e1 = ot_off[q + 1];
                for (u32 e = ot_off[q]; e < e1; e++) {
                    const ansx_isb_list L = ot[e];
                    const u32* __restrict__ list = ids + L.at;
                    const u64 p = bx_lower(list, 0, L.n, t[k]);
                    topkq_take(list, pay ? pay + L.at : nullptr, 0, p, L.n, t[k], ow[e], sc[k], cnt[k]);
                }
                pass[k] = cnt[k] >= msm[q];
            }
    }
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = i0 + k * ANSX_ISECT_NT + tid;
        if (live[k]) score[i] = sc[k];
        isect_ballot(pass[k], i - (tid & 63u), n, k * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    isect_tile_count(wcnt, counts);
}

// A workgroup per ANSX_ISECT_TILE heads h < min(*total, n), as k_union_counts: idx[h] its position in the merged buffer,
// hseg the queries' bounds among the heads, seg those of the merged buffer.  The ballot bit of head h of query j:
// end - idx[h] >= msm[j].  The grid covers n > 0; a tile at or beyond the total leaves zero ballot words and a zero count.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topkq_atleast(const u32* __restrict__ idx, const u32* __restrict__ hseg,
    const u32* __restrict__ seg, u32 Q, const u64* __restrict__ total, u32 n, const u32* __restrict__ msm, u64* __restrict__ ballots,
    u64* __restrict__ counts, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 tot = total[0] < n ? total[0] : n;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (i0 >= tot) {  // (the whole workgroup; i0 < n: the grid)
        if (tid < ANSX_ISECT_WORDS && i0 + 64ull * tid < n) ballots[(i0 >> 6) + tid] = 0ull;
        if (tid == 0) counts[blockIdx.x] = 0ull;
        return;
    }
    if (tid == 0) {
        const u64 last = (i0 + ANSX_ISECT_TILE < tot ? i0 + ANSX_ISECT_TILE : tot) - 1;
        qb[0] = isb_query_of(hseg, 0, Q - 1, (u32)i0);
        qb[1] = isb_query_of(hseg, qb[0], Q - 1, (u32)last);
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 h = i0 + k * ANSX_ISECT_NT + tid;
        bool keep = false;
        if (h < tot) {
            const u32 j = isb_query_of(hseg, qb[0], qb[1], (u32)h);
            const u32 end = h + 1 < hseg[j + 1] && h + 1 < tot ? idx[h + 1] : seg[j + 1];
            keep = end - idx[h] >= msm[j];
        }
        isect_ballot(keep, h - (tid & 63u), n, k * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    isect_tile_count(wcnt, counts);
}
