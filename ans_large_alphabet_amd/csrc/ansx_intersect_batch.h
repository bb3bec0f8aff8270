// Intersection of many queries in one call (ansx_intersect_batch_dev): the steps of ansx_intersect.h over the survivors
// of ALL queries of a group at once; DESIGN.md section 3j.  gfx950 only.
//
// A group's referenced lists are decoded back to back into one buffer and scanned into ids (the pass decoder, the
// segmented scan of ansx_sums.h).  The candidates of its Q queries lie back to back too, query j's in
// [seg[j], seg[j + 1]) -- seg has Q + 1 entries, ascending from 0 to the candidates' count nc, and an empty segment is
// a run of equal entries.  The query of candidate i is the LAST j with seg[j] <= i, so an empty segment is never found.
//   k_isectb_gather  every query's driver ids -> the first candidates, and the first seg (a list may drive many queries).
//   k_isectb_match   a round: candidate i of query j is looked up in the list the round table names for (j, round) --
//                    rt[rt_off[j] + round] while that lies below rt_off[j + 1], else the query has no list in this round
//                    and its candidates pass through -- by a lower bound over the whole list:
//                    member = found && id at the lower bound == candidate, never a comparison with ANSX_NO_ID.  Ends as
//                    k_isect_match does: isect_ballot, isect_tile_count.
//   k_dr_scan<u64, false>, k_isect_compact   as they are (ansx_intersect.h): the members -> the other candidate buffer.
//   k_isectb_bounds  a lane per entry of seg: the members in front of candidate seg[j] = its tile's offset + the
//                    popcounts of the tile's earlier ballot words + the bits of its own word below it -> the next seg.
// No workgroup waits for another.
//
// Memory safety for ANY content of the containers.  Every index comes from the host: the tables (ansx_plan.h,
// isb_plan: src + count and at + n lie inside the buffer it laid out from the checked headers; rt_off ascends to the
// entries of rt) and seg, whose first form is the table's dst and whose later forms k_isectb_bounds derives from
// counts of ballot bits, so 0 <= seg[j] <= seg[j + 1] <= nc always: what the frame's pieces (ansx_query_tile.h) assume,
// and their contracts are not repeated here.  k_isectb_gather writes candidate i < nc and entry i <= Q of seg, and
// nothing when the scan's flag word names a list.  k_isectb_match reads candidate i < nc and ids [at, at + n) only
// (bx_lower), and writes through isect_ballot and isect_tile_count.
// k_isectb_bounds reads ballot words of tiles that hold a candidate below nc and writes entry j <= Q.  The host
// enqueues no round before the decode's and the scan's flag words have come back clean.
#pragma once

#include "ansx_intersect.h"

// A workgroup per ANSX_ISECT_TILE indices i: candidate i < nc is id (i - dst) of its query's driver, the query the last
// j with G[j].dst <= i (G[Q].dst == nc): the frame's search with G[].dst as its key, seg being this kernel's output;
// entry i <= Q of seg is G[i].dst.  The grid covers max(nc, Q + 1): a tile at or beyond nc writes entries of seg only.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_isectb_gather(const u32* __restrict__ ids,
    const ansx_isb_query* __restrict__ G, u32 Q, u32* __restrict__ cand, u32 nc, u32* __restrict__ seg,
    const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;  // (the scan is through: every thread may read it itself)
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    const auto dst = [G](u32 j) { return G[j].dst; };
    qt_prologue_by(dst, Q, i0, nc, qb);
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = qt_elem(i0, k, tid);
        if (i <= Q) seg[i] = (u32)G[i].dst;
        if (i >= nc) continue;
        const u32 q = qt_last_le(dst, qb[0], qb[1], i);
        cand[i] = ids[G[q].src + (i - G[q].dst)];
    }
}

// Round `round` (0: every query's first list behind its driver) over the nc > 0 candidates.  k_isect_match's launch shape.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_isectb_match(const u32* __restrict__ ids, const u32* __restrict__ cand,
    u32 nc, const u32* __restrict__ seg, u32 Q, const u32* __restrict__ rt_off, const ansx_isb_list* __restrict__ rt,
    u32 round, u64* __restrict__ ballots, u64* __restrict__ counts)
{
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    qt_prologue(seg, Q, i0, nc, qb);  // (the grid: i0 < nc)
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = qt_elem(i0, k, tid);
        bool member = false;
        if (i < nc) {
            const u32 q = isb_query_of(seg, qb[0], qb[1], (u32)i);
            const u32 e = rt_off[q] + round;
            member = true;  // no list in this round: passed through
            if (e >= rt_off[q] && e < rt_off[q + 1]) {
                const u32 t = cand[i];
                const ansx_isb_list L = rt[e];
                const u32* list = ids + L.at;
                const u64 p = bx_lower(list, 0, L.n, t);
                member = p < L.n && list[p] == t;
            }
        }
        isect_ballot(member, i - (tid & 63u), nc, k * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    isect_tile_count(wcnt, counts);
}

// A lane per entry j <= Q of seg: the members of the round in front of candidate seg[j] -> next[j]; from seg[j] == nc on
// that is all of them, *total.  toff: the scanned tile counts.
__global__ __launch_bounds__(256) void k_isectb_bounds(const u32* __restrict__ seg, u32 Q, u32 nc,
    const u64* __restrict__ ballots, const u64* __restrict__ toff, const u64* __restrict__ total, u32* __restrict__ next)
{
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j > Q) return;
    const u32 i = seg[j];
    if (i >= nc) {
        next[j] = (u32)total[0];
        return;
    }
    const u32 tile = i / ANSX_ISECT_TILE, w = (i % ANSX_ISECT_TILE) / 64u;
    const u64* wb = ballots + (u64)tile * ANSX_ISECT_WORDS;
    u32 a = (u32)toff[tile];
    for (u32 k = 0; k < w; k++) a += (u32)__popcll(wb[k]);
    next[j] = a + (u32)__popcll(wb[w] & ((1ull << (i & 63u)) - 1ull));
}
