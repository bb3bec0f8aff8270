// Range filters over document columns (ansx_topk_filter_batch_dev): which ids of every query's result set R(q) pass all
// of the query's clauses, a clause being lo <= column[id] <= hi or its negation over a column of one uint32 per document
// id; DESIGN.md section 3s.  gfx950 only.
//
// A group runs as one of ansx_topk_facets_batch_dev with one step more, behind the last step that filters the candidates
// (k_topkq_atleast, k_topkq_should, the exclusion step) and in front of k_facet_count, k_topkb_check and the select:
//   k_filter_mark   over the candidates h < min(*total, n) of the group, query j's in [hseg[j], hseg[j + 1]) -- the frame of
//                   ansx_query_tile.h: tiles of ANSX_ISECT_TILE candidates, the limit by qt_limit, the queries of a tile's
//                   ends by qt_prologue, the query of an element by isb_query_of.  Query j's clauses are
//                   fc[foff[j] .. foff[j + 1]) of the table the host uploads with the group's other tables, the column's
//                   address in every clause (no table of pointers is indexed).  A query without clauses keeps every
//                   candidate and looks nothing up.  Per candidate that is alive, of a query with a clause: the id is
//                   compared with ndocs in 64 bits (filter_lookup) BEFORE anything is read at it -- an id of ndocs or more
//                   lowers the bad-id word to its query and is dropped (one atomicMin per thread, at the kernel's end: an atomic
//                   in front of the clause loads would keep the compiler from taking them as scalar loads) -- then the clauses in order
//                   (filter_pass), none behind the first that fails.  The ballot bit is "alive and every clause passes".
//                   A tile inside one query, the long-query case: the query's number is made a scalar (readfirstlane), so
//                   its offsets and clauses come through SCALAR loads, once per wave and clause, never per lane.  The
//                   clauses run in the outer loop and the thread's ANSX_ISECT_CPT candidates in the inner one: the four
//                   gathers of a clause are issued together and waited for once.  A wave none of whose candidates is
//                   alive leaves the loop.
//                   A tile that spans queries: per candidate its query, then its clauses, read per lane.
//                   PRIOR (the fused form): the kernel runs between k_bool_exclude and that step's compact step.  Alive
//                   is then the candidate's bit in the ballot word the exclusion wrote (filter_prior_bit); a candidate
//                   whose bit is clear is not looked up and not reported, and the word and the tile's count are written
//                   again (filter_and is what the ballot of "alive and passes" amounts to).  Not PRIOR (the own form):
//                   every candidate below the limit is alive.
//                   Ends as k_topkq_atleast does: isect_ballot per word, the tile's count (filter_tile_count); a tile at
//                   or beyond the limit leaves zero ballot words and a zero count, as a whole workgroup.
//   k_dr_scan<u64, false>, k_isect_compact (ids, then scores), k_isectb_bounds   as they are (compact_step).
// No workgroup waits for another, and no loop spins: every loop counts clauses or elements, or halves an interval.  The
// kernel returns at once when the scan's flag word names a list.
//
// Memory safety for ANY content of the ids, hseg, the columns and the clauses' bounds.  n is the host's bound of the
// candidates and lies inside the buffers of ids; the device's total is clamped to it (qt_limit), so every h read is below
// n, and the ballot word read for it (PRIOR) is word h / 64 < ceil(n / 64), which k_bool_exclude wrote for the same n.
// hseg has Q + 1 entries; the searches read entries [0, Q - 1] and [qb[0], qb[1]] of it and return a query j inside them
// whatever it holds, so j < Q.  foff has Q + 1 entries and comes from the host: ascending from 0 to the entries of fc it
// uploaded, at most ANSX_FILTER_MAX_CLAUSES apart, so [foff[j], foff[j + 1]) lies inside fc for every j < Q.  Every
// clause's column is one the host checked: not null, 4-byte aligned, ndocs entries.  An id is compared with ndocs, in 64
// bits, BEFORE column[id] is read; a value, lo, hi and flags are only compared.  The writes: word h / 64 of the ballots
// for a wave whose first candidate is below n, the tile's own count, the atomic minimum of the bad-id word, the
// workgroup's own LDS.  All of them are vector stores or atomics.
#pragma once

#include "ansx_topk.h"

#define ANSX_FILTER_FORM_DEFAULT 0u  // (fused where the group excludes something: DESIGN.md section 3s)
#define ANSX_FILTER_FORM_OWN 1u
#define ANSX_FILTER_FORM_FUSED 2u

// A clause as the kernel reads it: the host resolves the column.  24 bytes.
struct ansx_filter_dev {
    const u32* col;
    u32 lo, hi, flags, pad;
};

// (a column's address comes out of the table as a generic pointer; it is global memory, and saying so gives global loads)
typedef const __attribute__((address_space(1))) u32* filter_col;

// ids / hseg / total / n: the candidates (above; total may be null: n then).  foff / fc: the group's clause table.  The
// grid covers n > 0.  PRIOR: ballots and counts hold the step's in front, over the same n.
template <bool PRIOR>
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_filter_mark(const u32* __restrict__ ids, const u32* __restrict__ hseg, u32 Q,
    const u64* __restrict__ total, u32 n, const u32* __restrict__ foff, const ansx_filter_dev* __restrict__ fc, u64 ndocs,
    u64* __restrict__ ballots, u64* __restrict__ counts, u32* __restrict__ badw, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 tot = qt_limit(total, n);
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (i0 >= tot) {  // (the whole workgroup; i0 < n: the grid)
        if (tid < ANSX_ISECT_WORDS && i0 + 64ull * tid < n) ballots[(i0 >> 6) + tid] = 0ull;
        if (tid == 0) counts[blockIdx.x] = 0ull;
        return;
    }
    qt_prologue(hseg, Q, i0, (u32)tot, qb);
    const u32 q0 = qb[0], q1 = qb[1];
    u32 id[ANSX_ISECT_CPT];
    bool alive[ANSX_ISECT_CPT];
    u32 badq = ANSX_TOPK_NONE;  // the first query of this thread's with a bad id: one atomic at the end, behind every load
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 h = qt_elem(i0, k, tid);
        alive[k] = h < tot;
        if (PRIOR && alive[k]) alive[k] = filter_prior_bit(ballots[h >> 6], tid & 63u);  // (h < n: the word is there)
        id[k] = h < tot ? ids[h] : 0u;
    }
    if (q0 == q1) {  // inside one query: its clauses are the workgroup's, read through scalar loads
        const u32 j = (u32)__builtin_amdgcn_readfirstlane((int)q0);
        const u32 e0 = foff[j], e1 = foff[j + 1];
        if (e0 < e1) {
#pragma unroll
            for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
                if (alive[k] && !filter_lookup(id[k], ndocs)) badq = j, alive[k] = false;
            for (u32 e = e0; e < e1; e++) {
                bool any = false;
#pragma unroll
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++) any = any || alive[k];
                if (__ballot(any) == 0ull) break;  // (the wave's)
                const ansx_filter_dev c = fc[e];
                const filter_col col = (filter_col)c.col;
                u32 v[ANSX_ISECT_CPT];
#pragma unroll
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++) v[k] = alive[k] ? col[id[k]] : 0u;  // (the four loads, then one wait)
#pragma unroll
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++) alive[k] = alive[k] && filter_pass(v[k], c.lo, c.hi, c.flags);
            }
        }
    } else {  // spanning queries: per candidate its query and its clauses
#pragma unroll
        for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
            if (alive[k]) {
                const u32 j = isb_query_of(hseg, q0, q1, (u32)qt_elem(i0, k, tid));
                const u32 e1 = foff[j + 1];
                u32 e = foff[j];
                if (e < e1 && !filter_lookup(id[k], ndocs)) {
                    badq = badq < j ? badq : j;
                    alive[k] = false;
                    continue;
                }
                for (; e < e1; e++) {
                    const ansx_filter_dev c = fc[e];
                    if (!filter_pass(((filter_col)c.col)[id[k]], c.lo, c.hi, c.flags)) {
                        alive[k] = false;
                        break;
                    }
                }
            }
    }
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 h = qt_elem(i0, k, tid);
        isect_ballot(alive[k], h - (tid & 63u), n, k * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    if (badq != ANSX_TOPK_NONE) atomicMin(badw, badq);
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = filter_tile_count(wcnt);
}
