// The frame of the query kernels (ansx_intersect.h .. ansx_topk_query.h): a workgroup of ANSX_ISECT_NT threads over a
// tile of ANSX_ISECT_TILE elements that lie back to back, query j's in [seg[j], seg[j + 1]); DESIGN.md section 3o-2.
// Two parts.  The arithmetic is ANSX_PLAN_FN, as in ansx_plan_types.h: the kernels inline it and the host compiler
// alone builds it, so tests/tools/query_tile_check.cpp runs, under the sanitizers, the code the kernels run.  The
// device pieces (ANSX_D) add the thread that does it and the barrier, and are there for the kernels only.
// On it today: k_isectb_gather, k_isectb_match, k_union_heads, k_topk_hist, k_topk_gather, k_facet_count, k_filter_mark
// (and k_topkb_check's limit).
// The other kernels of the same shape still write their frame out, and every kernel its ballot (isect_ballot): DESIGN.md
// section 3o-2 says which pieces changed their code generation and are therefore not here.
//
// What every piece assumes about seg: Q + 1 entries for Q >= 1 queries, seg[0] == 0, ascending, seg[Q] >= the limit n
// the piece is given.  The host's tables and k_isectb_bounds give that (ansx_intersect_batch.h).  With ANY content of
// seg the searches still read entries [lo, hi] of their arguments only and return a value inside them.
#pragma once

#include "ansx_plan_types.h"

#define ANSX_ISECT_NT 256u
#define ANSX_ISECT_CPT 4u                                   // elements per thread
#define ANSX_ISECT_TILE (ANSX_ISECT_NT * ANSX_ISECT_CPT)    // ... per workgroup: 16 ballot words
#define ANSX_ISECT_WORDS (ANSX_ISECT_TILE / 64u)

// ---- the arithmetic ----------------------------------------------------------------------------------------------

// The last j in [lo, hi] with key(j) <= i, lo where there is none.  Reads key(mid) for lo < mid <= hi only.  (The
// accessor form of isb_query_of below, for k_isectb_gather, whose bounds are G[].dst: seg is that kernel's output.)
template <class K, class I> ANSX_PLAN_FN u32 qt_last_le(K key, u32 lo, u32 hi, I i)
{
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (key(mid) <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The query of element i: the last j in [lo, hi] with seg[j] <= i (seg[lo] <= i), so an empty query -- a run of equal
// entries -- is never found for an i below seg[Q].  Narrowed to the queries of two elements around i it gives what the
// whole [0, Q - 1] gives.
ANSX_PLAN_FN u32 isb_query_of(const u32* __restrict__ seg, u32 lo, u32 hi, u32 i)
{
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (seg[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the first j in [lo, hi) with list[j] >= t, hi where there is none.  Reads list[mid] with lo <= mid < hi only.
template <class P> ANSX_PLAN_FN u64 bx_lower(P list, u64 lo, u64 hi, u32 t)
{
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (list[mid] >= t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the first j in [lo, hi) with list[j] > t, hi where there is none.  Reads as bx_lower.
template <class P> ANSX_PLAN_FN u64 bx_upper(P list, u64 lo, u64 hi, u32 t)
{
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (list[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The elements a launch looks at: the device's count of them clamped to the host's bound n; qt_limit where a caller
// may give no count (null): n then.
ANSX_PLAN_FN u64 qt_clamp(u64 total, u32 n) { return total < n ? total : n; }
ANSX_PLAN_FN u64 qt_limit(const u64* total, u32 n) { return total ? qt_clamp(total[0], n) : n; }

// A tile starts at element i0 = tile * ANSX_ISECT_TILE.  Thread tid's k-th element, k < ANSX_ISECT_CPT:
ANSX_PLAN_FN u64 qt_elem(u64 i0, u32 k, u32 tid) { return i0 + k * ANSX_ISECT_NT + tid; }
// ... the last element of the tile below n (i0 < n)
ANSX_PLAN_FN u64 qt_tile_last(u64 i0, u32 n) { return (i0 + ANSX_ISECT_TILE < n ? i0 + ANSX_ISECT_TILE : n) - 1; }
// ... the queries of its first and last element (i0 < n).  Over seg the comparison is 32 bits wide: the search is
// scalar code there, and a 64-bit comparison takes it through the vector unit at every step.
ANSX_PLAN_FN void qt_tile_queries(const u32* __restrict__ seg, u32 Q, u64 i0, u32 n, u32* qb)
{
    qb[0] = isb_query_of(seg, 0, Q - 1, (u32)i0);
    qb[1] = isb_query_of(seg, qb[0], Q - 1, (u32)qt_tile_last(i0, n));
}
template <class K> ANSX_PLAN_FN void qt_tile_queries_by(K key, u32 Q, u64 i0, u32 n, u32* qb)
{
    qb[0] = qt_last_le(key, 0, Q - 1, i0);
    qb[1] = qt_last_le(key, qb[0], Q - 1, qt_tile_last(i0, n));
}

// ---- the facet step (ansx_facet.h, k_facet_count) ----------------------------------------
// The tiles of `tot` elements, and the chunk of them that workgroup wg of `grid` walks in the persistent form: tiles
// [t[0], t[1]), contiguous, the chunks of wg = 0 .. grid - 1 back to back from 0 to ntiles, their lengths at most one
// apart; grid > ntiles leaves some of them empty.  (ntiles * grid stays far below 2^64: ntiles <= 2^22, grid a u32.)
ANSX_PLAN_FN u64 facet_tiles(u64 tot) { return (tot + ANSX_ISECT_TILE - 1u) / ANSX_ISECT_TILE; }
ANSX_PLAN_FN void facet_chunk(u64 ntiles, u32 grid, u32 wg, u64* t)
{
    t[0] = ntiles * wg / grid, t[1] = ntiles * ((u64)wg + 1u) / grid;
}
// Is this id looked up (in 64 bits: ndocs == 2^32 admits 0xFFFFFFFF); is this value counted; query j's row of counts
ANSX_PLAN_FN bool facet_lookup(u32 id, u64 ndocs) { return (u64)id < ndocs; }
ANSX_PLAN_FN bool facet_counted(u32 v, u32 nvalues) { return v < nvalues; }
ANSX_PLAN_FN u64 facet_row(u32 j, u32 nvalues) { return (u64)j * nvalues; }

// ---- the filter step (ansx_filter.h, k_filter_mark) --------------------------------------
// Is this id looked up (in 64 bits, as facet_lookup); does value v pass the clause [lo, hi] with `flags` -- lo > hi is the
// empty range, which with ANSX_FILTER_NOT (bit 0) admits everything; no value is special
ANSX_PLAN_FN bool filter_lookup(u32 id, u64 ndocs) { return (u64)id < ndocs; }
ANSX_PLAN_FN bool filter_pass(u32 v, u32 lo, u32 hi, u32 flags) { return (lo <= v && v <= hi) != ((flags & 1u) != 0); }
// The fused form: is lane's candidate alive in the ballot word the step in front wrote; the word that goes back -- the
// AND of that word and the filter's verdicts, which is what the ballot of "alive and passes" gives
ANSX_PLAN_FN bool filter_prior_bit(u64 word, u32 lane) { return ((word >> lane) & 1u) != 0; }
ANSX_PLAN_FN u64 filter_and(u64 prior, u64 verdict) { return prior & verdict; }
// the tile's count: the popcounts of its ANSX_ISECT_WORDS ballot words, one per word in wcnt
ANSX_PLAN_FN u32 filter_tile_count(const u32* wcnt)
{
    u32 a = 0;
    for (u32 k = 0; k < ANSX_ISECT_WORDS; k++) a += wcnt[k];
    return a;
}

// ---- the device pieces -------------------------------------------------------------------------------------------
#ifdef ANSX_D

// The prologue: thread 0 writes the queries of the tile's first and last element below n to qb[0 .. 1] (LDS), a
// barrier follows, and element i of the tile then searches isb_query_of(seg, qb[0], qb[1], i): no step while the tile
// lies inside one query.  Every thread of the workgroup calls it, with i0 < n (the caller's grid, or its exit for a
// tile at or beyond the limit).  qt_prologue_by: the same over any key, and a tile at or beyond n leaves qb unwritten.
ANSX_D void qt_prologue(const u32* __restrict__ seg, u32 Q, u64 i0, u32 n, u32* qb)
{
    if (threadIdx.x == 0) qt_tile_queries(seg, Q, i0, n, qb);
    __syncthreads();
}
template <class K> ANSX_D void qt_prologue_by(K key, u32 Q, u64 i0, u32 n, u32* qb)
{
    if (threadIdx.x == 0 && i0 < n) qt_tile_queries_by(key, Q, i0, n, qb);
    __syncthreads();
}

#endif  // ANSX_D
