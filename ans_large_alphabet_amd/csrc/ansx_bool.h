// Exclusion behind a batch of queries (ansx_bool_batch_dev): which candidates of every query occur in none of the
// query's excluded lists; DESIGN.md section 3l.  gfx950 only.
//
// The positive phase -- ansx_intersect_batch_dev's rounds or ansx_union_batch_dev's merge and unique step -- leaves the
// candidates of a group's Q queries back to back, query j's in [seg[j], seg[j + 1]), ascending inside a query, and every
// decoded list is ascending too.  ONE step then serves all queries and all their excluded lists:
//   k_bool_exclude   k_isectb_match's launch shape.  Candidate i of query j is KEPT when it is a member of none of
//                    xt[xt_off[j] .. xt_off[j + 1]) (the host's table, ansx_plan.h); member = found && id at the lower
//                    bound == candidate, never a comparison with ANSX_NO_ID.
//                    A tile inside one query (the queries of its first and last candidate are equal) walks the query's
//                    lists as a workgroup: two threads take the lower bound of the tile's first candidate and the upper
//                    bound of its last, the only ids [lo, hi) of the list the tile can meet.  An empty range skips the
//                    list; one of at most ANSX_BOOL_STAGE ints goes to LDS, lanes on consecutive dwords, and every
//                    thread takes the lower bound of its still-kept candidates there; a longer one is searched in
//                    global memory, inside [lo, hi) only.
//                    A tile that spans queries -- many small ones -- has no barrier: per candidate its query
//                    (isb_query_of), then k_isectb_match's whole-list lower bound over each of its lists, up to the
//                    first hit.
//                    Ends as k_isectb_match does: isect_ballot, isect_tile_count, the bit "kept".
//   k_dr_scan<u64, false>, k_isect_compact, k_isectb_bounds   as they are: the kept -> the other buffer, the next seg.
// Behind a union the candidates' count is on the device (the unique step's total): n is then the host's bound, the grid
// covers it, and a tile at or beyond the total leaves as a whole workgroup with zero ballot words and a zero count, so
// that the scan, the compaction and the bounds behind it read defined words.
// No workgroup waits for another.  Every thread returns at once when the scan's flag word names a list.
//
// Memory safety for ANY content of the containers.  Every at / n comes from the host's plan (at + n inside the buffer
// it laid out from the checked headers; xt_off ascends to the entries of xt), seg from the host's table or
// k_isectb_bounds (0 <= seg[j] <= seg[j + 1] <= n), the total is clamped to n.  bx_lower and bx_upper return a value
// in [lo, hi] of their arguments and read list[mid] with lo <= mid < hi only; the range of a list is clamped to
// lo <= hi <= L.n whatever the candidates' order: unsorted candidates -- which cannot occur with a clear flag word --
// may be judged against the wrong part of the list but read nothing outside it.  The staged part is hi - lo <=
// ANSX_BOOL_STAGE ints read from [lo, hi), and the search in LDS stays below that length.  Every loop halves an
// interval or counts to a table bound.  Writes: word i / 64 of the ballots for i < n, and the tile's own count.
#pragma once

#include "ansx_intersect_batch.h"

// The ints of a list a tile stages in LDS: 4096, 16 KiB a workgroup, which leaves a CU its 8 workgroups.  8192 (5
// workgroups) was slower on every shape that moved, 5.5 against 3.1 ms on 521 M candidates, and staging whenever the
// range fits -- the default rule, and "staged" -- was never slower than searching; DESIGN.md section 3l.
#ifndef ANSX_BOOL_STAGE
#define ANSX_BOOL_STAGE 4096u
#endif

#define ANSX_BOOL_FORM_DEFAULT 0u
#define ANSX_BOOL_FORM_SEARCH 1u  // never stages
#define ANSX_BOOL_FORM_STAGED 2u  // stages whenever the range fits

// (bx_lower, bx_upper: ansx_query_tile.h)

// cand[0, n): the candidates, those of query j in [seg[j], seg[j + 1]); total: null, or the device's count of them
// (clamped to n).  The grid covers n > 0.  form: ANSX_BOOL_FORM_*.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_bool_exclude(const u32* __restrict__ ids, const u32* __restrict__ cand, u32 n,
    const u64* __restrict__ total, const u32* __restrict__ seg, u32 Q, const u32* __restrict__ xt_off,
    const ansx_isb_list* __restrict__ xt, u32 form, u64* __restrict__ ballots, u64* __restrict__ counts,
    const u32* __restrict__ sflag)
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
    u32 t[ANSX_ISECT_CPT];
    bool keep[ANSX_ISECT_CPT];
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = i0 + k * ANSX_ISECT_NT + tid;
        keep[k] = i < nc;
        t[k] = keep[k] ? cand[i] : 0u;
    }
    if (q0 == q1) {  // inside one query: its lists one after the other, as a workgroup
        const u32 tf = cand[i0], tl = cand[last];
        const u32 e0 = xt_off[q0], e1 = xt_off[q0 + 1];
        for (u32 e = e0; e < e1; e++) {
            const ansx_isb_list L = xt[e];
            const u32* __restrict__ list = ids + L.at;
            u64* r = rng[(e - e0) & 1u];  // (two pairs in turn: a pair is written again two barriers after its readers)
            if (tid == 0) r[0] = bx_lower(list, 0, L.n, tf);
            if (tid == 64) r[1] = bx_upper(list, 0, L.n, tl);
            __syncthreads();  // (and every search in `stage` for the list before is through)
            const u64 lo = r[0];
            u64 hi = r[1];
            hi = hi < lo ? lo : hi;  // (lo <= L.n and hi <= L.n: bx_lower, bx_upper)
            if (lo == hi) continue;
            const u64 len = hi - lo;
            if (form != ANSX_BOOL_FORM_SEARCH && len <= ANSX_BOOL_STAGE) {
                const u32 m = (u32)len;
                for (u32 j = tid; j < m; j += ANSX_ISECT_NT) stage[j] = list[lo + j];
                __syncthreads();
#pragma unroll
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
                    if (keep[k]) {
                        const u32 p = (u32)bx_lower((const u32*)stage, 0, m, t[k]);
                        if (p < m && stage[p] == t[k]) keep[k] = false;
                    }
            } else {
#pragma unroll
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
                    if (keep[k]) {
                        const u64 p = bx_lower(list, lo, hi, t[k]);
                        if (p < hi && list[p] == t[k]) keep[k] = false;
                    }
            }
        }
    } else {  // spanning queries: no barrier
#pragma unroll
        for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
            if (keep[k]) {
                const u32 q = isb_query_of(seg, q0, q1, (u32)(i0 + k * ANSX_ISECT_NT + tid));
                const u32 e1 = xt_off[q + 1];
                for (u32 e = xt_off[q]; e < e1; e++) {
                    const ansx_isb_list L = xt[e];
                    const u32* __restrict__ list = ids + L.at;
                    const u64 p = bx_lower(list, 0, L.n, t[k]);
                    if (p < L.n && list[p] == t[k]) {
                        keep[k] = false;
                        break;
                    }
                }
            }
    }
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = i0 + k * ANSX_ISECT_NT + tid;
        isect_ballot(keep[k], i - (tid & 63u), n, k * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    isect_tile_count(wcnt, counts);
}
