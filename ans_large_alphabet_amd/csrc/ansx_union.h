// Union of many queries in one call (ansx_union_batch_dev): the distinct ids of every query's lists and, per id, how
// often it occurs in them; DESIGN.md section 3k.  gfx950 only.
//
// A group's referenced lists are decoded back to back into one buffer and scanned into ids, as for
// ansx_intersect_batch_dev.  Every list is then a sorted run, and a query of m terms is m runs that the host's pair
// tables (ansx_plan.h, unb_plan) merge pairwise in ceil(log2 m) rounds, all queries of the group in the same launches:
//   k_union_merge   a round: a workgroup per tile of ANSX_UNION_TILE outputs of one pair.  Two merge-path searches in
//                   global memory bound the tile's part of A and of B, which go to LDS; every thread finds its own
//                   diagonal there, merges its ANSX_UNION_CPT outputs and the tile leaves through LDS, lanes on consecutive dwords.
//                   A query's first round reads the buffer of lists, its later ones the other merge buffer.
//   k_union_heads   over the last round's buffer, query j in [seg[j], seg[j + 1]): element p is a head when it is the
//                   first of its query or differs from the one in front.  Ends as k_isectb_match does: isect_ballot,
//                   isect_tile_count.
//   k_dr_scan<u64, false>, k_isect_compact, k_isectb_bounds   as they are: the heads -> the other merge buffer, their
//                   positions (when counts are asked for) and the queries' bounds among them.
//   k_union_counts  per head k of query j: the entries equal to it = the next head's position, or the end of
//                   the query's span, minus its own.
// No workgroup waits for another.  Every kernel returns at once when the scan's flag word names a list (a list whose
// sum left 32 bits is not sorted); k_union_heads then raises the word k_isect_compact takes as its decode flags.
//
// Memory safety for ANY content of the containers.  Every offset and length comes from the host (unb_plan: a + na and
// b + nb lie inside the buffer the sources are read from, dst + na + nb inside the merge buffers, both laid out from the
// checked headers; the tiles of a pair are ceil((na + nb) / TILE)).  k_union_merge clamps the tile's partition to
// i0 <= i1 <= na, j0 <= j1 <= nb, (i1 - i0) + (j1 - j0) = the tile's outputs <= TILE: un_diag returns
// max(0, d - nb) <= i <= min(d, na) whatever it reads, and reads A[mid] with mid < na, B[d - 1 - mid] inside [0, nb).
// The per-thread partition inside LDS is the same function over the staged part, and the serial merge reads a side only
// below its staged length.  Unsorted runs -- which cannot occur with a clear flag word -- may give a wrong order but no
// access outside the runs and the pair's span.  Every loop halves an interval or counts to a constant.
// k_union_heads reads x[p] and x[p - 1] for seg[j] < p < n only; k_union_counts reads heads below the total, which
// k_isect_compact wrote, and the two arrays of bounds at j <= Q.
#pragma once

#include "ansx_intersect_batch.h"

// The outputs of a thread and of a workgroup of k_union_merge: 16 and 4096, which was 3 to 7 % of the call faster than 4
// and 1024 on 4096 queries over lists of 64 Ki ids.  32 KiB of LDS per workgroup.
#ifndef ANSX_UNION_CPT
#define ANSX_UNION_CPT 16u  // (a multiple of 4: a thread's outputs leave as 16-byte stores)
#endif
#define ANSX_UNION_TILE (ANSX_ISECT_NT * ANSX_UNION_CPT)

// How many of the first d outputs of merging A[0, na) and B[0, nb) come from A (ties: A first); d <= na + nb.
ANSX_D u32 un_diag(const u32* A, u32 na, const u32* B, u32 nb, u32 d)
{
    u32 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2u;
        if (A[mid] <= B[d - 1u - mid]) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// A round: P[0 .. np) its pairs (np > 0), the grid its tiles.  lists: the group's ids; prev / next: the merge buffer
// the round reads (not in a query's first round) and the one it writes.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_union_merge(const u32* __restrict__ lists, const u32* __restrict__ prev,
    u32* __restrict__ next, const ansx_unb_pair* __restrict__ P, u32 np, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;  // (the scan is through: every thread may read it itself)
    __shared__ u32 in[ANSX_UNION_TILE];
    __shared__ __align__(16) u32 out[ANSX_UNION_TILE];
    __shared__ u32 part[2];
    const u32 tid = threadIdx.x, t = blockIdx.x;
    u32 lo = 0, hi = np - 1u;  // the last pair with tile <= t (wave-uniform; P[0].tile == 0)
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1u) / 2u;
        if (P[mid].tile <= t) lo = mid;
        else hi = mid - 1u;
    }
    const ansx_unb_pair p = P[lo];
    const u32 na = p.na, nb = p.nb, n = na + nb;  // (below 2^32: the query's ints are)
    const u64 at = (u64)(t - p.tile) * ANSX_UNION_TILE;
    if (at >= n) return;  // (not with the host's table)
    const u32 d0 = (u32)at, nt = n - d0 < ANSX_UNION_TILE ? n - d0 : ANSX_UNION_TILE;
    const u32* A = (p.from_lists ? lists : prev) + p.a;
    const u32* B = (p.from_lists ? lists : prev) + p.b;
    if (tid == 0) part[0] = un_diag(A, na, B, nb, d0);
    if (tid == 64) part[1] = un_diag(A, na, B, nb, d0 + nt);
    __syncthreads();
    const u32 i0 = part[0], j0 = d0 - i0;
    u32 i1 = part[1];
    i1 = i1 < i0 ? i0 : i1;
    i1 = i1 - i0 > nt ? i0 + nt : i1;
    const u32 la = i1 - i0, lb = nt - la;  // (j0 + lb <= nb: see the head)
    for (u32 k = tid; k < nt; k += ANSX_ISECT_NT) in[k] = k < la ? A[i0 + k] : B[j0 + (k - la)];
    __syncthreads();
    const u32 d = ANSX_UNION_CPT * tid;
    if (d < nt) {
        const u32* sb = in + la;
        u32 li = un_diag(in, la, sb, lb, d), lj = d - li;
        u32 av = li < la ? in[li] : 0u, bv = lj < lb ? sb[lj] : 0u;
        u32 o[ANSX_UNION_CPT];
#pragma unroll
        for (u32 q = 0; q < ANSX_UNION_CPT; q++) {  // (behind the tile's end neither side is left: nothing is read)
            const bool ta = li < la && (lj >= lb || av <= bv);
            o[q] = ta ? av : bv;
            if (ta) li++, av = li < la ? in[li] : 0u;
            else lj++, bv = lj < lb ? sb[lj] : 0u;
        }
#pragma unroll
        for (u32 q = 0; q < ANSX_UNION_CPT; q += 4) *(uint4*)&out[d + q] = make_uint4(o[q], o[q + 1], o[q + 2], o[q + 3]);
    }
    __syncthreads();
    u32* dst = next + p.dst + d0;  // (any alignment: a run starts at any int)
    for (u32 k = tid; k < nt; k += ANSX_ISECT_NT) dst[k] = out[k];
}

// A workgroup per ANSX_ISECT_TILE elements of x[0, n), n > 0; seg[0 .. Q] ascends from 0 to n.  The query of element p
// is the last j with seg[j] <= p (an empty one is never found), so the last id of a query is never compared with the
// first of the next.  uflag: raised when the scan's flag word names a list.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_union_heads(const u32* __restrict__ x, u32 n, const u32* __restrict__ seg,
    u32 Q, u64* __restrict__ ballots, u64* __restrict__ counts, const u32* __restrict__ sflag, u32* __restrict__ uflag)
{
    if (sflag[0] != ANSX_SS_NONE) {
        if (blockIdx.x == 0 && threadIdx.x == 0) uflag[0] = 1u;
        return;
    }
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    qt_prologue(seg, Q, i0, n, qb);  // (the grid: i0 < n)
#pragma unroll
    for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
        const u64 i = qt_elem(i0, k, tid);
        bool head = false;
        if (i < n) {
            const u32 q = isb_query_of(seg, qb[0], qb[1], (u32)i);
            head = (u32)i == seg[q] || x[i] != x[i - 1];
        }
        isect_ballot(head, i - (tid & 63u), n, k * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    isect_tile_count(wcnt, counts);
}

// A workgroup per ANSX_ISECT_TILE heads k < min(*total, n): idx[k] its position in the merged buffer, hseg the queries'
// bounds among the heads (k_isectb_bounds), seg those of the merged buffer.  The query is found as in k_union_heads:
// between those of the tile's first and last head, so no step while a tile lies inside one query.  The grid covers n.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_union_counts(const u32* __restrict__ idx, const u32* __restrict__ hseg,
    const u32* __restrict__ seg, u32 Q, const u64* __restrict__ total, u32 n, u32* __restrict__ cnt,
    const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 tot = total[0] < n ? total[0] : n;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (i0 >= tot) return;  // (the whole workgroup)
    if (tid == 0) {
        const u64 last = (i0 + ANSX_ISECT_TILE < tot ? i0 + ANSX_ISECT_TILE : tot) - 1;
        qb[0] = isb_query_of(hseg, 0, Q - 1, (u32)i0);
        qb[1] = isb_query_of(hseg, qb[0], Q - 1, (u32)last);
    }
    __syncthreads();
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u64 k = i0 + q * ANSX_ISECT_NT + tid;
        if (k >= tot) continue;
        const u32 j = isb_query_of(hseg, qb[0], qb[1], (u32)k);
        const u32 end = k + 1 < hseg[j + 1] && k + 1 < tot ? idx[k + 1] : seg[j + 1];
        cnt[k] = end - idx[k];
    }
}
