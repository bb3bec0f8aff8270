// Facet counts of ranked queries (ansx_topk_facets_batch_dev): how the ids of every query's result set R(q) fall over one
// column of values, a uint32 per document id; DESIGN.md section 3r.  gfx950 only.
//
// A group runs as one of ansx_topk_scored_batch_dev (ansx_topk_scored.h) with ONE launch more, behind the last step that
// filters the candidates (k_topkq_atleast, k_topkq_should, the exclusion step) and in front of the select:
//   k_facet_count   over the candidates h < min(*total, n) of the group, distinct ids that ascend inside a query, query
//                   j's in [hseg[j], hseg[j + 1]) -- the frame of ansx_query_tile.h: tiles of ANSX_ISECT_TILE candidates,
//                   the queries of a tile's ends by qt_prologue, the query of an element by isb_query_of.  Per candidate
//                   (facet_lookup, facet_counted, facet_row, ansx_query_tile.h): an id below ndocs loads values[id], and a
//                   value below nvalues adds one to counts[j * nvalues + value]; a value of nvalues or more is counted
//                   nowhere.  An id of ndocs or more: nothing is read at it, and the bad-id word is lowered to its query
//                   (atomicMin), which the group's last wait brings home beside the overflow word.
//                   Two forms.  "atomic" (LDS false): a tile per workgroup, one global atomicAdd per counted candidate.
//                   "lds" (LDS true; nvalues <= ANSX_FACET_LDS_VALUES): the grid is at most what the chip holds at the
//                   kernel's occupancy, and workgroup w walks the CONTIGUOUS tiles facet_chunk gives it, computed here
//                   from the clamped total.  While the tiles lie inside one query the counts are kept in nvalues words of
//                   LDS; they are flushed -- one global atomicAdd per bin that is not zero -- and cleared when the query
//                   changes and at the chunk's end.  A tile whose ends belong to different queries flushes what is held,
//                   and its own candidates go through global atomics: they write the rows of several queries.  One long
//                   query so costs at most grid x nvalues global atomics, not one per candidate.  COMBINE: a wave whose
//                   counted candidates all have one value adds their number once, as k_topk_hist does for a shared digit
//                   (64 atomics on one word of LDS serialise).
// No workgroup waits for another, and no loop spins: every loop counts tiles, bins or elements, or halves an interval.
// The kernel returns at once when the scan's flag word names a list.
//
// Memory safety for ANY content of the containers and the column.  n is the host's bound of the candidates and lies
// inside the buffers of ids; the device's total is clamped to it (qt_clamp), so every h read is below n.  hseg has
// Q + 1 entries; the searches read entries [0, Q - 1] and [qb[0], qb[1]] of it and return a query j inside them whatever
// it holds, so j < Q and a row of counts is one of the group's Q rows (the host passes the address of the group's first
// row).  An id is compared with ndocs, in 64 bits, BEFORE values[id] is read.  A value is compared with nvalues BEFORE it
// indexes a row or the LDS, which holds nvalues words; the flush walks bins below nvalues.  The chunk of a workgroup lies
// inside [0, tiles of the clamped total), so the first element of each of its tiles is below the total, as qt_prologue
// asks.  The writes: atomic adds into the group's rows at a value below nvalues, the atomic minimum of the bad-id word,
// the workgroup's own LDS.
#pragma once

#include "ansx_topk.h"

#define ANSX_FACET_FORM_DEFAULT 0u  // (lds where it applies: DESIGN.md section 3r)
#define ANSX_FACET_FORM_ATOMIC 1u
#define ANSX_FACET_FORM_LDS 2u
#define ANSX_FACET_LDS_VALUES 4096u  // the most values the lds form counts: 16 KiB of dynamic LDS

// One candidate of query j: -> whether it is counted, its value to *v; a bad id lowers badw
ANSX_D bool facet_candidate(u32 id, u32 j, const u32* __restrict__ values, u64 ndocs, u32 nvalues, u32* __restrict__ badw, u32* v)
{
    if (!facet_lookup(id, ndocs)) {
        atomicMin(badw, j);
        return false;
    }
    *v = values[id];
    return facet_counted(*v, nvalues);
}

// ids / hseg / total / n: the candidates (above).  counts: the row of the group's first query.  The grid: the tiles of
// n ("atomic"), or any number of workgroups ("lds", with nvalues words of dynamic LDS).
template <bool LDS, bool COMBINE>
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_facet_count(const u32* __restrict__ ids, const u32* __restrict__ hseg, u32 Q,
    const u64* __restrict__ total, u32 n, const u32* __restrict__ values, u64 ndocs, u32 nvalues, u32* __restrict__ counts,
    u32* __restrict__ badw, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    extern __shared__ u32 facet_bins[];
    __shared__ u32 qb[2][2];  // (two sets: a workgroup of the lds form writes the next tile's while the last one's are read)
    const u32 tid = threadIdx.x;
    const u64 tot = qt_clamp(total[0], n);
    if (!LDS) {
        const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
        if (i0 >= tot) return;  // (the whole workgroup)
        qt_prologue(hseg, Q, i0, (u32)tot, qb[0]);
        const u32 q0 = qb[0][0], q1 = qb[0][1];
#pragma unroll
        for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
            const u64 h = qt_elem(i0, k, tid);
            if (h >= tot) continue;
            const u32 j = isb_query_of(hseg, q0, q1, (u32)h);
            u32 v;
            if (facet_candidate(ids[h], j, values, ndocs, nvalues, badw, &v)) atomicAdd(&counts[facet_row(j, nvalues) + v], 1u);
        }
        return;
    }
    u64 chunk[2];
    facet_chunk(facet_tiles(tot), gridDim.x, blockIdx.x, chunk);
    if (chunk[0] >= chunk[1]) return;  // (the whole workgroup: more workgroups than tiles)
    for (u32 i = tid; i < nvalues; i += ANSX_ISECT_NT) facet_bins[i] = 0;  // (in front of the first prologue's barrier)
    u32 held = ANSX_TOPK_NONE;  // the query whose counts the LDS holds (the workgroup's)
    // what is held -> its row, and the bins cleared; every thread its own bins, and a barrier behind them
    auto flush = [&]() {
        for (u32 i = tid; i < nvalues; i += ANSX_ISECT_NT) {
            const u32 cnt = facet_bins[i];
            if (cnt) atomicAdd(&counts[facet_row(held, nvalues) + i], cnt), facet_bins[i] = 0;
        }
        held = ANSX_TOPK_NONE;
        __syncthreads();
    };
    for (u64 t = chunk[0]; t < chunk[1]; t++) {
        const u64 i0 = t * ANSX_ISECT_TILE;
        u32* const b = qb[t & 1u];
        qt_prologue(hseg, Q, i0, (u32)tot, b);  // (its barrier: the last tile's adds to the LDS are through)
        const u32 q0 = b[0], q1 = b[1];
        const bool one = q0 == q1;  // (the workgroup's)
        if (held != ANSX_TOPK_NONE && (!one || held != q0)) flush();
        if (one) held = q0;
#pragma unroll
        for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
            const u64 h = qt_elem(i0, k, tid);
            const bool in = h < tot;
            u32 v = 0;
            if (one) {
                const bool cnt = in && facet_candidate(ids[h], q0, values, ndocs, nvalues, badw, &v);
                if (COMBINE) {  // (every lane gets here)
                    const u64 m = __ballot(cnt);
                    if (m == 0) continue;  // (the wave's)
                    const u32 first = (u32)__ffsll((unsigned long long)m) - 1u;
                    const u32 v0 = __shfl(v, first, 64);
                    if (__ballot(cnt && v == v0) == m) {
                        if ((tid & 63u) == first) atomicAdd(&facet_bins[v0], (u32)__popcll(m));
                        continue;
                    }
                }
                if (cnt) atomicAdd(&facet_bins[v], 1u);
            } else if (in) {
                const u32 j = isb_query_of(hseg, q0, q1, (u32)h);
                if (facet_candidate(ids[h], j, values, ndocs, nvalues, badw, &v)) atomicAdd(&counts[facet_row(j, nvalues) + v], 1u);
            }
        }
    }
    __syncthreads();
    if (held != ANSX_TOPK_NONE) flush();
}
