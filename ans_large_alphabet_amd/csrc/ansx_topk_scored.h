// Ranked queries with length-normalised scores (ansx_topk_scored_batch_dev): ansx_topk_query_batch_dev in which the
// contribution of a posting is sat32(weight * table[min(payload, rows - 1)][norm[id]]) -- a quantised BM25 impact -- and
// not weight * payload; DESIGN.md section 3q.  gfx950 only.
//
// A group runs as one of ansx_topk_query_batch_dev (ansx_topk_query.h) with ONE launch more, behind the scan that makes
// the group's ids and in front of the first kernel that reads a payload (k_topk_merge, k_topkb_match, k_topkq_should):
//   k_topk_impacts   rewrites, in place, the payload of every posting of every list of the group that has one into its
//                    impact.  The host's table (impact_plan, ansx_plan.h) names those lists, {at, n, first tile, place
//                    in the group}; a workgroup finds the list of its tile by a wave-uniform binary search over it, as
//                    k_topk_merge finds its pair.  A tile is ROUNDS x 256 uint4 of the two buffers, counted from the
//                    list's start rounded DOWN to four ints (ansx_plan_types.h): a lane loads 16 bytes of ids and 16 of
//                    payloads and stores 16 of impacts wherever its four ints are the list's own, whatever `at` is; the
//                    uint4 at either edge of a list goes int by int, and the ints of a neighbour in it are neither read
//                    nor written.  The norms are a gather of bytes; inside a dense list the ids ascend and a wave's reads
//                    fall into few lines.
//                    Two forms of the table lookup.  "global" (STAGED false) reads the caller's table where it is, one
//                    tile per workgroup.  "staged" (STAGED true) copies the table's first `srows` rows into LDS once per
//                    workgroup -- a tile of 1024 postings would load more table words than it looks up, so the grid is
//                    at most what the chip holds at the kernel's occupancy and a workgroup walks tiles with a grid
//                    stride; a payload that selects a later row reads the caller's table.
//                    An id of ndocs or more: nothing is read at it, its payload stays, and the scan's flag word is
//                    lowered to the list's place in the group (ss_report, as k_sums_apply lowers it for a sum that
//                    leaves 32 bits): every later kernel returns at once, and the wait that brings the flag home names
//                    the list.  The kernel itself does not look at the flag: the ids of a list whose sum left 32 bits
//                    mean nothing, but they are compared like any other before anything is read at them, and the
//                    smallest place wins whichever kernel found it.
// No workgroup waits for another.
//
// Memory safety for ANY content of the containers and payloads.  Every at / n / tile comes from the host's table
// (impact_plan over the group's own layout: at + n inside the buffer of ids, the buffer of payloads of the same layout
// and size); the list of a tile is an entry below np, and a tile at or beyond its list's end does nothing.  Both
// buffers start at a multiple of 16 bytes (the workspace's start and a multiple of four ints behind it), so the uint4
// at a multiple of four ints is aligned; it is loaded or stored whole only where impact_mask says all four ints are the
// list's, else the ints of the mask one by one.  An id is compared with ndocs, in 64 bits, BEFORE norms[id] is read.  The
// table's word is impact_word: the row clamped to rows - 1 whatever the payload, the column a byte, so it lies below
// rows * 256; the staged copy is read only for a word below srows * 256 <= rows * 256, the words that were staged.  The
// only writes are the impacts of the thread's own postings and the flag's atomic minimum.  Every loop counts to a bound
// of the host's (tiles, rows) or halves an interval.
#pragma once

#include "ansx_topk_query.h"

#define ANSX_IMPACT_NT 256u
#define ANSX_IMPACT_FORM_DEFAULT 0u  // (staged: DESIGN.md section 3q)
#define ANSX_IMPACT_FORM_GLOBAL 1u
#define ANSX_IMPACT_FORM_STAGED 2u
#define ANSX_IMPACT_STAGE_ROWS 16u     // S: the rows of the table the staged form keeps in LDS (16 KiB)
#define ANSX_IMPACT_STAGE_MAX 64u      // ... and the most a debug key may ask for (64 KiB: dynamic LDS without an opt-in)
#define ANSX_IMPACT_ROUNDS_DEFAULT 2u  // uint4 per lane and tile: a tile of 2048 postings ("the tile")

// ids / pay: the group's two buffers (16-byte aligned).  P[0 .. np): the host's table, np > 0; ntiles: its tiles.  The
// grid: ntiles ("global") or any number of workgroups up to it ("staged").  stage: srows * 256 words of dynamic LDS
// (STAGED; srows <= rows).
template <u32 ROUNDS, bool STAGED>
__global__ __launch_bounds__(ANSX_IMPACT_NT) void k_topk_impacts(const u32* __restrict__ ids, u32* __restrict__ pay,
    const ansx_impact_list* __restrict__ P, u32 np, u32 ntiles, const u8* __restrict__ norms, u64 ndocs, const u32* __restrict__ table,
    u32 rows, u32 srows, u32* __restrict__ sflag)
{
    extern __shared__ u32 impact_stage[];
    constexpr u32 TILE = ROUNDS * ANSX_IMPACT_NT * 4u;
    const u32 tid = threadIdx.x;
    const u32 swords = STAGED ? srows * ANSX_IMPACT_COLS : 0u;
    if (STAGED) {
        for (u32 i = tid; i < swords; i += ANSX_IMPACT_NT) impact_stage[i] = table[i];
        __syncthreads();
    }
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ansx_impact_list L = P[impact_list_of(P, np, t)];  // (wave-uniform)
        const u64 s0 = impact_tile_start(L, t, TILE);
        if (s0 >= L.at + L.n) continue;  // (not with the host's table)
        u32 id[ROUNDS][4], tf[ROUNDS][4], m[ROUNDS];
#pragma unroll
        for (u32 r = 0; r < ROUNDS; r++) {
            const u64 i = s0 + (u64)(r * ANSX_IMPACT_NT + tid) * 4u;
            m[r] = i < L.at + L.n ? impact_mask(L, i) : 0u;
            if (m[r] == 15u) {
                const uint4 a = *(const uint4*)(ids + i), b = *(const uint4*)(pay + i);
                id[r][0] = a.x, id[r][1] = a.y, id[r][2] = a.z, id[r][3] = a.w;
                tf[r][0] = b.x, tf[r][1] = b.y, tf[r][2] = b.z, tf[r][3] = b.w;
            } else {
#pragma unroll
                for (u32 j = 0; j < 4u; j++) {
                    const bool in = (m[r] >> j) & 1u;
                    id[r][j] = in ? ids[i + j] : 0u, tf[r][j] = in ? pay[i + j] : 0u;
                }
            }
        }
        bool bad = false;
        u32 w[ROUNDS][4];  // the table's word of every posting (the gather of the norms: all of a lane's in flight)
#pragma unroll
        for (u32 r = 0; r < ROUNDS; r++)
#pragma unroll
            for (u32 j = 0; j < 4u; j++) {
                const bool in = (m[r] >> j) & 1u;
                const bool off = in && impact_bad_id(id[r][j], ndocs);
                bad |= off;
                if (off) m[r] &= ~(1u << j);  // (nothing is read at it, and its payload stays)
                w[r][j] = in && !off ? impact_word(tf[r][j], norms[id[r][j]], rows) : 0u;
            }
#pragma unroll
        for (u32 r = 0; r < ROUNDS; r++) {
            const u64 i = s0 + (u64)(r * ANSX_IMPACT_NT + tid) * 4u;
            u32 v[4];
#pragma unroll
            for (u32 j = 0; j < 4u; j++) {
                const bool in = (m[r] >> j) & 1u;
                v[j] = !in ? tf[r][j] : STAGED && w[r][j] < swords ? impact_stage[w[r][j]] : table[w[r][j]];
            }
            if (m[r] == 15u) {
                *(uint4*)(pay + i) = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (u32 j = 0; j < 4u; j++)
                    if ((m[r] >> j) & 1u) pay[i + j] = v[j];
            }
        }
        if (bad) ss_report(sflag, L.pos);  // (ansx_sums.h: the scan's own atomic minimum)
    }
}
