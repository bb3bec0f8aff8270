// Intersection (ansx_intersect_ids_dev, ansx_intersect_dev): which ids of a candidate array are in a gap-coded list,
// written back to back; DESIGN.md section 3i.  gfx950 only.
//
// A step is a match and a compaction.  The match has two forms with the same outputs:
//   k_isect_match       (selective) the way out of the ansx_next_geq_dev path in k_ng_search's place: k_ng_locate, the
//                       device planner, the decode of the touched blocks and range_sums_scan in front of it, unchanged;
//                       a lane per candidate takes k_ng_search's clamped lower bound in its block of the work list.
//   k_isect_match_full  (full) over the whole list decoded and scanned into workspace: a lane per candidate finds its
//                       block with k_ng_locate's search (ng_stage, ng_find_block), checks the block's two bases against
//                       the ids and takes the lower bound inside the block.
// Both derive member = found && id at the lower bound == candidate -- never a comparison with ANSX_NO_ID -- and store
// one 64-bit ballot word per wave, one member count per tile and, when positions are asked for, pos per member.
//   k_dr_scan<u64, false>  one workgroup: the tile counts -> exclusive offsets, and the total.
//   k_isect_compact     a workgroup per tile: member's slot = its tile's offset + the popcounts of the tile's earlier
//                       ballot words + the set bits of its own word below its lane (mbcnt).
// No workgroup waits for another; nothing is written when a flag word is set or the total exceeds the capacity.
//
// The tile is ANSX_ISECT_TILE = 1024 candidates, four per thread of a 256-thread workgroup: the launch shape of
// k_ng_search, 16 ballot words per tile, so a lane of k_isect_compact adds at most 15 popcounts it reads from LDS, and
// the one-workgroup scan of the tile counts takes one round of ANSX_DR_TILE per 4 Mi candidates.
//
// Memory safety for ANY content of bases and candidates.  k_isect_match reads the work list inside the block the
// planner placed there (as k_ng_search).  k_isect_match_full derives b < nblocks from nblocks only (ng_find_block), so
// [b * bi, min((b + 1) * bi, n)) lies inside the decoded list, and its lower bound is clamped to it.  Both write entry
// i of pos, word i / 64 of the ballots and their own tile's count.  k_isect_compact's slots are below the total of the
// counts the same match wrote, and it writes nothing unless total <= capacity.
#pragma once

#include "ansx_nextgeq.h"
#include "ansx_query_tile.h"  // the tile's size (ANSX_ISECT_NT, _CPT, _TILE, _WORDS) and the frame of the batch kernels

// The ballot of `member` over the wave -> word (i0 / 64) of ballots, i0 the wave's first candidate, when that is one;
// its popcount to wcnt[k], k the word's index in the tile.  Every lane of the wave calls it.
__device__ __forceinline__ void isect_ballot(bool member, u64 i0, u32 nc, u32 k, u64* __restrict__ ballots, u32* wcnt)
{
    const u64 bal = __ballot(member);
    if ((threadIdx.x & 63u) == 0) {
        if (i0 < nc) ballots[i0 >> 6] = bal;
        wcnt[k] = (u32)__popcll(bal);
    }
}

// wcnt[0 .. ANSX_ISECT_WORDS) -> counts[tile]
__device__ __forceinline__ void isect_tile_count(const u32* wcnt, u64* __restrict__ counts)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 a = 0;
#pragma unroll
        for (u32 k = 0; k < ANSX_ISECT_WORDS; k++) a += wcnt[k];
        counts[blockIdx.x] = a;
    }
}

// Selective.  Candidate i found by k_ng_locate (count 1): its piece R[offsets[i]] starts at its block in the work list
// (k_ng_search's words); the lower bound of the candidate in the block, clamped to it.  wpos may be null.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_isect_match(const u32* __restrict__ list, u64 n_sub, u64 bi,
    const u32* __restrict__ cand, u32 nc, const u64* __restrict__ first, const u32* __restrict__ count,
    const u64* __restrict__ offsets, const ansx_range_piece* __restrict__ R, u64* __restrict__ ballots,
    u64* __restrict__ counts, u64* __restrict__ wpos, const u32* __restrict__ gflags, const u32* __restrict__ dflags)
{
    if (gflags[ANSX_G_ERR] | dflags[0]) return;  // (nobody sets them any more: every thread may read them itself)
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    const u32 tid = threadIdx.x;
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u64 i = (u64)blockIdx.x * ANSX_ISECT_TILE + q * ANSX_ISECT_NT + tid;
        bool member = false;
        if (i < nc && count[i]) {
            const u32 t = cand[i];
            const u64 src = R[offsets[i]].src, left = n_sub - src;  // (src = k * bi: a block start of the work list)
            const u32 len = (u32)(left < bi ? left : bi);
            const u32* blk = list + src;
            u32 lo = 0, hi = len;  // the first j with blk[j] >= t; blk[len - 1] >= t (see the head of ansx_nextgeq.h)
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (blk[mid] >= t) hi = mid;
                else lo = mid + 1;
            }
            if (lo >= len) lo = len - 1u;
            member = blk[lo] == t;
            if (member && wpos) wpos[i] = first[i] + lo;
        }
        isect_ballot(member, i - (tid & 63u), nc, q * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    isect_tile_count(wcnt, counts);
}

// Full.  ids: the n ids of the whole list, blocks of bi; bases[nb + 1] the caller's.  sflag: the flag word of the scan
// that made the ids (ANSX_SS_NONE, or the list's sum left 32 bits: ANSX_ERR_DOMAIN into gflags, nothing else is done).
// A candidate's block whose bases are not the ids in front of it and at its end sets the format bit.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_isect_match_full(const u32* __restrict__ ids, u64 n, u64 bi,
    const u32* __restrict__ bases, u32 nb, const u32* __restrict__ cand, u32 nc, u64* __restrict__ ballots,
    u64* __restrict__ counts, u64* __restrict__ wpos, u32* __restrict__ gflags, const u32* __restrict__ sflag)
{
    __shared__ u32 smp[ANSX_NG_LDS];
    __shared__ u32 wcnt[ANSX_ISECT_WORDS];
    __shared__ u32 sh_err;
    const u32 tid = threadIdx.x;
    if (tid == 0) {  // (this kernel sets the format bit itself: one read per workgroup, so that all of it leaves or stays)
        const u32 dom = sflag[0] != ANSX_SS_NONE ? 1u << 6 /* ANSX_ERR_DOMAIN */ : 0u;
        if (dom && blockIdx.x == 0) atomicOr(&gflags[ANSX_G_ERR], dom);
        sh_err = dom | __hip_atomic_load(&gflags[ANSX_G_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    u32 stride, m;
    ng_stage(bases, nb, smp, tid, &stride, &m);  // (ends in a barrier)
    if (sh_err) return;
    const u32 last = smp[m - 1];  // bases[nb]
    bool bad = false;
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u64 i = (u64)blockIdx.x * ANSX_ISECT_TILE + q * ANSX_ISECT_NT + tid;
        bool member = false;
        const u32 t = i < nc ? cand[i] : 0u;
        if (i < nc && t <= last) {
            const u32 b = ng_find_block(smp, m, stride, bases, nb, t);
            const u64 s0 = (u64)b * bi, e0 = s0 + bi < n ? s0 + bi : n;
            if (s0 >= n || (b == 0 ? bases[0] != 0u : ids[s0 - 1] != bases[b]) || ids[e0 - 1] != bases[b + 1]) bad = true;
            else {
                const u32* blk = ids + s0;
                const u32 len = (u32)(e0 - s0);
                u32 lo = 0, hi = len;  // the first j with blk[j] >= t; blk[len - 1] = bases[b + 1], read as >= t
                while (lo < hi) {
                    const u32 mid = (lo + hi) >> 1;
                    if (blk[mid] >= t) hi = mid;
                    else lo = mid + 1;
                }
                if (lo >= len) lo = len - 1u;
                member = blk[lo] == t;
                if (member && wpos) wpos[i] = s0 + lo;
            }
        }
        isect_ballot(member, i - (tid & 63u), nc, q * (ANSX_ISECT_NT / 64u) + (tid >> 6), ballots, wcnt);
    }
    if (bad) rs_flag_format(gflags);
    isect_tile_count(wcnt, counts);
}

// A workgroup per tile, toff the scanned tile counts, *total their sum.  Member i goes to slot toff[tile] + the members
// of the tile in front of it; every output that is given is written.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_isect_compact(const u32* __restrict__ cand, u32 nc,
    const u64* __restrict__ ballots, const u64* __restrict__ toff, const u64* __restrict__ total, u64 cap,
    const u64* __restrict__ wpos, u32* __restrict__ out_ids, u32* __restrict__ out_idx, u64* __restrict__ out_pos,
    const u32* __restrict__ gflags, const u32* __restrict__ dflags)
{
    if (gflags[ANSX_G_ERR] | dflags[0]) return;  // (nobody sets them any more: every thread may read them itself)
    if (total[0] > cap) return;
    __shared__ u64 wb[ANSX_ISECT_WORDS];
    const u32 tid = threadIdx.x;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (tid < ANSX_ISECT_WORDS) wb[tid] = i0 + 64ull * tid < nc ? ballots[(i0 >> 6) + tid] : 0ull;
    __syncthreads();
    const u64 base = toff[blockIdx.x];
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u32 k = q * (ANSX_ISECT_NT / 64u) + (tid >> 6);
        u32 pre = 0;
        for (u32 j = 0; j < k; j++) pre += (u32)__popcll(wb[j]);  // (k is the wave's: no divergence)
        const u64 own = wb[k];
        if (!((own >> (tid & 63u)) & 1ull)) continue;
        const u32 below = __builtin_amdgcn_mbcnt_hi((u32)(own >> 32), __builtin_amdgcn_mbcnt_lo((u32)own, 0u));
        const u64 i = i0 + q * ANSX_ISECT_NT + tid, slot = base + pre + below;
        if (out_ids) out_ids[slot] = cand[i];
        if (out_idx) out_idx[slot] = (u32)i;
        if (out_pos) out_pos[slot] = wpos[i];
    }
}
