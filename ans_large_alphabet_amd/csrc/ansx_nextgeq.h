// Search by value (ansx_next_geq_dev): the first id >= t of a gap-coded list, the block bases as its skip table;
// DESIGN.md section 3g.  gfx950 only.
//
// Two kernels around the sums range call (ansx_decode_device_ranges_sums_dev) with one range of one int per target:
//   k_ng_locate   target t -> the smallest block b with bases[b + 1] >= t (bases[b + 1] is the last id of block b), written
//                 as the range first = b * bi, count = 1; count = 0 for t > bases[nblocks], which touches no block.
//   (the device planner over first / count, the decode of the touched blocks, range_sums_scan: unchanged.  With counts of
//   0 and 1 the planner's offsets[i] is the index of target i's piece in R, R[offsets[i]].src where its block starts in
//   the work list, and the planner's total the number of targets found.)
//   k_ng_search   in the place of k_range_gather: the lower bound of t over the block's scanned ids in the work list.
//
// Memory safety for ANY content of bases.  k_ng_locate reads bases only at indices it derives from nblocks -- bounds of
// its search intervals, never a value it has read -- so every read is inside bases[1 .. nblocks], and every loop halves
// an interval of indices.  Its b is below nblocks, so the range is one the planner accepts.  k_ng_search reads the work
// list inside the block the planner placed there and writes entry i of the outputs only.
//
// Why the search finds an element.  k_ng_locate keeps, through both levels, the upper end of its interval on an entry
// it has READ as >= t: the b it returns satisfies bases[b + 1] >= t on the value read, whatever the other entries hold.
// k_ng_search runs only behind a clean flag word, and then range_sums_scan has tied bases[b + 1] to the block:
// bases[b] + (the block's sum in 64 bits) = bases[b + 1], so the block's ids do not wrap, are non-decreasing and end on
// bases[b + 1] >= t.  The lower bound therefore lies inside the block and k_ng_search needs no error path.  (Its index
// is clamped to the block all the same: a caller who changes the bases during the call, against the contract, gets a
// wrong answer and no access out of bounds.)  What is NOT checked: entries of bases at untouched blocks.  A wrong one
// there can send a target to a block that is not its own, and the answer is then the lower bound inside that block.
#pragma once

#include "ansx_rangesums.h"

#define ANSX_NG_NT 256u
#define ANSX_NG_TPT 8u                                  // targets per thread of k_ng_locate
#define ANSX_NG_TILE (ANSX_NG_NT * ANSX_NG_TPT)         // ... per workgroup
// Staged entries of bases per workgroup of k_ng_locate: 16 KiB of the CU's 160 KiB, so the LDS admits ten workgroups
// where the wave slots admit eight -- the staging costs no occupancy.  The 4096 blocks of the 64 Mi list of DESIGN.md 3f
// are staged whole; 16384 blocks are sampled at every 4th entry and leave two levels to global memory.
#define ANSX_NG_LDS 4096u

// The entries e[b] = bases[b + 1], b in [0, nb), are searched in two levels: smp[k] = the last entry of group k of
// `stride` consecutive ones (stride 1: every entry) in LDS, staged once per workgroup with independent loads; then the
// group itself in global memory, ceil(log2 stride) dependent loads.  ng_stage and ng_find_block are the two levels,
// shared with k_isect_match_full (ansx_intersect.h), so that the argument at the head of the file is made once.
// smp[ANSX_NG_LDS] <- the samples; *stride, *m: the group length and count (nb >= 1; m <= ANSX_NG_LDS).  Ends in a barrier.
__device__ __forceinline__ void ng_stage(const u32* __restrict__ bases, u32 nb, u32* smp, u32 tid, u32* stride, u32* m)
{
    const u32 st = (nb + ANSX_NG_LDS - 1) / ANSX_NG_LDS, mm = (nb + st - 1) / st;
    for (u32 k = tid; k < mm; k += ANSX_NG_NT) {
        const u64 e = ((u64)k + 1) * st;
        smp[k] = bases[e < nb ? e : nb];  // (the last group may be short: it ends on bases[nb])
    }
    __syncthreads();
    *stride = st, *m = mm;
}

// The smallest block b with bases[b + 1] >= t, for t <= smp[m - 1] = bases[nb]
__device__ __forceinline__ u32 ng_find_block(const u32* smp, u32 m, u32 stride, const u32* __restrict__ bases, u32 nb, u32 t)
{
    u32 lo = 0, hi = m - 1;  // smp[hi] >= t, here and after every step
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (smp[mid] >= t) hi = mid;
        else lo = mid + 1;
    }
    const u64 gend = ((u64)hi + 1) * stride;
    u32 glo = hi * stride, ghi = (u32)(gend < nb ? gend : nb) - 1u;  // bases[ghi + 1] is smp[hi]: read as >= t
    while (glo < ghi) {
        const u32 mid = (glo + ghi) >> 1;
        if (bases[mid + 1] >= t) ghi = mid;
        else glo = mid + 1;
    }
    return ghi;
}

// Per target the block that holds its answer, as a range for the device planner.  first[i] / count[i]: the workspace
// the planner reads.
__global__ __launch_bounds__(ANSX_NG_NT) void k_ng_locate(const u32* __restrict__ bases, u32 nb, u64 bi,
    const u32* __restrict__ targets, u32 nt, u64* __restrict__ first, u32* __restrict__ count)
{
    __shared__ u32 smp[ANSX_NG_LDS];
    const u32 tid = threadIdx.x;
    u32 stride, m;
    ng_stage(bases, nb, smp, tid, &stride, &m);
    const u32 last = smp[m - 1];  // bases[nb], the last id of the list
#pragma unroll
    for (u32 q = 0; q < ANSX_NG_TPT; q++) {  // (coalesced: target q * 256 + tid of the tile)
        const u64 i = (u64)blockIdx.x * ANSX_NG_TILE + q * ANSX_NG_NT + tid;
        if (i >= nt) continue;
        const u32 t = targets[i];
        if (t > last) {
            first[i] = 0, count[i] = 0;
            continue;
        }
        first[i] = (u64)ng_find_block(smp, m, stride, bases, nb, t) * bi, count[i] = 1;
    }
}

// A lane per target.  Found (count 1): its piece R[offsets[i]] starts at its block in the work list, block k = src / bi of
// the list, len ints of ids (short for the source's last block); pos = first[i] + the lower bound of t in them.  Not
// found: n and ANSX_NO_ID.  Nothing is written when the decode, the scan (gflags) or the index of a touched block
// (dflags) reported an error.  pos or ids may be null.
__global__ __launch_bounds__(ANSX_NG_NT) void k_ng_search(const u32* __restrict__ list, u64 n_sub, u64 bi, u64 n,
    const u32* __restrict__ targets, u32 nt, const u64* __restrict__ first, const u32* __restrict__ count,
    const u64* __restrict__ offsets, const ansx_range_piece* __restrict__ R, u64* __restrict__ pos, u32* __restrict__ ids,
    const u32* __restrict__ gflags, const u32* __restrict__ dflags)
{
    if (gflags[ANSX_G_ERR] | dflags[0]) return;  // (nobody sets them any more: every thread may read them itself)
    const u64 i = (u64)blockIdx.x * ANSX_NG_NT + threadIdx.x;
    if (i >= nt) return;
    u64 p = n;
    u32 id = 0xFFFFFFFFu /* ANSX_NO_ID */;
    if (count[i]) {
        const u32 t = targets[i];
        const u64 src = R[offsets[i]].src, left = n_sub - src;  // (src = k * bi: a block start of the work list)
        const u32 len = (u32)(left < bi ? left : bi);
        const u32* blk = list + src;
        u32 lo = 0, hi = len;  // the first j with blk[j] >= t; blk[len - 1] >= t (see the head of the file)
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (blk[mid] >= t) hi = mid;
            else lo = mid + 1;
        }
        if (lo >= len) lo = len - 1u;
        p = first[i] + lo, id = blk[lo];
    }
    if (pos) pos[i] = p;
    if (ids) ids[i] = id;
}

// No target found (the planner's total is 0 and no tail runs): n and ANSX_NO_ID everywhere
__global__ __launch_bounds__(ANSX_NG_NT) void k_ng_none(u64 n, u32 nt, u64* __restrict__ pos, u32* __restrict__ ids)
{
    const u64 i = (u64)blockIdx.x * ANSX_NG_NT + threadIdx.x;
    if (i >= nt) return;
    if (pos) pos[i] = n;
    if (ids) ids[i] = 0xFFFFFFFFu /* ANSX_NO_ID */;
}
