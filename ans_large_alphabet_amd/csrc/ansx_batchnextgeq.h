// Search by value over a batch of gap-coded lists (ansx_next_geq_batch_dev); DESIGN.md section 3h.  gfx950 only.
//
// Two kernels around the passes of ansx_decode_batch_ranges_sums_dev with one range of one int per found target:
//   k_ngb_locate   target i of list C[rid[i]] -> blk[i], the smallest block b of that list with bases[b + 1] >= t
//                  (bases[b + 1] is the last id of block b), or ANSX_NGB_NONE for t > bases[nblocks]; for those it also
//                  writes the answer, n of the list and ANSX_NO_ID.  A plain binary search in global memory: the lists
//                  of a batch are mostly a few blocks long.
//   (the host reads blk back, checks every value and plans the passes over the found targets; per pass the decode of the
//   touched blocks and the scan of ansx_batchrangesums.h, unchanged)
//   k_ngb_search   in the place of k_piece_gather, a lane per piece of the pass: the lower bound of t over the scanned
//                  ids of the piece's block, clamped to the block's own length.
//
// Memory safety for ANY content of the bases is that of ansx_nextgeq.h.  k_ngb_locate reads a list's bases only at
// indices it derives from nblocks -- the bounds of its interval, never a value it has read -- so every read is inside
// bases[1 .. nblocks] of a REFERENCED container and every loop halves an interval of indices; the upper end of the
// interval stays on an entry read as >= t.  The host accepts b < nblocks only.  k_ngb_search reads the work list inside
// the block the host's plan placed there (kk[i] < T is checked) and writes entry P[i].dst < ntargets of the outputs only.
#pragma once

#include "ansx_batchranges.h"
#include "ansx_batchrangesums.h"

#define ANSX_NGB_NT 256u
#define ANSX_NGB_NONE 0xFFFFFFFFu  // blk[i]: the target lies beyond its list's last id

struct ansx_ngb_list {  // a referenced list: its bases, its ids and its blocks
    u64 bases;          // device address of nblocks + 1 entries
    u64 n;
    u32 nblocks;        // >= 1
    u32 pad_;
};

__global__ __launch_bounds__(ANSX_NGB_NT) void k_ngb_locate(const ansx_ngb_list* __restrict__ C, const u32* __restrict__ rid,
    const u32* __restrict__ targets, u32 nt, u32* __restrict__ blk, u64* __restrict__ pos, u32* __restrict__ ids)
{
    const u64 i = (u64)blockIdx.x * ANSX_NGB_NT + threadIdx.x;
    if (i >= nt) return;
    const ansx_ngb_list L = C[rid[i]];
    const u32* __restrict__ bases = (const u32*)(uintptr_t)L.bases;
    const u32 t = targets[i];
    if (bases[L.nblocks] < t) {
        blk[i] = ANSX_NGB_NONE;
        if (pos) pos[i] = L.n;
        if (ids) ids[i] = 0xFFFFFFFFu /* ANSX_NO_ID */;
        return;
    }
    u32 lo = 0, hi = L.nblocks - 1u;  // bases[hi + 1] has been read as >= t, here and after every step
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (bases[mid + 1] >= t) hi = mid;
        else lo = mid + 1;
    }
    blk[i] = hi;
}

// Piece i of the pass (np of them): target P[i].dst, whose block is block kk[i] of the pass -- O[kk[i]] in the scanned
// work list, block B[kk[i]].b of its list.  pos = b * bi + the lower bound of t in the block's ids, and the id there.
// Nothing is written when the decode, the scan (gflags) or the index of a touched block (dflags) reported an error.
// pos or ids may be null.
__global__ __launch_bounds__(ANSX_NGB_NT) void k_ngb_search(const u32* __restrict__ list, const ansx_blk_out* __restrict__ O,
    const ansx_batch_blk* __restrict__ B, u32 T, u64 bi, const ansx_piece* __restrict__ P, const u32* __restrict__ kk, u32 np,
    const u32* __restrict__ targets, u64* __restrict__ pos, u32* __restrict__ ids, const u32* __restrict__ gflags,
    const u32* __restrict__ dflags)
{
    if (gflags[ANSX_G_ERR] | dflags[0]) return;  // (nobody sets them any more: every thread may read them itself)
    const u64 i = (u64)blockIdx.x * ANSX_NGB_NT + threadIdx.x;
    if (i >= np) return;
    const u32 k = kk[i];
    if (k >= T) return;
    const ansx_blk_out o = O[k];
    if (!o.n) return;
    const u64 dst = P[i].dst;
    const u32 t = targets[dst];
    const u32* blk = list + o.off;
    u32 lo = 0, hi = o.n;  // the first j with blk[j] >= t; blk[o.n - 1] = bases[b + 1] >= t behind a clean scan
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (blk[mid] >= t) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= o.n) lo = o.n - 1u;
    if (pos) pos[dst] = (u64)B[k].b * bi + lo;
    if (ids) ids[dst] = blk[lo];
}
