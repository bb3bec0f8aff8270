// ansx_batchranges.h -- ranges of a batch of containers in one call (ansx_decode_batch_ranges_dev, DESIGN.md
// section 3d).
//
// The host groups the referenced containers by geometry and cuts every group's touched (container, block) pairs, sorted
// and unique, into passes; a pass is a sub-container built and decoded exactly as a pass of ansx_decode_batch_dev
// (ansx_batch.h).  What differs is the way out of the pass's work list: the ranges of a query are mostly short -- point
// lookups are one int each -- and k_range_gather's workgroup per piece would spend a launch-sized grid on four bytes a
// workgroup.  k_piece_gather divides the pass's piece STREAM, the pieces laid end to end, into chunks of
// ANSX_PIECE_CHUNK ints, so its grid follows the ints asked for and never the piece count.
#pragma once

#include "ansx_ranges.h"

// (ansx_piece, ANSX_PIECE_CHUNK: ansx_plan_types.h)

// d[0..m) = s[0..m), m <= ANSX_PIECE_CHUNK, by the 256 threads of the workgroup: the body of k_range_gather's loop --
// 16-byte accesses where source and destination agree modulo 16 bytes, dwords otherwise.
__device__ __forceinline__ void piece_copy_chunk(u32* __restrict__ d, const u32* __restrict__ s, u32 m, u32 tid)
{
    u32 head = (u32)(((16 - ((uintptr_t)d & 15)) & 15) >> 2);
    if (head > m) head = m;
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
        if (tid < head) d[tid] = s[tid];
        const u32 nq = (m - head) >> 2;
        const uint4* s16 = (const uint4*)(s + head);
        uint4* d16 = (uint4*)(d + head);
        if (nq) {  // every load before the first store; a lane past the end loads the last 16 bytes again and stores nothing
            const u32 j0 = tid, j1 = tid + 256u, j2 = tid + 512u, j3 = tid + 768u, last = nq - 1;
            const uint4 v0 = s16[j0 < last ? j0 : last], v1 = s16[j1 < last ? j1 : last], v2 = s16[j2 < last ? j2 : last],
                        v3 = s16[j3 < last ? j3 : last];
            if (j0 < nq) d16[j0] = v0;
            if (j1 < nq) d16[j1] = v1;
            if (j2 < nq) d16[j2] = v2;
            if (j3 < nq) d16[j3] = v3;
        }
        const u32 done = head + 4 * nq;
        if (done + tid < m) d[done + tid] = s[done + tid];
    } else {
        u32 v[16];
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (tid + 256u * q < m) v[q] = s[tid + 256u * q];
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (tid + 256u * q < m) d[tid + 256u * q] = v[q];
    }
}

// The last i in [lo, hi) with a[i] <= v (a ascending, a[lo] <= v)
template <class T, class V> __device__ __forceinline__ u32 piece_find(const T* __restrict__ a, u32 lo, u32 hi, V v)
{
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// out[P[i].dst + j] = sub[P[i].src + j] for every piece i of the pass (np of them, wpos[np] = total ints), nothing if
// the decode flagged an error.  Workgroup w takes ints [w * CHUNK, (w + 1) * CHUNK) of the piece stream (grid-stride
// beyond the grid's cap).  Its first and last piece are found once, by one lane each.  A chunk inside one piece is
// copied as k_range_gather copies its chunks.  A chunk of several pieces (at most CHUNK of them: no piece is empty)
// brings their starts, relative to the chunk, into LDS; lane t then takes ints t, t + 256, ... of the chunk and finds
// the piece of each by a binary search over those starts -- neighbouring lanes hold neighbouring ints, so wherever the
// pieces are longer than a few ints the loads and stores of a wave coalesce as they would in a plain copy.
__global__ __launch_bounds__(256) void k_piece_gather(const u32* __restrict__ sub, const ansx_piece* __restrict__ P,
    const u64* __restrict__ wpos, u32 np, u64 total, u32* __restrict__ out, const u32* __restrict__ gflags)
{
    __shared__ u32 rel[ANSX_PIECE_CHUNK + 1];  // rel[i]: first int of piece p0 + i in the chunk (0 for the piece the chunk starts in)
    __shared__ u32 ends[2];
    const u32 tid = threadIdx.x;
    if (gflags[ANSX_G_ERR]) return;  // the decode of the sub-container failed: the caller's buffer is not written
    const u64 nchunks = (total + ANSX_PIECE_CHUNK - 1) / ANSX_PIECE_CHUNK;
    for (u64 w = blockIdx.x; w < nchunks; w += gridDim.x) {
        const u64 c0 = w * ANSX_PIECE_CHUNK;
        const u32 m = (u32)(total - c0 < ANSX_PIECE_CHUNK ? total - c0 : ANSX_PIECE_CHUNK);
        if (tid == 0) ends[0] = piece_find(wpos, 0u, np, c0);
        if (tid == 64) ends[1] = piece_find(wpos, 0u, np, c0 + m - 1);
        __syncthreads();
        const u32 p0 = ends[0], p1 = ends[1];
        if (p0 == p1) {
            const ansx_piece r = P[p0];
            const u64 off = c0 - wpos[p0];
            piece_copy_chunk(out + r.dst + off, sub + r.src + off, m, tid);
        } else {
            const u32 k = p1 - p0 + 1;  // (<= m: every piece of the chunk but the first starts at an int of its own)
            for (u32 i = tid; i < k; i += 256) rel[i] = i ? (u32)(wpos[p0 + i] - c0) : 0u;
            const u64 into0 = c0 - wpos[p0];  // the chunk starts this far into its first piece
            __syncthreads();
#pragma unroll 4
            for (u32 j = tid; j < m; j += 256) {
                const u32 i = piece_find(rel, 0u, k, j);
                const ansx_piece r = P[p0 + i];
                const u64 off = i ? (u64)(j - rel[i]) : into0 + j;
                out[r.dst + off] = sub[r.src + off];
            }
        }
        __syncthreads();  // (ends and rel are rewritten by the next chunk)
    }
}
