// ansx_batch.h -- a batch of containers in one call (ansx_decode_batch_dev).
//
// k_batch_headers brings every container's 64-byte header into one array (one read-back for the whole batch).  The
// host checks them, groups the containers by geometry and cuts every group into passes of at most P blocks.  A pass's
// blocks, from as many containers as it spans, become one sub-container laid out as make_plan lays out a container of
// that many blocks (k_batch_index, k_batch_copy: the multi-source form of k_range_index / k_range_copy).  The ordinary
// decode path decodes it with a per-block table (ansx_geo::bout: each block's ints and output offset), so that short
// blocks of many containers sit back to back in the pass's work list; k_range_gather copies every container's ints to
// the caller.
#pragma once

#include "ansx_ranges.h"

// (ansx_batch_src, ansx_batch_blk: ansx_plan_types.h)

// hdr[i] = the 64 bytes at ptrs[i], zeros where ptrs[i] is 0 (an input the host has already found too short); four
// lanes per header, 16 bytes each (every input is 16-byte aligned: checked by the entry point).
__global__ __launch_bounds__(256) void k_batch_headers(const u64* __restrict__ ptrs, u64 count, uint4* __restrict__ hdr)
{
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= 4 * count) return;
    const u64 p = ptrs[t >> 2];
    hdr[t] = p ? ((const uint4*)p)[t & 3] : make_uint4(0u, 0u, 0u, 0u);
}

// Stream length of pass block k, 0 if its index entries are not those of a well-formed container -- checked against
// its own source's block count and payload size (the sub-container's geometry g supplies the rest).
__device__ __forceinline__ u64 batch_block_len(const ansx_geo& g, const ansx_batch_src* __restrict__ S,
    const ansx_batch_blk* __restrict__ B, u32 k, u32* __restrict__ flags)
{
    const ansx_batch_blk e = B[k];
    const ansx_batch_src s = S[e.src];
    ansx_geo gs = g;
    gs.nblocks = s.nblocks;
    gs.payload_bytes = s.payload_bytes;
    return range_block_len(gs, (const u64*)(s.base + 64), e.b, flags);
}

// The sub-container's index and header (one workgroup, as k_range_index)
__global__ __launch_bounds__(1024) void k_batch_index(const ansx_batch_src* __restrict__ S,
    const ansx_batch_blk* __restrict__ B, ansx_geo g, u32 T, ansx_container_header hsub, u8* __restrict__ dst,
    u64 cap_pay, u32* __restrict__ flags)
{
    range_index_body(T, [&](u32 i) { return batch_block_len(g, S, B, i, flags); }, hsub, dst, cap_pay, flags);
}

// One workgroup per pass block: its restart points, parse hints and stream from its source (as k_range_copy)
__global__ __launch_bounds__(256) void k_batch_copy(const ansx_batch_src* __restrict__ S,
    const ansx_batch_blk* __restrict__ B, ansx_geo g, ansx_range_lay dl, u8* __restrict__ dst, u64 cap_pay,
    u32* __restrict__ flags)
{
    const u32 k = blockIdx.x;
    const ansx_batch_blk e = B[k];
    const ansx_batch_src s = S[e.src];
    const ansx_range_lay sl = { s.ckoff_off, s.ckstate_off, s.hint_off, s.payload_off };
    range_copy_block((const u8*)s.base, g, sl, dl, k, e.b, dst, cap_pay, flags);
}
