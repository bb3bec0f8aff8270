// Docids of ranges of a batch (ansx_decode_batch_ranges_sums_dev), the scan ansx_next_geq_batch_dev shares with it, and
// the bases of a batch from the writer (ansx_encode_batch_gaps_bases_dev); DESIGN.md section 3h.  gfx950 only.
//
// Input.  The work list of a pass (pass_build in ansx.hip): block k of the pass is the ints [O[k].off, O[k].off + O[k].n)
// of `list`, block B[k].b of source B[k].src; SB[B[k].src] holds that source's bases and its block count.  O[k].off is a
// multiple of 4 and the list 16-byte aligned, so every block starts on a 16-byte boundary; ANY block may be short (it
// may be its container's last), and up to 3 padding ints lie between the runs of two containers.  Output: the list in
// place, list[O[k].off + j] = bases[b] + x[0] + ... + x[j] modulo 2^32 with bases the block's own source's.  Of a
// source's bases only entries b and b + 1 of the pass's blocks are read, and bases[b] + (the block's sum in 64 bits)
// must be bases[b + 1]: else the format bit of the decode's flag word, as in ansx_rangesums.h.  Nothing but the blocks'
// own ints is read or written: no padding int, nothing behind the pass's last block.
//
// The bodies are those of ansx_rangesums.h (rs_wave_block, rs_wg_block, rs_carry_block, rs_apply_chunk) and so are the
// three shapes, chosen by the block size bi of the pass's geometry (batch_sums_scan in ansx.hip):
//   bi <= ANSX_RS_CHUNK      k_brs_scan_small: a wave per block, four blocks per workgroup, no LDS and no barrier.
//   bi <= ANSX_RS_WG_MAX     k_brs_scan_block: a workgroup per block.
//   larger                   k_brs_reduce, k_brs_carry, k_brs_apply: tpb = ceil(bi / ANSX_RS_TILE) tiles per block,
//                            whatever its own length (a chunk behind a short block's end is empty).
// Every grid is T / 4, T or T * tpb workgroups, T the pass's blocks; no workgroup waits for another.
#pragma once

#include "ansx_batch.h"
#include "ansx_rangesums.h"

// (ansx_brs_src: ansx_plan_types.h)

// (seed, end) of block k of the pass: entries b and b + 1 of its source's bases; a block number outside the source (no
// plan names one) fails the check without a read
ANSX_D bool brs_bases_of(const ansx_batch_blk* __restrict__ B, const ansx_brs_src* __restrict__ SB, u32 k, u32* seed, u32* end)
{
    const ansx_batch_blk bk = B[k];
    const ansx_brs_src sb = SB[bk.src];
    if (bk.b >= sb.nblocks) {
        *seed = 0, *end = 0;
        return false;
    }
    const u32* bases = (const u32*)(uintptr_t)sb.bases;
    *seed = bases[bk.b], *end = bases[bk.b + 1];
    return true;
}

// bi <= ANSX_RS_CHUNK: wave w of workgroup g scans block 4 g + w of the pass
__global__ __launch_bounds__(ANSX_RS_NT) void k_brs_scan_small(u32* __restrict__ list, const ansx_blk_out* __restrict__ O,
    const ansx_batch_blk* __restrict__ B, const ansx_brs_src* __restrict__ SB, u32 T, u32* __restrict__ gflags)
{
    const u32 lane = threadIdx.x & 63u, k = blockIdx.x * (ANSX_RS_NT / 64u) + (threadIdx.x >> 6);
    if (k >= T || rs_wave_err(gflags)) return;  // (both the same for the whole wave)
    const ansx_blk_out o = O[k];
    u32 seed, end;
    const bool ok = brs_bases_of(B, SB, k, &seed, &end);
    rs_wave_block(list + o.off, o.n < ANSX_RS_CHUNK ? o.n : ANSX_RS_CHUNK, lane, ok && o.n <= ANSX_RS_CHUNK, seed, end, gflags);
}

// ANSX_RS_CHUNK < bi <= ANSX_RS_WG_MAX: workgroup k scans block k of the pass
__global__ __launch_bounds__(ANSX_RS_NT) void k_brs_scan_block(u32* __restrict__ list, const ansx_blk_out* __restrict__ O,
    const ansx_batch_blk* __restrict__ B, const ansx_brs_src* __restrict__ SB, u32* __restrict__ gflags)
{
    __shared__ u64 wtot[2][ANSX_RS_NT / 64u];
    __shared__ u32 sh_err;
    const u32 tid = threadIdx.x, k = blockIdx.x;
    if (rs_wg_err(gflags, &sh_err, tid)) return;
    const ansx_blk_out o = O[k];
    u32 seed, end;
    const bool ok = brs_bases_of(B, SB, k, &seed, &end);
    rs_wg_block(list + o.off, o.n, tid, ok, seed, end, wtot, gflags);
}

// Phase 1: workgroup g takes tile g % tpb of block g / tpb, its wave w chunk w of it -> agg[4 g + w] (0 for a chunk
// behind the block's end)
__global__ __launch_bounds__(ANSX_RS_NT) void k_brs_reduce(const u32* __restrict__ list, const ansx_blk_out* __restrict__ O,
    u32 tpb, u64* __restrict__ agg, const u32* __restrict__ gflags)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (rs_wave_err(gflags)) return;
    const ansx_blk_out o = O[blockIdx.x / tpb];
    const u64 off = (u64)(blockIdx.x % tpb) * ANSX_RS_TILE + wave * ANSX_RS_CHUNK;
    ansx_rs_items t;
    rs_load(list + o.off + off, rs_chunk_len(o.n, off), lane, t);
    const u64 tot = rs_total(t);
    if (lane == 0) agg[(u64)blockIdx.x * (ANSX_RS_NT / 64u) + wave] = tot;
}

// Phase 2, workgroup k: the `per` aggregates of block k scanned exclusively from its seed, in place, and the check
__global__ __launch_bounds__(ANSX_RS_NT) void k_brs_carry(u64* __restrict__ agg, u32 per, const ansx_batch_blk* __restrict__ B,
    const ansx_brs_src* __restrict__ SB, u32* __restrict__ gflags)
{
    __shared__ u64 wsum[4];
    __shared__ u32 sh_err;
    const u32 tid = threadIdx.x, k = blockIdx.x;
    if (rs_wg_err(gflags, &sh_err, tid)) return;
    u32 seed, end;
    const bool ok = brs_bases_of(B, SB, k, &seed, &end);
    rs_carry_block(agg + (u64)k * per, per, tid, ok, seed, end, wsum, gflags);
}

// Phase 3, the geometry of k_brs_reduce: every chunk scanned from its carry and stored over itself
__global__ __launch_bounds__(ANSX_RS_NT) void k_brs_apply(u32* __restrict__ list, const ansx_blk_out* __restrict__ O, u32 tpb,
    const u64* __restrict__ carry, const u32* __restrict__ gflags)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (rs_wave_err(gflags)) return;
    const ansx_blk_out o = O[blockIdx.x / tpb];
    const u64 off = (u64)(blockIdx.x % tpb) * ANSX_RS_TILE + wave * ANSX_RS_CHUNK;
    const u32 len = rs_chunk_len(o.n, off);
    if (!len) return;
    rs_apply_chunk(list + o.off + off, len, lane, (u32)carry[(u64)blockIdx.x * (ANSX_RS_NT / 64u) + wave]);
}

// ansx_encode_batch_gaps_bases_dev: the bases of every list read off the sorted ids, one thread per entry.  offs[i]:
// list i's first id in `ids`, boffs[i]: its first entry in `bases` (count + 1 each; total = boffs[count]).
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_batch_ids_bases(const u32* __restrict__ ids, const u64* __restrict__ offs,
    const u64* __restrict__ boffs, u32 count, u32 bi, u64 total, u32* __restrict__ bases)
{
    const u64 e = (u64)blockIdx.x * ANSX_RS_NT + threadIdx.x;
    if (e >= total) return;
    u32 lo = 0, hi = count;  // the last list i with boffs[i] <= e (boffs ascends strictly, boffs[0] = 0)
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (boffs[mid] <= e) lo = mid;
        else hi = mid;
    }
    const u64 b = e - boffs[lo], nb = boffs[lo + 1] - boffs[lo] - 1, n = offs[lo + 1] - offs[lo];
    bases[e] = b == 0 ? 0u : ids[offs[lo] + (b == nb ? n : b * bi) - 1];
}
