// Docids of ranges (ansx_decode_ranges_sums_dev, ansx_decode_device_ranges_sums_dev) and the block bases they start
// from (ansx_block_bases_dev, ansx_encode_gaps_bases_dev); DESIGN.md section 3f.  gfx950 only.
//
// Input.  The work list of range_tail: T touched blocks, block k the ints [k * bi, k * bi + len_k) of `list`, len_k = bi
// except for a short last one (n_sub ints in all), tb[k] its block number in the source.  The list is 16-byte aligned
// and bi a multiple of 4, so every block starts on a 16-byte boundary.  Output: the list in place,
// list[k * bi + j] = bases[tb[k]] + x[0] + ... + x[j] modulo 2^32.  Of bases only the entries tb[k] and tb[k] + 1 are
// read; bases[tb[k]] + (the sum of block k, in 64 bits) must be bases[tb[k] + 1], else the bases are not this
// container's: the format bit of the decode's flag word, which the gather behind looks at and the decode's own
// read-back carries home.  Nothing beyond n_sub ints is read or written.
//
// The unit is a wave and a chunk of ANSX_RS_CHUNK = 1024 ints: four rounds of one uint4 per lane, a round 1 KiB
// contiguous, scan order (round, lane, int).  A wave scans its chunk on its own -- a 64-bit DPP scan of the lanes' sums
// per round -- so only the sum in front of the chunk has to come from elsewhere.  Only a chunk that holds the end of a
// short last block touches single ints.
//
// Three shapes, chosen by bi (range_sums_scan in ansx.hip):
//   bi <= ANSX_RS_CHUNK      k_rs_scan_small: a wave per block, four blocks per workgroup, no LDS and no barrier.
//   bi <= ANSX_RS_WG_MAX     k_rs_scan_block: a workgroup per block, tile (four chunks, ANSX_RS_TILE ints) after tile
//                            with the running sum carried along, the next tile's loads issued before the scan of the
//                            one at hand; the waves' totals meet in LDS, one barrier per tile.  Read once, written once.
//   larger                   three phases per block, no workgroup waiting for another: k_rs_reduce (a 64-bit aggregate
//                            per chunk), k_rs_carry (a workgroup per block: the aggregates scanned exclusively from
//                            bases[tb[k]], and the check), k_rs_apply (every chunk scanned from its carry).
// Every grid is T, T / 4 or T * ceil(bi / ANSX_RS_TILE) workgroups, never the source's block count.
//
// ansx_block_bases_dev runs k_rs_reduce over the whole decoded list (every block "touched") and k_rs_bases, one
// workgroup that scans all aggregates and writes a base wherever a block ends.
#pragma once

#include "ansx_ranges.h"
#include "ansx_sums.h"

#define ANSX_RS_NT 256u
#define ANSX_RS_CHUNK 1024u                            // ints per wave: 4 rounds of a uint4 per lane
#define ANSX_RS_TILE ANSX_SS_TILE                      // ints per workgroup and step: a chunk per wave
#define ANSX_RS_WG_MAX (16u * ANSX_RS_TILE)            // the largest block k_rs_scan_block takes
#define ANSX_RS_BASES_IPT 8u                           // aggregates per thread and round of k_rs_bases

struct ansx_rs_items {
    u32 x[4][4];  // [round][int]
};

// the wave's chunk p[0 .. len), len <= ANSX_RS_CHUNK, p 16-byte aligned: 0 where outside
ANSX_D void rs_load(const u32* __restrict__ p, u32 len, u32 lane, ansx_rs_items& t)
{
#pragma unroll
    for (u32 r = 0; r < 4; r++) {
        const u32 i = (r * 64u + lane) * 4u;
        if (i + 4u <= len) {
            const uint4 q = *(const uint4*)(p + i);
            t.x[r][0] = q.x, t.x[r][1] = q.y, t.x[r][2] = q.z, t.x[r][3] = q.w;
        } else {
#pragma unroll
            for (u32 j = 0; j < 4; j++) t.x[r][j] = i + j < len ? p[i + j] : 0u;
        }
    }
}

ANSX_D u64 rs_sum4(const ansx_rs_items& t, u32 r) { return (u64)t.x[r][0] + t.x[r][1] + t.x[r][2] + t.x[r][3]; }

// inc[r]: the sum of the chunk up to and including the lane's uint4 of round r; returns the chunk's sum.  (Every lane of
// the wave takes part.)
ANSX_D u64 rs_scan(const ansx_rs_items& t, u64 (&inc)[4])
{
    u64 run = 0;
#pragma unroll
    for (u32 r = 0; r < 4; r++) {
        const u64 s = wave_incl_scan(rs_sum4(t, r));
        inc[r] = run + s;
        run += wave_last(s);
    }
    return run;
}

// the chunk's sum alone
ANSX_D u64 rs_total(const ansx_rs_items& t)
{
    return wave_sum(rs_sum4(t, 0) + rs_sum4(t, 1) + rs_sum4(t, 2) + rs_sum4(t, 3));
}

// the chunk's running sums, `pre` in front of it, over p[0 .. len)
ANSX_D void rs_store(u32* __restrict__ p, u32 len, u32 lane, const ansx_rs_items& t, const u64 (&inc)[4], u32 pre)
{
#pragma unroll
    for (u32 r = 0; r < 4; r++) {
        const u32 i = (r * 64u + lane) * 4u;
        u32 run = pre + (u32)(inc[r] - rs_sum4(t, r)), o[4];
#pragma unroll
        for (u32 j = 0; j < 4; j++) o[j] = run += t.x[r][j];
        if (i + 4u <= len) {
            *(uint4*)(p + i) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (u32 j = 0; j < 4; j++)
                if (i + j < len) p[i + j] = o[j];
        }
    }
}

// ints of work-list block k
ANSX_D u32 rs_block_len(u64 n_sub, u32 bi, u32 k)
{
    const u64 left = n_sub - (u64)k * bi;
    return left < bi ? (u32)left : bi;
}

// ints of the chunk at `off` of a block of blen ints
ANSX_D u32 rs_chunk_len(u32 blen, u64 off) { return off >= blen ? 0u : (blen - off < ANSX_RS_CHUNK ? (u32)(blen - off) : ANSX_RS_CHUNK); }

// bases[b] and bases[b + 1] of touched block k: (seed, the sum the block must end on); a block number outside the
// source (no plan names one) fails the check without a read
ANSX_D bool rs_bases_of(const u32* __restrict__ tb, u32 k, u32 nblocks, const u32* __restrict__ bases, u32* seed, u32* end)
{
    const u32 b = tb[k];
    if (b >= nblocks) {
        *seed = 0, *end = 0;
        return false;
    }
    *seed = bases[b], *end = bases[b + 1];
    return true;
}

ANSX_D void rs_flag_format(u32* gflags) { atomicOr(&gflags[ANSX_G_ERR], 1u << 3 /* ANSX_ERR_FORMAT */); }

// the decode's error word, the same value in every thread of the workgroup (other workgroups may be setting it)
ANSX_D u32 rs_wg_err(const u32* gflags, u32* sh, u32 tid)
{
    if (tid == 0) *sh = __hip_atomic_load(&gflags[ANSX_G_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return *sh;
}
// ... in every lane of the wave
ANSX_D u32 rs_wave_err(const u32* gflags)
{
    return (u32)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&gflags[ANSX_G_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// The bodies of the kernels below, by where a block lies: here at k * bi of the list, in ansx_batchrangesums.h wherever
// a pass's table puts it.  (ok, seed, end): rs_bases_of's verdict on the block.

// a wave scans the block p[0 .. len), len <= ANSX_RS_CHUNK, on its own
ANSX_D void rs_wave_block(u32* __restrict__ p, u32 len, u32 lane, bool ok, u32 seed, u32 end, u32* __restrict__ gflags)
{
    ansx_rs_items t;
    rs_load(p, len, lane, t);
    u64 inc[4];
    const u64 tot = rs_scan(t, inc);
    if (!ok || (u64)seed + tot != (u64)end) {
        if (lane == 0) rs_flag_format(gflags);
        return;
    }
    rs_store(p, len, lane, t, inc, seed);
}

// a workgroup scans the block blk[0 .. blen), tile after tile (wtot: two rows of a total per wave)
ANSX_D void rs_wg_block(u32* __restrict__ blk, u32 blen, u32 tid, bool ok, u32 seed, u32 end, u64 (*wtot)[ANSX_RS_NT / 64u],
    u32* __restrict__ gflags)
{
    const u32 lane = tid & 63u, wave = tid >> 6, ntile = (blen + ANSX_RS_TILE - 1) / ANSX_RS_TILE;
    u64 carry = seed;  // the sum in front of the tile at hand
    ansx_rs_items cur, nxt;
    rs_load(blk + wave * ANSX_RS_CHUNK, rs_chunk_len(blen, wave * ANSX_RS_CHUNK), lane, cur);
    for (u32 t = 0; t < ntile; t++) {
        const u64 off = (u64)t * ANSX_RS_TILE + wave * ANSX_RS_CHUNK;
        if (t + 1 < ntile) rs_load(blk + off + ANSX_RS_TILE, rs_chunk_len(blen, off + ANSX_RS_TILE), lane, nxt);
        u64 inc[4];
        const u64 tot = rs_scan(cur, inc);
        if (lane == 0) wtot[t & 1u][wave] = tot;
        __syncthreads();  // (one per tile: wtot[t & 1] is next written two tiles on, behind the barrier in between)
        u64 pre = carry;
#pragma unroll
        for (u32 i = 0; i < ANSX_RS_NT / 64u; i++) {
            const u64 v = wtot[t & 1u][i];
            if (i < wave) pre += v;
            carry += v;
        }
        rs_store(blk + off, rs_chunk_len(blen, off), lane, cur, inc, (u32)pre);
        if (t + 1 < ntile) cur = nxt;
    }
    if (tid == 0 && (!ok || carry != (u64)end)) rs_flag_format(gflags);
}

// a workgroup scans the `per` aggregates a[] of one block exclusively from its seed, in place, and checks the end
ANSX_D void rs_carry_block(u64* __restrict__ a, u32 per, u32 tid, bool ok, u32 seed, u32 end, u64* wsum, u32* __restrict__ gflags)
{
    u64 carry = seed;
    for (u32 base = 0; base < per; base += ANSX_RS_NT * 4u) {
        const u32 i0 = base + tid * 4u;
        u64 v[4], s = 0, all;
#pragma unroll
        for (u32 q = 0; q < 4; q++) {
            v[q] = i0 + q < per ? a[i0 + q] : 0ull;
            s += v[q];
        }
        u64 run = carry + dr_block_excl(s, wsum, tid, &all, ansx_op_add());
#pragma unroll
        for (u32 q = 0; q < 4; q++) {
            if (i0 + q < per) a[i0 + q] = run;
            run += v[q];
        }
        carry += all;
    }
    if (tid == 0 && (!ok || carry != (u64)end)) rs_flag_format(gflags);
}

// a wave scans the chunk p[0 .. len) from the sum `pre` in front of it
ANSX_D void rs_apply_chunk(u32* __restrict__ p, u32 len, u32 lane, u32 pre)
{
    ansx_rs_items t;
    rs_load(p, len, lane, t);
    u64 inc[4];
    (void)rs_scan(t, inc);
    rs_store(p, len, lane, t, inc, pre);
}

// bi <= ANSX_RS_CHUNK: wave w of workgroup g scans block 4 g + w
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_scan_small(u32* __restrict__ list, u64 n_sub, u32 bi, u32 T,
    const u32* __restrict__ tb, u32 nblocks, const u32* __restrict__ bases, u32* __restrict__ gflags)
{
    const u32 lane = threadIdx.x & 63u, k = blockIdx.x * (ANSX_RS_NT / 64u) + (threadIdx.x >> 6);
    if (k >= T || rs_wave_err(gflags)) return;  // (both the same for the whole wave)
    u32 seed, end;
    const bool ok = rs_bases_of(tb, k, nblocks, bases, &seed, &end);
    rs_wave_block(list + (u64)k * bi, rs_block_len(n_sub, bi, k), lane, ok, seed, end, gflags);
}

// ANSX_RS_CHUNK < bi <= ANSX_RS_WG_MAX: workgroup k scans block k, tile after tile
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_scan_block(u32* __restrict__ list, u64 n_sub, u32 bi,
    const u32* __restrict__ tb, u32 nblocks, const u32* __restrict__ bases, u32* __restrict__ gflags)
{
    __shared__ u64 wtot[2][ANSX_RS_NT / 64u];
    __shared__ u32 sh_err;
    const u32 tid = threadIdx.x, k = blockIdx.x;
    if (rs_wg_err(gflags, &sh_err, tid)) return;
    u32 seed, end;
    const bool ok = rs_bases_of(tb, k, nblocks, bases, &seed, &end);
    rs_wg_block(list + (u64)k * bi, rs_block_len(n_sub, bi, k), tid, ok, seed, end, wtot, gflags);
}

// Phase 1, a wave per chunk: its 64-bit sum -> agg.  per_block == 1 (bi <= ANSX_RS_CHUNK, ansx_block_bases_dev only):
// wave w of workgroup g takes block 4 g + w, agg[block].  Else workgroup g takes tile g % tpb of block g / tpb, its wave
// w chunk w of it, agg[4 g + w] (0 for a chunk behind the end of a short block).
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_reduce(const u32* __restrict__ list, u64 n_sub, u32 bi, u32 T, u32 tpb,
    u64* __restrict__ agg, const u32* __restrict__ gflags)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (rs_wave_err(gflags)) return;
    u32 k;
    u64 off, slot;
    if (tpb == 0) {
        k = blockIdx.x * (ANSX_RS_NT / 64u) + wave, off = 0, slot = k;
        if (k >= T) return;
    } else {
        k = blockIdx.x / tpb, off = (u64)(blockIdx.x % tpb) * ANSX_RS_TILE + wave * ANSX_RS_CHUNK;
        slot = (u64)blockIdx.x * (ANSX_RS_NT / 64u) + wave;
    }
    ansx_rs_items t;
    rs_load(list + (u64)k * bi + off, rs_chunk_len(rs_block_len(n_sub, bi, k), off), lane, t);
    const u64 tot = rs_total(t);
    if (lane == 0) agg[slot] = tot;
}

// Phase 2, workgroup k: the `per` aggregates of block k scanned exclusively from bases[tb[k]], in place (agg[i] becomes
// the sum in front of chunk i), and the check
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_carry(u64* __restrict__ agg, u32 per, const u32* __restrict__ tb,
    u32 nblocks, const u32* __restrict__ bases, u32* __restrict__ gflags)
{
    __shared__ u64 wsum[4];
    __shared__ u32 sh_err;
    const u32 tid = threadIdx.x, k = blockIdx.x;
    if (rs_wg_err(gflags, &sh_err, tid)) return;
    u32 seed, end;
    const bool ok = rs_bases_of(tb, k, nblocks, bases, &seed, &end);
    rs_carry_block(agg + (u64)k * per, per, tid, ok, seed, end, wsum, gflags);
}

// Phase 3, the geometry of k_rs_reduce's tiles: every chunk scanned from its carry and stored over itself
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_apply(u32* __restrict__ list, u64 n_sub, u32 bi, u32 tpb,
    const u64* __restrict__ carry, const u32* __restrict__ gflags)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (rs_wave_err(gflags)) return;
    const u32 k = blockIdx.x / tpb;
    const u64 off = (u64)(blockIdx.x % tpb) * ANSX_RS_TILE + wave * ANSX_RS_CHUNK;
    const u32 len = rs_chunk_len(rs_block_len(n_sub, bi, k), off);
    if (!len) return;
    rs_apply_chunk(list + (u64)k * bi + off, len, lane, (u32)carry[(u64)blockIdx.x * (ANSX_RS_NT / 64u) + wave]);
}

// ansx_block_bases_dev, one workgroup: agg[0 .. nblocks * per) scanned inclusively; where block b ends -- behind its
// `per` aggregates -- the sum so far is bases[b + 1].  A total above 2^32 - 1 is the domain bit of the decode's flags.
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_bases(const u64* __restrict__ agg, u32 per, u32 nblocks,
    u32* __restrict__ bases, u32* __restrict__ gflags)
{
    __shared__ u64 wsum[4];
    __shared__ u32 sh_err;
    const u32 tid = threadIdx.x;
    if (rs_wg_err(gflags, &sh_err, tid)) return;
    const u64 m = (u64)nblocks * per;
    u64 carry = 0;
    for (u64 base = 0; base < m; base += ANSX_RS_NT * ANSX_RS_BASES_IPT) {
        const u64 i0 = base + (u64)tid * ANSX_RS_BASES_IPT;
        u64 v[ANSX_RS_BASES_IPT], s = 0, all;
#pragma unroll
        for (u32 q = 0; q < ANSX_RS_BASES_IPT; q++) {
            v[q] = i0 + q < m ? agg[i0 + q] : 0ull;
            s += v[q];
        }
        u64 run = carry + dr_block_excl(s, wsum, tid, &all, ansx_op_add());
        u64 b = i0 / per;          // the block of the aggregate at hand
        u32 r = (u32)(i0 % per);   // ... and its place in it
#pragma unroll
        for (u32 q = 0; q < ANSX_RS_BASES_IPT; q++) {
            run += v[q];
            if (i0 + q < m && ++r == per) {
                bases[++b] = (u32)run;
                r = 0;
            }
        }
        carry += all;
    }
    if (tid == 0) {
        bases[0] = 0;
        if (carry > 0xFFFFFFFFull) atomicOr(&gflags[ANSX_G_ERR], 1u << 6 /* ANSX_ERR_DOMAIN */);
    }
}

// ansx_encode_gaps_bases_dev: the bases read off the sorted ids, one thread per entry
__global__ __launch_bounds__(ANSX_RS_NT) void k_rs_ids_bases(const u32* __restrict__ ids, u64 n, u32 bi, u32 nblocks,
    u32* __restrict__ bases)
{
    const u64 b = (u64)blockIdx.x * ANSX_RS_NT + threadIdx.x;
    if (b > nblocks) return;
    bases[b] = b == 0 ? 0u : ids[(b == nblocks ? n : b * bi) - 1];
}
