// Running sums and gaps over whole lists (ansx_decode_sums_dev, ansx_decode_batch_sums_dev, ansx_encode_gaps_dev,
// ansx_encode_batch_gaps_dev): a segmented inclusive scan of a flat u32 array in place, restarting
// at every list, and its inverse.  gfx950 only.
//
// Layout.  The array starts at any int; `base` is its address rounded DOWN to 16 bytes and `head` (0..3) the ints in
// between, so int i of the array is base[head + i] and every uint4 of base is aligned.  A tile is ANSX_SS_TILE ints of
// base; a workgroup of four waves takes one tile, wave w the 4 KiB [w * 1024, w * 1024 + 1024) of it in four rounds of
// one uint4 per lane: every access of the body is one full-width 16-byte access per lane, a wave's round 1 KiB
// contiguous.  The ints in front of the array (head) and behind it are neither read nor written: a uint4 that holds one
// is handled int by int.  In scan order a tile is (wave, round, lane, int).
//
// Lists.  offs[0 .. count] (u64, device) are the list starts, offs[0] == 0 and offs[count] == n; the list of int i is the
// LAST j with offs[j] <= i, so empty lists are passed over.  Thread 0 of a tile finds the lists of the tile's first and
// last int (a binary search over offs, then doubling steps from there); every thread then searches between them for the first int of each of its
// rounds -- no steps at all while the tile lies inside one list -- and walks from there, so each int may be a list of its
// own.
//
// The scan value is a pair (sum since the last list start, a start was seen), packed in a u64: bit 63 the flag, bits
// 0..62 the sum.  Its operator, (a then b) = b.flag ? b : (a.sum + b.sum, a.flag), is associative and has 0 as its
// identity, which is what wave_incl_scan needs of the lanes it fills in.  (A sum that reaches 2^63 -- 2^31 ints and more
// in one list -- runs into the flag; that list left 32 bits long before and was reported in the tile where it did, and
// what goes wrong behind it concerns that list and later ones, which the smallest reported list does not depend on.)
//
// Most tiles of long lists lie inside one list (no start in them: seg[2] of ss_tile_lists, the same for the whole
// workgroup).  They take a short way: k_sums_reduce a plain 64-bit sum, k_sums_apply 32-bit scans -- what it stores is
// the sums modulo 2^32 anyway -- with the 64-bit question, does the list leave 32 bits in this tile, answered from the
// tile's carry and aggregate; k_gaps has no start to look for.  The general way is about 150 vector instructions per
// round of a wave, which is what bounds it, not the memory: 0.81 -> 0.61 ms for the three kernels on 256 Mi ints.
#pragma once

#include "ansx_dev.h"

#define ANSX_SS_NT 256u
#define ANSX_SS_ROUNDS 4u
#define ANSX_SS_TILE (ANSX_SS_NT * ANSX_SS_ROUNDS * 4u)  // 4096 ints
#define ANSX_SS_SCAN_NT 1024u
#define ANSX_SS_SCAN_IPT 4u
#define ANSX_SS_SCAN_CHUNK (ANSX_SS_SCAN_NT * ANSX_SS_SCAN_IPT)  // tile aggregates per round of k_sums_carry
#define ANSX_SS_FLAG (1ull << 63)
#define ANSX_SS_NONE 0xFFFFFFFFu  // the flag word while no list is at fault

// (later, earlier) -> earlier then later: the argument order wave_incl_scan applies its operator in
struct ansx_ss_op {
    ANSX_D u64 operator()(u64 cur, u64 prev) const { return (cur >> 63) ? cur : cur + prev; }
};

// last j in [lo, hi] with offs[j] <= i (offs[lo] <= i)
ANSX_D u32 ss_seg_of(const u64* __restrict__ offs, u32 lo, u32 hi, u64 i)
{
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (offs[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// What a thread holds of its tile
struct ansx_ss_items {
    u32 x[ANSX_SS_ROUNDS][4];
    u32 valid;  // bit 4k + j: int j of round k lies inside the array
    u32 start;  // bit 4k + j: ... and is the first of its list
};

// index into base of the thread's uint4 of round k
ANSX_D u64 ss_at(u64 tile, u32 tid, u32 k)
{
    return (u64)tile * ANSX_SS_TILE + (u64)(((tid >> 6) * ANSX_SS_ROUNDS + k) * 64u + (tid & 63u)) * 4u;
}

// the lists of the tile's first and last int -> seg[0], seg[1], and whether any list starts inside the tile -> seg[2]
// (shared), for every thread
ANSX_D void ss_tile_lists(const u64* __restrict__ offs, u32 count, u32 head, u64 n, u64 tile, u32 tid, u32* seg)
{
    if (tid == 0) {
        const u64 v0 = tile * ANSX_SS_TILE;
        const u64 end = v0 + ANSX_SS_TILE - head;  // (one behind the tile's last int, were the array that long)
        const u64 first = (v0 > head ? v0 : head) - head, last = (end < n ? end : n) - 1;
        const u32 lo = ss_seg_of(offs, 0, count - 1, first);
        // the last int's list is rarely far from the first's: doubling steps from there, then the search between
        u64 at = lo, step = 1;
        while (at + step < count && offs[at + step] <= last) at += step, step *= 2;
        seg[0] = lo;
        seg[1] = ss_seg_of(offs, (u32)at, (u32)(at + step < count ? at + step - 1 : count - 1), last);
        seg[2] = seg[1] != seg[0] || offs[seg[0]] == first;
    }
    __syncthreads();
}

// the thread's ints (0 where outside the array)
ANSX_D void ss_load_ints(const u32* __restrict__ base, u32 head, u64 n, u64 tile, u32 tid, ansx_ss_items& t)
{
    t.valid = 0, t.start = 0;
#pragma unroll
    for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) {
        const u64 v = ss_at(tile, tid, k);
        if (v >= head && v + 3 < head + n) {
            const uint4 q = *(const uint4*)(base + v);
            t.x[k][0] = q.x, t.x[k][1] = q.y, t.x[k][2] = q.z, t.x[k][3] = q.w;
            t.valid |= 15u << (4 * k);
        } else {
#pragma unroll
            for (u32 j = 0; j < 4; j++) {
                const bool in = v + j >= head && v + j < head + n;
                t.x[k][j] = in ? base[v + j] : 0u;
                t.valid |= (in ? 1u : 0u) << (4 * k + j);
            }
        }
    }
}

// ... and which of them start a list
ANSX_D void ss_mark_starts(u32 head, const u64* __restrict__ offs, u32 lo, u32 hi, u64 tile, u32 tid, ansx_ss_items& t)
{
    u32 seg = lo;
    u64 cs = offs[seg], nb = offs[seg + 1];  // the list at hand is [cs, nb)
#pragma unroll
    for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) {
        const u32 vk = (t.valid >> (4 * k)) & 15u;
        if (!vk) continue;
        const u64 v = ss_at(tile, tid, k);
        const u64 p0 = v + (u32)__builtin_ctz(vk) - head;  // the round's first int: a jump from the last one
        if (p0 >= nb) {
            seg = ss_seg_of(offs, seg, hi, p0);
            cs = offs[seg], nb = offs[seg + 1];
        }
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            if (!((vk >> j) & 1u)) continue;
            const u64 p = v + j - head;
            while (p >= nb) cs = nb, nb = offs[++seg + 1];  // (ends: offs[count] == n > p)
            t.start |= (p == cs ? 1u : 0u) << (4 * k + j);
        }
    }
}

// the thread's four ints of round k under the scan operator
ANSX_D u64 ss_fold(const ansx_ss_items& t, u32 k)
{
    u64 p = 0;
#pragma unroll
    for (u32 j = 0; j < 4; j++) {
        const u32 b = 4 * k + j;
        if ((t.valid >> b) & 1u) p = ((t.start >> b) & 1u) ? (ANSX_SS_FLAG | t.x[k][j]) : p + t.x[k][j];
    }
    return p;
}

// the thread's uint4 of round k: whole where it lies inside the array, else the ints that do
ANSX_D void ss_store(u32* __restrict__ base, u64 v, u32 vk, const u32* o)
{
    if (vk == 15u) {
        *(uint4*)(base + v) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (u32 j = 0; j < 4; j++)
            if ((vk >> j) & 1u) base[v + j] = o[j];
    }
}

// list `seg` is at fault: the smallest one stays in *bad.  (Looked at first: once a small list stands there, the threads of
// a long list at fault -- every one behind its first excess -- have nothing to add, and a stale look costs one atomic.)
ANSX_D void ss_report(u32* bad, u32 seg)
{
    if (seg < *(volatile u32*)bad) atomicMin(bad, seg);
}

ANSX_D u64 ss_lane_before(u64 v, u32 lane)  // the lane below's value, 0 in lane 0
{
    const u64 r = (u64)__shfl_up((unsigned long long)v, 1);
    return lane ? r : 0ull;
}

// Phase 1, per tile: its aggregate under the scan operator -- the sum behind its last list start (of the whole tile when
// it has none) and whether it has one -> agg[tile]
__global__ __launch_bounds__(ANSX_SS_NT) void k_sums_reduce(const u32* __restrict__ base, u32 head, u64 n,
    const u64* __restrict__ offs, u32 count, u64* __restrict__ agg)
{
    __shared__ u32 seg[3];
    __shared__ u64 wtot[ANSX_SS_NT / 64];
    const u32 tid = threadIdx.x;
    const u64 tile = blockIdx.x;
    const ansx_ss_op op;
    ansx_ss_items t;
    ss_load_ints(base, head, n, tile, tid, t);  // (under way while thread 0 searches)
    ss_tile_lists(offs, count, head, n, tile, tid, seg);
    u64 w = 0;
    if (!seg[2]) {  // inside one list: a plain sum, one reduction per wave
#pragma unroll
        for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) w += (u64)t.x[k][0] + t.x[k][1] + t.x[k][2] + t.x[k][3];
        w = wave_sum(w);
        if ((tid & 63u) == 0) wtot[tid >> 6] = w;
        __syncthreads();
        if (tid == 0) {
            u64 a = 0;
            for (u32 i = 0; i < ANSX_SS_NT / 64; i++) a += wtot[i];
            agg[tile] = a;
        }
        return;
    }
    ss_mark_starts(head, offs, seg[0], seg[1], tile, tid, t);
#pragma unroll
    for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) w = op(wave_last(wave_incl_scan(ss_fold(t, k), op)), w);
    if ((tid & 63u) == 0) wtot[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        u64 a = 0;
        for (u32 i = 0; i < ANSX_SS_NT / 64; i++) a = op(wtot[i], a);
        agg[tile] = a;
    }
}

// Phase 2, one workgroup: agg[0 .. ntiles) scanned exclusively under the scan operator -> carry[tile], the carry into the
// tile: the sum so far of the list that is open at its first int
__global__ __launch_bounds__(ANSX_SS_SCAN_NT) void k_sums_carry(const u64* __restrict__ agg, u64* __restrict__ carry_out,
    u64 ntiles)
{
    __shared__ u64 wtot[ANSX_SS_SCAN_NT / 64];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const ansx_ss_op op;
    u64 carry = 0, next[ANSX_SS_SCAN_IPT];  // next: the round's aggregates, loaded one round ahead
#pragma unroll
    for (u32 q = 0; q < ANSX_SS_SCAN_IPT; q++) next[q] = (u64)tid * ANSX_SS_SCAN_IPT + q < ntiles ? agg[(u64)tid * ANSX_SS_SCAN_IPT + q] : 0ull;
    for (u64 b = 0; b < ntiles; b += ANSX_SS_SCAN_CHUNK) {
        const u64 i0 = b + (u64)tid * ANSX_SS_SCAN_IPT;
        u64 v[ANSX_SS_SCAN_IPT], p = 0;
#pragma unroll
        for (u32 q = 0; q < ANSX_SS_SCAN_IPT; q++) {
            v[q] = next[q];
            p = op(v[q], p);
            const u64 i1 = i0 + ANSX_SS_SCAN_CHUNK + q;
            next[q] = i1 < ntiles ? agg[i1] : 0ull;
        }
        const u64 inc = wave_incl_scan(p, op);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        u64 pre = carry;  // everything in front of the wave, then of the thread's first aggregate
        for (u32 i = 0; i < ANSX_SS_SCAN_NT / 64; i++) {
            if (i == wave) pre = carry;
            carry = op(wtot[i], carry);
        }
        u64 run = op(ss_lane_before(inc, lane), pre);
#pragma unroll
        for (u32 q = 0; q < ANSX_SS_SCAN_IPT; q++) {
            if (i0 + q < ntiles) carry_out[i0 + q] = run & ~ANSX_SS_FLAG;
            run = op(v[q], run);
        }
        __syncthreads();  // (wtot is written again in the next round)
    }
}

// Phase 3, per tile: the tile scanned from its carry and stored over itself.  A running sum above 2^32 - 1 puts its
// list into *bad (the smallest such list wins); what is stored of that list is then its sums modulo 2^32.
__global__ __launch_bounds__(ANSX_SS_NT) void k_sums_apply(u32* __restrict__ base, u32 head, u64 n,
    const u64* __restrict__ offs, u32 count, const u64* __restrict__ agg, const u64* __restrict__ carry, u32* bad)
{
    __shared__ u32 seg[3];
    __shared__ u64 wtot[ANSX_SS_NT / 64];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u64 tile = blockIdx.x;
    const ansx_ss_op op;
    ansx_ss_items t;
    ss_load_ints(base, head, n, tile, tid, t);  // (under way while thread 0 searches)
    ss_tile_lists(offs, count, head, n, tile, tid, seg);
    if (!seg[2]) {
        // Inside one list: the stored sums are sums modulo 2^32, so 32-bit scans do; whether the list's running sum
        // leaves 32 bits inside this tile is told by the carry and the tile's aggregate, both exact
        __shared__ u32 wtot32[ANSX_SS_NT / 64];
        u32 inc[ANSX_SS_ROUNDS], tot[ANSX_SS_ROUNDS], w = 0;
#pragma unroll
        for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) {
            inc[k] = wave_incl_scan(t.x[k][0] + t.x[k][1] + t.x[k][2] + t.x[k][3]);
            tot[k] = wave_last(inc[k]);
            w += tot[k];
        }
        if (lane == 0) wtot32[wave] = w;
        __syncthreads();
        const u64 cin = carry[tile];
        u32 pre = (u32)cin;
        for (u32 i = 0; i < wave; i++) pre += wtot32[i];
#pragma unroll
        for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) {
            const u32 before = __shfl_up(inc[k], 1);
            u32 run = pre + (lane ? before : 0u), o[4];
#pragma unroll
            for (u32 j = 0; j < 4; j++) o[j] = run += t.x[k][j];
            const u32 vk = (t.valid >> (4 * k)) & 15u;
            if (vk) ss_store(base, ss_at(tile, tid, k), vk, o);
            pre += tot[k];
        }
        if (tid == 0 && cin + agg[tile] > 0xFFFFFFFFull) ss_report(bad, seg[0]);
        return;
    }
    ss_mark_starts(head, offs, seg[0], seg[1], tile, tid, t);
    u64 inc[ANSX_SS_ROUNDS], tot[ANSX_SS_ROUNDS], w = 0;
#pragma unroll
    for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) {
        inc[k] = wave_incl_scan(ss_fold(t, k), op);
        tot[k] = wave_last(inc[k]);
        w = op(tot[k], w);
    }
    if (lane == 0) wtot[wave] = w;
    __syncthreads();
    u64 pre = carry[tile];  // everything in front of the wave, then of its round k
    for (u32 i = 0; i < wave; i++) pre = op(wtot[i], pre);
    u64 over = ~0ull;  // the thread's first int whose running sum does not fit
#pragma unroll
    for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) {
        u64 run = op(ss_lane_before(inc[k], lane), pre) & ~ANSX_SS_FLAG;
        const u32 vk = (t.valid >> (4 * k)) & 15u;
        const u64 v = ss_at(tile, tid, k);
        u32 o[4];
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            const u32 b = 4 * k + j;
            if (!((t.valid >> b) & 1u)) continue;
            run = ((t.start >> b) & 1u) ? (u64)t.x[k][j] : run + t.x[k][j];
            if (run > 0xFFFFFFFFull && over == ~0ull) over = v + j - head;
            o[j] = (u32)run;
        }
        if (vk) ss_store(base, v, vk, o);
        pre = op(tot[k], pre);
    }
    if (over != ~0ull) ss_report(bad, ss_seg_of(offs, 0, count - 1, over));
}

// Gaps, per tile: out[i] = in[i] at a list start, in[i] - in[i - 1] elsewhere, through the same tiles (base_out has the
// input's head, so the body is 16-byte accesses on both sides).  A neighbour pair that DEcreases inside a list puts the
// list into *bad (the smallest wins): decided on the values, the wrapped difference would not tell.
__global__ __launch_bounds__(ANSX_SS_NT) void k_gaps(const u32* __restrict__ base, u32* __restrict__ base_out, u32 head,
    u64 n, const u64* __restrict__ offs, u32 count, u32* bad)
{
    __shared__ u32 seg[3];
    const u32 tid = threadIdx.x;
    const u64 tile = blockIdx.x;
    ansx_ss_items t;
    ss_load_ints(base, head, n, tile, tid, t);  // (under way while thread 0 searches)
    ss_tile_lists(offs, count, head, n, tile, tid, seg);
    if (seg[2]) ss_mark_starts(head, offs, seg[0], seg[1], tile, tid, t);  // (else inside one list: no start to look for)
    u64 dec = ~0ull;  // the thread's first int below its predecessor
#pragma unroll
    for (u32 k = 0; k < ANSX_SS_ROUNDS; k++) {
        const u32 vk = (t.valid >> (4 * k)) & 15u;
        if (!vk) continue;
        const u64 v = ss_at(tile, tid, k);
        const u64 v0 = v + (u32)__builtin_ctz(vk);  // the round's first int: its predecessor is one int of overlap
        u32 prev = v0 > head ? base[v0 - 1] : 0u;
        u32 o[4];
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            const u32 b = 4 * k + j;
            if (!((t.valid >> b) & 1u)) continue;
            const u32 x = t.x[k][j];
            const bool st = (t.start >> b) & 1u;
            if (!st && x < prev && dec == ~0ull) dec = v + j - head;
            o[j] = st ? x : x - prev;
            prev = x;
        }
        ss_store(base_out, v, vk, o);
    }
    if (dec != ~0ull) ss_report(bad, ss_seg_of(offs, 0, count - 1, dec));
}
