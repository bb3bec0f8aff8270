// ansx_ranges.h -- random access (ansx_decode_ranges_dev).
//
// The blocks a call's ranges touch are gathered into a container of their own, laid out exactly as make_plan lays out a
// container of that many ints (k_range_index: header and rebased block index; k_range_copy: restart points, parse hints
// and block streams).  The ordinary decode path decodes it; k_range_gather then copies every range's span of the
// decoded sub-list to the caller's buffer in range order.  Only the touched blocks' index entries and bytes are read.
#pragma once

#include "ansx_kernels.h"

struct ansx_range_lay {  // byte offsets of a container's sections (the index is at 64)
    u64 ckoff_off, ckstate_off, hint_off, payload_off;
};

// (ansx_range_piece, ANSX_RANGE_CHUNK: ansx_plan_types.h)

// Byte length of touched block k's stream (source block b), 0 if its index entries are not those of a well-formed
// container (index_entry_ok: the checks of k_validate_index): such a block sets the format flag and is not copied.
__device__ __forceinline__ u64 range_block_len(const ansx_geo& g, const u64* __restrict__ boff, u32 b,
    u32* __restrict__ flags)
{
    const u64 a = b < g.nblocks ? boff[b] : 0, e = b < g.nblocks ? boff[b + 1] : 0;
    if (b >= g.nblocks || !index_entry_ok(g, b, a, e)) {
        atomicOr(&flags[0], 1u << 3 /* ANSX_ERR_FORMAT */);
        return 0;
    }
    return e - a;
}

// One workgroup: exclusive scan of the touched blocks' stream lengths into the sub-container's index (the pattern of
// k_scan_sizes: every wave owns a contiguous range of entries, its lanes on consecutive ones), then the header --
// the host's image with the payload size filled in.  len(i): the stream length of the sub-container's block i, 0 for an
// invalid one (flagged by len itself).
template <class Len>
__device__ __forceinline__ void range_index_body(u32 T, Len len, const ansx_container_header& hsub, u8* __restrict__ dst,
    u64 cap_pay, u32* __restrict__ flags)
{
    __shared__ u64 part[20];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64* sboff = (u64*)(dst + 64);
    const u32 per = ((T + 15) / 16 + 63) & ~63u;  // entries per wave, a multiple of 64
    const u32 lo = wave * per < T ? wave * per : T, hi = (lo + per) < T ? (lo + per) : T;
    u64 sum = 0;
    for (u32 i = lo + lane; i < hi; i += 64) sum += len(i);
    sum = wave_sum(sum);
    u64 total;
    u64 run = block_excl_scan<u64>(lane == 63 ? sum : 0ull, part, tid, 1024, &total);
    run = wave_last(run);
    for (u32 i0 = lo; i0 < hi; i0 += 64) {
        const u32 i = i0 + lane;
        const u64 v = i < hi ? len(i) : 0ull;
        const u64 incl = wave_incl_scan(v);
        if (i < hi) sboff[i] = run + incl - v;
        run += wave_last(incl);
    }
    if (tid == 0) {
        sboff[T] = total;
        if (total > cap_pay) atomicOr(&flags[0], 1u << 3);  // (only entries that overlap can add up to this)
    }
    if (tid < 16) {  // 64 header bytes, one dword per lane; payload_bytes is dwords 12, 13
        const u32* w = (const u32*)&hsub;
        u32 v = w[tid];
        if (tid == 12) v = (u32)total;
        if (tid == 13) v = (u32)(total >> 32);
        ((u32*)dst)[tid] = v;
    }
}

__global__ __launch_bounds__(1024) void k_range_index(const u8* __restrict__ src, ansx_geo g,
    const u32* __restrict__ tb, u32 T, ansx_container_header hsub, u8* __restrict__ dst, u64 cap_pay,
    u32* __restrict__ flags)
{
    const u64* boff = (const u64*)(src + 64);
    range_index_body(T, [&](u32 i) { return range_block_len(g, boff, tb[i], flags); }, hsub, dst, cap_pay, flags);
}

// dst[0..n) = src[0..n): 16-byte stores on dst's aligned body, fed by 16-byte loads where src is aligned alike and by
// unaligned dword loads otherwise; single bytes at both ends.
__device__ __forceinline__ void range_copy_bytes(u8* __restrict__ dst, const u8* __restrict__ src, u64 n, u32 tid, u32 nt)
{
    u64 head = (u64)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const u64 nq = (n - head) >> 4;
    uint4* d16 = (uint4*)(dst + head);
    const u8* s1 = src + head;
    if (((uintptr_t)s1 & 15) == 0) {
        const uint4* s16 = (const uint4*)s1;
        u64 j = tid;
        for (; j + 3 * (u64)nt < nq; j += 4 * (u64)nt) {
            const uint4 v0 = s16[j], v1 = s16[j + nt], v2 = s16[j + 2 * nt], v3 = s16[j + 3 * nt];
            d16[j] = v0;
            d16[j + nt] = v1;
            d16[j + 2 * nt] = v2;
            d16[j + 3 * nt] = v3;
        }
        for (; j < nq; j += nt) d16[j] = s16[j];
    } else {
        auto ld16 = [&](u64 j) {
            const u8* p = s1 + 16 * j;
            return make_uint4(ld_u32_unaligned(p), ld_u32_unaligned(p + 4), ld_u32_unaligned(p + 8), ld_u32_unaligned(p + 12));
        };
        u64 j = tid;
        for (; j + 3 * (u64)nt < nq; j += 4 * (u64)nt) {
            const uint4 v0 = ld16(j), v1 = ld16(j + nt), v2 = ld16(j + 2 * nt), v3 = ld16(j + 3 * nt);
            d16[j] = v0;
            d16[j + nt] = v1;
            d16[j + 2 * nt] = v2;
            d16[j + 3 * nt] = v3;
        }
        for (; j < nq; j += nt) d16[j] = ld16(j);
    }
    const u64 done = head + 16 * nq;
    if (done + tid < n) dst[done + tid] = src[done + tid];
}

// One workgroup per touched block (k-th of the sorted list, block b of the source): its restart points, parse hints
// and stream to their places in the sub-container.  Runs after k_range_index, whose index it reads.
__device__ __forceinline__ void range_copy_block(const u8* __restrict__ src, const ansx_geo& g, const ansx_range_lay& sl,
    const ansx_range_lay& dl, u32 k, u32 b, u8* __restrict__ dst, u64 cap_pay, u32* __restrict__ flags)
{
    const u32 tid = threadIdx.x;
    const u64* sboff = (const u64*)(dst + 64);
    const u64 d0 = sboff[k], d1 = sboff[k + 1];
    if (d1 <= d0 || d1 > cap_pay) {  // an invalid entry (flagged by k_range_index) or a sum past the workspace
        if (tid == 0 && d1 > cap_pay) atomicOr(&flags[0], 1u << 3);
        return;
    }
    if (g.ckw) {  // wide restart points: u32 cursors, then 4 x u64 states
        range_copy_bytes(dst + dl.ckoff_off + 4ull * k * g.nckf, src + sl.ckoff_off + 4ull * b * g.nckf, 4ull * g.nckf, tid, 256);
        range_copy_bytes(dst + dl.ckstate_off + 32ull * k * g.nckf, src + sl.ckstate_off + 32ull * b * g.nckf, 32ull * g.nckf, tid, 256);
    } else {
        range_copy_bytes(dst + dl.ckoff_off + (u64)ANSX_CK_RECORD * k * g.nckf, src + sl.ckoff_off + (u64)ANSX_CK_RECORD * b * g.nckf,
            (u64)ANSX_CK_RECORD * g.nckf, tid, 256);
    }
    if (tid < 8) ((u32*)(dst + dl.hint_off + 32ull * k))[tid] = ((const u32*)(src + sl.hint_off + 32ull * b))[tid];
    const u64* boff = (const u64*)(src + 64);
    range_copy_bytes(dst + dl.payload_off + d0, src + sl.payload_off + boff[b], d1 - d0, tid, 256);
}

__global__ __launch_bounds__(256) void k_range_copy(const u8* __restrict__ src, ansx_geo g, ansx_range_lay sl,
    ansx_range_lay dl, const u32* __restrict__ tb, u8* __restrict__ dst, u64 cap_pay, u32* __restrict__ flags)
{
    range_copy_block(src, g, sl, dl, blockIdx.x, tb[blockIdx.x], dst, cap_pay, flags);
}

// out[p.dst + i] = sub[p.src + i] for every range piece, nothing if the decode flagged an error: workgroup w takes ints
// [c * CHUNK, (c + 1) * CHUNK) of the range whose pieces cover w (pstart: first piece of each range, pstart[nr] =
// npieces).  16-byte accesses where source and destination agree modulo 16 bytes, dwords otherwise.
__global__ __launch_bounds__(256) void k_range_gather(const u32* __restrict__ sub, const ansx_range_piece* __restrict__ R,
    const u32* __restrict__ pstart, u32 nr, u32 npieces, u32* __restrict__ out, const u32* __restrict__ gflags)
{
    const u32 tid = threadIdx.x;
    if (gflags[ANSX_G_ERR]) return;  // the decode of the sub-container failed: the caller's buffer is not written
    for (u32 p = blockIdx.x; p < npieces; p += gridDim.x) {
        u32 lo = 0, hi = nr;  // the last range with pstart[r] <= p
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (pstart[mid] <= p) lo = mid;
            else hi = mid;
        }
        const ansx_range_piece r = R[lo];
        const u64 off = (u64)(p - pstart[lo]) * ANSX_RANGE_CHUNK;
        const u32 m = (u32)(r.count - off < ANSX_RANGE_CHUNK ? r.count - off : ANSX_RANGE_CHUNK);
        const u32* s = sub + r.src + off;
        u32* d = out + r.dst + off;
        u32 head = (u32)(((16 - ((uintptr_t)d & 15)) & 15) >> 2);
        if (head > m) head = m;
        if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
            if (tid < head) d[tid] = s[tid];
            const u32 nq = (m - head) >> 2;
            const uint4* s16 = (const uint4*)(s + head);
            uint4* d16 = (uint4*)(d + head);
            uint4 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (tid + 256u * q < nq) v[q] = s16[tid + 256u * q];
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (tid + 256u * q < nq) d16[tid + 256u * q] = v[q];
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
}

// ------------------------------------------------------------------------------------------------ device plan
// ansx_decode_device_ranges_dev ("device plan"): the plan the host builds for
// ansx_decode_ranges_dev -- touched blocks tb[T], range pieces, pstart -- built on the device from first / count in
// device memory.  Sorted span j (non-empty ranges by first block b0, last block b1) adds blocks [s_j, b1_j] to the
// union, s_j = max(b0_j, 1 + max b1 of the spans before it); off_j (exclusive sum of the added counts) is its first
// position in tb.  s is non-decreasing, so a touched block b is position off_i + (b - s_i) of the last span i with
// s_i <= b, and tb position k belongs to the last span i with off_i <= k.
//
// Every kernel runs 256 threads over tiles of ANSX_DR_TILE items, 16 consecutive items per thread (in index order, so
// the scans and the radix sort's scatter are stable).  Up to ANSX_DR_TILE ranges one workgroup does it all
// (k_dr_plan_small); beyond, each step is a kernel over ceil(nranges / ANSX_DR_TILE) tiles, and the per-tile partials
// are scanned by one workgroup (k_dr_scan).  Grids scale with nranges, never with the container's block count.
//
// Scalars (u64 sc[8], read back in one copy): 0 sum(count), 1 non-empty ranges, 2 pieces, 3 invalid ranges,
// 4 1 + largest last block, 5 T; the low word of 6 is the tail's format flag.

#define ANSX_DR_NT 256u
#define ANSX_DR_IPT 16u
#define ANSX_DR_TILE (ANSX_DR_NT * ANSX_DR_IPT)
enum { ANSX_DR_TOTAL = 0, ANSX_DR_NNE = 1, ANSX_DR_NPIECES = 2, ANSX_DR_BAD = 3, ANSX_DR_LASTB1 = 4, ANSX_DR_T = 5,
    ANSX_DR_FLAGS = 6 };

// Exclusive scan over the 256 threads of the workgroup under op (identity 0: add, unsigned max); *total = the whole.
// wsum: 4 entries of LDS.  Ends in a barrier, so the next call may reuse wsum.
template <typename T, typename Op> __device__ __forceinline__ T dr_block_excl(T v, T* wsum, u32 tid, T* total, Op op)
{
    const T incl = wave_incl_scan(v, op);
    const u32 w = tid >> 6;
    if ((tid & 63) == 63) wsum[w] = incl;
    T ex = __shfl_up(incl, 1);
    if ((tid & 63) == 0) ex = 0;
    __syncthreads();
    T pre = 0, all = 0;
#pragma unroll
    for (u32 k = 0; k < ANSX_DR_NT / 64; k++) {
        const T x = wsum[k];
        if (k < w) pre = op(pre, x);
        all = op(all, x);
    }
    __syncthreads();
    *total = all;
    return op(pre, ex);
}

// The thread's 16 ranges from index i0 on: count as given for a valid range, 0 for an invalid one (counted in *bad)
// and past nr.
__device__ __forceinline__ void dr_load(const u64* __restrict__ first, const u32* __restrict__ count, u64 nr, u64 n,
    u64 i0, u64 (&f)[ANSX_DR_IPT], u32 (&c)[ANSX_DR_IPT], u32* bad)
{
    u32 nb = 0;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        f[q] = 0;
        c[q] = 0;
        if (i0 + q < nr) {
            const u64 fi = first[i0 + q];
            const u32 ci = count[i0 + q];
            if (fi > n || (u64)ci > n - fi) nb++;
            else {
                f[q] = fi;
                c[q] = ci;
            }
        }
    }
    *bad = nb;
}

__device__ __forceinline__ u64 dr_pieces(u32 c) { return ((u64)c + ANSX_RANGE_CHUNK - 1) / ANSX_RANGE_CHUNK; }

// Stable rank of each of the thread's first nv digits (4 bits each) among the equal digits of the workgroup's items
// in item order: 16 counters of 16 bits in 4 words, scanned across the workgroup (a tile holds at most 4096 items, so
// no field carries into the next).  *tot: the workgroup's counts in the same packing.
__device__ __forceinline__ void dr_rank16(const u32 (&d)[ANSX_DR_IPT], u32 nv, u64* wsum, u32 tid,
    u32 (&pos)[ANSX_DR_IPT], u64 (&tot)[4])
{
    u64 c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (q >= nv) continue;
        const u64 inc = 1ull << (16 * (d[q] & 3));
        const u32 w = d[q] >> 2;
        c0 += w == 0 ? inc : 0;
        c1 += w == 1 ? inc : 0;
        c2 += w == 2 ? inc : 0;
        c3 += w == 3 ? inc : 0;
    }
    c0 = dr_block_excl(c0, wsum, tid, &tot[0], ansx_op_add());
    c1 = dr_block_excl(c1, wsum, tid, &tot[1], ansx_op_add());
    c2 = dr_block_excl(c2, wsum, tid, &tot[2], ansx_op_add());
    c3 = dr_block_excl(c3, wsum, tid, &tot[3], ansx_op_add());
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (q >= nv) continue;
        const u32 sh = 16 * (d[q] & 3), w = d[q] >> 2;
        const u64 p = w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
        pos[q] = (u32)(p >> sh) & 0xFFFFu;
        const u64 inc = 1ull << sh;
        c0 += w == 0 ? inc : 0;
        c1 += w == 1 ? inc : 0;
        c2 += w == 2 ? inc : 0;
        c3 += w == 3 ? inc : 0;
    }
}

// Union step over the thread's nv sorted spans (b0[q], b1p[q] = b1 + 1), cover = 1 + max b1 of every span before
// them: s[q] and the count a[q] of blocks each adds.  Returns the thread's sum of a.
__device__ __forceinline__ u32 dr_union(const u32 (&b0)[ANSX_DR_IPT], const u32 (&b1p)[ANSX_DR_IPT], u32 nv, u32 cover,
    u32 (&s)[ANSX_DR_IPT], u32 (&a)[ANSX_DR_IPT])
{
    u32 sum = 0;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        s[q] = b0[q] > cover ? b0[q] : cover;
        a[q] = q < nv && b1p[q] > s[q] ? b1p[q] - s[q] : 0;
        if (q < nv && b1p[q] > cover) cover = b1p[q];
        sum += a[q];
    }
    return sum;
}

// The last index i in [0, m) with key(i) <= v (key non-decreasing, key(0) <= v)
template <typename F> __device__ __forceinline__ u32 dr_last_le(u32 m, u64 v, F key)
{
    u32 lo = 0, hi = m;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (key(mid) <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Up to ANSX_DR_TILE ranges, the whole plan in one workgroup: validation and the three scans, the radix sort of the
// spans in LDS (kb key bits), the union, the pieces.  S / offl: the union (for k_dr_blocks); parta[0] = 0.
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_plan_small(const u64* __restrict__ first, const u32* __restrict__ count,
    u32 nr, u64 n, u64 bi, u32 kb, u64* __restrict__ offsets, ansx_range_piece* __restrict__ R, u32* __restrict__ pstart,
    u32* __restrict__ S, u32* __restrict__ offl, u64* __restrict__ parta, u64* __restrict__ sc)
{
    __shared__ u32 lk[ANSX_DR_TILE], lv[ANSX_DR_TILE];
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x;
    u64 f[ANSX_DR_IPT];
    u32 c[ANSX_DR_IPT], bad;
    dr_load(first, count, nr, n, (u64)tid * ANSX_DR_IPT, f, c, &bad);
    u64 sc_ = 0, sp = 0;
    u32 sn = 0;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        sc_ += c[q];
        sn += c[q] != 0;
        sp += dr_pieces(c[q]);
    }
    u64 total, nne64, npieces, nbad;
    u64 dst = dr_block_excl(sc_, wsum, tid, &total, ansx_op_add());
    const u32 j0 = (u32)dr_block_excl((u64)sn, wsum, tid, &nne64, ansx_op_add());
    u64 p = dr_block_excl(sp, wsum, tid, &npieces, ansx_op_add());
    (void)dr_block_excl((u64)bad, wsum, tid, &nbad, ansx_op_add());
    const u32 nne = (u32)nne64;
    {
        u32 j = j0;
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) {
            const u32 i = tid * ANSX_DR_IPT + q;
            if (i < nr && offsets) offsets[i] = dst;
            if (c[q]) {
                lk[j] = (u32)(f[q] / bi);
                lv[j] = (u32)((f[q] + c[q] - 1) / bi) + 1u;
                pstart[j] = (u32)p;
                j++;
            }
            dst += c[q];
            p += dr_pieces(c[q]);
        }
    }
    if (tid == 0) {
        if (offsets) offsets[nr] = total;
        pstart[nne] = (u32)npieces;
    }
    __syncthreads();
    const u32 nv = nne > tid * ANSX_DR_IPT ? min(nne - tid * ANSX_DR_IPT, ANSX_DR_IPT) : 0u;
    u32 k0[ANSX_DR_IPT], k1[ANSX_DR_IPT];
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        k0[q] = q < nv ? lk[tid * ANSX_DR_IPT + q] : 0u;
        k1[q] = q < nv ? lv[tid * ANSX_DR_IPT + q] : 0u;
    }
    for (u32 sh = 0; sh < kb && nne > 1; sh += 4) {  // LSD radix sort by b0, 4 bits a pass
        u32 d[ANSX_DR_IPT], pos[ANSX_DR_IPT];
        u64 tot[4];
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) d[q] = (k0[q] >> sh) & 15u;
        dr_rank16(d, nv, wsum, tid, pos, tot);  // (ends in a barrier: every thread holds its items)
        u64 ex[4];  // digit bases: exclusive sums of the 16 digit counts, 4 in a word plus the words before
        u64 carry = 0;
#pragma unroll
        for (u32 w = 0; w < 4; w++) {
            ex[w] = tot[w] * 0x0001000100010000ull + carry * 0x0001000100010001ull;
            carry += (tot[w] * 0x0001000100010001ull) >> 48;
        }
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) {
            if (q >= nv) continue;
            const u32 w = d[q] >> 2;
            const u64 e = w == 0 ? ex[0] : w == 1 ? ex[1] : w == 2 ? ex[2] : ex[3];
            const u32 at = ((u32)(e >> (16 * (d[q] & 3))) & 0xFFFFu) + pos[q];
            lk[at] = k0[q];
            lv[at] = k1[q];
        }
        __syncthreads();
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) {
            k0[q] = q < nv ? lk[tid * ANSX_DR_IPT + q] : 0u;
            k1[q] = q < nv ? lv[tid * ANSX_DR_IPT + q] : 0u;
        }
        __syncthreads();
    }
    u32 mx = 0;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) mx = max(mx, k1[q]);
    u64 lastb1;
    const u32 cover = (u32)dr_block_excl((u64)mx, wsum, tid, &lastb1, ansx_op_max());
    u32 s[ANSX_DR_IPT], a[ANSX_DR_IPT];
    const u32 asum = dr_union(k0, k1, nv, cover, s, a);
    u64 T;
    u32 off = (u32)dr_block_excl((u64)asum, wsum, tid, &T, ansx_op_add());
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (q >= nv) continue;
        const u32 i = tid * ANSX_DR_IPT + q;
        lk[i] = S[i] = s[q];
        lv[i] = offl[i] = off;
        off += a[q];
    }
    __syncthreads();
    dst = dst - sc_;  // back to the thread's first range
    u32 j = j0;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (!c[q]) continue;
        const u64 b0 = f[q] / bi;
        const u32 i = dr_last_le(nne, b0, [&](u32 x) { return (u64)lk[x]; });
        const u64 k = lv[i] + (b0 - lk[i]);
        R[j++] = { k * bi + (f[q] - b0 * bi), dst, (u64)c[q] };
        dst += c[q];
    }
    if (tid == 0) {
        parta[0] = 0;
        sc[ANSX_DR_TOTAL] = total;
        sc[ANSX_DR_NNE] = nne;
        sc[ANSX_DR_NPIECES] = npieces;
        sc[ANSX_DR_BAD] = nbad;
        sc[ANSX_DR_LASTB1] = lastb1;
        sc[ANSX_DR_T] = T;
        sc[ANSX_DR_FLAGS] = 0;
    }
}

// ---- more than ANSX_DR_TILE ranges: one kernel per step, grid = ntiles = ceil(nr / ANSX_DR_TILE)

// Per tile: sum(count), non-empty ranges, pieces, invalid ranges -> part[{0, 1, 2, 3} * ntiles + tile]
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_spans(const u64* __restrict__ first, const u32* __restrict__ count,
    u64 nr, u64 n, u64* __restrict__ part)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x, nt = gridDim.x;
    u64 f[ANSX_DR_IPT];
    u32 c[ANSX_DR_IPT], bad;
    dr_load(first, count, nr, n, (u64)blockIdx.x * ANSX_DR_TILE + tid * ANSX_DR_IPT, f, c, &bad);
    u64 sc_ = 0, sp = 0, sn = 0, t;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        sc_ += c[q];
        sn += c[q] != 0;
        sp += dr_pieces(c[q]);
    }
    (void)dr_block_excl(sc_, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[blockIdx.x] = t;
    (void)dr_block_excl(sn, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[nt + blockIdx.x] = t;
    (void)dr_block_excl(sp, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[2 * nt + blockIdx.x] = t;
    (void)dr_block_excl((u64)bad, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[3 * nt + blockIdx.x] = t;
}

// One workgroup: narr arrays of len values each (stride apart) scanned exclusively in place under + or max; the
// totals to tot[0..narr) when given; *zero = 0 when given.
template <typename T, bool MAX> __global__ __launch_bounds__(ANSX_DR_NT) void k_dr_scan(T* __restrict__ a, u64 len,
    u32 narr, u64 stride, u64* __restrict__ tot, u32* __restrict__ zero)
{
    __shared__ T wsum[4];
    const u32 tid = threadIdx.x;
    auto op = [](T x, T y) { return MAX ? (x > y ? x : y) : x + y; };
    for (u32 r = 0; r < narr; r++) {
        T* x = a + r * stride;
        T carry = 0;
        for (u64 base = 0; base < len; base += ANSX_DR_TILE) {
            const u64 i0 = base + (u64)tid * ANSX_DR_IPT;
            T v[ANSX_DR_IPT], s = 0, all;
#pragma unroll
            for (u32 q = 0; q < ANSX_DR_IPT; q++) {
                v[q] = i0 + q < len ? x[i0 + q] : (T)0;
                s = op(s, v[q]);
            }
            T run;
            if constexpr (MAX) run = op(carry, dr_block_excl(s, wsum, tid, &all, ansx_op_max()));
            else run = op(carry, dr_block_excl(s, wsum, tid, &all, ansx_op_add()));
#pragma unroll
            for (u32 q = 0; q < ANSX_DR_IPT; q++) {
                if (i0 + q < len) x[i0 + q] = run;
                run = op(run, v[q]);
            }
            carry = op(carry, all);
        }
        if (tid == 0 && tot) tot[r] = (u64)carry;
    }
    if (tid == 0 && zero) *zero = 0;
}

// Per tile, with part scanned: offsets, and for every non-empty range j its span keys[j] = b0, vals[j] = b1 + 1,
// its piece R[j] (src = first until k_dr_pieces) and pstart[j]; pstart[nne] and offsets[nr] from the last tile.
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_compact(const u64* __restrict__ first, const u32* __restrict__ count,
    u64 nr, u64 n, u64 bi, const u64* __restrict__ part, const u64* __restrict__ sc, u64* __restrict__ offsets,
    u32* __restrict__ keys, u32* __restrict__ vals, ansx_range_piece* __restrict__ R, u32* __restrict__ pstart)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x, nt = gridDim.x, tile = blockIdx.x;
    const u64 i0 = (u64)tile * ANSX_DR_TILE + tid * ANSX_DR_IPT;
    u64 f[ANSX_DR_IPT];
    u32 c[ANSX_DR_IPT], bad;
    dr_load(first, count, nr, n, i0, f, c, &bad);
    u64 sc_ = 0, sp = 0, sn = 0, t;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        sc_ += c[q];
        sn += c[q] != 0;
        sp += dr_pieces(c[q]);
    }
    u64 dst = part[tile] + dr_block_excl(sc_, wsum, tid, &t, ansx_op_add());
    u64 j = part[nt + tile] + dr_block_excl(sn, wsum, tid, &t, ansx_op_add());
    u64 p = part[2 * nt + tile] + dr_block_excl(sp, wsum, tid, &t, ansx_op_add());
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (i0 + q < nr && offsets) offsets[i0 + q] = dst;
        if (c[q]) {
            keys[j] = (u32)(f[q] / bi);
            vals[j] = (u32)((f[q] + c[q] - 1) / bi) + 1u;
            R[j] = { f[q], dst, (u64)c[q] };
            pstart[j] = (u32)p;
            j++;
        }
        dst += c[q];
        p += dr_pieces(c[q]);
    }
    if (i0 <= nr - 1 && nr - 1 < i0 + ANSX_DR_IPT) {  // the thread of the last range
        if (offsets) offsets[nr] = sc[ANSX_DR_TOTAL];
        pstart[sc[ANSX_DR_NNE]] = (u32)sc[ANSX_DR_NPIECES];
    }
}

// Radix pass, step 1: per tile the counts of the 16 values of key digit (keys >> sh) & 15 -> hist[d * ntiles + tile]
// (digit-major: its exclusive scan is every (digit, tile)'s first output position)
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_digit_count(const u32* __restrict__ keys, const u64* __restrict__ sc,
    u32 sh, u32* __restrict__ hist)
{
    __shared__ u32 h[16];
    const u32 tid = threadIdx.x, nt = gridDim.x;
    const u64 nne = sc[ANSX_DR_NNE];
    if (tid < 16) h[tid] = 0;
    __syncthreads();
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {  // (coalesced: item q * 256 + tid of the tile)
        const u64 i = (u64)blockIdx.x * ANSX_DR_TILE + q * ANSX_DR_NT + tid;
        if (i < nne) atomicAdd(&h[(keys[i] >> sh) & 15u], 1u);
    }
    __syncthreads();
    if (tid < 16) hist[(u64)tid * nt + blockIdx.x] = h[tid];
}

// Radix pass, step 3 (hist scanned): every span to its place, stably
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_digit_scatter(const u32* __restrict__ kin, const u32* __restrict__ vin,
    u32* __restrict__ kout, u32* __restrict__ vout, const u64* __restrict__ sc, u32 sh, const u32* __restrict__ hist)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x, nt = gridDim.x;
    const u64 nne = sc[ANSX_DR_NNE], i0 = (u64)blockIdx.x * ANSX_DR_TILE + tid * ANSX_DR_IPT;
    const u32 nv = nne > i0 ? (u32)min(nne - i0, (u64)ANSX_DR_IPT) : 0u;
    u32 k[ANSX_DR_IPT], v[ANSX_DR_IPT], d[ANSX_DR_IPT], pos[ANSX_DR_IPT];
    u64 tot[4];
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        k[q] = q < nv ? kin[i0 + q] : 0u;
        v[q] = q < nv ? vin[i0 + q] : 0u;
        d[q] = (k[q] >> sh) & 15u;
    }
    dr_rank16(d, nv, wsum, tid, pos, tot);
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (q >= nv) continue;
        const u32 at = hist[(u64)d[q] * nt + blockIdx.x] + pos[q];
        kout[at] = k[q];
        vout[at] = v[q];
    }
}

// Union, step 1: per tile of sorted spans, 1 + the largest last block -> partm[tile]
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_tile_max(const u32* __restrict__ vals, const u64* __restrict__ sc,
    u64* __restrict__ partm)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x;
    const u64 nne = sc[ANSX_DR_NNE];
    u32 mx = 0;
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        const u64 i = (u64)blockIdx.x * ANSX_DR_TILE + q * ANSX_DR_NT + tid;
        if (i < nne) mx = max(mx, vals[i]);
    }
    u64 t;
    (void)dr_block_excl((u64)mx, wsum, tid, &t, ansx_op_max());
    if (tid == 0) partm[blockIdx.x] = t;
}

// Union, step 3 (partm max-scanned): S[j] = s_j, offl[j] = off_j less the tile's carry, the tile's added blocks ->
// parta[tile]
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_adds(const u32* __restrict__ keys, const u32* __restrict__ vals,
    const u64* __restrict__ sc, const u64* __restrict__ partm, u32* __restrict__ S, u32* __restrict__ offl,
    u64* __restrict__ parta)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x;
    const u64 nne = sc[ANSX_DR_NNE], i0 = (u64)blockIdx.x * ANSX_DR_TILE + tid * ANSX_DR_IPT;
    const u32 nv = nne > i0 ? (u32)min(nne - i0, (u64)ANSX_DR_IPT) : 0u;
    u32 b0[ANSX_DR_IPT], b1p[ANSX_DR_IPT], s[ANSX_DR_IPT], a[ANSX_DR_IPT], mx = 0;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        b0[q] = q < nv ? keys[i0 + q] : 0u;
        b1p[q] = q < nv ? vals[i0 + q] : 0u;
        mx = max(mx, b1p[q]);
    }
    u64 t;
    const u64 cov = dr_block_excl((u64)mx, wsum, tid, &t, ansx_op_max());
    const u64 pm = partm[blockIdx.x];
    const u32 asum = dr_union(b0, b1p, nv, (u32)(cov > pm ? cov : pm), s, a);
    u32 off = (u32)dr_block_excl((u64)asum, wsum, tid, &t, ansx_op_add());
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (q >= nv) continue;
        S[i0 + q] = s[q];
        offl[i0 + q] = off;
        off += a[q];
    }
    if (tid == 0) parta[blockIdx.x] = t;
}

// Pieces: R[j].src (= first) -> the range's position in the sub-list; one thread per non-empty range
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_pieces(ansx_range_piece* __restrict__ R, const u64* __restrict__ sc,
    u64 bi, const u32* __restrict__ S, const u32* __restrict__ offl, const u64* __restrict__ parta)
{
    const u64 j = (u64)blockIdx.x * ANSX_DR_NT + threadIdx.x, nne = sc[ANSX_DR_NNE];
    if (j >= nne) return;
    const u64 f = R[j].src, b0 = f / bi;
    const u32 i = dr_last_le((u32)nne, b0, [&](u32 x) { return (u64)S[x]; });
    const u64 k = parta[i / ANSX_DR_TILE] + offl[i] + (b0 - S[i]);
    R[j].src = k * bi + (f - b0 * bi);
}

// After the read-back (T known, grid ceil(T / 256)): tb[k] = the k-th touched block
__global__ __launch_bounds__(ANSX_DR_NT) void k_dr_blocks(u32* __restrict__ tb, u32 T, u32 nne,
    const u32* __restrict__ S, const u32* __restrict__ offl, const u64* __restrict__ parta)
{
    const u32 k = blockIdx.x * ANSX_DR_NT + threadIdx.x;
    if (k >= T) return;
    auto off = [&](u32 x) { return parta[x / ANSX_DR_TILE] + offl[x]; };
    const u32 i = dr_last_le(nne, k, off);
    tb[k] = S[i] + (u32)(k - off(i));
}
