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

struct ansx_range_piece {  // one range with count > 0: where its ints sit in the sub-list and in the output
    u64 src, dst, count;
};

#define ANSX_RANGE_CHUNK 4096u  // ints per workgroup of k_range_gather

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
// the host's image with the payload size filled in.
__global__ __launch_bounds__(1024) void k_range_index(const u8* __restrict__ src, ansx_geo g,
    const u32* __restrict__ tb, u32 T, ansx_container_header hsub, u8* __restrict__ dst, u64 cap_pay,
    u32* __restrict__ flags)
{
    __shared__ u64 part[20];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64* boff = (const u64*)(src + 64);
    u64* sboff = (u64*)(dst + 64);
    const u32 per = ((T + 15) / 16 + 63) & ~63u;  // entries per wave, a multiple of 64
    const u32 lo = wave * per < T ? wave * per : T, hi = (lo + per) < T ? (lo + per) : T;
    u64 sum = 0;
    for (u32 i = lo + lane; i < hi; i += 64) sum += range_block_len(g, boff, tb[i], flags);
    sum = wave_sum(sum);
    u64 total;
    u64 run = block_excl_scan<u64>(lane == 63 ? sum : 0ull, part, tid, 1024, &total);
    run = wave_last(run);
    for (u32 i0 = lo; i0 < hi; i0 += 64) {
        const u32 i = i0 + lane;
        const u64 v = i < hi ? range_block_len(g, boff, tb[i], flags) : 0ull;
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
__global__ __launch_bounds__(256) void k_range_copy(const u8* __restrict__ src, ansx_geo g, ansx_range_lay sl,
    ansx_range_lay dl, const u32* __restrict__ tb, u8* __restrict__ dst, u64 cap_pay, u32* __restrict__ flags)
{
    const u32 k = blockIdx.x, tid = threadIdx.x;
    const u32 b = tb[k];
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
