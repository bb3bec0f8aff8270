// ansx_encbatch.h -- a batch of lists in one call (ansx_encode_batch_dev).
//
// The host cuts the batch, in order and at list boundaries only, into passes of at most P blocks.  A pass is one work
// list of blocks (ansx_geo::bin: each block's ints and where they start in the caller's input), which the ordinary
// encode phases -- histogram, model, prelude, encoder, with their retry ladder -- run over as if it were one list; the
// restart points and parse hints of the pass go to a work area in the wide form.  The two kernels here replace
// k_assemble: k_encb_scan sums the stream sizes per list, decides every list's restart-point form from its own largest
// frame and places the containers back to back on 16-byte boundaries; k_encb_write assembles every container straight
// from the stream scratch into the caller's buffer -- header with the list's own maxima, rebased index, restart points
// in the form the list needs (packed with the inverse of ckpt_load), hints, payload, zeroed padding.
#pragma once

#include "ansx_kernels.h"

// (ansx_encb_list, ansx_encb_max and ansx_encb_res, the tables of a pass's lists, are in ansx_plan_types.h: the host lays
// them out in ansx_plan.h)

struct ansx_encb_args {
    const ansx_blk_in* bin;       // the pass's blocks
    const ansx_encb_list* lists;  // nl + 1 entries
    ansx_encb_max* mx;            // nl entries, zeroed before the pass
    ansx_encb_res* res;           // nl entries, then {valid, total bytes of the pass}
    u64* bsum;                    // NB + 1: stream bytes in front of every block of the pass
    u32 nl;
    u32 ns_cap;                   // the attempt's alphabet assumption (0: none), see k_encb_scan
    u32 forced;                   // the attempt runs on the host's frame decisions (resolve_near): close calls do not hold it back
    u32 must_wide;                // the geometry or the options ask for wide restart points in every container
    u32 wide_at;                  // frames above 2^this need them
    u64 base, cap;                // the pass starts at byte `base` of the caller's buffer of `cap` bytes
    // the pass's restart points (wide form) and parse hints in the work area
    const u32* w_ckoff;
    const u64* w_ckstate;
    const u32* w_hints;
};

// make_plan's container layout for a list of nbk blocks (layout_of in ansx.hip)
struct ansx_encb_lay {
    u64 ckoff_off, ckstate_off, hint_off, payload_off;
};
__device__ __forceinline__ ansx_encb_lay encb_layout(u32 nbk, u32 nckf, bool wide)
{
    ansx_encb_lay L;
    const u64 nck = (u64)nbk * nckf;
    L.ckoff_off = 64 + 8 * ((u64)nbk + 1);
    if (wide) {
        L.ckstate_off = (L.ckoff_off + 4 * nck + 7) & ~7ull;
        L.hint_off = (L.ckstate_off + 32 * nck + 15) & ~15ull;
    } else {
        L.ckstate_off = L.ckoff_off;
        L.hint_off = (L.ckoff_off + (u64)ANSX_CK_RECORD * nck + 15) & ~15ull;
    }
    L.payload_off = L.hint_off + 32 * (u64)nbk;
    return L;
}

// One workgroup.  Phase 1: exclusive scan of the stream sizes over the pass's blocks, and every list's maxima.
// Phase 2: per list its restart-point form, container size and offset (a scan of the sizes rounded up to 16).
// res[nl] = {valid, total}: valid = 0 when the attempt will be refused by the host (an error flag, a hint that did not
// hold, no room) or repeated by it (close calls of the stop rule) -- k_encb_write then writes nothing, so a refused
// or repeated attempt never touches the caller's buffer.
__global__ __launch_bounds__(1024) void k_encb_scan(ansx_geo g, ansx_encb_args A, const ansx_blk* __restrict__ blk,
    const u32* __restrict__ sizes, u64* __restrict__ result, u32* __restrict__ gflags)
{
    __shared__ u64 part[20];
    const u32 tid = threadIdx.x;
    const u32 NB = g.nblocks;
    u64 carry = 0;
    for (u32 b0 = 0; b0 < NB; b0 += 1024) {
        const u32 b = b0 + tid;
        u64 v = 0;
        if (b < NB) {
            v = sizes[b];
            const ansx_blk* B = &blk[b];
            // (a one-value block of the compaction layer is marked resolved but has no model: as in the call's own maxima,
            // k_select_model, it does not count)
            if (!B->status && B->resolved && B->pa_sigma != 1) {
                ansx_encb_max* m = &A.mx[A.bin[b].list];
                atomicMax(&m->logM, B->logM);
                atomicMax(&m->ns, B->max_sym + 1u);
                atomicMax(&m->sigma, B->sigma);
            }
        }
        u64 tot;
        const u64 ex = block_excl_scan<u64>(v, part, tid, 1024, &tot);
        if (b < NB) A.bsum[b] = carry + ex;
        carry += tot;
        __syncthreads();  // (part is reused)
    }
    if (tid == 0) A.bsum[NB] = carry;
    __threadfence();
    __syncthreads();
    u64 run = 0;
    for (u32 i0 = 0; i0 < A.nl; i0 += 1024) {
        const u32 i = i0 + tid;
        u64 r16 = 0, bytes = 0;
        if (i < A.nl) {
            const u32 fb = A.lists[i].fb, fe = A.lists[i + 1].fb;
            const u32 mlog = __hip_atomic_load(&A.mx[i].logM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool wide = A.must_wide || (g.nckf != 0 && mlog > A.wide_at);
            A.mx[i].wide = wide ? 1u : 0u;
            const u64 pay = __hip_atomic_load(&A.bsum[fe], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                - __hip_atomic_load(&A.bsum[fb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bytes = encb_layout(fe - fb, g.nckf, wide).payload_off + pay;
            r16 = (bytes + 15) & ~15ull;
        }
        u64 tot;
        const u64 ex = block_excl_scan<u64>(r16, part, tid, 1024, &tot);
        if (i < A.nl) {
            A.res[i].off = A.base + run + ex;
            A.res[i].bytes = bytes;
        }
        run += tot;
        __syncthreads();
    }
    if (tid == 0) {
        const bool fits = A.base + run <= A.cap;
        if (!fits) atomicOr(&gflags[ANSX_G_ERR], 1u << 2 /* CAPACITY */);
        const u32 err = __hip_atomic_load(&gflags[ANSX_G_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (the host's own conditions, encode_finish: the status bits; on an optimistic attempt also its assumptions)
        bool ok = fits && (err & ((1u << 6) | (1u << 7) | (1u << 2) | (1u << 3))) == 0;
        if (A.ns_cap != 0)
            ok = ok && (err & (1u << ANSX_G_VIOL_BIT)) == 0
                && __hip_atomic_load(&gflags[ANSX_G_PAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0
                && __hip_atomic_load(&gflags[ANSX_G_MAXLOGM], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 16
                && __hip_atomic_load(&gflags[ANSX_G_MAXNSYMS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= A.ns_cap;
        // close calls of the stop rule: the host looks at them first and repeats the pass on its decisions
        if (!A.forced) ok = ok && __hip_atomic_load(&gflags[ANSX_G_NEAR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
        A.res[A.nl].off = ok ? 1 : 0;
        A.res[A.nl].bytes = run;
        result[0] = carry;  // payload bytes of the pass
    }
}

// One workgroup per block of the pass: its stream, index entry, restart points and hints into its list's container;
// the workgroup of a list's first block also writes the header and zeroes the layout's gaps and the padding behind
// the container.
__global__ __launch_bounds__(256) void k_encb_write(ansx_geo g, ansx_encb_args A, const u32* __restrict__ sizes,
    const u8* __restrict__ scratch, u64 scr_stride, u8* __restrict__ out)
{
    if (A.res[A.nl].off == 0) return;
    const u32 b = blockIdx.x, tid = threadIdx.x;
    const u32 li = A.bin[b].list;
    const u32 fb = A.lists[li].fb, fe = A.lists[li + 1].fb;
    const u32 nbk = fe - fb, j = b - fb;
    const ansx_encb_max mx = A.mx[li];
    const bool wide = mx.wide != 0;
    const ansx_encb_lay L = encb_layout(nbk, g.nckf, wide);
    const u64 bytes = A.res[li].bytes;
    u8* dst = out + A.res[li].off;  // (16-byte aligned)
    const u64 boff = A.bsum[b] - A.bsum[fb];
    const u32 size = sizes[b];
    u64* index = (u64*)(dst + 64);
    if (tid == 0) {
        index[j] = boff;
        if (j == nbk - 1) index[nbk] = boff + size;
    }
    // restart points: all nckf slots of the block (slots a short block does not use are zero in the work area)
    for (u32 t = tid; t < g.nckf; t += 256) {
        const u64 si = (u64)b * g.nckf + t, di = (u64)j * g.nckf + t;
        const u32 cur = A.w_ckoff[si];
        const u64 s0 = A.w_ckstate[si * 4], s1 = A.w_ckstate[si * 4 + 1], s2 = A.w_ckstate[si * 4 + 2], s3 = A.w_ckstate[si * 4 + 3];
        if (wide) {
            ((u32*)(dst + L.ckoff_off))[di] = cur;
            u64* st = (u64*)(dst + L.ckstate_off) + di * 4;
            st[0] = s0, st[1] = s1, st[2] = s2, st[3] = s3;
        } else {
            // packed record (ansx_dev.h, the inverse of ckpt_load): two states per 104-bit integer, then the 24-bit cursor
            u8* rec = dst + L.ckoff_off + di * ANSX_CK_RECORD;
            const u64 mask = (1ull << ANSX_CK_STATE_BITS) - 1ull;
            st_u64_unaligned(rec, (s0 & mask) | (s1 << ANSX_CK_STATE_BITS));
            st_u32_unaligned(rec + 8, (u32)(s1 >> 12));
            rec[12] = (u8)(s1 >> 44);
            st_u64_unaligned(rec + 13, (s2 & mask) | (s3 << ANSX_CK_STATE_BITS));
            st_u32_unaligned(rec + 21, (u32)(s3 >> 12));
            rec[25] = (u8)(s3 >> 44);
            st_u16_unaligned(rec + 26, (u16)cur);
            rec[28] = (u8)(cur >> 16);
        }
    }
    if (tid < 8) ((u32*)(dst + L.hint_off))[(u64)j * 8 + tid] = A.w_hints[(u64)b * 8 + tid];
    if (j == 0) {
        if (tid == 0) {
            // ansx_container_header, little endian (include/ansx.h), as k_assemble writes it
            const char magic[8] = { 'A', 'N', 'S', 'X', 'v', '3', 0, 0 };
            for (int i = 0; i < 6; i++) dst[i] = (u8)magic[i];
            *(u16*)(dst + 6) = (u16)(mx.sigma ? mx.sigma - 1u : 0u);
            u32* w = (u32*)(dst + 8);
            w[0] = g.kind | (g.pa ? 0x100u : 0u) | (wide ? ANSX_KIND_WIDE_RESTART : 0u);
            w[1] = g.f;
            *(u64*)(dst + 16) = A.lists[li].n;
            w = (u32*)(dst + 24);
            w[0] = g.block_ints;
            w[1] = g.ckpt;
            w[2] = nbk;
            w[3] = mx.logM;
            w[4] = mx.ns;
            w[5] = g.nckf;
            *(u64*)(dst + 48) = A.bsum[fe] - A.bsum[fb];
            *(u64*)(dst + 56) = L.payload_off;
        }
        // the layout's alignment gaps and the padding up to the next container: fewer than 8 + 16 + 16 bytes
        const u64 nck = (u64)nbk * g.nckf;
        const u64 g0 = wide ? L.ckoff_off + 4 * nck : L.hint_off, g0e = wide ? L.ckstate_off : L.hint_off;
        const u64 g1 = wide ? L.ckstate_off + 32 * nck : L.ckoff_off + (u64)ANSX_CK_RECORD * nck, g1e = L.hint_off;
        const u64 g2 = bytes, g2e = (bytes + 15) & ~15ull;
        if (g0 + tid < g0e) dst[g0 + tid] = 0;
        if (g1 + tid < g1e) dst[g1 + tid] = 0;
        if (g2 + tid < g2e) dst[g2 + tid] = 0;
    }
    if (size == 0) return;
    const u8* src = scratch + (u64)b * scr_stride;
    u8* pd = dst + L.payload_off + boff;
    // as k_assemble: bytes until pd is 16-byte aligned, then 16-byte pieces
    u32 head = (u32)((16 - ((uintptr_t)pd & 15)) & 15);
    if (head > size) head = size;
    if (tid < head) pd[tid] = src[tid];
    const u32 nq = (size - head) >> 4;
    uint4* d16 = (uint4*)(pd + head);
    const u8* s1 = src + head;
    auto ld16 = [&](u32 q) {
        const u8* p = s1 + 16 * (u64)q;
        return make_uint4(ld_u32_unaligned(p), ld_u32_unaligned(p + 4), ld_u32_unaligned(p + 8), ld_u32_unaligned(p + 12));
    };
    u32 q = tid;
    for (; q + 3 * 256 < nq; q += 4 * 256) {
        const uint4 v0 = ld16(q), v1 = ld16(q + 256), v2 = ld16(q + 512), v3 = ld16(q + 768);
        d16[q] = v0;
        d16[q + 256] = v1;
        d16[q + 512] = v2;
        d16[q + 768] = v3;
    }
    for (; q < nq; q += 256) d16[q] = ld16(q);
    const u32 done = head + 16 * nq;
    if (done + tid < size) pd[done + tid] = src[done + tid];
}
