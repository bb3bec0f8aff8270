// ansx_batchdevranges.h -- ranges of a batch with (src, first, count) in device memory
// (ansx_decode_batch_device_ranges_dev, DESIGN.md section 3d, "device plan").  gfx950 only.
//
// What ansx_decode_batch_ranges_dev plans on the host (ansx_plan.h: br_refs, br_runs, br_pieces) is planned here, so
// that nothing on the host grows with the number of ranges:
//   front    k_bdr_mark: a lane per range checks src < count and its container's pointers (atomicMin of the failing
//            index) and marks the container; k_bdr_slots: one workgroup scans the marks into every container's slot and
//            the list of the referenced ones, whose headers k_batch_headers then brings home.
//   plan     The host lays the referenced containers end to end, group after group (ansx_plan_types.h, ansx_bdr_ref):
//            a range is a span of GLOBAL blocks, and section 3a's planner applies as it stands -- k_bdr_spans,
//            k_bdr_compact in the place of k_dr_spans, k_dr_compact; the radix sort, the union and the scans are
//            ansx_ranges.h's own kernels (k_dr_digit_count, k_dr_digit_scatter, k_dr_tile_max, k_dr_adds, k_dr_scan).
//            k_bdr_k0 finds every range's first entry of tb, k_bdr_groups every group's, k_bdr_blocks writes tb, and
//            k_bdr_pass_blocks / k_bdr_pass_pieces sum every pass's scalars (ansx_bdr_pass) for the one read-back.
//   a pass   k_bdr_pass_table writes the B and O tables of the pass's entries of tb, k_bdr_piece_part / k_dr_scan /
//            k_bdr_piece_put the pieces of the ranges that cross it and their prefix; k_batch_index, k_batch_copy, the
//            decode and k_piece_gather follow as in a pass of the host-array call.
// Every kernel runs 256 threads; those that scan take tiles of ANSX_DR_TILE items, 16 consecutive ones per thread.
#pragma once

#include "ansx_batchranges.h"

// the planner's scalars: ANSX_DR_TOTAL, _NNE, _LASTB1, _T, _FLAGS as in ansx_ranges.h, and the smallest failing range
enum { ANSX_BDR_BADRANGE = 7, ANSX_BDR_SCALARS = 8 };
// the front's scalars
enum { ANSX_BDR_F_BADSRC = 0, ANSX_BDR_F_BADPTR = 1, ANSX_BDR_F_NREF = 2, ANSX_BDR_F_SCALARS = 8 };

ANSX_D void bdr_min(u64* p, u64 v) { atomicMin((unsigned long long*)p, (unsigned long long)v); }
ANSX_D void bdr_add(u64* p, u64 v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// ------------------------------------------------------------------------------------------------ front
// A lane per range: src < count, the named container's pointers, its mark.  bases: null for the plain call.
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_mark(const u32* __restrict__ src, u64 nr, u32 count,
    const u64* __restrict__ addr, const u64* __restrict__ bases, u32* __restrict__ mark, u64* __restrict__ fs)
{
    const u64 i = (u64)blockIdx.x * ANSX_DR_NT + threadIdx.x;
    if (i >= nr) return;
    const u32 s = src[i];
    if (s >= count) {
        bdr_min(&fs[ANSX_BDR_F_BADSRC], i);
        return;
    }
    mark[s] = 1u;
    const u64 a = addr[s];
    bool bad = !a || (a & 15u);
    if (bases) {
        const u64 b = bases[s];
        bad = bad || !b || (b & 3u);
    }
    if (bad) bdr_min(&fs[ANSX_BDR_F_BADPTR], i);
}

// One workgroup: slot[j] = the marked containers before j; the marked ones to ref[], with the address their header is
// read from (0 for an input too short to hold one, as batch_headers passes it); their number.  4 bytes of mark per
// container are read, no container.
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_slots(const u32* __restrict__ mark, u32 count, const u64* __restrict__ addr,
    const u64* __restrict__ inb, u32* __restrict__ slot, u32* __restrict__ ref, u64* __restrict__ refaddr, u64* __restrict__ fs)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x;
    u64 carry = 0;
    for (u64 base = 0; base < count; base += ANSX_DR_TILE) {
        const u64 i0 = base + (u64)tid * ANSX_DR_IPT;
        u32 m[ANSX_DR_IPT];
        u64 sum = 0, all;
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) {
            m[q] = i0 + q < count ? mark[i0 + q] : 0u;
            sum += m[q];
        }
        u64 run = carry + dr_block_excl(sum, wsum, tid, &all, ansx_op_add());
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) {
            if (i0 + q >= count) continue;
            slot[i0 + q] = (u32)run;
            if (m[q]) {
                ref[run] = (u32)(i0 + q);
                refaddr[run] = inb[i0 + q] >= 64 ? addr[i0 + q] : 0;
                run++;
            }
        }
        carry += all;
    }
    if (tid == 0) fs[ANSX_BDR_F_NREF] = carry;
}

// ------------------------------------------------------------------------------------------------ plan
// The thread's 16 ranges from index i0 on: the referenced container, first and count of a valid one; count 0 for an
// invalid one (its index to sc's minimum when sc is given) and past nr.
ANSX_D void bdr_load(const u32* __restrict__ src, const u64* __restrict__ first, const u32* __restrict__ cnt, u64 nr,
    const u32* __restrict__ slot, const u32* __restrict__ rmap, const ansx_bdr_ref* __restrict__ R, u64 i0,
    u64 (&f)[ANSX_DR_IPT], u32 (&c)[ANSX_DR_IPT], u32 (&r)[ANSX_DR_IPT], u64* __restrict__ sc)
{
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        f[q] = 0, c[q] = 0, r[q] = 0;
        if (i0 + q >= nr) continue;
        const u32 rr = rmap[slot[src[i0 + q]]];
        const u64 n = R[rr].n, fi = first[i0 + q];
        const u32 ci = cnt[i0 + q];
        if (fi > n || (u64)ci > n - fi) {
            if (sc) bdr_min(&sc[ANSX_BDR_BADRANGE], i0 + q);
        } else f[q] = fi, c[q] = ci, r[q] = rr;
    }
}

// Per tile: sum(count) and the non-empty ranges -> part[{0, 1} * ntiles + tile]; the smallest invalid range
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_spans(const u32* __restrict__ src, const u64* __restrict__ first,
    const u32* __restrict__ cnt, u64 nr, const u32* __restrict__ slot, const u32* __restrict__ rmap,
    const ansx_bdr_ref* __restrict__ R, u64* __restrict__ part, u64* __restrict__ sc)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x, nt = gridDim.x;
    u64 f[ANSX_DR_IPT];
    u32 c[ANSX_DR_IPT], r[ANSX_DR_IPT];
    bdr_load(src, first, cnt, nr, slot, rmap, R, (u64)blockIdx.x * ANSX_DR_TILE + tid * ANSX_DR_IPT, f, c, r, sc);
    u64 sc_ = 0, sn = 0, t;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        sc_ += c[q];
        sn += c[q] != 0;
    }
    (void)dr_block_excl(sc_, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[blockIdx.x] = t;
    (void)dr_block_excl(sn, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[nt + blockIdx.x] = t;
}

// Per tile, with part scanned: the offsets, and for every non-empty range j, in range order, its span of global blocks
// keys[j] = first, vals[j] = last + 1, and its record (k0 is k_bdr_k0's)
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_compact(const u32* __restrict__ src, const u64* __restrict__ first,
    const u32* __restrict__ cnt, u64 nr, const u32* __restrict__ slot, const u32* __restrict__ rmap,
    const ansx_bdr_ref* __restrict__ R, const ansx_bdr_group* __restrict__ G, const u64* __restrict__ part,
    const u64* __restrict__ sc, u64* __restrict__ offsets, u32* __restrict__ keys, u32* __restrict__ vals,
    ansx_bdr_range* __restrict__ rng)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x, nt = gridDim.x, tile = blockIdx.x;
    const u64 i0 = (u64)tile * ANSX_DR_TILE + tid * ANSX_DR_IPT;
    u64 f[ANSX_DR_IPT];
    u32 c[ANSX_DR_IPT], r[ANSX_DR_IPT];
    bdr_load(src, first, cnt, nr, slot, rmap, R, i0, f, c, r, nullptr);
    u64 sc_ = 0, sn = 0, t;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        sc_ += c[q];
        sn += c[q] != 0;
    }
    u64 dst = part[tile] + dr_block_excl(sc_, wsum, tid, &t, ansx_op_add());
    u64 j = part[nt + tile] + dr_block_excl(sn, wsum, tid, &t, ansx_op_add());
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (i0 + q < nr && offsets) offsets[i0 + q] = dst;
        if (c[q]) {
            const ansx_bdr_ref rec = R[r[q]];
            u32 gb0, gb1p;
            bdr_span(f[q], c[q], G[rec.group].bi, rec.gbase, &gb0, &gb1p);
            keys[j] = gb0;
            vals[j] = gb1p;
            rng[j] = { f[q], dst, c[q], r[q], 0u, 0u };
            j++;
        }
        dst += c[q];
    }
    if (offsets && i0 <= nr - 1 && nr - 1 < i0 + ANSX_DR_IPT) offsets[nr] = sc[ANSX_DR_TOTAL];  // the thread of the last range
}

// With the union done (S, offl, parta: k_dr_adds and its scan): every non-empty range's first entry of tb
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_k0(ansx_bdr_range* __restrict__ rng, const u64* __restrict__ sc,
    const ansx_bdr_ref* __restrict__ R, const ansx_bdr_group* __restrict__ G, const u32* __restrict__ S,
    const u32* __restrict__ offl, const u64* __restrict__ parta)
{
    const u64 j = (u64)blockIdx.x * ANSX_DR_NT + threadIdx.x, nne = sc[ANSX_DR_NNE];
    if (j >= nne) return;
    const ansx_bdr_ref rec = R[rng[j].r];
    const u32 gb0 = rec.gbase + (u32)(rng[j].first / G[rec.group].bi);
    const u32 i = dr_last_le((u32)nne, gb0, [&](u32 x) { return (u64)S[x]; });
    rng[j].k0 = (u32)(parta[i / ANSX_DR_TILE] + offl[i]) + (gb0 - S[i]);
}

// A lane per group (and one behind the last): tg[g] = the touched blocks below the group's first global block -- the
// position in tb of the first sorted span that starts in it (no span crosses a container, so none crosses a group);
// tg[ng] = T
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_groups(const ansx_bdr_group* __restrict__ G, u32 ng, const u32* __restrict__ keys,
    const u32* __restrict__ offl, const u64* __restrict__ parta, const u64* __restrict__ sc, u64* __restrict__ tg)
{
    const u32 g = blockIdx.x * ANSX_DR_NT + threadIdx.x;
    if (g > ng) return;
    const u32 nne = (u32)sc[ANSX_DR_NNE];
    u32 lo = nne;
    if (g < ng) lo = bdr_lower_bound(keys, nne, G[g].gbase);
    tg[g] = lo < nne ? parta[lo / ANSX_DR_TILE] + offl[lo] : sc[ANSX_DR_T];
}

// tb[k] = the k-th touched global block (k_dr_blocks with T on the device: the grid is the host's bound, in strides)
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_blocks(u32* __restrict__ tb, const u64* __restrict__ sc,
    const u32* __restrict__ S, const u32* __restrict__ offl, const u64* __restrict__ parta)
{
    const u64 T = sc[ANSX_DR_T];
    const u32 nne = (u32)sc[ANSX_DR_NNE];
    auto off = [&](u32 x) { return parta[x / ANSX_DR_TILE] + offl[x]; };
    for (u64 k = (u64)blockIdx.x * ANSX_DR_NT + threadIdx.x; k < T; k += (u64)gridDim.x * ANSX_DR_NT) {
        const u32 i = dr_last_le(nne, k, off);
        tb[k] = S[i] + (u32)(k - off(i));
    }
}

// v added to ps[slot].*field for every thread with slot != ~0: once per workgroup where all its threads agree on the slot
// (the common case: a pass holds thousands of entries; adds to ONE address from every wave of a large grid would run
// one after the other), thread by thread otherwise.  Called by all 256 threads; ends in a barrier.
template <class Field> ANSX_D void bdr_group_add(ansx_bdr_pass* __restrict__ ps, u32 slot, u64 v, u64* wsum, u32* agree, Field field)
{
    const u32 tid = threadIdx.x;
    if (tid == 0) agree[0] = slot, agree[1] = 1u;
    __syncthreads();
    const u32 s0 = agree[0];
    if (slot != s0) agree[1] = 0u;  // (a thread without a slot disagrees with one that has one: both paths below are right then)
    __syncthreads();
    const bool same = agree[1] != 0u;
    u64 all;
    (void)dr_block_excl(same ? v : (u64)0, wsum, tid, &all, ansx_op_add());  // (ends in a barrier: agree may be rewritten)
    if (same) {
        if (tid == 0 && s0 != 0xFFFFFFFFu && all) bdr_add(field(&ps[s0]), all);
    } else if (slot != 0xFFFFFFFFu && v) bdr_add(field(&ps[slot]), v);
}

// The pass scalars that follow the blocks: a lane per entry of tb adds its ints, rounded up to 4, to its pass's work
// list; the last entry of a pass leaves its length; the first entry of a (pass, container) run adds that source's
// share of the payload bound.
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_pass_blocks(const u32* __restrict__ tb, const u64* __restrict__ sc,
    const ansx_bdr_ref* __restrict__ R, u32 nref, const ansx_bdr_group* __restrict__ G, const u64* __restrict__ tg, u32 PB,
    ansx_bdr_pass* __restrict__ ps)
{
    __shared__ u64 wsum[4];
    __shared__ u32 agree[2];
    const u64 T = sc[ANSX_DR_T];
    for (u64 base = (u64)blockIdx.x * ANSX_DR_NT; base < T; base += (u64)gridDim.x * ANSX_DR_NT) {  // (the same trips for a whole workgroup)
        const u64 k64 = base + threadIdx.x;
        u32 slot = 0xFFFFFFFFu;
        u64 wl = 0, cp = 0;
        if (k64 < T) {
            const u32 k = (u32)k64, gb = tb[k];
            const ansx_bdr_ref rec = R[bdr_ref_of(R, nref, gb)];
            const ansx_bdr_group grp = G[rec.group];
            const u32 t0 = (u32)tg[rec.group], t1 = (u32)tg[rec.group + 1];
            const u32 p = bdr_pass_of(k, t0, PB), ka = bdr_pass_first(p, t0, PB);
            const u32 kb = (u64)ka + PB < t1 ? ka + PB : t1;
            const u32 nk = bdr_block_ints(rec.n, grp.bi, gb - rec.gbase);
            slot = grp.pslot + p;
            wl = bdr_rup4(nk);
            if (k + 1 == kb) ps[slot].last_n = nk;
            if (k == ka || tb[k - 1] < rec.gbase) {
                u32 e = bdr_lower_bound(tb, (u32)T, rec.gbase + rec.nblocks);
                if (e > kb) e = kb;
                cp = bdr_src_bound(rec.payload_bytes, e - k, grp.bbound);
            }
        }
        bdr_group_add(ps, slot, wl, wsum, agree, [](ansx_bdr_pass* p) { return &p->wl; });
        bdr_group_add(ps, slot, cp, wsum, agree, [](ansx_bdr_pass* p) { return &p->cap_pay; });
    }
}

// The pass scalars that follow the ranges: a piece and its ints to every pass a non-empty range crosses.  A tile of
// ANSX_DR_TILE ranges per workgroup, 16 consecutive ones per thread: a thread sums what goes to the pass of its first
// range, and the workgroup adds once where all its threads ended on the same pass.
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_pass_pieces(const ansx_bdr_range* __restrict__ rng, const u64* __restrict__ sc,
    const ansx_bdr_ref* __restrict__ R, const ansx_bdr_group* __restrict__ G, const u64* __restrict__ tg, u32 PB,
    ansx_bdr_pass* __restrict__ ps)
{
    __shared__ u64 wsum[4];
    __shared__ u32 agree[2];
    const u64 nne = sc[ANSX_DR_NNE], j0 = (u64)blockIdx.x * ANSX_DR_TILE + threadIdx.x * ANSX_DR_IPT;
    u32 slot = 0xFFFFFFFFu;  // the pass the thread is summing for
    u64 ints = 0, np = 0;
    for (u32 q = 0; q < ANSX_DR_IPT && j0 + q < nne; q++) {
        const ansx_bdr_range g = rng[j0 + q];
        const ansx_bdr_group grp = G[R[g.r].group];
        const u32 t0 = (u32)tg[R[g.r].group], t1 = (u32)tg[R[g.r].group + 1];
        const u32 k1 = g.k0 + ((u32)((g.first + g.count - 1) / grp.bi) - (u32)(g.first / grp.bi));
        const u32 p0 = bdr_pass_of(g.k0, t0, PB), p1 = bdr_pass_of(k1, t0, PB);
        if (p0 == p1 && (slot == 0xFFFFFFFFu || slot == grp.pslot + p0)) {
            slot = grp.pslot + p0, ints += g.count, np++;
            continue;
        }
        for (u32 p = p0; p <= p1; p++) {  // (a range across passes, or in another pass than the thread's first)
            const u32 ka = bdr_pass_first(p, t0, PB), kb = (u64)ka + PB < t1 ? ka + PB : t1;
            u64 start;
            u32 k, b;
            const u32 m = bdr_piece(g, grp.bi, ka, kb, &start, &k, &b);
            bdr_add(&ps[grp.pslot + p].np, 1);
            bdr_add(&ps[grp.pslot + p].ints, m);
        }
    }
    bdr_group_add(ps, slot, ints, wsum, agree, [](ansx_bdr_pass* p) { return &p->ints; });
    bdr_group_add(ps, slot, np, wsum, agree, [](ansx_bdr_pass* p) { return &p->np; });
}

// ------------------------------------------------------------------------------------------------ a pass
// One workgroup: the pass's entries tbp[0 .. T) of tb -> its blocks B (src: the referenced container, whose
// ansx_batch_src the call holds at that index) and its table O, a block's ints from the exclusive sum of the lengths
// before it, each rounded up to 4 -- the work list br_runs lays out; the pass's flag words zeroed.
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_pass_table(const u32* __restrict__ tbp, u32 T, const ansx_bdr_ref* __restrict__ R,
    u32 nref, u32 bi, u32* __restrict__ flags, ansx_batch_blk* __restrict__ B, ansx_blk_out* __restrict__ O)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x;
    if (tid < 4) flags[tid] = 0;
    u64 carry = 0;
    for (u32 base = 0; base < T; base += ANSX_DR_TILE) {
        const u32 i0 = base + tid * ANSX_DR_IPT;
        u32 r[ANSX_DR_IPT], b[ANSX_DR_IPT], nk[ANSX_DR_IPT];
        u64 sum = 0, all;
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) {
            r[q] = b[q] = nk[q] = 0;
            if (i0 + q < T) {
                const u32 gb = tbp[i0 + q];
                r[q] = bdr_ref_of(R, nref, gb);
                b[q] = gb - R[r[q]].gbase;
                nk[q] = bdr_block_ints(R[r[q]].n, bi, b[q]);
            }
            sum += bdr_rup4(nk[q]);
        }
        u64 run = carry + dr_block_excl(sum, wsum, tid, &all, ansx_op_add());
#pragma unroll
        for (u32 q = 0; q < ANSX_DR_IPT; q++) {
            if (i0 + q >= T) continue;
            B[i0 + q] = { r[q], b[q] };
            O[i0 + q] = { run, nk[q], 0u };
            run += bdr_rup4(nk[q]);
        }
        carry += all;
    }
}

// The thread's 16 non-empty ranges from j0 on against the pass [ka, kb): the ints m[q] of each one's piece (0: none),
// where it starts in its container, and its first entry of tb and block
ANSX_D void bdr_pieces_of(const ansx_bdr_range* __restrict__ rng, u64 nne, u64 j0, const ansx_bdr_ref* __restrict__ R,
    const ansx_bdr_group* __restrict__ G, u32 ka, u32 kb, u32 (&m)[ANSX_DR_IPT], u64 (&start)[ANSX_DR_IPT],
    u32 (&k)[ANSX_DR_IPT], u32 (&b)[ANSX_DR_IPT], u32 (&bi)[ANSX_DR_IPT])
{
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        m[q] = 0, start[q] = 0, k[q] = 0, b[q] = 0, bi[q] = 1;
        if (j0 + q >= nne) continue;
        const ansx_bdr_range g = rng[j0 + q];
        bi[q] = G[R[g.r].group].bi;  // (its own group's: k0 counts in tb, whichever group the pass belongs to)
        m[q] = bdr_piece(g, bi[q], ka, kb, &start[q], &k[q], &b[q]);
    }
}

// Per tile of non-empty ranges: the pieces of the pass and their ints -> part[{0, 1} * ntiles + tile]
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_piece_part(const ansx_bdr_range* __restrict__ rng, const u64* __restrict__ sc,
    const ansx_bdr_ref* __restrict__ R, const ansx_bdr_group* __restrict__ G, u32 ka, u32 kb, u64* __restrict__ part)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x, nt = gridDim.x;
    u32 m[ANSX_DR_IPT], k[ANSX_DR_IPT], b[ANSX_DR_IPT], bi[ANSX_DR_IPT];
    u64 start[ANSX_DR_IPT];
    bdr_pieces_of(rng, sc[ANSX_DR_NNE], (u64)blockIdx.x * ANSX_DR_TILE + tid * ANSX_DR_IPT, R, G, ka, kb, m, start, k, b, bi);
    u64 sp = 0, si = 0, t;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        sp += m[q] != 0;
        si += m[q];
    }
    (void)dr_block_excl(sp, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[blockIdx.x] = t;
    (void)dr_block_excl(si, wsum, tid, &t, ansx_op_add());
    if (tid == 0) part[nt + blockIdx.x] = t;
}

// Per tile, with part scanned: the pass's pieces in range order -- src in the pass's work list (O: its table), dst in
// the caller's buffer -- and wpos, the exclusive prefix of their ints; wpos[np] = the pass's ints
__global__ __launch_bounds__(ANSX_DR_NT) void k_bdr_piece_put(const ansx_bdr_range* __restrict__ rng, const u64* __restrict__ sc,
    const ansx_bdr_ref* __restrict__ R, const ansx_bdr_group* __restrict__ G, u32 ka, u32 kb, const u64* __restrict__ part,
    const ansx_blk_out* __restrict__ O, ansx_piece* __restrict__ P, u64* __restrict__ wpos, u64 np, u64 ints)
{
    __shared__ u64 wsum[4];
    const u32 tid = threadIdx.x, nt = gridDim.x, tile = blockIdx.x;
    const u64 j0 = (u64)tile * ANSX_DR_TILE + tid * ANSX_DR_IPT;
    u32 m[ANSX_DR_IPT], k[ANSX_DR_IPT], b[ANSX_DR_IPT], bi[ANSX_DR_IPT];
    u64 start[ANSX_DR_IPT];
    bdr_pieces_of(rng, sc[ANSX_DR_NNE], j0, R, G, ka, kb, m, start, k, b, bi);
    u64 sp = 0, si = 0, t;
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        sp += m[q] != 0;
        si += m[q];
    }
    u64 at = part[tile] + dr_block_excl(sp, wsum, tid, &t, ansx_op_add());
    u64 w = part[nt + tile] + dr_block_excl(si, wsum, tid, &t, ansx_op_add());
#pragma unroll
    for (u32 q = 0; q < ANSX_DR_IPT; q++) {
        if (!m[q] || at >= np) continue;  // (at < np: the counts are the planner's own)
        const ansx_bdr_range g = rng[j0 + q];
        P[at] = { O[k[q] - ka].off + (start[q] - (u64)b[q] * bi[q]), g.dst + (start[q] - g.first) };
        wpos[at] = w;
        at++;
        w += m[q];
    }
    if (tile == 0 && tid == 0) wpos[np] = ints;
}
