// Ranked disjunctive queries in one call (ansx_topk_batch_dev): per query the k ids of its lists' union with the
// largest scores, score(d) = sum over the query's postings of d of weight * payload; DESIGN.md section 3m.  gfx950 only.
//
// A group runs as one of ansx_union_batch_dev (ansx_union.h) up to the heads, with a u32 value beside every key:
//   k_topk_merge    k_union_merge carrying a value: the same partition and staging.  In a query's first round the value
//                   of a posting is sat32(weight of its side * its payload), the payload read from the buffer of payloads
//                   at the key's own offset (without payloads: the weight); later rounds move the value with its key.
//                   The tile stays ANSX_UNION_TILE and the LDS 32 KiB: a thread keeps its outputs in registers and,
//                   behind a barrier, writes them over the staged input.
//   k_union_heads, k_dr_scan<u64, false>, k_isect_compact (with positions), k_isectb_bounds   as they are.
//   k_topk_scores   per head, the 64-bit sum of the values from its position to the next head's (or the query's end)
//                   -> its u32 score; a sum of 2^32 - 1 or more lowers the overflow word to the query (atomicMin).
// and then selects, all queries of the group in the same launches, over the keys topk_key(score, id) (ansx_plan_types.h),
// which are distinct inside a query:
//   k_topk_hist     a round of the radix select (ANSX_TOPK_DIGIT_BITS = 8 bits, 8 rounds, top digit first): a workgroup
//                   per ANSX_ISECT_TILE heads counts the round's digit of the heads that still agree with their query's
//                   prefix, in LDS where the tile lies inside one query (a wave whose candidates share the digit adds
//                   once), with atomics on the query's histogram otherwise.
//   k_topk_pick     a wave per query: the digit that holds its want-th largest key -> the prefix, what is left to find
//                   below it, and the histogram cleared for the next round.  Round 0 sets want = min(k, its heads).
//   k_topk_gather   every head with key >= its query's prefix -- the want-th largest key itself behind the last round --
//                   goes to the query's slot of k keys through an atomic cursor: exactly want of them.
//   k_topk_sort     a workgroup per query: its <= 1024 keys sorted in LDS (bitonic, descending) and written as ids and
//                   scores to the caller's arrays at q * k, ANSX_NO_ID / 0 behind them.
// No workgroup waits for another.  Every kernel returns at once when the scan's flag word names a list.
//
// Memory safety for ANY content of the containers and payloads.  Every offset, length and grid comes from the host
// (unb_plan, as in ansx_union.h: the same clamps hold in k_topk_merge, and a value is read at the index its key is read
// at, in a buffer of the same layout and size).  Payload VALUES are only multiplied and added; ids only compared.
// k_topk_scores reads positions idx[h] < n that k_isect_compact wrote and sums [idx[h], end) with end clamped to n: a
// loop over at most the query's span.  k_topk_hist / k_topk_gather read heads below min(*total, n) and the bounds at
// j <= Q; a digit is < 256 by its mask; the cursor's value is compared with k before the slot is written, so a slot
// never overflows whatever the prefix is.  k_topk_pick reads and clears 256 bins of query j < Q.  k_topk_sort reads
// min(k, heads of the query) <= 1024 keys of its own slot and writes exactly k entries at (q0 + j) * k.
#pragma once

#include "ansx_union.h"

// A round: as k_union_merge; vlists: the group's payloads (null: every payload is 1), laid out as lists; W: two weights
// per pair of P (sides a, b), read in a query's first round; prevv / nextv: the values beside prev / next.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topk_merge(const u32* __restrict__ lists, const u32* __restrict__ vlists,
    const u32* __restrict__ prev, const u32* __restrict__ prevv, u32* __restrict__ next, u32* __restrict__ nextv,
    const ansx_unb_pair* __restrict__ P, const u32* __restrict__ W, u32 np, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    __shared__ __align__(16) u32 in[ANSX_UNION_TILE];
    __shared__ __align__(16) u32 inv[ANSX_UNION_TILE];
    __shared__ u32 part[2];
    const u32 tid = threadIdx.x, t = blockIdx.x;
    u32 lo = 0, hi = np - 1u;  // the last pair with tile <= t (wave-uniform; P[0].tile == 0)
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1u) / 2u;
        if (P[mid].tile <= t) lo = mid;
        else hi = mid - 1u;
    }
    const ansx_unb_pair p = P[lo];
    const u32 na = p.na, nb = p.nb, n = na + nb;
    const u64 at = (u64)(t - p.tile) * ANSX_UNION_TILE;
    if (at >= n) return;  // (not with the host's table)
    const u32 d0 = (u32)at, nt = n - d0 < ANSX_UNION_TILE ? n - d0 : ANSX_UNION_TILE;
    const u32* A = (p.from_lists ? lists : prev) + p.a;
    const u32* B = (p.from_lists ? lists : prev) + p.b;
    if (tid == 0) part[0] = un_diag(A, na, B, nb, d0);
    if (tid == 64) part[1] = un_diag(A, na, B, nb, d0 + nt);
    __syncthreads();
    const u32 i0 = part[0], j0 = d0 - i0;
    u32 i1 = part[1];
    i1 = i1 < i0 ? i0 : i1;
    i1 = i1 - i0 > nt ? i0 + nt : i1;
    const u32 la = i1 - i0, lb = nt - la;  // (j0 + lb <= nb: ansx_union.h)
    if (p.from_lists) {
        const u32 wa = W[2u * lo], wb = W[2u * lo + 1u];
        const u32* VA = vlists ? vlists + p.a : nullptr;
        const u32* VB = vlists ? vlists + p.b : nullptr;
        for (u32 k = tid; k < nt; k += ANSX_ISECT_NT) {
            const bool a = k < la;
            in[k] = a ? A[i0 + k] : B[j0 + (k - la)];
            inv[k] = !vlists ? (a ? wa : wb) : a ? topk_sat32(wa, VA[i0 + k]) : topk_sat32(wb, VB[j0 + (k - la)]);
        }
    } else {
        const u32* VA = prevv + p.a;
        const u32* VB = prevv + p.b;
        for (u32 k = tid; k < nt; k += ANSX_ISECT_NT) {
            const bool a = k < la;
            in[k] = a ? A[i0 + k] : B[j0 + (k - la)];
            inv[k] = a ? VA[i0 + k] : VB[j0 + (k - la)];
        }
    }
    __syncthreads();
    const u32 d = ANSX_UNION_CPT * tid;
    u32 o[ANSX_UNION_CPT], ov[ANSX_UNION_CPT];
    if (d < nt) {
        const u32* sb = in + la;
        const u32* sv = inv + la;
        u32 li = un_diag(in, la, sb, lb, d), lj = d - li;
        u32 av = li < la ? in[li] : 0u, bv = lj < lb ? sb[lj] : 0u;
#pragma unroll
        for (u32 q = 0; q < ANSX_UNION_CPT; q++) {  // (behind the tile's end neither side is left: nothing is read)
            const bool ta = li < la && (lj >= lb || av <= bv);
            o[q] = ta ? av : bv;
            ov[q] = ta ? inv[li] : lj < lb ? sv[lj] : 0u;
            if (ta) li++, av = li < la ? in[li] : 0u;
            else lj++, bv = lj < lb ? sb[lj] : 0u;
        }
    }
    __syncthreads();  // every thread has read its part of the staged input: the outputs take its place
    if (d < nt) {
#pragma unroll
        for (u32 q = 0; q < ANSX_UNION_CPT; q += 4) {
            *(uint4*)&in[d + q] = make_uint4(o[q], o[q + 1], o[q + 2], o[q + 3]);
            *(uint4*)&inv[d + q] = make_uint4(ov[q], ov[q + 1], ov[q + 2], ov[q + 3]);
        }
    }
    __syncthreads();
    u32* dst = next + p.dst + d0;  // (any alignment: a run starts at any int)
    u32* dstv = nextv + p.dst + d0;
    for (u32 k = tid; k < nt; k += ANSX_ISECT_NT) dst[k] = in[k], dstv[k] = inv[k];
}

// A workgroup per ANSX_ISECT_TILE heads h < min(*total, n), as k_union_counts: idx[h] its position in the merged buffer,
// val the values there.  score[h] = the sum of val over [idx[h], the next head's position or the query's end); a sum of
// 2^32 - 1 or more: oflow[0] = min(oflow[0], the query), the score saturated.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topk_scores(const u32* __restrict__ idx, const u32* __restrict__ val,
    const u32* __restrict__ hseg, const u32* __restrict__ seg, u32 Q, const u64* __restrict__ total, u32 n,
    u32* __restrict__ score, u32* __restrict__ oflow, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 tot = total[0] < n ? total[0] : n;
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (i0 >= tot) return;  // (the whole workgroup)
    if (tid == 0) {
        const u64 last = (i0 + ANSX_ISECT_TILE < tot ? i0 + ANSX_ISECT_TILE : tot) - 1;
        qb[0] = isb_query_of(hseg, 0, Q - 1, (u32)i0);
        qb[1] = isb_query_of(hseg, qb[0], Q - 1, (u32)last);
    }
    __syncthreads();
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u64 h = i0 + q * ANSX_ISECT_NT + tid;
        if (h >= tot) continue;
        const u32 j = isb_query_of(hseg, qb[0], qb[1], (u32)h);
        u32 end = h + 1 < hseg[j + 1] && h + 1 < tot ? idx[h + 1] : seg[j + 1];
        end = end < n ? end : n;
        u64 sum = 0;
        for (u32 p = idx[h]; p < end; p++) sum += val[p];
        if (sum >= 0xFFFFFFFFull) atomicMin(oflow, j), sum = 0xFFFFFFFFull;
        score[h] = (u32)sum;
    }
}

// Round r of the select, a workgroup per ANSX_ISECT_TILE heads (ids[h], score[h]) below min(*total, n): hist[j * 256 + d]
// += the heads of query j with digit d that are candidates (topk_candidate against prefix[j]; all of them in round 0).
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topk_hist(const u32* __restrict__ ids, const u32* __restrict__ score,
    const u32* __restrict__ hseg, u32 Q, const u64* __restrict__ total, u32 n, u32 r, const u64* __restrict__ prefix,
    u32* __restrict__ hist, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    __shared__ u32 qb[2];
    __shared__ u32 lh[ANSX_TOPK_BINS];
    const u32 tid = threadIdx.x;
    const u64 tot = qt_clamp(total[0], n);
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (i0 >= tot) return;  // (the whole workgroup)
    if (tid < ANSX_TOPK_BINS) lh[tid] = 0;  // (in front of the prologue's barrier)
    qt_prologue(hseg, Q, i0, (u32)tot, qb);
    const u32 q0 = qb[0], q1 = qb[1];
    const bool one = q0 == q1;  // (the workgroup's)
    const u64 pre1 = r ? prefix[q0] : 0ull;
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u64 h = qt_elem(i0, q, tid);
        const u64 key = h < tot ? topk_key(score[h], ids[h]) : 0ull;
        const u32 dg = topk_digit(key, r);
        if (one) {
            // (every lane gets here.)  Where all candidates of the wave share the digit -- the rounds over the empty top
            // bytes of small scores, and over the ids' top bytes -- one lane adds their number: 64 atomics on one bin
            // of LDS serialise.
            const bool cand = h < tot && topk_candidate(key, pre1, r);
            const u64 m = __ballot(cand);
            if (m == 0) continue;  // (the wave's)
            const u32 first = (u32)__ffsll((unsigned long long)m) - 1u;
            const u32 d0 = __shfl(dg, first, 64);
            if (__ballot(cand && dg == d0) == m) {
                if ((tid & 63u) == first) atomicAdd(&lh[d0], (u32)__popcll(m));
            } else if (cand) {
                atomicAdd(&lh[dg], 1u);
            }
        } else if (h < tot) {
            const u32 j = isb_query_of(hseg, q0, q1, (u32)h);
            if (topk_candidate(key, r ? prefix[j] : 0ull, r)) atomicAdd(&hist[(u64)j * ANSX_TOPK_BINS + dg], 1u);
        }
    }
    if (!one) return;
    __syncthreads();
    if (tid < ANSX_TOPK_BINS && lh[tid]) atomicAdd(&hist[(u64)q0 * ANSX_TOPK_BINS + tid], lh[tid]);
}

// Round r, a wave per query j < Q: want[j] (round 0: min(k, its heads)) -> the digit of its want-th largest candidate
// (topk_pick over four bins a lane), prefix[j] with that digit, want[j] less the candidates above it; the bins cleared.
// A query of no heads gets a prefix no key reaches.
__global__ __launch_bounds__(256) void k_topk_pick(const u32* __restrict__ hseg, u32 Q, u32 k, u32 r, u64* __restrict__ prefix,
    u32* __restrict__ want, u32* __restrict__ hist, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    const u32 lane = threadIdx.x & 63u;
    const u64 j = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (j >= Q) return;  // (the whole wave)
    const u32 heads = hseg[j + 1] - hseg[j];
    u32* h = hist + j * ANSX_TOPK_BINS + 4u * lane;
    const uint4 v = *(const uint4*)h;
    *(uint4*)h = make_uint4(0u, 0u, 0u, 0u);
    if (heads == 0) {
        if (lane == 0) prefix[j] = ~0ull, want[j] = 0;
        return;
    }
    const u32 w = r ? want[j] : (k < heads ? k : heads);
    const u32 b[4] = { v.x, v.y, v.z, v.w };
    const u32 own = v.x + v.y + v.z + v.w;
    u32 incl = own;  // the candidates in this lane's bins and in those of the lanes above
#pragma unroll
    for (u32 o = 1; o < 64u; o <<= 1) {
        const u32 up = __shfl_down(incl, o, 64);
        if (lane + o < 64u) incl += up;
    }
    const u32 above = incl - own;
    const bool mine = above < w && w <= incl;
    // (no lane where the histogram holds fewer than w candidates -- not behind k_topk_hist: lane 0 then takes digit 0)
    const u64 any = __ballot(mine);
    if (mine || (!any && lane == 0)) {
        u32 a = 0;
        const u32 d = mine ? topk_pick(b, 4u, w - above, &a) : 0u;
        prefix[j] = topk_with_digit(r ? prefix[j] : 0ull, r, 4u * lane + d);
        want[j] = mine ? w - above - a : 1u;
    }
}

// A workgroup per ANSX_ISECT_TILE heads below min(*total, n): a head whose key is >= prefix[its query] takes the next
// place of the query's slot, slots[j * k + cursor[j]++], while there is one.  A tile inside one query takes its places
// a wave at a time.
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topk_gather(const u32* __restrict__ ids, const u32* __restrict__ score,
    const u32* __restrict__ hseg, u32 Q, const u64* __restrict__ total, u32 n, u32 k, const u64* __restrict__ prefix,
    u32* __restrict__ cursor, u64* __restrict__ slots, const u32* __restrict__ sflag)
{
    if (sflag[0] != ANSX_SS_NONE) return;
    __shared__ u32 qb[2];
    const u32 tid = threadIdx.x;
    const u64 tot = qt_clamp(total[0], n);
    const u64 i0 = (u64)blockIdx.x * ANSX_ISECT_TILE;
    if (i0 >= tot) return;  // (the whole workgroup)
    qt_prologue(hseg, Q, i0, (u32)tot, qb);
    const u32 q0 = qb[0], q1 = qb[1];
    const bool one = q0 == q1;  // (the workgroup's)
    const u64 pre1 = prefix[q0];
#pragma unroll
    for (u32 q = 0; q < ANSX_ISECT_CPT; q++) {
        const u64 h = qt_elem(i0, q, tid);
        const u64 key = h < tot ? topk_key(score[h], ids[h]) : 0ull;
        if (one) {  // (every lane gets here): one atomic per wave, the lanes take consecutive places behind it
            const bool take = h < tot && key >= pre1;
            const u64 m = __ballot(take);
            if (m == 0) continue;  // (the wave's)
            const u32 first = (u32)__ffsll((unsigned long long)m) - 1u;
            u32 base = 0;
            if ((tid & 63u) == first) base = atomicAdd(&cursor[q0], (u32)__popcll(m));
            base = __shfl(base, first, 64);
            const u32 at = base + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
            if (take && at < k) slots[(u64)q0 * k + at] = key;
        } else if (h < tot) {
            const u32 j = isb_query_of(hseg, q0, q1, (u32)h);
            if (key < prefix[j]) continue;
            const u32 at = atomicAdd(&cursor[j], 1u);
            if (at < k) slots[(u64)j * k + at] = key;
        }
    }
}

// A workgroup per query j of the group (the grid: Q): its min(k, heads) keys, slots[j * k ..], sorted descending in LDS
// -- a bitonic network over `pow2` entries, the power of two >= k (<= ANSX_TOPK_SORT_MAX), zeros behind the keys -- ->
// out_ids / out_scores (null: not asked for) at (q0 + j) * k, ANSX_NO_ID / 0 behind them.  hseg null: no query has a head.
#define ANSX_TOPK_SORT_MAX 1024u
__global__ __launch_bounds__(ANSX_ISECT_NT) void k_topk_sort(const u64* __restrict__ slots, const u32* __restrict__ hseg,
    u64 q0, u32 k, u32 pow2, u32* __restrict__ out_ids, u32* __restrict__ out_scores, const u32* __restrict__ sflag)
{
    if (sflag && sflag[0] != ANSX_SS_NONE) return;
    __shared__ u64 key[ANSX_TOPK_SORT_MAX];
    const u32 tid = threadIdx.x, j = blockIdx.x;
    const u32 heads = hseg ? hseg[j + 1] - hseg[j] : 0u;
    const u32 cnt = k < heads ? k : heads;
    pow2 = pow2 > ANSX_TOPK_SORT_MAX ? ANSX_TOPK_SORT_MAX : pow2;  // (the host's: a power of two >= k)
    if (cnt > 1) {
        for (u32 i = tid; i < pow2; i += ANSX_ISECT_NT) key[i] = i < cnt ? slots[(u64)j * k + i] : 0ull;
        for (u32 size = 2; size <= pow2; size <<= 1)
            for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (u32 i = tid; i < pow2 / 2u; i += ANSX_ISECT_NT) {
                    const u32 a = 2u * i - (i & (stride - 1u)), b = a + stride;  // (a's bit `stride` is clear)
                    const bool desc = (a & size) == 0;
                    const u64 x = key[a], y = key[b];
                    if (desc ? x < y : x > y) key[a] = y, key[b] = x;
                }
            }
        __syncthreads();
    } else if (cnt == 1 && tid == 0) {
        key[0] = slots[(u64)j * k];
    }
    if (cnt == 1) __syncthreads();
    u32* oi = out_ids + (q0 + j) * k;
    u32* os = out_scores ? out_scores + (q0 + j) * k : nullptr;
    for (u32 i = tid; i < k; i += ANSX_ISECT_NT) {
        const bool have = i < cnt;  // (cnt <= pow2: key[i] is the sort's)
        const u64 x = have ? key[i] : 0ull;
        oi[i] = have ? topk_key_id(x) : ANSX_NO_ID;
        if (os) os[i] = have ? topk_key_score(x) : 0u;
    }
}
