// ansx -- the integer names and the plain structs and constants the host's plans (ansx_plan.h) fill and the kernels read
// them through.  No code but the arithmetic of ansx_topk_batch_dev's selection, of a tile of k_topk_impacts and of the
// device plan of ansx_decode_batch_device_ranges_dev at its end: it builds with a plain host compiler, and the kernel
// headers take it through ansx_dev.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;

// One block of a batch pass: its ints and where they start in the pass's output.  Blocks of many containers share one
// sub-container there, so any of them may be short and the output of block b does not start at b * block_ints.
struct ansx_blk_out {
    u64 off;  // first int in the output (a multiple of 4: the decoders' 16-byte stores)
    u32 n;    // ints
    u32 pad_;
};

struct ansx_range_piece {  // one range with count > 0: where its ints sit in the sub-list and in the output
    u64 src, dst, count;
};

#define ANSX_RANGE_CHUNK 4096u  // ints per workgroup of k_range_gather

struct ansx_batch_src {  // a source container of a pass
    u64 base;            // its device address
    u64 ckoff_off, ckstate_off, hint_off, payload_off;  // its layout (make_plan's for its own n)
    u64 payload_bytes;   // its header's: index_entry_ok on its own entries
    u32 nblocks;
    u32 pad_;
};

struct ansx_batch_blk {  // block k of a pass is block b of source src
    u32 src, b;
};

struct ansx_piece {  // ints [src, src + count) of the pass's work list go to [dst, dst + count) of the caller's buffer;
    u64 src, dst;    // count = wpos[i + 1] - wpos[i], wpos the exclusive prefix of the counts over the pass (count > 0)
};

#define ANSX_PIECE_CHUNK 4096u  // ints per workgroup of k_piece_gather (k_range_gather's chunk)

// LDS geometry of the decode kernels, shared with the host's choice of the decode form (ansx_decode_form.h), which
// sizes the dynamic LDS the kernels carve.
#define ANSX_PF_SW 128u            // k_parse_prelude_fast: staged words per lane
#define ANSX_PAR_SW 32u            // k_parse_prelude_par: staged words per lane
#define ANSX_PAR_STK 11u           // stack rows of its value-array form: depth <= 10 (subtrees of <= 1023 items) + dump
#define ANSX_PAR_SLICE_WORDS ((ANSX_PAR_SW + 48u) * 64u)  // a wave's LDS slice: stage + the windowed form's 3 x 16 stack rows
// per-quad stream ring of the block decoder: ANSX_RING_CHK steps per refill check, 32 bytes per lane and step of check
// interval per refill (>= the 28 bytes a quad can consume per step)
#ifndef ANSX_RING_CHK
#define ANSX_RING_CHK 4
#endif
#define ANSX_DEC_SCRATCH 96u  // k_decode_rank: scan scratch + error flag between the tables and the stream area
#define ANSX_RING_BYTES (128 * ANSX_RING_CHK)
#define ANSX_RING_STRIDE (ANSX_RING_BYTES + 16)  // + 8 mirror bytes (ring bytes 0..7 once more) and padding to 16
#define ANSX_SRING_BYTES 256                       // the speculative small ring, see dec_segments_ring_small
#define ANSX_SRING_STRIDE (ANSX_SRING_BYTES + 16)

// LDS geometry and size rules of the encode kernels, shared with the host's choice of the encode forms
// (ansx_encode_form.h) and with the pass tables of ansx_encode_batch_dev (ansx_plan.h).
#define ANSX_HCOPY_PAD 8u          // k_fold_hist: pad between its four histogram copies
#define ANSX_VMAX 256u             // k_sort_entropy: frequencies below this are binned, the larger ones ranked separately
#define ANSX_CAND_SL 64u           // k_candidates: symbols per LDS stage (NT = 5: 12.5 KB per wave, three 4-wave workgroups per CU)
#define ANSX_CAND_ROW (ANSX_CAND_SL + 1u)  // entries per block row (odd: rows start in different banks)
#define ANSX_CAND_WAVES 4u         // ... and its waves per workgroup, each with its own LDS slice
#define ANSX_ENC_HOT 577  // MODE 2: words per LDS row = 1152 u16 running sums (1151 hot symbols) + a zero sentinel pair (odd stride; 16 rows = 36.9 KB per wave)
#define ANSX_RF_SLOTS 20480u       // k_rfold_remap_hash: >= 1.25 x 16384 values per block
#define ANSX_RF_SMALL_INTS 1024u   // k_rfold_remap_small: the longest block of its class ...
#define ANSX_RF_SMALL_SLOTS 2048u  // ... 2 x the most values such a block has
// per wave: the (count, value) pairs of the block's distinct values | keys | counts, then ranks (two u16 per word)
#define ANSX_RF_SMALL_LDS (8u * ANSX_RF_SMALL_INTS + 6u * ANSX_RF_SMALL_SLOTS)
#define ANSX_PA_SLOTS 20480u       // k_pa_remap: hash set capacity, >= 1.25 x 16384 values per block
#define ANSX_PA_MAX_BLOCK 16384u   // the longest block the compaction layer takes
#define ANSX_PA_SMALL_INTS 1024u   // k_pa_remap_small: the longest block of its class
#define ANSX_SP_MAX_SIGMA 16384u   // rank-space ANSint: distinct values per block (ranks are symbols of the 16384-slot ANSint model)

// Block-range pipeline of the model kernels (model_fast; measurements: DESIGN.md section 6): the values of
// ANSX_MODEL_PIPELINE besides a range count, and the size rule.
#define ANSX_PIPE_NEVER (-1)
#define ANSX_PIPE_ALWAYS (-2)
#define ANSX_PIPE_MAX_RANGES 64
// A call pipelines by itself from ANSX_PIPE_MIN_BLOCKS blocks and ANSX_PIPE_MIN_INTS ints on, in ANSX_PIPE_RANGES ranges.
// Measured on MI355X (encode call, serial -> pipelined): 16384 blocks of 16 Ki ints ANSfold-1 1.226 -> 1.173 ms with 2, 3 or
// 5 ranges, 1.213 with 6, 1.261 with 8 (k_sort_entropy and k_candidates have latency floors that every range pays again);
// 8192 blocks break even for ANSfold-1 and gain for ANSfold-5 (2.91 -> 2.70 ms); 4096 blocks and fewer lose 0.003-0.07 ms
// to the cross-stream waits.  Two ranges were never slower than the serial form on any list of that size, three lost
// their gain on uniform data.
#define ANSX_PIPE_RANGES 2u
#define ANSX_PIPE_MIN_BLOCKS 8192u
#define ANSX_PIPE_MIN_INTS ((u64)1 << 27)

// One block of an encode batch pass: its ints and where they start in the caller's input.  Blocks of many lists share
// one work list there; a list may start at any int, so nothing about the alignment of `off` is promised.
struct ansx_blk_in {
    u64 off;   // first int in the input
    u32 n;     // ints
    u32 list;  // the list of the pass it belongs to
};

struct ansx_encb_list {  // list i of a pass: blocks [fb, next list's fb); the entry behind the last list closes it
    u64 n;               // its ints
    u32 fb;
    u32 pad_;
};

struct ansx_encb_max {  // maxima over a list's own blocks (the container header's), and the form of its restart points
    u32 logM, ns, sigma, wide;
};

struct ansx_encb_res {  // where container i went (relative to the caller's buffer) and its exact size
    u64 off, bytes;
};

struct ansx_brs_src {  // a source of a pass, beside its ansx_batch_src: the caller's bases of that container
    u64 bases;         // device address of its nblocks + 1 entries (4-byte aligned)
    u32 nblocks;
    u32 pad_;
};

// A group of conjunctive queries (ansx_intersect_batch_dev, ansx_intersect_batch.h).  Both count in ints of the group's
// buffer of ids, the lists the group decodes back to back.
struct ansx_isb_query {  // query j of the group: its driver's ids lie from src on and become candidates [dst, next dst);
    u64 src, dst;        // the entry behind the last query closes it: dst = the group's candidates
};
struct ansx_isb_list {  // a round of a query: the list's ids [at, at + n) of the buffer; an empty list has n = 0
    u64 at, n;          // (also an entry of xt, the lists a query of ansx_bool_batch_dev excludes: ansx_bool.h)
};

// A group of disjunctive queries (ansx_union_batch_dev, ansx_union.h).  A pair of a round: the sorted runs A and B
// become one sorted run of na + nb ints at dst of the round's merge buffer.  from_lists: a and b count in ints of the
// group's buffer of ids (the pair is the first of its query); otherwise in ints of the other merge buffer, where
// a == dst and b == a + na.  nb == 0: a copy.  tile: the round's tiles of ANSX_UNION_TILE outputs in front of this pair.
struct ansx_unb_pair {
    u64 a, b;
    u32 na, nb;
    u32 dst, tile;
    u32 from_lists, pad_;
};

// Ranked disjunctive queries (ansx_topk_batch_dev, ansx_topk.h).  The only code of this header: the arithmetic of the
// selection, which the kernels and the CPU check (tests/tools/topk_plan_check.cpp) both run, so it is written once and
// builds for either side.
#ifndef ANSX_PLAN_FN  // (ansx_dev.h names the kernels' side before it includes this header)
#define ANSX_PLAN_FN static inline
#endif

#define ANSX_TOPK_NONE 0xFFFFFFFFu  // the overflow word while no query's score has left 32 bits; no term behind a side of a pair
#define ANSX_TOPK_DIGIT_BITS 8u     // the radix select's digit ...
#define ANSX_TOPK_BINS (1u << ANSX_TOPK_DIGIT_BITS)
#define ANSX_TOPK_ROUNDS (64u / ANSX_TOPK_DIGIT_BITS)  // ... and its rounds over a 64-bit key, from the top digit down

// weight * payload in 64 bits, saturated
ANSX_PLAN_FN u32 topk_sat32(u32 w, u32 p)
{
    const u64 v = (u64)w * p;
    return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)v;
}

// a + b, saturated: with u32 terms the result is 0xFFFFFFFF exactly when the 64-bit sum of all of them reaches 2^32 - 1
// (ansx_topk_bool_batch_dev, ansx_topk_bool.h, and tests/tools/topk_bool_plan_check.cpp)
ANSX_PLAN_FN u32 topk_sat_add(u32 a, u32 b)
{
    const u64 v = (u64)a + b;
    return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)v;
}

// The key of an id inside its query: larger = ranked earlier (score descending, id ascending); distinct ids, distinct keys.
ANSX_PLAN_FN u64 topk_key(u32 score, u32 id) { return ((u64)score << 32) | (u32)~id; }
ANSX_PLAN_FN u32 topk_key_id(u64 key) { return ~(u32)key; }
ANSX_PLAN_FN u32 topk_key_score(u64 key) { return (u32)(key >> 32); }

// round r = 0 .. ANSX_TOPK_ROUNDS - 1 looks at this digit of a key ...
ANSX_PLAN_FN u32 topk_digit(u64 key, u32 r) { return (u32)(key >> (64u - ANSX_TOPK_DIGIT_BITS * (r + 1u))) & (ANSX_TOPK_BINS - 1u); }

// ... of the keys that agree with the prefix found so far in the digits of the rounds before
ANSX_PLAN_FN bool topk_candidate(u64 key, u64 prefix, u32 r)
{
    const u32 sh = 64u - ANSX_TOPK_DIGIT_BITS * r;
    return r == 0 || (key >> sh) == (prefix >> sh);
}
ANSX_PLAN_FN u64 topk_with_digit(u64 prefix, u32 r, u32 d) { return prefix | ((u64)d << (64u - ANSX_TOPK_DIGIT_BITS * (r + 1u))); }

// The digit that holds the want-th largest (want >= 1) of the keys counted in h[0 .. n): the largest d with
// h[d] + ... + h[n - 1] >= want; *above: the keys in the digits above it (< want).  Fewer than `want` keys in all -- not
// with a histogram of at least `want` keys -- gives digit 0.
ANSX_PLAN_FN u32 topk_pick(const u32* h, u32 n, u32 want, u32* above)
{
    u32 a = 0, d = n;
    while (d > 0) {
        d--;
        if (h[d] >= want - a) break;  // (a < want: no wrap)
        a += h[d];  // (still below want)
    }
    *above = a;
    return d;
}

// Length-normalised scores (ansx_topk_scored_batch_dev, ansx_topk_scored.h).  k_topk_impacts
// rewrites the payloads of a group's lists in place; the host's table (ansx_plan.h, impact_plan) has an entry per list
// that has a payload.  A tile is `tile` ints (a multiple of 4) of the group's buffers, counted from the list's start
// rounded DOWN to four ints, so that every uint4 of a tile is aligned: tile t of a list covers the buffer's ints
// [at - (at & 3) + t * tile, ... + tile), cut to the list's own [at, at + n).  The arithmetic of one tile and one
// posting is written here once: the kernel and the CPU check (tests/tools/topk_scored_plan_check.cpp) both run it.
struct ansx_impact_list {
    u64 at, n;  // the list's ids and payloads: ints [at, at + n) of the group's two buffers (n > 0)
    u32 tile;   // the launch's tiles in front of this list (strictly ascending; the first is 0)
    u32 pos;    // its place in the group's lists: what the scan's flag word names
};

#define ANSX_IMPACT_COLS 256u  // the columns of a scorer's table: a norm is a byte
#define ANSX_IMPACT_MAX_ROWS 256u  // ... and the most rows it may have (ansx_scorer.tf_rows)

// the tiles of a list
ANSX_PLAN_FN u64 impact_tiles(u64 at, u64 n, u32 tile) { return ((at & 3u) + n + tile - 1u) / tile; }

// the list of tile t: the last entry of P[0 .. np) with tile <= t (P[0].tile == 0)
ANSX_PLAN_FN u32 impact_list_of(const ansx_impact_list* P, u32 np, u32 t)
{
    u32 lo = 0, hi = np - 1u;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1u) / 2u;
        if (P[mid].tile <= t) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// the buffer's int where tile t of the list starts (a multiple of 4)
ANSX_PLAN_FN u64 impact_tile_start(const ansx_impact_list& L, u32 t, u32 tile) { return (L.at & ~(u64)3u) + (u64)(t - L.tile) * tile; }

// bit j: int i + j of the buffer (i a multiple of 4) belongs to the list; 15: the uint4 at i is the list's own
ANSX_PLAN_FN u32 impact_mask(const ansx_impact_list& L, u64 i)
{
    u32 m = 0;
    for (u32 j = 0; j < 4u; j++) m |= (i + j >= L.at && i + j < L.at + L.n) ? 1u << j : 0u;
    return m;
}

// an id the norms have no entry for (64 bits: ndocs == 2^32 admits every id)
ANSX_PLAN_FN bool impact_bad_id(u32 id, u64 ndocs) { return (u64)id >= ndocs; }

// the table's word of (payload, norm): below rows * ANSX_IMPACT_COLS whatever the payload, for a norm below 256
ANSX_PLAN_FN u32 impact_word(u32 tf, u32 norm, u32 rows) { return (tf < rows - 1u ? tf : rows - 1u) * ANSX_IMPACT_COLS + norm; }

// Ranges of a batch planned on the device (ansx_decode_batch_device_ranges_dev, ansx_batchdevranges.h; DESIGN.md
// section 3d, "device plan").  The referenced containers, ordered by geometry group and by batch position inside a
// group, are laid end to end as one virtual container: block b of referenced container r is GLOBAL block
// R[r].gbase + b.  The touched global blocks, sorted and unique, are tb[0 .. T); a group's stretch of tb starts at
// tg[group] and is cut into passes every PB entries.  The arithmetic of one item -- a range, an entry of tb, a piece --
// is written here once: the kernels and the CPU check (tests/tools/batch_dev_plan_check.cpp) both run it.
struct ansx_bdr_ref {    // a referenced container, in the order of the global blocks
    u64 n;               // its ints
    u64 payload_bytes;   // its header's
    u32 gbase;           // its first global block (strictly ascending: no container is empty)
    u32 nblocks;
    u32 group;
    u32 pad_;
};
struct ansx_bdr_group {  // a geometry group: containers of one block size, decoded together
    u64 bbound;          // the most bytes a block's stream takes in this geometry
    u32 gbase;           // its first global block
    u32 pslot;           // the slot of its first pass among the call's pass scalars
    u32 bi;              // ints per block
    u32 pad_;
};
struct ansx_bdr_pass {   // the scalars of a pass, summed on the device and read back once with the planner's own
    u64 wl;              // ints of its work list: every block's rounded up to 4
    u64 cap_pay;         // the bound of its payload: over its sources, min(payload_bytes, blocks in the pass x bbound)
    u64 np, ints;        // its pieces and their ints
    u32 last_n, pad_;    // ints of its last block
    u64 pad2_;
};
struct ansx_bdr_range {  // a non-empty range, in range order
    u64 first, dst;      // its first int in its container, and in the caller's buffer
    u32 count, r;        // r: its referenced container
    u32 k0, pad_;        // the entry of tb its first block is; its blocks are consecutive entries from there
};

ANSX_PLAN_FN u32 bdr_rup4(u32 n) { return (n + 3u) & ~3u; }

// range -> its span of global blocks [*gb0, *gb1p) (count > 0)
ANSX_PLAN_FN void bdr_span(u64 first, u32 count, u32 bi, u32 gbase, u32* gb0, u32* gb1p)
{
    *gb0 = gbase + (u32)(first / bi);
    *gb1p = gbase + (u32)((first + count - 1) / bi) + 1u;
}

// the referenced container a global block lies in: the last r with R[r].gbase <= gb
ANSX_PLAN_FN u32 bdr_ref_of(const ansx_bdr_ref* R, u32 nref, u32 gb)
{
    u32 lo = 0, hi = nref;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (R[mid].gbase <= gb) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ints of block b of a container of n ints in blocks of bi: only its last block is short
ANSX_PLAN_FN u32 bdr_block_ints(u64 n, u32 bi, u32 b)
{
    const u64 left = n - (u64)b * bi;
    return left < bi ? (u32)left : bi;
}

// entry k of tb, in a group whose stretch starts at tg: its pass among the group's, and that pass's first entry
ANSX_PLAN_FN u32 bdr_pass_of(u32 k, u32 tg, u32 PB) { return (k - tg) / PB; }
ANSX_PLAN_FN u32 bdr_pass_first(u32 p, u32 tg, u32 PB) { return tg + p * PB; }  // (below T: no wrap)

// the first entry of tb[0 .. T) that is not below gb
ANSX_PLAN_FN u32 bdr_lower_bound(const u32* tb, u32 T, u32 gb)
{
    u32 lo = 0, hi = T;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (tb[mid] < gb) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// what a source adds to the payload bound of a pass that holds nblk of its blocks
ANSX_PLAN_FN u64 bdr_src_bound(u64 payload_bytes, u32 nblk, u64 bbound)
{
    const u64 v = (u64)nblk * bbound;
    return payload_bytes < v ? payload_bytes : v;
}

// The part of a range that lies in the pass of tb entries [ka, kb): ints [*start, *start + count) of its container,
// the first of them in entry *k of tb, which is block *b.  -> count, 0 if the range has no block in the pass.  A range
// that crosses passes gives one piece in each.
ANSX_PLAN_FN u32 bdr_piece(const ansx_bdr_range& g, u32 bi, u32 ka, u32 kb, u64* start, u32* k, u32* b)
{
    const u32 b0 = (u32)(g.first / bi), b1 = (u32)((g.first + g.count - 1) / bi);
    const u32 k1 = g.k0 + (b1 - b0);
    if (g.k0 >= kb || k1 < ka) return 0;
    const u32 kA = g.k0 > ka ? g.k0 : ka, kB = k1 < kb - 1 ? k1 : kb - 1;
    const u32 bA = b0 + (kA - g.k0), bB = b0 + (kB - g.k0);
    const u64 lo = (u64)bA * bi, hi = ((u64)bB + 1) * bi, end = g.first + g.count;
    const u64 s = g.first > lo ? g.first : lo, e = end < hi ? end : hi;
    *start = s, *k = kA, *b = bA;
    return (u32)(e - s);
}
