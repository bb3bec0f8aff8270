// ansx -- the host's plans of the random-access calls ("Host side of the random-access calls"):
// which blocks a set of ranges touches, where every range's ints lie in the work list those blocks decode to, and the
// tables a pass over blocks of many containers takes; and the steps and pass tables of a batch of lists to encode
// (ansx_encode_batch_dev); and the groups, drivers and round tables of a batch of conjunctive queries
// (ansx_intersect_batch_dev); and the groups, rounds and pair tables of a batch of disjunctive queries
// (ansx_union_batch_dev, and with the terms behind the pairs of ansx_topk_batch_dev); and the host's tables of the device
// plan of ansx_decode_batch_device_ranges_dev (tests/tools/batch_dev_plan_check.cpp).  Pure host arithmetic: no context, no stream, no device pointer
// (addresses travel as integers), so it builds with a plain host compiler and is tested on the CPU
// (tests/tools/plan_check.cpp, tests/tools/isect_batch_plan_check.cpp, tests/tools/union_plan_check.cpp, tests/tools/topk_plan_check.cpp).  The plain structs the kernels read these plans through are in ansx_plan_types.h,
// which the kernel headers include.
#pragma once
#include "../../include/ansx.h"
#include "ansx_plan_types.h"

#include <algorithm>
#include <array>
#include <map>
#include <utility>
#include <vector>

namespace ansx_plan {

// (Every function here is static inline: with external linkage the compiler stopped folding the planners into their
// one caller, and the batch calls over thousands of containers ran 2-5 % longer.)

static inline size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Layout {  // container layout, a pure function of the geometry (restart-point format included)
    u64 index_off, ckoff_off, ckstate_off, hint_off, payload_off;
};

struct BatchSrc {  // a container of the batch, checked
    ansx_container_header H;
    Layout lay;
    u64 base;
    u32 nblocks;
};

// ------------------------------------------------------------------------------- ranges of one container
// The plan of ansx_decode_ranges_dev: tb, the T touched blocks (ascending, unique; last_b the last); one piece per
// non-empty range, in range order, src counted in the work list the touched blocks decode to (block tb[k] at k * bi);
// pstart[nr + 1], every piece's first chunk of ANSX_RANGE_CHUNK ints among the npieces chunks.
struct RangePlan {
    u64 T = 0, last_b = 0, npieces = 0, total = 0;
    std::vector<u32> tb, pstart;
    std::vector<ansx_range_piece> pieces;
};

// Ranges [first[i], first[i] + count[i]) of a list of n ints in blocks of bi, for an output of cap ints.  ANSX_ERR_ARG
// for the first range that leaves the list, then ANSX_ERR_CAPACITY; ANSX_OK with total == 0 (and T == 0) where there is
// nothing to decode.
// (Kept out of line, like batch_pass_plan below: folded into their callers by the compiler, the call on 2^20 point
// ranges ran 7 % longer and the batch call on 4096 containers 3 %.)
__attribute__((noinline)) static int range_plan(u64 n, u64 bi, const u64* first, const u32* count, size_t nranges, u64 cap, RangePlan* R)
{
    // ranges -> block spans; their union as sorted runs of consecutive blocks, each numbered from its first touched block
    u64 total = 0;
    std::vector<std::pair<u64, u64>> span;  // [first block, last block] of every non-empty range
    span.reserve(nranges);
    for (size_t i = 0; i < nranges; i++) {
        if (first[i] > n || (u64)count[i] > n - first[i]) return ANSX_ERR_ARG;
        if (!count[i]) continue;
        span.push_back({ first[i] / bi, (first[i] + count[i] - 1) / bi });
        total += count[i];  // (at most 2^32 - 1 per range: no wrap below 2^32 ranges)
    }
    if (total > cap) return ANSX_ERR_CAPACITY;
    if (total == 0) return ANSX_OK;
    std::sort(span.begin(), span.end());
    struct Run {
        u64 b0, b1, k0;  // blocks b0..b1 are touched blocks k0.. of the sub-container
    };
    std::vector<Run> runs;
    u64 T = 0;
    for (const auto& sp : span) {
        if (!runs.empty() && sp.first <= runs.back().b1 + 1) {
            if (sp.second > runs.back().b1) {
                T += sp.second - runs.back().b1;
                runs.back().b1 = sp.second;
            }
            continue;
        }
        runs.push_back({ sp.first, sp.second, T });
        T += sp.second - sp.first + 1;
    }
    R->pieces.reserve(span.size());
    R->pstart.reserve(span.size() + 1);
    u64 npieces = 0, dst = 0;
    for (size_t i = 0; i < nranges; i++) {
        if (!count[i]) continue;
        const u64 b0 = first[i] / bi;
        auto it = std::upper_bound(runs.begin(), runs.end(), b0, [](u64 v, const Run& r) { return v < r.b0; });
        const Run& r = *(it - 1);
        R->pieces.push_back({ (r.k0 + (b0 - r.b0)) * bi + (first[i] - b0 * bi), dst, (u64)count[i] });
        R->pstart.push_back((u32)npieces);
        dst += count[i];
        npieces += (count[i] + ANSX_RANGE_CHUNK - 1) / ANSX_RANGE_CHUNK;
    }
    if (npieces > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    R->pstart.push_back((u32)npieces);
    R->tb.reserve(T);
    for (const Run& r : runs)
        for (u64 b = r.b0; b <= r.b1; b++) R->tb.push_back((u32)b);
    R->T = T, R->last_b = runs.back().b1, R->npieces = npieces, R->total = total;
    return ANSX_OK;
}

// ------------------------------------------------------------------------------- batches
// the geometry a container's blocks are grouped by: block_ints, restart interval, compaction, restart-point format
typedef std::array<u32, 4> Geometry;
static inline Geometry br_geometry(const ansx_container_header& H)
{
    return { H.block_ints, H.ckpt_interval, (H.kind >> 8) & 1u, (H.kind >> 9) & 1u };
}

// The containers the ranges name (src[i] < count), in batch order, and every range's place among them.  A batch that is
// not much larger than the query is marked in an array over its positions, a larger one is found by sorting the names.
static inline void br_refs(const u32* src, size_t nranges, size_t count, std::vector<u32>* ref, std::vector<u32>* rid)
{
    ref->clear(), rid->resize(nranges);
    if (count <= 4 * nranges + 1024) {
        std::vector<u32> slot(count, 0);
        for (size_t i = 0; i < nranges; i++) slot[src[i]] = 1;
        for (size_t j = 0; j < count; j++)
            if (slot[j]) slot[j] = (u32)ref->size(), ref->push_back((u32)j);
        for (size_t i = 0; i < nranges; i++) (*rid)[i] = slot[src[i]];
        return;
    }
    ref->assign(src, src + nranges);
    std::sort(ref->begin(), ref->end());
    ref->erase(std::unique(ref->begin(), ref->end()), ref->end());
    for (size_t i = 0; i < nranges; i++) (*rid)[i] = (u32)(std::lower_bound(ref->begin(), ref->end(), src[i]) - ref->begin());
}

// The source list of a ranked call with payloads (ansx_topk_batch_dev, ansx_topk_bool_batch_dev):
// the id container of every list `named` refers to, ascending by batch index, and behind each list that is a TERM --
// one of named[0 .. nt), the rest are excluded lists -- the container of its payload.  A list that is only excluded
// has no payload entry.  With nothing excluded, list u of the referenced ones stands at entry 2u and its payload at
// 2u + 1.  The front end reads the headers of the entries in this order; the planners read rid.
struct QuerySources {
    std::vector<u32> uniq;   // the referenced lists, ascending (batch indices)
    std::vector<u32> idpos;  // per referenced list: the entry of its id container
    std::vector<u32> owner;  // per entry: the referenced list (its place in uniq) the container belongs to
    std::vector<u8> pay;     // per entry: 1 its owner's payload container, 0 its id container
    std::vector<u32> payof;  // per entry: the entry of its payload (an id container of a term), else ANSX_TOPK_NONE
    std::vector<u32> rid;    // per name: the entry of its id container
    size_t batch_index(size_t e) const { return uniq[owner[e]]; }
};
static inline void query_sources(const u32* named, size_t nt, size_t nnamed, size_t count, QuerySources* S)
{
    std::vector<u32> urid;
    br_refs(named, nnamed, count, &S->uniq, &urid);
    const size_t nu = S->uniq.size();
    std::vector<u8> term(nu, 0);
    for (size_t j = 0; j < nt; j++) term[urid[j]] = 1;
    S->idpos.resize(nu), S->owner.clear(), S->pay.clear(), S->payof.clear();
    for (size_t u = 0; u < nu; u++) {
        const u32 e = (u32)S->owner.size();
        S->idpos[u] = e;
        S->owner.push_back((u32)u), S->pay.push_back(0), S->payof.push_back(term[u] ? e + 1u : ANSX_TOPK_NONE);
        if (term[u]) S->owner.push_back((u32)u), S->pay.push_back(1), S->payof.push_back(ANSX_TOPK_NONE);
    }
    S->rid.resize(nnamed);
    for (size_t j = 0; j < nnamed; j++) S->rid[j] = S->idpos[urid[j]];
}

// The first entry of the source list that is at fault, given the headers rs of the entries and `failed`, the first
// entry whose header fails the checks (every entry in front of it passed; the number of entries: none fails): the first
// id container in front of `failed` whose payload differs from it in n, else `failed`.  Entries ascend by batch index,
// so batch_index() of the result is the smallest batch index at fault.
static inline size_t query_sources_first_bad(const QuerySources& S, const std::vector<BatchSrc>& rs, size_t failed)
{
    for (size_t e = 0; e + 1 < failed; e++)
        if (S.payof[e] != ANSX_TOPK_NONE && rs[e].H.n != rs[e + 1].H.n) return e;
    return failed;
}

struct BrRun {     // consecutive touched blocks b0..b1 of referenced container r, inside one pass
    u32 r, b0, b1, pass;
    u64 wl;        // its first int in the pass's work list (a multiple of 4)
    u32 k0;        // ... and block b0's number among the pass's blocks
};
struct BrPiece {   // a range, or the part of one that lies in one run
    u32 pass;
    u64 src, dst, count;
    u32 k;         // the block of the pass its first int lies in
};

// The union of one container's block spans sp[0..m) (first block << 32 | last block) as ascending stretches of
// consecutive blocks with a gap between any two, appended to out.  More spans than the container has blocks (point
// lookups) are counted into a difference array over its blocks; fewer are sorted.
static inline void br_union(u64* sp, size_t m, u32 nblocks, std::vector<u32>& diff, std::vector<std::pair<u32, u32>>& out)
{
    if (m > nblocks) {
        diff.assign((size_t)nblocks + 1, 0);
        for (size_t i = 0; i < m; i++) diff[sp[i] >> 32]++, diff[(u32)sp[i] + 1]--;
        u32 depth = 0, b0 = 0;
        for (u32 b = 0; b <= nblocks; b++) {
            const u32 d = depth + diff[b];  // (spans that cover block b; 0 at b = nblocks)
            if (!depth && d) b0 = b;
            if (depth && !d) out.push_back({ b0, b - 1 });
            depth = d;
        }
        return;
    }
    std::sort(sp, sp + m);
    u32 b0 = (u32)(sp[0] >> 32), e = (u32)sp[0];
    for (size_t i = 1; i < m; i++) {
        const u32 f = (u32)(sp[i] >> 32), l = (u32)sp[i];
        if (f <= e + 1) {
            e = std::max(e, l);
            continue;
        }
        out.push_back({ b0, e });
        b0 = f, e = l;
    }
    out.push_back({ b0, e });
}

// The touched blocks of the ranges `ids` (non-empty, of one geometry: bi ints per block) as runs, sorted by
// (container, block) and cut where a pass holds PB blocks.  A run's ints start at a multiple of 4 in its pass's work list.
static inline void br_runs(const std::vector<BatchSrc>& rs, const std::vector<u32>& rid, const u64* first, const u32* cnt,
    const std::vector<u32>& ids, u64 bi, u32 PB, std::vector<BrRun>* runs)
{
    // the spans bucketed by container (a counting sort over the referenced containers)
    std::vector<size_t> at(rs.size() + 1, 0);
    for (const u32 i : ids) at[rid[i] + 1]++;
    for (size_t r = 0; r < rs.size(); r++) at[r + 1] += at[r];
    std::vector<u64> span(ids.size());
    {
        std::vector<size_t> put(at.begin(), at.end() - 1);
        for (const u32 i : ids) span[put[rid[i]]++] = (first[i] / bi) << 32 | ((first[i] + cnt[i] - 1) / bi);
    }
    u32 pass = 0, pb = 0;  // the pass being filled, its blocks so far
    u64 wl = 0;            // ... and its work-list ints
    std::vector<u32> diff;
    std::vector<std::pair<u32, u32>> stretch;
    for (size_t r = 0; r < rs.size(); r++) {
        if (at[r] == at[r + 1]) continue;
        stretch.clear();
        br_union(span.data() + at[r], at[r + 1] - at[r], rs[r].nblocks, diff, stretch);
        const u64 n = rs[r].H.n;
        for (const auto& st : stretch)
            for (u32 b = st.first; b <= st.second;) {
                const u32 take = (u32)std::min<u64>((u64)st.second - b + 1, PB - pb);
                runs->push_back({ (u32)r, b, b + take - 1, pass, wl, pb });
                wl += rup(std::min<u64>(n, ((u64)b + take) * bi) - (u64)b * bi, 4);
                pb += take;
                b += take;
                if (pb == PB) pass++, pb = 0, wl = 0;
            }
    }
}

// Every range's pieces, one per run it crosses (runs cut from one stretch of blocks follow each other), bucketed by
// pass in range order: pieces PP and their counts PC, pass p's from pfirst[p] to pfirst[p + 1].  PK (optional): the
// block of its pass every piece starts in.
static inline void br_pieces(const std::vector<BatchSrc>& rs, const std::vector<u32>& rid, const u64* first, const u32* cnt,
    const std::vector<u64>& off, const std::vector<u32>& ids, u64 bi, const std::vector<BrRun>& runs,
    std::vector<ansx_piece>* PP, std::vector<u64>* PC, std::vector<u64>* pfirst, std::vector<u32>* PK = nullptr)
{
    const u32 npass = runs.back().pass + 1;
    std::vector<BrPiece> pieces;
    pieces.reserve(ids.size());
    pfirst->assign((size_t)npass + 1, 0);
    for (const u32 i : ids) {
        const u32 r = rid[i], b0 = (u32)(first[i] / bi);
        const u64 n = rs[r].H.n;
        auto it = std::upper_bound(runs.begin(), runs.end(), b0,
            [r](u32 v, const BrRun& x) { return x.r != r ? r < x.r : v < x.b0; });
        size_t k = (size_t)(it - runs.begin()) - 1;
        u64 pos = first[i], left = cnt[i], dst = off[i];
        for (; left; k++) {
            const BrRun& rn = runs[k];
            const u64 take = std::min<u64>(left, std::min<u64>(n, ((u64)rn.b1 + 1) * bi) - pos);
            pieces.push_back({ rn.pass, rn.wl + (pos - (u64)rn.b0 * bi), dst, take, rn.k0 + ((u32)(pos / bi) - rn.b0) });
            (*pfirst)[rn.pass + 1]++;
            pos += take, dst += take, left -= take;
        }
    }
    for (u32 p = 0; p < npass; p++) (*pfirst)[p + 1] += (*pfirst)[p];
    PP->resize(pieces.size());
    PC->resize(pieces.size());
    if (PK) PK->resize(pieces.size());
    std::vector<u64> put(pfirst->begin(), pfirst->end() - 1);
    for (const BrPiece& q : pieces) {  // (stable: range order inside a pass)
        (*PP)[put[q.pass]] = { q.src, q.dst };
        if (PK) (*PK)[put[q.pass]] = q.k;
        (*PC)[put[q.pass]++] = q.count;
    }
}

// A pass over blocks of containers of one geometry: its sources S (one per container, `cont` its number among the
// caller's), its blocks B, the decoders' table O over the pass's work list of wl ints, the header Hs of the
// sub-container they make (H0's geometry, the maxima over the sources) and cap_pay, the bound of its payload.
struct Pass {
    std::vector<ansx_batch_src> S;
    std::vector<ansx_batch_blk> B;
    std::vector<ansx_blk_out> O;
    std::vector<u32> cont;
    ansx_container_header Hs;
    u64 cap_pay, wl;
    u32 last_blocks;  // blocks of the last source so far: close() adds its share of the payload bound

    void open(const ansx_container_header& H0)
    {
        S.clear(), B.clear(), O.clear(), cont.clear();
        Hs = H0;
        Hs.max_nsyms = 0, Hs.max_log2_frame = 0, Hs.max_present_m1 = 0;
        cap_pay = wl = 0, last_blocks = 0;
    }
    void close(u64 bbound)
    {
        if (!S.empty()) cap_pay += std::min<u64>(S.back().payload_bytes, (u64)last_blocks * bbound);
        last_blocks = 0;
    }
    // Blocks b0..b1 of container r (cs; blocks of bi ints, streams of at most bbound bytes) behind what the pass holds,
    // their ints from `at` of the work list (a multiple of 4) on: a new source where the container changes.  close()
    // behind the last.  -> their ints
    u64 append(const BatchSrc& cs, u32 r, u32 b0, u32 b1, u64 at, u64 bi, u64 bbound)
    {
        if (S.empty() || cont.back() != r) {
            close(bbound);
            S.push_back({ cs.base, cs.lay.ckoff_off, cs.lay.ckstate_off, cs.lay.hint_off, cs.lay.payload_off,
                cs.H.payload_bytes, cs.nblocks, 0 });
            cont.push_back(r);
            Hs.max_nsyms = std::max(Hs.max_nsyms, cs.H.max_nsyms);
            Hs.max_log2_frame = std::max(Hs.max_log2_frame, cs.H.max_log2_frame);
            Hs.max_present_m1 = std::max(Hs.max_present_m1, cs.H.max_present_m1);
        }
        for (u32 b = b0; b <= b1; b++) {
            B.push_back({ (u32)S.size() - 1, b });
            O.push_back({ at + (u64)(b - b0) * bi, (u32)std::min<u64>(bi, cs.H.n - (u64)b * bi), 0 });
        }
        last_blocks += b1 - b0 + 1;
        const u64 ints = std::min<u64>(cs.H.n, ((u64)b1 + 1) * bi) - (u64)b0 * bi;
        wl = at + rup(ints, 4);
        return ints;
    }
    // Pass p of br_runs' runs, which start at runs[k], opened on H0 -> the first run behind them.  (B and O get their
    // room at once: growing them block by block showed in the calls over thousands of containers.)
    size_t take_runs(const ansx_container_header& H0, const std::vector<BatchSrc>& rs, const std::vector<BrRun>& runs,
        size_t k, u32 p, u64 bi, u64 bbound)
    {
        open(H0);
        size_t e = k, T = 0;
        for (; e < runs.size() && runs[e].pass == p; e++) T += runs[e].b1 - runs[e].b0 + 1;
        B.reserve(T), O.reserve(T);
        for (; k < e; k++) append(rs[runs[k].r], runs[k].r, runs[k].b0, runs[k].b1, runs[k].wl, bi, bbound);
        close(bbound);
        return k;
    }
};

// A pass of ansx_decode_batch_dev: whole containers ids[*ci..] of one geometry (src[i] at off[i] of the caller's
// buffer), from block *b0 of the first, up to PB blocks; moves *ci / *b0 past them.  R, pstart[nr + 1]: one gather
// piece per source and every piece's first chunk of ANSX_RANGE_CHUNK ints; -> the chunks.
__attribute__((noinline)) static u64 batch_pass_plan(const std::vector<BatchSrc>& src, const std::vector<u64>& off, const std::vector<u32>& ids,
    size_t* ci, u32* b0, u32 PB, u64 bbound, Pass* P, std::vector<ansx_range_piece>* R, std::vector<u32>* pstart)
{
    const ansx_container_header& H0 = src[ids[*ci]].H;
    const u64 bi = H0.block_ints;
    P->open(H0);  // (the table: every container's blocks back to back, from a multiple of 4 ints)
    R->clear(), pstart->clear();
    u64 npieces = 0;
    u64 T = 0;  // (room for the pass's blocks at once, as take_runs finds it)
    for (size_t j = *ci; j < ids.size() && T < PB; j++) T += src[ids[j]].nblocks;
    P->B.reserve(std::min<u64>(T, PB)), P->O.reserve(std::min<u64>(T, PB));
    while (*ci < ids.size() && P->B.size() < PB) {
        const u32 i = ids[*ci];
        const BatchSrc& cs = src[i];
        const u32 take = (u32)std::min<u64>(cs.nblocks - *b0, PB - P->B.size());
        const u64 at = P->wl, ints = P->append(cs, i, *b0, *b0 + take - 1, at, bi, bbound);
        R->push_back({ at, off[i] + (u64)*b0 * bi, ints });
        pstart->push_back((u32)npieces);  // (checked by the caller: npieces stays below 2^32)
        npieces += (ints + ANSX_RANGE_CHUNK - 1) / ANSX_RANGE_CHUNK;
        *b0 += take;
        if (*b0 == cs.nblocks) (*ci)++, *b0 = 0;
    }
    P->close(bbound);
    pstart->push_back((u32)npieces);
    return npieces;
}

// ------------------------------------------------------------------------------- ranges of a batch, planned on the device
// The host's part of ansx_decode_batch_device_ranges_dev ("device plan"), O(referenced
// containers): rs, the referenced containers in batch order, laid end to end as global blocks -- geometry group after
// group, batch order inside a group.  R / S (and rmap, a container's place among them) are in that order; G: the groups,
// each with its first global block, its first pass slot (a group of NB blocks makes at most ceil(NB / PB) passes) and
// bbound(H) of its geometry; Hs: a group's sub-header, its geometry with the maxima over its referenced containers.
struct BdrTables {
    std::vector<u32> rmap;
    std::vector<ansx_bdr_ref> R;
    std::vector<ansx_bdr_group> G;
    std::vector<ansx_batch_src> S;
    std::vector<ansx_container_header> Hs;
    u64 nbtot = 0, nslots = 0;  // global blocks, pass slots
};
// -> false if the containers have 2^32 - 1 blocks or more together (a global block, and one behind the last, is a u32)
template <class Bound> static inline bool bdr_tables(const std::vector<BatchSrc>& rs, u32 PB, const Bound& bbound, BdrTables* T)
{
    std::map<Geometry, std::vector<u32>> groups;
    for (size_t j = 0; j < rs.size(); j++) groups[br_geometry(rs[j].H)].push_back((u32)j);
    T->rmap.resize(rs.size());
    T->R.reserve(rs.size()), T->S.reserve(rs.size());
    for (const auto& gr : groups) {
        const ansx_container_header& H0 = rs[gr.second[0]].H;
        ansx_container_header H = H0;
        H.max_nsyms = 0, H.max_log2_frame = 0, H.max_present_m1 = 0;
        const u64 gb0 = T->nbtot;
        for (const u32 j : gr.second) {
            const BatchSrc& cs = rs[j];
            T->rmap[j] = (u32)T->R.size();
            T->R.push_back({ cs.H.n, cs.H.payload_bytes, (u32)T->nbtot, cs.nblocks, (u32)T->G.size(), 0 });
            T->S.push_back({ cs.base, cs.lay.ckoff_off, cs.lay.ckstate_off, cs.lay.hint_off, cs.lay.payload_off, cs.H.payload_bytes,
                cs.nblocks, 0 });
            H.max_nsyms = std::max(H.max_nsyms, cs.H.max_nsyms);
            H.max_log2_frame = std::max(H.max_log2_frame, cs.H.max_log2_frame);
            H.max_present_m1 = std::max(H.max_present_m1, cs.H.max_present_m1);
            T->nbtot += cs.nblocks;
            if (T->nbtot >= 0xFFFFFFFFull) return false;
        }
        T->G.push_back({ (u64)bbound(H0), (u32)gb0, (u32)T->nslots, H0.block_ints, 0 });
        T->Hs.push_back(H);
        T->nslots += (T->nbtot - gb0 + PB - 1) / PB;
    }
    return true;
}

// ------------------------------------------------------------------------------- batches of lists to encode
// ansx_encode_batch_dev cuts its batch, in order and at list boundaries, into steps: a list alone through the ordinary
// encode, or lists [l0, l1) as one pass of NB blocks.

// A list with this many full blocks amortises its own launches and read-back, and the ordinary path gives it the
// encoder forms a pass cannot take (the buffer-view pipeline of k_encode<1>, k_encode_pc): the (C) criterion of
// choose_encoder_form.  Such a list goes alone.
#define ANSX_ENCB_LONG_BLOCKS 16u

struct EncStep {
    size_t l0, l1;
    u32 NB;  // 0: list l0 alone (l1 = l0 + 1)
};
// The step that starts at list i (< count) of lists offsets[0 .. count] in blocks of bi ints, for passes of at most PB
// blocks.  batched: the geometry has a batched form at all.  Alone goes every list of more than PB blocks or of
// ANSX_ENCB_LONG_BLOCKS full blocks, and a pass ends in front of one.
static inline EncStep encb_step(const u64* offsets, size_t count, size_t i, u64 bi, u32 PB, bool batched)
{
    const u64 n = offsets[i + 1] - offsets[i];
    if (!batched || (n + bi - 1) / bi > PB || n / bi >= ANSX_ENCB_LONG_BLOCKS) return { i, i + 1, 0 };
    size_t j = i;
    u64 blocks = 0;
    while (j < count) {
        const u64 nj = (offsets[j + 1] - offsets[j] + bi - 1) / bi;
        if (blocks + nj > PB || (offsets[j + 1] - offsets[j]) / bi >= ANSX_ENCB_LONG_BLOCKS) break;
        blocks += nj;
        j++;
    }
    return { i, j, (u32)blocks };
}

// Remap classes of a pass's blocks, by block length: ANSrfold's (ansx_rfold.h; below T ints a block cannot have T
// distinct values) and the compaction layer's (ansx_pa.h)
enum { RF_CLS_IDENTITY = 0, RF_CLS_SMALL = 1, RF_CLS_LARGE = 2 };
enum { PA_CLS_SMALL = 0, PA_CLS_LARGE = 1 };
enum { ENCB_REMAP_NONE, ENCB_REMAP_RFOLD, ENCB_REMAP_PA };
static inline u32 encb_class(int remap, u32 T, u32 nb)
{
    if (remap == ENCB_REMAP_PA) return nb <= ANSX_PA_SMALL_INTS ? PA_CLS_SMALL : PA_CLS_LARGE;
    return nb < T ? RF_CLS_IDENTITY : (nb <= ANSX_RF_SMALL_INTS ? RF_CLS_SMALL : RF_CLS_LARGE);
}

// The plan of a pass of NB blocks in nl lists, one upload from pinned memory: blocks | lists | the block ids by remap
// class (where the form has a remap front) -- bytes [0, o_m); behind it on the device: maxima | results | block sums.
// Every section starts on a 16-byte boundary.
struct EncPassLayout {
    size_t o_l, o_i, o_m, o_r, o_s, plan_bytes;
};
static inline EncPassLayout encb_layout(u32 NB, u32 nl, bool ids)
{
    EncPassLayout L;
    L.o_l = sizeof(ansx_blk_in) * (size_t)NB;
    L.o_i = L.o_l + sizeof(ansx_encb_list) * ((size_t)nl + 1);
    L.o_m = L.o_i + (ids ? rup(4 * (size_t)NB, 16) : 0);
    L.o_r = L.o_m + sizeof(ansx_encb_max) * (size_t)nl;
    L.o_s = L.o_r + sizeof(ansx_encb_res) * ((size_t)nl + 1);
    L.plan_bytes = L.o_s + 8 * ((size_t)NB + 1);
    return L;
}

// The tables of the pass over lists [l0, l1), written into the upload image hb (L.o_m bytes): the work list (every
// list's ints in blocks of bi, in order), the list table and -- remap != ENCB_REMAP_NONE -- the block ids by remap
// class, every class's in block order, with the classes' counts in ncls.  -> false if the lists do not have NB blocks.
struct EncPassTables {
    u32 longest;  // ints of the pass's longest block
    u32 ncls[3];
};
static inline bool encb_pass_tables(const u64* offsets, size_t l0, size_t l1, u64 bi, u32 NB, int remap, u32 T, const EncPassLayout& L,
    u8* hb, EncPassTables* out)
{
    ansx_blk_in* hblk = (ansx_blk_in*)hb;
    ansx_encb_list* hl = (ansx_encb_list*)(hb + L.o_l);
    u32 k = 0, longest = 0;
    for (size_t i = l0; i < l1; i++) {
        const u64 n = offsets[i + 1] - offsets[i];
        hl[i - l0] = { n, k, 0 };
        for (u64 at = 0; at < n; at += bi, k++) {
            if (k == NB) return false;  // (the image has room for NB blocks)
            const u32 nb = (u32)std::min<u64>(bi, n - at);
            hblk[k] = { offsets[i] + at, nb, (u32)(i - l0) };
            longest = std::max(longest, nb);
        }
    }
    hl[l1 - l0] = { 0, k, 0 };
    if (k != NB) return false;
    out->longest = longest;
    out->ncls[0] = out->ncls[1] = out->ncls[2] = 0;
    if (remap != ENCB_REMAP_NONE) {  // counted, then every class's ids in block order
        for (u32 b = 0; b < NB; b++) out->ncls[encb_class(remap, T, hblk[b].n)]++;
        u32* hid = (u32*)(hb + L.o_i);
        u32 at[3] = { 0, out->ncls[0], out->ncls[0] + out->ncls[1] };
        for (u32 b = 0; b < NB; b++) hid[at[encb_class(remap, T, hblk[b].n)]++] = b;
    }
    return true;
}

// ------------------------------------------------------------------------------- batches of conjunctive queries
// ansx_intersect_batch_dev cuts its queries, in order, into groups that are decoded and
// intersected together.  Query q names the referenced lists rid[qoff[q] .. qoff[q + 1]) (br_refs' places), list r has
// n[r] ints.  Its driver is the list of fewest ints, of equal ones the earliest position in the query; the others
// follow by ascending n (ties: the earlier position) as its rounds 0, 1, ...

// The ints a group may take -- its referenced lists once and its drivers' twice (two candidate buffers) -- unless
// ANSX_ISECT_BATCH_INTS says otherwise: 2^28 ints, 1 GiB of workspace, the size of section 3h's batch of 4096 lists of
// 64 Ki ids.  A bound on the workspace, not a tuned value: no other budget has been measured.
// ansx_union_batch_dev's groups take the same budget: their lists once and their queries' lists as named twice (two
// merge buffers).
#define ANSX_ISECT_BATCH_INTS_DEFAULT ((u64)1 << 28)

// What isb_plan and unb_plan share.  The lists t[0 .. m) that group gid has not stamped yet -> fresh, their ints -> add.
static inline void plan_fresh(const u32* t, size_t m, const u64* n, u32 gid, std::vector<u32>& stamp, std::vector<u32>& fresh, u64& add)
{
    for (size_t j = 0; j < m; j++)
        if (stamp[t[j]] != gid) stamp[t[j]] = gid, fresh.push_back(t[j]), add += n[t[j]];
}

// ansx_bool_batch_dev: query q also EXCLUDES the referenced lists xrid[xqoff[q] .. xqoff[q + 1]).
// They are decoded with the group's other lists -- a list counts once in the budget, however it is named -- and the
// group gets a second table: query j's excluded lists are xt[xt_off[j] .. xt_off[j + 1]), {at, n} into the buffer of
// ids, an empty list kept as n = 0.  Without xqoff the tables stay empty; a group excludes something when xt is not.
static inline void plan_excl_tables(const u64* n, const u32* xrid, const u64* xqoff, size_t q0, size_t q1,
    const std::vector<u64>& at, const std::vector<u32>& slot, std::vector<u32>* xt_off, std::vector<ansx_isb_list>* xt,
    std::vector<u32>* xt_list)
{
    if (!xqoff) return;
    xt_off->resize(q1 - q0 + 1);
    for (size_t q = q0; q < q1; q++) {
        (*xt_off)[q - q0] = (u32)xt->size();
        for (u64 j = xqoff[q]; j < xqoff[q + 1]; j++) {
            const u32 r = xrid[j];
            xt->push_back({ n[r] ? at[slot[r]] : 0, n[r] });
            xt_list->push_back(r);
        }
    }
    (*xt_off)[q1 - q0] = (u32)xt->size();
}

struct IsbGroup {
    size_t q0, q1;                   // its queries
    std::vector<u32> lists;          // the non-empty referenced lists it decodes, ascending: its buffer, back to back
    std::vector<u64> at;             // lists.size() + 1: where each one's ids start in the buffer; the last: its ints
    std::vector<ansx_isb_query> G;   // q1 - q0 + 1: every query's driver and segment; the last closes them
    std::vector<u32> rt_off;         // q1 - q0 + 1: query j's rounds are rt[rt_off[j] .. rt_off[j + 1])
    std::vector<ansx_isb_list> rt;   // the round table
    std::vector<u32> rt_list, drv;   // the referenced list behind every entry of rt, and every query's driver (what the CPU check holds the tables against)
    std::vector<u32> xt_off;         // with exclusions (plan_excl_tables): q1 - q0 + 1
    std::vector<ansx_isb_list> xt;   // ... every query's excluded lists
    std::vector<u32> xt_list;        // ... the referenced list behind every entry of xt
    std::vector<u32> dterm, rterm;   // with want_terms (ansx_topk_bool_batch_dev): the named term (its place in rid) behind
                                     // every query's driver and behind every entry of rt -- a ranked query lays its weights there
    std::vector<u32> ot_off;         // with optional terms (ansx_topk_query_batch_dev; plan_excl_tables over them): q1 - q0 + 1
    std::vector<ansx_isb_list> ot;   // ... every query's optional lists
    std::vector<u32> ot_list, oterm; // ... the referenced list behind every entry of ot, and the named term (its place in
                                     // orid) -- the optional step lays its weights there
    u64 ints;                        // buffer + twice the candidates: what the budget bounds
    u32 rounds;                      // most rounds of a query
};

// -> ANSX_OK, or ANSX_ERR_ARG with *bad_query the first query whose driver has 2^32 ints or more (a step takes at most
// 2^32 - 1 candidates).  A group ends in front of the query that would take it over `budget` ints or its candidates to
// 2^32; a query over the budget alone is a group of its own.  A list two groups name is decoded in both.
// xrid / xqoff: null, or the lists every query excludes (plan_excl_tables).
// want_terms: dterm and rterm are filled beside drv and rt; nothing else differs.
// orid / oqoff: null, or the OPTIONAL terms of every query (ansx_topk_query_batch_dev; rid / qoff are then its required
// terms): their lists are decoded with the group's and count once in the budget as the excluded ones do, and the group
// gets the tables ot_off / ot / ot_list / oterm.  They choose no driver and take no round.
static inline int isb_plan(const u64* n, size_t nref, const u32* rid, const u64* qoff, size_t nq, u64 budget,
    std::vector<IsbGroup>* groups, size_t* bad_query, const u32* xrid = nullptr, const u64* xqoff = nullptr,
    bool want_terms = false, const u32* orid = nullptr, const u64* oqoff = nullptr)
{
    groups->clear();
    std::vector<u32> stamp(nref, 0xFFFFFFFFu), slot(nref, 0), fresh, ord;
    for (size_t q = 0; q < nq;) {
        groups->emplace_back();
        IsbGroup& g = groups->back();
        const u32 gid = (u32)(groups->size() - 1);
        g.q0 = q, g.ints = 0, g.rounds = 0;
        u64 cand = 0;
        for (; q < nq; q++) {  // the queries it takes
            const u32* t = rid + qoff[q];
            const size_t m = (size_t)(qoff[q + 1] - qoff[q]);
            u64 nd = n[t[0]], add = 0;
            for (size_t j = 1; j < m; j++) nd = std::min(nd, n[t[j]]);
            if (nd > 0xFFFFFFFFull) {
                if (bad_query) *bad_query = q;
                return ANSX_ERR_ARG;
            }
            fresh.clear();
            plan_fresh(t, m, n, gid, stamp, fresh, add);
            if (xqoff) plan_fresh(xrid + xqoff[q], (size_t)(xqoff[q + 1] - xqoff[q]), n, gid, stamp, fresh, add);
            if (oqoff) plan_fresh(orid + oqoff[q], (size_t)(oqoff[q + 1] - oqoff[q]), n, gid, stamp, fresh, add);
            add += 2 * nd;
            // (the stamps of a query that does not fit stay behind: the next group has another number)
            if (q > g.q0 && (add > budget || g.ints > budget - add || cand + nd > 0xFFFFFFFFull)) break;
            for (const u32 r : fresh)
                if (n[r]) g.lists.push_back(r);
            g.ints += add, cand += nd;
        }
        g.q1 = q;
        std::sort(g.lists.begin(), g.lists.end());
        g.at.resize(g.lists.size() + 1);
        u64 at = 0;
        for (size_t k = 0; k < g.lists.size(); k++) g.at[k] = at, slot[g.lists[k]] = (u32)k, at += n[g.lists[k]];
        g.at.back() = at;
        const size_t Q = g.q1 - g.q0;
        g.G.resize(Q + 1), g.rt_off.resize(Q + 1), g.drv.resize(Q);
        g.rt.reserve((size_t)(qoff[g.q1] - qoff[g.q0]) - Q), g.rt_list.reserve(g.rt.capacity());
        u64 dst = 0;
        for (size_t j = 0; j < Q; j++) {
            const u32* t = rid + qoff[g.q0 + j];
            const size_t m = (size_t)(qoff[g.q0 + j + 1] - qoff[g.q0 + j]);
            ord.resize(m);
            for (size_t k = 0; k < m; k++) ord[k] = (u32)k;
            std::stable_sort(ord.begin(), ord.end(), [&](u32 x, u32 y) { return n[t[x]] < n[t[y]]; });
            const u32 d = t[ord[0]];
            g.drv[j] = d;
            if (want_terms) g.dterm.push_back((u32)(qoff[g.q0 + j] + ord[0]));
            g.G[j] = { n[d] ? g.at[slot[d]] : 0, dst };
            dst += n[d];
            g.rt_off[j] = (u32)g.rt.size();
            for (size_t k = 1; k < m; k++) {
                const u32 r = t[ord[k]];
                g.rt.push_back({ n[r] ? g.at[slot[r]] : 0, n[r] });
                g.rt_list.push_back(r);
                if (want_terms) g.rterm.push_back((u32)(qoff[g.q0 + j] + ord[k]));
            }
            g.rounds = std::max(g.rounds, (u32)(m - 1));
        }
        g.G[Q] = { 0, dst };
        g.rt_off[Q] = (u32)g.rt.size();
        plan_excl_tables(n, xrid, xqoff, g.q0, g.q1, g.at, slot, &g.xt_off, &g.xt, &g.xt_list);
        plan_excl_tables(n, orid, oqoff, g.q0, g.q1, g.at, slot, &g.ot_off, &g.ot, &g.ot_list);
        if (oqoff)
            for (u64 j = oqoff[g.q0]; j < oqoff[g.q1]; j++) g.oterm.push_back((u32)j);
    }
    return ANSX_OK;
}

// ------------------------------------------------------------------------------- batches of disjunctive queries
// ansx_union_batch_dev cuts its queries, in order, into groups as isb_plan does, under the same
// budget (ANSX_ISECT_BATCH_INTS): the group's referenced lists once and, twice, the ints of every query's lists as
// named -- the two merge buffers, in which query j's runs stand back to back in query order from seg[j] on.
//
// A query of m terms takes rq = max(1, ceil(log2 m)) rounds of pairwise merges; the group takes R, the most of its
// queries, and query j runs in the LAST rq of them, so that all queries end in the same buffer and none is copied
// through a round it has no merge in.  Its first round reads the runs where the decode left them, in the buffer of
// lists; round r writes merge buffer r & 1 and, from a query's second round on, reads the other.  In its local round
// k, runs 2i and 2i + 1 of 2^k terms each become one at the place of the first; a run without a partner is a pair
// with nb = 0.  A pair of no ints is left out.  A pair's span is the same before and after, so every offset of every
// round is known here.

struct UnbGroup {
    size_t q0, q1;                     // its queries
    std::vector<u32> lists;            // the non-empty referenced lists it decodes, ascending: its buffer, back to back
    std::vector<u64> at;               // lists.size() + 1: where each one's ids start in the buffer; the last: its ints
    std::vector<u32> seg;              // q1 - q0 + 1: query j's span of the merge buffers; the last: their ints
    std::vector<ansx_unb_pair> pairs;  // every round's pairs, round after round, queries in order inside a round
    std::vector<u32> roff;             // rounds + 1: round r's pairs are pairs[roff[r] .. roff[r + 1])
    std::vector<u64> tiles;            // rounds: the tiles of round r
    std::vector<u32> xt_off;           // with exclusions (plan_excl_tables): q1 - q0 + 1
    std::vector<ansx_isb_list> xt;     // ... every query's excluded lists
    std::vector<u32> xt_list;          // ... the referenced list behind every entry of xt
    std::vector<u32> pterm;            // with want_terms (ansx_topk_batch_dev): two per pair -- the named term (its place in
                                       // rid) sides a and b of a first-round pair came from, ANSX_TOPK_NONE for a side of no
                                       // ints and for every side of a later round
    u64 ints;                          // buffer + twice the merge buffer: what the budget bounds
    u32 rounds;                        // R
};

static inline u32 unb_rounds(u64 m)
{
    u32 r = 0;
    while (((u64)1 << r) < m) r++;
    return r ? r : 1u;
}

// -> ANSX_OK, or ANSX_ERR_ARG with *bad_query the first query whose lists together have 2^32 ints or more (a run offset
// is a u32).  A group ends in front of the query that would take it over `budget` ints or its merge buffer to 2^32; a
// query over the budget alone is a group of its own.  A list two groups name is decoded in both.  tile: the outputs
// of a workgroup of the merge.  xrid / xqoff: null, or the lists every query excludes (plan_excl_tables).
// want_terms: pterm is filled beside pairs (a ranked query lays its weights there); nothing else differs.
static inline int unb_plan(const u64* n, size_t nref, const u32* rid, const u64* qoff, size_t nq, u64 budget, u32 tile,
    std::vector<UnbGroup>* groups, size_t* bad_query, const u32* xrid = nullptr, const u64* xqoff = nullptr,
    bool want_terms = false)
{
    groups->clear();
    std::vector<u64> tot(nq);
    for (size_t q = 0; q < nq; q++) {
        u64 a = 0;
        for (u64 j = qoff[q]; j < qoff[q + 1] && a <= 0xFFFFFFFFull; j++) a = n[rid[j]] > 0xFFFFFFFFull ? ~0ull : a + n[rid[j]];
        if (a > 0xFFFFFFFFull) {
            if (bad_query) *bad_query = q;
            return ANSX_ERR_ARG;
        }
        tot[q] = a;
    }
    std::vector<u32> stamp(nref, 0xFFFFFFFFu), slot(nref, 0), fresh;
    std::vector<std::vector<ansx_unb_pair>> byround;
    std::vector<std::vector<u32>> byterm;   // (want_terms: two per pair of byround)
    std::vector<std::pair<u32, u32>> runs;  // (where in the merge buffers, ints)
    for (size_t q = 0; q < nq;) {
        groups->emplace_back();
        UnbGroup& g = groups->back();
        const u32 gid = (u32)(groups->size() - 1);
        g.q0 = q, g.ints = 0, g.rounds = 1;
        u64 merge = 0;
        for (; q < nq; q++) {  // the queries it takes
            const u32* t = rid + qoff[q];
            const size_t m = (size_t)(qoff[q + 1] - qoff[q]);
            u64 add = 0;
            fresh.clear();
            plan_fresh(t, m, n, gid, stamp, fresh, add);
            if (xqoff) plan_fresh(xrid + xqoff[q], (size_t)(xqoff[q + 1] - xqoff[q]), n, gid, stamp, fresh, add);
            add += 2 * tot[q];
            // (the stamps of a query that does not fit stay behind: the next group has another number)
            if (q > g.q0 && (add > budget || g.ints > budget - add || merge + tot[q] > 0xFFFFFFFFull)) break;
            for (const u32 r : fresh)
                if (n[r]) g.lists.push_back(r);
            g.ints += add, merge += tot[q];
            g.rounds = std::max(g.rounds, unb_rounds(m));
        }
        g.q1 = q;
        std::sort(g.lists.begin(), g.lists.end());
        g.at.resize(g.lists.size() + 1);
        u64 at = 0;
        for (size_t k = 0; k < g.lists.size(); k++) g.at[k] = at, slot[g.lists[k]] = (u32)k, at += n[g.lists[k]];
        g.at.back() = at;
        const size_t Q = g.q1 - g.q0;
        const u32 R = g.rounds;
        g.seg.resize(Q + 1);
        byround.assign(R, {});
        byterm.assign(want_terms ? R : 0, {});
        u32 dst = 0;
        for (size_t j = 0; j < Q; j++) {
            const u32* t = rid + qoff[g.q0 + j];
            const size_t m = (size_t)(qoff[g.q0 + j + 1] - qoff[g.q0 + j]);
            g.seg[j] = dst;
            runs.resize(m);
            for (size_t k = 0; k < m; k++) runs[k] = { dst, (u32)n[t[k]] }, dst += (u32)n[t[k]];
            const u32 rq = unb_rounds(m);
            size_t have = m;
            for (u32 k = 0; k < rq; k++, have = (have + 1) / 2)
                for (size_t i = 0; 2 * i < have; i++) {
                    const std::pair<u32, u32> A = runs[2 * i], B = 2 * i + 1 < have ? runs[2 * i + 1] : std::pair<u32, u32>(0, 0);
                    runs[i] = { A.first, A.second + B.second };
                    if (A.second + B.second == 0) continue;
                    ansx_unb_pair p = { A.first, B.first, A.second, B.second, A.first, 0, 0, 0 };
                    if (k == 0) {  // where the decode left them
                        const u32 ra = t[2 * i], rb = 2 * i + 1 < m ? t[2 * i + 1] : ra;
                        p.a = A.second ? g.at[slot[ra]] : 0, p.b = B.second ? g.at[slot[rb]] : 0, p.from_lists = 1;
                    }
                    byround[R - rq + k].push_back(p);
                    if (want_terms) {
                        const u64 ta = qoff[g.q0 + j] + 2 * i;
                        byterm[R - rq + k].push_back(k == 0 && A.second ? (u32)ta : ANSX_TOPK_NONE);
                        byterm[R - rq + k].push_back(k == 0 && B.second ? (u32)(ta + 1) : ANSX_TOPK_NONE);
                    }
                }
        }
        g.seg[Q] = dst;
        g.roff.assign(1, 0), g.tiles.clear();
        for (u32 r = 0; r < R; r++) {
            u64 first = 0;
            for (ansx_unb_pair& p : byround[r]) {
                p.tile = (u32)first;  // (the caller refuses a round of 2^31 tiles or more)
                first += ((u64)p.na + p.nb + tile - 1) / tile;
            }
            g.pairs.insert(g.pairs.end(), byround[r].begin(), byround[r].end());
            if (want_terms) g.pterm.insert(g.pterm.end(), byterm[r].begin(), byterm[r].end());
            g.roff.push_back((u32)g.pairs.size());
            g.tiles.push_back(first);
        }
        plan_excl_tables(n, xrid, xqoff, g.q0, g.q1, g.at, slot, &g.xt_off, &g.xt, &g.xt_list);
    }
    return ANSX_OK;
}

// ------------------------------------------------------------------------------- required, optional, excluded terms
// ansx_topk_query_batch_dev.  The terms of every query, split by occur (null: all optional): the
// required ones for isb_plan's rid / qoff, the optional ones for its orid / oqoff, each with its list (rid[j], the
// front end's entry of term j) and its place j in the caller's arrays, which is where its weight stands.  msm (null: all
// zero) -> m: the threshold as it applies, msm[q] with a required term and max(msm[q], 1) without one.
struct QuerySplit {
    std::vector<u32> rrid, rpos, orid, opos;  // per required / per optional term: its list and its place in `terms`
    std::vector<u64> rqoff, oqoff;            // nq + 1 each
    std::vector<u32> m;                       // nq
};
static inline void query_split(const u32* rid, const u8* occur, const u64* qoff, const u32* msm, size_t nq, QuerySplit* S)
{
    S->rqoff.assign(nq + 1, 0), S->oqoff.assign(nq + 1, 0), S->m.resize(nq);
    for (size_t q = 0; q < nq; q++) {
        for (u64 j = qoff[q]; j < qoff[q + 1]; j++)
            if (occur && occur[j]) S->rrid.push_back(rid[j]), S->rpos.push_back((u32)j);
            else S->orid.push_back(rid[j]), S->opos.push_back((u32)j);
        S->rqoff[q + 1] = S->rrid.size(), S->oqoff[q + 1] = S->orid.size();
        const u32 t = msm ? msm[q] : 0u;
        S->m[q] = S->rqoff[q + 1] > S->rqoff[q] ? t : std::max(t, 1u);
    }
}

// The batch cut into maximal runs [a, b) of consecutive queries of one kind: req, "has a required term", or not.  Every
// run is planned by its kind's planner and its groups run in batch order.
struct QueryRun {
    size_t a, b;
    bool req;
};
static inline void query_runs(const u64* rqoff, size_t nq, std::vector<QueryRun>* runs)
{
    runs->clear();
    for (size_t q = 0; q < nq; q++) {
        const bool req = rqoff[q + 1] > rqoff[q];
        if (runs->empty() || runs->back().req != req) runs->push_back({ q, q + 1, req });
        else runs->back().b = q + 1;
    }
}

// The whole plan of a call: the split, the runs and every run's groups -- req for a run with required terms (isb_plan
// over them, the optional terms as orid / oqoff), opt for one without (unb_plan over the terms) -- with the groups' q0 / q1
// as the CALL's query numbers.
struct QueryPlan {
    struct Run {
        std::vector<IsbGroup> req;
        std::vector<UnbGroup> opt;
    };
    QuerySplit split;
    std::vector<QueryRun> runs;
    std::vector<Run> plans;  // one per run
};

// rid: the front end's entry of every term, xrid / xqoff (null: nothing is excluded) of every excluded term; tile: the
// outputs of a workgroup of the merge.  Every run is planned by its kind's planner over its own queries -- the offset
// arrays advanced to the run's first query, the term arrays whole -- under `budget`, and ALL runs are planned before the
// caller launches anything.  -> ANSX_OK, or ANSX_ERR_ARG with *bad_query the first query in BATCH order that exceeds
// its plan's limits: with a required term its shortest required list has 2^32 ints or more (isb_plan); without one its
// lists together have (unb_plan), or its group's round of merges has 2^31 tiles or more (then the group's first query).
static inline int query_plan(const u64* n, size_t nref, const u32* rid, const u8* occur, const u64* qoff, const u32* msm,
    const u32* xrid, const u64* xqoff, size_t nq, u64 budget, u32 tile, QueryPlan* P, size_t* bad_query)
{
    query_split(rid, occur, qoff, msm, nq, &P->split);
    const QuerySplit& S = P->split;
    query_runs(S.rqoff.data(), nq, &P->runs);
    P->plans.assign(P->runs.size(), {});
    for (size_t r = 0; r < P->runs.size(); r++) {
        const size_t a = P->runs[r].a, cnt = P->runs[r].b - a;
        const u64* xq = xqoff ? xqoff + a : nullptr;
        size_t bad = 0;  // (the planners count from the run's first query)
        int rc;
        if (P->runs[r].req) {
            rc = isb_plan(n, nref, S.rrid.data(), S.rqoff.data() + a, cnt, budget, &P->plans[r].req, &bad, xrid, xq, true, S.orid.data(),
                S.oqoff.data() + a);
            for (IsbGroup& g : P->plans[r].req) g.q0 += a, g.q1 += a;
        } else {
            rc = unb_plan(n, nref, rid, qoff + a, cnt, budget, tile, &P->plans[r].opt, &bad, xrid, xq, true);
            for (UnbGroup& g : P->plans[r].opt) {
                for (size_t k = 0; !rc && k < g.tiles.size(); k++)
                    if (g.tiles[k] > 0x7FFFFFFFull) rc = ANSX_ERR_ARG, bad = g.q0;  // (a grid; g.q0: still the run's own number)
                g.q0 += a, g.q1 += a;
            }
        }
        if (rc) {
            if (bad_query) *bad_query = a + bad;
            return rc;
        }
    }
    return ANSX_OK;
}

// ------------------------------------------------------------------------------- length-normalised scores
// ansx_topk_scored_batch_dev (ansx_topk_scored.h).  The lists of a group that k_topk_impacts
// rewrites: list lists[k] of the group, ints [at[k], at[k + 1]) of its buffers, gets an entry when it has ints and a
// payload (payof: per referenced list the entry of its payload or ANSX_TOPK_NONE -- a list that is only excluded has
// none; null: no list has one), in the order of the buffer, with the tiles of `tile` ints in front of it and its place
// k, which is what the scan's flag word names.  *tiles: the launch's tiles.  A group's lists are distinct, so a list
// several queries name is rewritten once.  -> ANSX_OK, or ANSX_ERR_ARG where the tiles exceed 2^31 - 1 (a grid, as
// merge_tiles_check has it for a round of merges).
static inline int impact_plan(const std::vector<u32>& lists, const std::vector<u64>& at, const std::vector<u32>* payof, u32 tile,
    std::vector<ansx_impact_list>* P, u64* tiles)
{
    P->clear();
    u64 t = 0;
    for (size_t k = 0; k < lists.size(); k++) {
        const u64 n = at[k + 1] - at[k];
        if (n == 0 || !payof || (*payof)[lists[k]] == ANSX_TOPK_NONE) continue;
        if (t > 0x7FFFFFFFull) return ANSX_ERR_ARG;  // (and no entry's `tile` wraps)
        P->push_back({ at[k], n, (u32)t, (u32)k });
        t += impact_tiles(at[k], n, tile);
    }
    *tiles = t;
    return t > 0x7FFFFFFFull ? ANSX_ERR_ARG : ANSX_OK;
}

}  // namespace ansx_plan
