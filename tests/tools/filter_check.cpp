// The filter step of ansx_topk_filter_batch_dev on the CPU (ans_large_alphabet_amd/csrc/ansx_query_tile.h: filter_lookup,
// filter_pass, filter_prior_bit, filter_and, filter_tile_count, and the frame's qt_limit, qt_tile_queries, qt_elem,
// isb_query_of -- the arithmetic k_filter_mark runs), over made-up candidates, bounds, columns and clauses.
//   1. Both forms of the kernel RUN the way ansx_filter.h runs them, thread by thread: a workgroup per tile of the host's
//      bound n, the limit from the device's total, a tile at or beyond it zeroed, the queries of the tile's ends, then per
//      candidate "alive" -- below the limit and, in the fused form, its bit in the ballot word the step in front wrote --
//      the id check in 64 bits, the clauses in order up to the first that fails, the ballot word per wave and the tile's
//      count.  Every read of a candidate goes through an accessor that refuses h at or beyond the limit, a column is a
//      function that refuses an id of ndocs or more, a clause is read through an accessor that refuses an entry outside
//      the query's range of the table, and a ballot word is written only where isect_ballot writes it.
//   2. The judge: a brute-force filter, query by query: the kept candidates, the smallest query with a live bad id, and the
//      number of column reads (no clause behind the first that fails, nothing for a dead candidate or a query without
//      clauses).
// Cases: totals of 0, 1, 63, 64, 65, 1023, 1024, 1025 and several tiles; a device total above and below n; one query,
// thousands of queries of 0 to 7 candidates, a long query between short ones, empty queries at both ends; 0, 1, 2 and 16
// clauses and queries with and without clauses in one tile; lo == hi, lo > hi and [0, 0xFFFFFFFF], each with and without
// NOT; values at lo - 1, lo, hi, hi + 1; ids at ndocs - 1 and ndocs, and ndocs = 2^32 with the id 0xFFFFFFFF; a prior
// ballot of all ones, all zeros and random; a dead candidate with a bad id is not reported.
// Built with -fsanitize=address,undefined and run by tests/test_filter_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_query_tile.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static const u32 NONE = 0xFFFFFFFFu;  // ANSX_TOPK_NONE
static const u32 NT = ANSX_ISECT_NT, TILE = ANSX_ISECT_TILE, WORDS = ANSX_ISECT_WORDS;
static long checks = 0;
static const char* what = "";
#define CHECK(cond)                                                                \
    do {                                                                           \
        checks++;                                                                  \
        if (!(cond)) {                                                             \
            fprintf(stderr, "%s:%d: %s -- %s\n", __FILE__, __LINE__, #cond, what); \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

static u32 mix(u32 x) { return (u32)(((u64)x * 2654435761ull) >> 7) ^ (x >> 3); }

struct Clause {
    u32 column, lo, hi, flags;
};

struct Columns {  // the value of every id below ndocs in every column, as a function: ndocs may be 2^32
    u64 ndocs;
    mutable u64 reads = 0;
    u32 at(u32 column, u32 id) const
    {
        CHECK((u64)id < ndocs);  // (the kernel compares before it reads)
        reads++;
        const u32 m = mix(id * 7u + column);
        if (m % 13u == 0) return 0xFFFFFFFFu;  // a caller's "no field": a value like any other
        if (m % 17u == 0) return 0u;
        return 100u + (m >> 4) % 10u;  // 100 .. 109: the bounds below lie at and around them
    }
};

struct Cands {  // the candidates of a group as the steps in front leave them
    std::vector<u32> ids, hseg;  // hseg: Q + 1 bounds
    u32 n;                       // the host's bound
    u64 total;                   // the device's count
    std::vector<u32> foff;       // Q + 1 offsets into cl
    std::vector<Clause> cl;
    std::vector<u64> prior;      // the fused form: the ballot words of the step in front, ceil(n / 64)
    u32 Q() const { return (u32)hseg.size() - 1; }
};

struct Out {
    std::vector<u64> ballots;
    std::vector<u64> counts;
    u32 bad = NONE;
    u64 reads = 0;
};

static void brute(const Cands& c, const Columns& col, bool prior, Out* o)
{
    const u64 tot = std::min<u64>(c.total, c.n);
    o->ballots.assign(((size_t)c.n + 63) / 64, 0), o->counts.assign(((size_t)c.n + TILE - 1) / TILE, 0);
    col.reads = 0;
    for (u32 j = 0; j < c.Q(); j++)
        for (u64 h = c.hseg[j]; h < c.hseg[j + 1] && h < tot; h++) {
            bool keep = !prior || ((c.prior[(size_t)(h >> 6)] >> (h & 63u)) & 1u);
            const u32 id = c.ids[(size_t)h];
            if (keep && c.foff[j] < c.foff[j + 1]) {
                if ((u64)id >= col.ndocs) o->bad = std::min(o->bad, j), keep = false;
                for (u32 e = c.foff[j]; keep && e < c.foff[j + 1]; e++) {
                    const Clause& k = c.cl[e];
                    const u32 v = col.at(k.column, id);
                    const bool in = k.lo <= v && v <= k.hi;
                    keep = (k.flags & 1u) ? !in : in;
                }
            }
            if (keep) o->ballots[(size_t)(h >> 6)] |= 1ull << (h & 63u), o->counts[(size_t)(h / TILE)]++;
        }
    o->reads = col.reads;
}

// k_filter_mark<PRIOR>, a workgroup after the other, a wave after the other, a lane after the other
static void run_kernel(const Cands& c, const Columns& col, bool prior, Out* o)
{
    const u64* total = &c.total;
    const u64 tot = qt_limit(total, c.n);
    const u32 grid = (u32)(((u64)c.n + TILE - 1) / TILE);  // the host's: the tiles of n
    const size_t nwords = ((size_t)c.n + 63) / 64;
    // (what the launch finds: the step's in front, or, in the own form, anything -- every word below n is written)
    o->ballots = prior ? c.prior : std::vector<u64>(nwords, 0xDEADBEEFDEADBEEFull);
    o->counts.assign(grid, 0xDEADull);
    col.reads = 0;
    std::vector<u8> seen((size_t)c.n, 0);
    auto id_at = [&](u64 h) {
        CHECK(h < tot && h < c.ids.size() && !seen[(size_t)h]);  // every candidate below the limit, once
        seen[(size_t)h] = 1;
        return c.ids[(size_t)h];
    };
    auto clause = [&](u32 j, u32 e) -> const Clause& {
        CHECK(j < c.Q() && e >= c.foff[j] && e < c.foff[j + 1] && e < c.cl.size());
        return c.cl[e];
    };
    for (u32 b = 0; b < grid; b++) {
        const u64 i0 = (u64)b * TILE;
        if (i0 >= tot) {
            for (u32 tid = 0; tid < WORDS; tid++)
                if (i0 + 64ull * tid < c.n) {
                    CHECK((size_t)((i0 >> 6) + tid) < nwords);
                    o->ballots[(size_t)((i0 >> 6) + tid)] = 0;
                }
            o->counts[b] = 0;
            continue;
        }
        u32 qb[2], wcnt[WORDS];
        qt_tile_queries(c.hseg.data(), c.Q(), i0, (u32)tot, qb);
        CHECK(qb[0] <= qb[1] && qb[1] < c.Q());
        for (u32 wave = 0; wave < NT / 64u; wave++)
            for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
                u64 bal = 0, pw = ~0ull;
                const u64 w0 = qt_elem(i0, k, wave * 64u);  // the wave's first candidate
                if (prior && w0 < tot) {
                    CHECK((size_t)(w0 >> 6) < nwords);
                    pw = o->ballots[(size_t)(w0 >> 6)];  // (read before this wave writes it)
                }
                for (u32 lane = 0; lane < 64u; lane++) {
                    const u32 tid = wave * 64u + lane;
                    const u64 h = qt_elem(i0, k, tid);
                    bool alive = h < tot;
                    if (prior && alive) alive = filter_prior_bit(pw, lane);
                    const u32 id = h < tot ? id_at(h) : 0u;
                    if (alive) {
                        const u32 j = qb[0] == qb[1] ? qb[0] : isb_query_of(c.hseg.data(), qb[0], qb[1], (u32)h);
                        CHECK(j < c.Q() && c.hseg[j] <= h && h < c.hseg[j + 1]);
                        const u32 e1 = c.foff[j + 1];
                        u32 e = c.foff[j];
                        if (e < e1 && !filter_lookup(id, col.ndocs)) o->bad = std::min(o->bad, j), alive = false;
                        for (; alive && e < e1; e++) {
                            const Clause& cl = clause(j, e);
                            alive = filter_pass(col.at(cl.column, id), cl.lo, cl.hi, cl.flags);
                        }
                    }
                    if (alive) bal |= 1ull << lane;
                }
                CHECK(bal == filter_and(pw, bal));  // (the fused form only clears bits)
                // isect_ballot: lane 0 writes the word when the wave's first candidate is one, and the popcount
                if (w0 < c.n) {
                    CHECK((size_t)(w0 >> 6) < nwords);
                    o->ballots[(size_t)(w0 >> 6)] = bal;
                }
                wcnt[k * (NT / 64u) + wave] = (u32)__builtin_popcountll(bal);
            }
        o->counts[b] = filter_tile_count(wcnt);
    }
    for (u64 h = 0; h < tot; h++) CHECK(seen[(size_t)h]);
    o->reads = col.reads;
}

// ---- the cases -----------------------------------------------------------------------------------------------------
enum Shape { ONE, MANY, LONG_BETWEEN, EMPTY_ENDS };
enum ClauseMode { C_NONE, C_ONE, C_TWO, C_SIXTEEN, C_MIXED };
enum Docs { D_ALL, D_LAST_BAD, D_FULL32 };

static Clause draw_clause(std::mt19937& rng)
{
    Clause k;
    k.column = rng() % 3u, k.flags = rng() & 1u;
    switch (rng() % 6u) {
    case 0: k.lo = k.hi = 100u + rng() % 10u; break;         // lo == hi
    case 1: k.lo = 106u, k.hi = 103u; break;                 // lo > hi: the empty range
    case 2: k.lo = 0u, k.hi = 0xFFFFFFFFu; break;            // everything
    case 3: k.lo = 0u, k.hi = 100u + rng() % 10u; break;     // "<= x": takes the zeros
    case 4: k.lo = 100u + rng() % 10u, k.hi = 0xFFFFFFFFu; break;  // ">= x": takes the markers
    default: k.lo = 99u + rng() % 6u, k.hi = k.lo + rng() % 6u; break;  // values at lo - 1, lo, hi, hi + 1 all occur
    }
    return k;
}

static void make(Shape shape, u64 total, int nmode, ClauseMode cm, Docs dm, int pm, u32 seed, Cands* c, Columns* col)
{
    std::mt19937 rng(seed);
    // the queries' sizes, summing to total
    std::vector<u64> len;
    if (shape == ONE) len = { total };
    else if (shape == MANY) {
        for (u64 left = total; left > 0 || len.empty();) {
            const u64 l = std::min<u64>(left, rng() % 8u);
            len.push_back(l), left -= l;
            if (len.size() > 100000) break;
        }
    } else if (shape == LONG_BETWEEN) {
        const u64 s = std::min<u64>(total / 4, 5);
        len = { s, 0, std::min<u64>(3, total - s), 0, 0, 0 };
        const u64 used = len[0] + len[2];
        const u64 tail = std::min<u64>(total - used, 7);
        len[3] = total - used - tail, len[4] = tail / 2, len[5] = tail - tail / 2;
    } else {
        len = { 0, 0, total / 2, total - total / 2, 0, 0, 0 };
    }
    c->hseg.assign(1, 0);
    for (u64 l : len) c->hseg.push_back((u32)(c->hseg.back() + l));
    c->total = total;
    c->n = nmode == 0 ? (u32)total : nmode == 1 ? (u32)(total - std::min<u64>(total, 1 + rng() % 70u)) : (u32)(total + 1 + rng() % 1500u);
    // ids: ascending inside a query, a step of 1 or 2; room for max(n, total) of them so that every h < n is there
    const size_t room = (size_t)std::max<u64>(c->n, total);
    c->ids.assign(room, 0);
    u32 top = 0;
    for (u32 j = 0; j < c->Q(); j++) {
        u32 id = rng() % 50u;
        for (u64 h = c->hseg[j]; h < c->hseg[j + 1]; h++) c->ids[(size_t)h] = id, top = std::max(top, id), id += 1u + (rng() & 1u);
    }
    for (size_t h = (size_t)total; h < room; h++) c->ids[h] = 0xFFFFFFF0u;  // (beyond the device's total: never looked at)
    col->ndocs = dm == D_ALL ? (u64)top + 1 : dm == D_LAST_BAD ? (u64)std::max(top, 1u) : 1ull << 32;  // ids at ndocs - 1 and ndocs
    if (dm == D_FULL32 && total > 0) {  // the last candidate of the last query that has one: 0xFFFFFFFF is a good id
        for (u32 j = c->Q(); j-- > 0;)
            if (c->hseg[j + 1] > c->hseg[j]) {
                c->ids[c->hseg[j + 1] - 1] = 0xFFFFFFFFu;
                break;
            }
    }
    c->foff.assign(1, 0), c->cl.clear();
    for (u32 j = 0; j < c->Q(); j++) {
        const u32 k = cm == C_NONE ? 0u : cm == C_ONE ? 1u : cm == C_TWO ? 2u : cm == C_SIXTEEN ? 16u
            : (rng() % 3u == 0 ? 0u : rng() % 9u == 0 ? 16u : 1u + rng() % 3u);
        for (u32 e = 0; e < k; e++) c->cl.push_back(draw_clause(rng));
        c->foff.push_back((u32)c->cl.size());
    }
    c->prior.assign(((size_t)c->n + 63) / 64, pm == 1 ? ~0ull : 0ull);
    if (pm == 3)
        for (u64& w : c->prior) w = ((u64)rng() << 32) | rng();
}

int main()
{
    const u64 totals[] = { 0, 1, 63, 64, 65, 1023, 1024, 1025, 3000, 5121 };
    long cases = 0, kept = 0, dropped = 0, bads = 0, dead_bad = 0;
    char name[160];
    for (u64 total : totals)
        for (int shape = ONE; shape <= EMPTY_ENDS; shape++)
            for (int nmode = 0; nmode < 3; nmode++)
                for (int cm = C_NONE; cm <= C_MIXED; cm++)
                    for (int dm = D_ALL; dm <= D_FULL32; dm++)
                        for (int pm = 0; pm < 4; pm++) {  // 0: the own form; 1 .. 3: fused, a prior of ones, zeros, random
                            snprintf(name, sizeof name, "total %llu shape %d nmode %d clauses %d docs %d prior %d",
                                (unsigned long long)total, shape, nmode, cm, dm, pm);
                            what = name;
                            Cands c;
                            Columns col;
                            make((Shape)shape, total, nmode, (ClauseMode)cm, (Docs)dm, pm, (u32)(cases * 7919 + 1), &c, &col);
                            Out exp, got;
                            brute(c, col, pm != 0, &exp);
                            run_kernel(c, col, pm != 0, &got);
                            CHECK(got.ballots == exp.ballots);
                            CHECK(got.counts == exp.counts);
                            CHECK(got.bad == exp.bad);
                            CHECK(got.reads == exp.reads);
                            if (cm == C_NONE || pm == 2) CHECK(got.reads == 0 && got.bad == NONE);  // nothing is looked up
                            if (cm == C_NONE && pm == 0) {  // not filtered: every candidate below the limit is kept
                                u64 sum = 0;
                                for (u64 x : got.counts) sum += x;
                                CHECK(sum == std::min<u64>(c.total, c.n));
                            }
                            const u64 tot = std::min<u64>(c.total, c.n);
                            for (u64 h = 0; h < tot; h++) ((got.ballots[(size_t)(h >> 6)] >> (h & 63u)) & 1u) ? kept++ : dropped++;
                            bads += got.bad != NONE;
                            if (pm == 3 && dm == D_LAST_BAD && cm != C_NONE) {  // a dead candidate with a bad id is not reported
                                Out all;
                                brute(c, col, false, &all);
                                dead_bad += all.bad != NONE && (got.bad == NONE || got.bad > all.bad);
                            }
                            cases++;
                        }
    what = "coverage";
    CHECK(kept > 0 && dropped > 0 && bads > 0 && dead_bad > 0);
    // the arithmetic by itself
    CHECK(filter_lookup(0xFFFFFFFFu, 1ull << 32) && !filter_lookup(0xFFFFFFFFu, 0xFFFFFFFFull) && !filter_lookup(5, 5) && filter_lookup(4, 5));
    CHECK(filter_pass(5, 5, 5, 0) && !filter_pass(4, 5, 5, 0) && !filter_pass(6, 5, 5, 0) && !filter_pass(5, 5, 5, 1) && filter_pass(6, 5, 5, 1));
    CHECK(!filter_pass(5, 6, 4, 0) && filter_pass(5, 6, 4, 1) && filter_pass(0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0) && !filter_pass(0, 0, 0xFFFFFFFFu, 1));
    CHECK(filter_prior_bit(1ull << 63, 63) && !filter_prior_bit(1ull << 63, 62) && filter_and(0xF0ull, 0x3Cull) == 0x30ull);
    printf("ok: %ld cases, %ld checks, %ld kept, %ld dropped, %ld with a bad id\n", cases, checks, kept, dropped, bads);
    return 0;
}
