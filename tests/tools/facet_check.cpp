// The facet step of ansx_topk_facets_batch_dev on the CPU (ans_large_alphabet_amd/csrc/ansx_query_tile.h: facet_tiles,
// facet_chunk, facet_lookup, facet_counted, facet_row, and the frame's qt_clamp, qt_tile_queries, qt_elem, isb_query_of --
// the arithmetic k_facet_count runs), over made-up candidates, bounds and columns.
//   1. Both forms of the kernel RUN the way ansx_facet.h runs them: "atomic", a tile per workgroup; "lds", `grid`
//      workgroups that each walk the contiguous chunk facet_chunk gives them over the tiles of the clamped total, keep
//      the counts of one query in nvalues bins, flush them when the query changes, at a tile that spans queries and at the
//      chunk's end, and send the candidates of a tile that spans queries through global adds.  Every read of a candidate
//      goes through an accessor that refuses h at or beyond the clamped total, the column is a function that refuses an
//      id of ndocs or more, the bins are a vector of exactly nvalues words, and a global add refuses a word outside the
//      Q rows.
//   2. The judge: a brute-force count, query by query, and the smallest query with an id of ndocs or more.
//   3. The chunks: back to back from 0 to the tiles, lengths at most one apart, for every grid.
//   4. The cost: the lds form issues at most grid x nvalues global adds plus those of the tiles that span queries.
// Cases: totals of 0, 1, 1023, 1024, 1025 and several tiles; grids of 1, 2, 3 and more workgroups than tiles; one query,
// thousands of queries of 0 to 7 results, a long query between short ones, empty queries at either end; nvalues of 1,
// 4095, 4096 and 4097 (above the cap: "atomic" only, as the host decides); column values at nvalues - 1, nvalues and
// 0xFFFFFFFF; ids at ndocs - 1 and ndocs, and ndocs = 2^32 with the id 0xFFFFFFFF; a device total above and below n.
// Built with -fsanitize=address,undefined and run by tests/test_facet_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_query_tile.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static const u32 NONE = 0xFFFFFFFFu;   // ANSX_TOPK_NONE
static const u32 LDS_VALUES = 4096u;   // ANSX_FACET_LDS_VALUES
static const u32 NT = ANSX_ISECT_NT, TILE = ANSX_ISECT_TILE;
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

struct Column {  // the value of every id below ndocs, as a function: ndocs may be 2^32
    u64 ndocs;
    u32 nvalues;
    bool constant;  // every document has the value nvalues - 1: the most contention
    u32 at(u32 id) const
    {
        CHECK((u64)id < ndocs);  // (the kernel compares before it reads)
        if (constant) return nvalues - 1;
        const u32 m = mix(id);
        switch (m & 7u) {
        case 0: return nvalues - 1;
        case 1: return nvalues;  // "no value"
        case 2: return 0xFFFFFFFFu;
        case 3: return 0;
        default: return (m >> 3) % nvalues;
        }
    }
};

struct Cands {  // the candidates of a group as the steps leave them
    std::vector<u32> ids, hseg;  // hseg: Q + 1 bounds
    u32 n;                       // the host's bound
    u64 total;                   // the device's count
    u32 Q() const { return (u32)hseg.size() - 1; }
};

struct Out {
    std::vector<u32> counts;
    u32 bad = NONE;
    u64 adds = 0;  // global adds issued
    bool operator==(const Out& o) const { return counts == o.counts && bad == o.bad; }
};

static void brute(const Cands& c, const Column& col, Out* o)
{
    const u64 tot = std::min<u64>(c.total, c.n);
    o->counts.assign((size_t)c.Q() * col.nvalues, 0);
    for (u32 j = 0; j < c.Q(); j++)
        for (u64 h = c.hseg[j]; h < c.hseg[j + 1] && h < tot; h++) {
            const u32 id = c.ids[(size_t)h];
            if ((u64)id >= col.ndocs) {
                o->bad = std::min(o->bad, j);
                continue;
            }
            const u32 v = col.at(id);
            if (v < col.nvalues) o->counts[(size_t)j * col.nvalues + v]++;
        }
}

struct Run {  // what both forms share: the checked accessors
    const Cands& c;
    const Column& col;
    Out* o;
    u64 tot;
    std::vector<u8> seen;
    Run(const Cands& c_, const Column& col_, Out* o_) : c(c_), col(col_), o(o_), tot(qt_clamp(c_.total, c_.n)), seen((size_t)c_.n, 0)
    {
        o->counts.assign((size_t)c.Q() * col.nvalues, 0);
    }
    u32 id(u64 h)
    {
        CHECK(h < tot && h < c.ids.size() && !seen[(size_t)h]);  // every candidate below the limit, once
        seen[(size_t)h] = 1;
        return c.ids[(size_t)h];
    }
    void add(u32 j, u32 v, u32 by)
    {
        CHECK(j < c.Q() && v < col.nvalues);
        const u64 w = facet_row(j, col.nvalues) + v;
        CHECK(w < o->counts.size());
        o->counts[(size_t)w] += by, o->adds++;
    }
    // one candidate of query j -> whether it is counted
    bool candidate(u32 id_, u32 j, u32* v)
    {
        if (!facet_lookup(id_, col.ndocs)) {
            o->bad = std::min(o->bad, j);
            return false;
        }
        *v = col.at(id_);
        return facet_counted(*v, col.nvalues);
    }
    void done()
    {
        for (u64 h = 0; h < tot; h++) CHECK(seen[(size_t)h]);
    }
};

static void run_atomic(const Cands& c, const Column& col, Out* o)
{
    Run R(c, col, o);
    const u32 grid = (u32)((c.n + TILE - 1) / TILE);  // the host's: the tiles of n
    for (u32 b = 0; b < grid; b++) {
        const u64 i0 = (u64)b * TILE;
        if (i0 >= R.tot) continue;
        u32 qb[2];
        qt_tile_queries(c.hseg.data(), c.Q(), i0, (u32)R.tot, qb);
        for (u32 tid = 0; tid < NT; tid++)
            for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
                const u64 h = qt_elem(i0, k, tid);
                if (h >= R.tot) continue;
                const u32 j = isb_query_of(c.hseg.data(), qb[0], qb[1], (u32)h);
                u32 v;
                if (R.candidate(R.id(h), j, &v)) R.add(j, v, 1);
            }
    }
    R.done();
}

static void run_lds(const Cands& c, const Column& col, u32 grid, Out* o)
{
    CHECK(col.nvalues <= LDS_VALUES && grid >= 1);
    Run R(c, col, o);
    const u64 ntiles = facet_tiles(R.tot);
    u64 next = 0, mixed = 0, longest = 0, shortest = ~0ull;
    for (u32 wg = 0; wg < grid; wg++) {
        u64 t[2];
        facet_chunk(ntiles, grid, wg, t);
        CHECK(t[0] == next && t[1] >= t[0] && t[1] <= ntiles);  // back to back
        next = t[1];
        longest = std::max(longest, t[1] - t[0]), shortest = std::min(shortest, t[1] - t[0]);
        if (t[0] >= t[1]) continue;
        std::vector<u32> bins(col.nvalues, 0);  // (exactly nvalues words: the sanitizer sees a step outside)
        u32 held = NONE;
        auto flush = [&]() {
            for (u32 i = 0; i < col.nvalues; i++)
                if (bins[i]) R.add(held, i, bins[i]), bins[i] = 0;
            held = NONE;
        };
        for (u64 tile = t[0]; tile < t[1]; tile++) {
            const u64 i0 = tile * TILE;
            CHECK(i0 < R.tot);  // (what qt_tile_queries asks)
            u32 qb[2];
            qt_tile_queries(c.hseg.data(), c.Q(), i0, (u32)R.tot, qb);
            const bool one = qb[0] == qb[1];
            if (held != NONE && (!one || held != qb[0])) flush();
            if (one) held = qb[0];
            else mixed += std::min<u64>(TILE, R.tot - i0);
            for (u32 tid = 0; tid < NT; tid++)
                for (u32 k = 0; k < ANSX_ISECT_CPT; k++) {
                    const u64 h = qt_elem(i0, k, tid);
                    if (h >= R.tot) continue;
                    u32 v;
                    if (one) {
                        if (R.candidate(R.id(h), qb[0], &v)) bins[v]++;
                    } else {
                        const u32 j = isb_query_of(c.hseg.data(), qb[0], qb[1], (u32)h);
                        if (R.candidate(R.id(h), j, &v)) R.add(j, v, 1);
                    }
                }
        }
        if (held != NONE) flush();
        for (u32 i = 0; i < col.nvalues; i++) CHECK(bins[i] == 0);
    }
    CHECK(next == ntiles && longest - shortest <= 1);
    R.done();
    // a flush per change of query inside a chunk and one at its end: with Q queries at most (grid + Q) x nvalues adds
    CHECK(o->adds <= ((u64)grid + c.Q()) * col.nvalues + mixed);
    if (c.Q() == 1) CHECK(o->adds <= (u64)grid * col.nvalues);  // one long query: grid x nvalues, not one per candidate
}

// candidates of the given sizes per query: distinct ids that ascend inside a query, below `top`
static Cands make(const std::vector<u32>& sizes, u64 top, std::mt19937_64& rng)
{
    Cands c;
    c.hseg.push_back(0);
    for (const u32 s : sizes) {
        CHECK((u64)s <= top);
        // s distinct ids: a random start and random gaps that fit below top
        const u64 room = top - s;
        std::vector<u64> cut(s);
        for (u64& x : cut) x = rng() % (room + 1);
        std::sort(cut.begin(), cut.end());
        for (u32 i = 0; i < s; i++) c.ids.push_back((u32)(cut[i] + i));
        c.hseg.push_back((u32)c.ids.size());
    }
    c.n = (u32)c.ids.size(), c.total = c.n;
    return c;
}

static void check_all(const Cands& c, const Column& col)
{
    Out want, got;
    brute(c, col, &want);
    run_atomic(c, col, &got);
    CHECK(got == want);
    if (col.nvalues > LDS_VALUES) return;  // (the host: "atomic" is the only form)
    const u32 ntiles = (u32)facet_tiles(std::min<u64>(c.total, c.n));
    for (const u32 grid : { 1u, 2u, 3u, ntiles + 1u, ntiles + 5u, 7u }) {
        Out o;
        run_lds(c, col, grid, &o);
        CHECK(o == want);
    }
}

int main()
{
    std::mt19937_64 rng(20241);
    const u32 nvals[] = { 1u, 2u, 16u, LDS_VALUES - 1, LDS_VALUES, LDS_VALUES + 1 };
    // ---- one query of every total around the tile; a device total of 0, below n and above n
    what = "totals";
    for (const u32 nv : nvals)
        for (const u32 n : { 1u, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 77 })
            for (const bool constant : { false, true }) {
                const Column col = { 1u << 20, nv, constant };
                Cands c = make({ n }, col.ndocs, rng);
                check_all(c, col);
                c.total = (u64)n + 12345, check_all(c, col);        // the clamp
                c.total = ~0ull, check_all(c, col);
                c.total = 0, check_all(c, col);                      // everything was filtered away
                c.total = n / 2, check_all(c, col);                  // (never with the real steps; still inside the buffers)
            }
    // ---- query shapes
    what = "query shapes";
    for (const u32 nv : nvals) {
        const Column col = { 1u << 22, nv, false };
        std::vector<u32> tiny(3000), mixed, ends;
        for (u32& s : tiny) s = (u32)(rng() % 8);           // thousands of queries of 0 to 7 results
        for (u32 i = 0; i < 40; i++) mixed.push_back((u32)(rng() % 8));
        mixed.push_back(3 * TILE + 5);                       // a long query between short ones
        for (u32 i = 0; i < 40; i++) mixed.push_back((u32)(rng() % 8));
        mixed.push_back(TILE), mixed.push_back(1), mixed.push_back(2 * TILE), mixed.push_back(TILE - 1);
        ends = { 0, 0, 0, 5, TILE, 0, 0, 2 * TILE + 3, 1, 0, 0 };  // empty queries at either end and in the middle
        for (const std::vector<u32>& sizes : { tiny, mixed, ends, std::vector<u32>{ 0, 0, 7 }, std::vector<u32>{ 7, 0, 0 },
                 std::vector<u32>{ 1, 1023, 1024, 1025, 2049 } }) {
            Cands c = make(sizes, col.ndocs, rng);
            check_all(c, col);
            c.total += 9, check_all(c, col);
        }
        const Column same = { 1u << 22, nv, true };
        check_all(make(mixed, same.ndocs, rng), same);
    }
    // ---- ids at ndocs - 1 and ndocs: the smallest query with a bad id, and nothing read at it
    what = "the bad id";
    for (const u32 nv : { 1u, 16u, LDS_VALUES, LDS_VALUES + 1 })
        for (u32 where = 0; where < 8; where++) {
            const Column col = { 5000, nv, false };
            Cands c = make({ 3, 2 * TILE + 9, 0, 40, 700, TILE }, col.ndocs, rng);
            // (the last id of a query: the ids still ascend)
            c.ids[c.hseg[2] - 1] = 4999;  // ndocs - 1: fine
            if (where & 1u) c.ids[c.hseg[2] - 1] = 5000;
            if (where & 2u) c.ids[c.hseg[4] - 1] = 5000;
            if (where & 4u) c.ids[c.hseg[6] - 1] = 0xFFFFFFFFu;
            Out want;
            brute(c, col, &want);
            CHECK(want.bad == ((where & 1u) ? 1u : (where & 2u) ? 3u : (where & 4u) ? 5u : NONE));
            check_all(c, col);
        }
    // ---- ndocs = 2^32 admits 0xFFFFFFFF
    what = "ndocs = 2^32";
    {
        const Column col = { (u64)1 << 32, 16, false };
        Cands c = make({ 5, TILE + 3, 2 }, col.ndocs, rng);
        c.ids[c.hseg[2] - 1] = 0xFFFFFFFFu, c.ids[c.hseg[3] - 1] = 0xFFFFFFFEu;
        Out want;
        brute(c, col, &want);
        CHECK(want.bad == NONE);
        check_all(c, col);
        CHECK(facet_lookup(0xFFFFFFFFu, (u64)1 << 32) && !facet_lookup(0xFFFFFFFFu, 0xFFFFFFFFull) && facet_lookup(0, 1) && !facet_lookup(1, 1));
        CHECK(facet_counted(15, 16) && !facet_counted(16, 16) && !facet_counted(0xFFFFFFFFu, 1u << 24));
        CHECK(facet_row(0xFFFFFFFEu, 1u << 24) == 0xFFFFFFFEull << 24);  // (64 bits)
    }
    // ---- the chunks alone, for tile counts and grids the runs above do not reach
    what = "chunks";
    for (const u64 ntiles : { 0ull, 1ull, 2ull, 63ull, 64ull, 65ull, 2047ull, 2048ull, 2049ull, 65536ull, 1ull << 22 })
        for (const u32 grid : { 1u, 2u, 3u, 255u, 256u, 2048u, 4096u, 0xFFFFFFFFu }) {
            u64 next = 0;
            const u32 step = grid > 5000 ? grid / 4099 : 1;  // (a sample of the workgroups of a huge grid, and its ends)
            for (u64 wg = 0; wg < grid; wg += step) {
                u64 t[2], p[2];
                facet_chunk(ntiles, grid, (u32)wg, t);
                if (wg) {
                    facet_chunk(ntiles, grid, (u32)wg - 1, p);
                    CHECK(p[1] == t[0]);
                } else {
                    CHECK(t[0] == 0);
                }
                CHECK(t[0] <= t[1] && t[1] - t[0] <= ntiles / grid + 1 && t[1] - t[0] >= ntiles / grid);
                next = t[1];
            }
            u64 t[2];
            facet_chunk(ntiles, grid, grid - 1, t);
            CHECK(t[1] == ntiles && next <= ntiles);
        }
    CHECK(facet_tiles(0) == 0 && facet_tiles(1) == 1 && facet_tiles(TILE) == 1 && facet_tiles(TILE + 1) == 2 && facet_tiles((u64)1 << 32) == 1u << 22);
    printf("ok: %ld checks\n", checks);
    return 0;
}
