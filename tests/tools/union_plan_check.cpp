// The host's plan of ansx_union_batch_dev (ans_large_alphabet_amd/csrc/ansx_plan.h, unb_plan) on the CPU, over synthetic
// headers: lists of given lengths whose ids are made up here.  The plan's own statements are checked -- every query in
// exactly one group, in order; the budget and the 2^32 limits; the rounds; that every round's pairs tile the span of
// every query that has that round exactly once and touch no other; sources inside the buffer they are read from; the
// first-tile column as the prefix sum it is, and the workgroup -> pair mapping the kernel derives from it; fewer than
// two pairs per term -- and then each group is RUN the way the kernels run it (the buffer of its lists back to back,
// std::merge per pair and round between two merge buffers, the heads of equal runs inside a query) and every query's
// ids and counts are compared with the std::set / std::multiset union computed directly.
// Built with -fsanitize=address,undefined and run by tests/test_union_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

using namespace ansx_plan;

static const u32 TILE = 1024;
static long checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        checks++;                                                                    \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: %s -- %s\n", __FILE__, __LINE__, #cond, what);   \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

struct Queries {
    std::vector<u32> rid;
    std::vector<u64> qoff{ 0 };
    void add(std::initializer_list<u32> t) { add(std::vector<u32>(t)); }
    void add(const std::vector<u32>& t)
    {
        rid.insert(rid.end(), t.begin(), t.end());
        qoff.push_back(rid.size());
    }
    size_t size() const { return qoff.size() - 1; }
};

static u32 rounds_of(size_t m)
{
    u32 r = 0;
    while (((size_t)1 << r) < m) r++;
    return r ? r : 1;
}

// what a query costs alone: its distinct lists once, its lists as named twice more
static u64 query_ints(const std::vector<u64>& n, const u32* t, size_t m)
{
    std::set<u32> seen(t, t + m);
    u64 a = 0;
    for (const u32 r : seen) a += n[r];
    for (size_t j = 0; j < m; j++) a += 2 * n[t[j]];
    return a;
}

// The statements of the plan; -> the number of groups.  ids: every list's ids (null: the lengths only, nothing is run).
static size_t check_plan(const char* what, const std::vector<u64>& n, const Queries& Q, u64 budget,
    const std::vector<std::vector<u32>>* ids)
{
    std::vector<UnbGroup> G;
    size_t bad = ~(size_t)0;
    CHECK(unb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, TILE, &G, &bad) == ANSX_OK);
    CHECK(bad == ~(size_t)0);
    size_t next = 0;
    for (size_t gi = 0; gi < G.size(); gi++) {
        const UnbGroup& g = G[gi];
        CHECK(g.q0 == next && g.q1 > g.q0 && g.q1 <= Q.size());  // every query once, in order
        next = g.q1;
        const size_t nq = g.q1 - g.q0;
        // its lists: the non-empty ones its queries name, ascending, back to back
        std::set<u32> named;
        for (u64 j = Q.qoff[g.q0]; j < Q.qoff[g.q1]; j++) named.insert(Q.rid[j]);
        u64 buf = 0;
        std::vector<u32> want;
        for (const u32 r : named) {
            buf += n[r];
            if (n[r]) want.push_back(r);
        }
        CHECK(g.lists == want && g.at.size() == want.size() + 1);
        u64 at = 0;
        for (size_t k = 0; k < want.size(); k++) {
            CHECK(g.at[k] == at);
            at += n[want[k]];
        }
        CHECK(g.at.back() == at && at == buf);
        auto place = [&](u32 r) { return g.at[(size_t)(std::lower_bound(want.begin(), want.end(), r) - want.begin())]; };
        // the queries' spans of the merge buffers and the rounds
        CHECK(g.seg.size() == nq + 1);
        u64 merge = 0, terms = 0;
        u32 R = 1;
        std::vector<u32> rq(nq);
        for (size_t j = 0; j < nq; j++) {
            const u32* t = Q.rid.data() + Q.qoff[g.q0 + j];
            const size_t m = (size_t)(Q.qoff[g.q0 + j + 1] - Q.qoff[g.q0 + j]);
            CHECK(g.seg[j] == merge);
            for (size_t k = 0; k < m; k++) merge += n[t[k]];
            rq[j] = rounds_of(m), R = std::max(R, rq[j]), terms += m;
        }
        CHECK(g.seg[nq] == merge && merge <= 0xFFFFFFFFull);
        CHECK(g.rounds == R && g.roff.size() == (size_t)R + 1 && g.tiles.size() == R && g.roff[0] == 0 && g.roff[R] == g.pairs.size());
        CHECK(g.ints == buf + 2 * merge);
        CHECK(nq == 1 || g.ints <= budget);
        CHECK(g.pairs.size() < 2 * terms);
        if (gi + 1 < G.size()) {  // it ended because the next query did not fit
            const u32* t = Q.rid.data() + Q.qoff[g.q1];
            const size_t m = (size_t)(Q.qoff[g.q1 + 1] - Q.qoff[g.q1]);
            u64 add = 0, tot = 0;
            std::set<u32> seen;
            for (size_t k = 0; k < m; k++) {
                if (!named.count(t[k]) && seen.insert(t[k]).second) add += n[t[k]];
                tot += n[t[k]];
            }
            CHECK(g.ints + add + 2 * tot > budget || merge + tot > 0xFFFFFFFFull);
        }
        // every round: the pairs of the queries that have it tile their spans once, in order; the first-tile column
        for (u32 r = 0; r < R; r++) {
            CHECK(g.roff[r] <= g.roff[r + 1]);
            struct Span {
                size_t j;
                u64 start, end;
            };
            std::vector<Span> spans;  // of the queries that have this round and ints
            for (size_t j = 0; j < nq; j++)
                if (r >= R - rq[j] && g.seg[j] < g.seg[j + 1]) spans.push_back({ j, g.seg[j], g.seg[j + 1] });
            CHECK(spans.empty() == (g.roff[r] == g.roff[r + 1]));
            size_t k = 0;
            u64 cursor = spans.empty() ? 0 : spans[0].start, tile = 0;
            for (u32 e = g.roff[r]; e < g.roff[r + 1]; e++) {
                const ansx_unb_pair& p = g.pairs[e];
                const u64 len = (u64)p.na + p.nb;
                CHECK(len > 0);  // (an empty pair is left out)
                if (cursor == spans[k].end) {
                    CHECK(++k < spans.size());
                    cursor = spans[k].start;
                }
                CHECK(p.dst == cursor && cursor + len <= spans[k].end);
                cursor += len;
                CHECK(p.from_lists == (r == R - rq[spans[k].j] ? 1u : 0u));
                if (p.from_lists) {
                    CHECK(p.a + p.na <= buf && p.b + p.nb <= buf);
                } else {
                    CHECK(p.a == p.dst && (p.nb == 0 || p.b == p.a + p.na) && p.a + len <= merge);
                }
                CHECK(p.tile == tile);
                tile += (len + TILE - 1) / TILE;
            }
            CHECK(spans.empty() || (k + 1 == spans.size() && cursor == spans[k].end));
            CHECK(g.tiles[r] == tile);
            // the kernel's mapping: workgroup t belongs to the last pair with tile <= t, and lies inside it
            const u32 np = g.roff[r + 1] - g.roff[r];
            const ansx_unb_pair* P = g.pairs.data() + g.roff[r];
            for (u64 t = 0; t < tile && tile < 100000; t++) {
                u32 lo = 0, hi = np - 1;
                while (lo < hi) {
                    const u32 mid = lo + (hi - lo + 1) / 2;
                    if (P[mid].tile <= t) lo = mid;
                    else hi = mid - 1;
                }
                CHECK(P[lo].tile <= t && (t - P[lo].tile) * TILE < (u64)P[lo].na + P[lo].nb);
            }
        }
        if (!ids) continue;

        // run it
        std::vector<u32> ws;
        for (const u32 r : want) ws.insert(ws.end(), (*ids)[r].begin(), (*ids)[r].end());
        CHECK(ws.size() == buf);
        std::vector<u32> mb[2] = { std::vector<u32>(merge, 0xDEADBEEFu), std::vector<u32>(merge, 0xDEADBEEFu) };
        for (u32 r = 0; r < R; r++)
            for (u32 e = g.roff[r]; e < g.roff[r + 1]; e++) {
                const ansx_unb_pair& p = g.pairs[e];
                const u32* src = p.from_lists ? ws.data() : mb[1 - (r & 1)].data();
                std::merge(src + p.a, src + p.a + p.na, src + p.b, src + p.b + p.nb, mb[r & 1].begin() + p.dst);
            }
        const std::vector<u32>& x = mb[(R - 1) & 1];
        for (size_t j = 0; j < nq; j++) {
            const u32* t = Q.rid.data() + Q.qoff[g.q0 + j];
            const size_t m = (size_t)(Q.qoff[g.q0 + j + 1] - Q.qoff[g.q0 + j]);
            std::multiset<u32> all;
            for (size_t k = 0; k < m; k++) {
                all.insert((*ids)[t[k]].begin(), (*ids)[t[k]].end());
                CHECK(n[t[k]] == 0 || place(t[k]) + n[t[k]] <= buf);
            }
            CHECK(std::vector<u32>(x.begin() + g.seg[j], x.begin() + g.seg[j + 1]) == std::vector<u32>(all.begin(), all.end()));
            // k_union_heads / k_union_counts
            std::vector<u32> head, cnt;
            for (u32 p = g.seg[j]; p < g.seg[j + 1]; p++)
                if (p == g.seg[j] || x[p] != x[p - 1]) head.push_back(p);
            std::set<u32> uni(all.begin(), all.end());
            CHECK(head.size() == uni.size());
            size_t k = 0;
            for (const u32 v : uni) {
                CHECK(x[head[k]] == v);
                CHECK((k + 1 < head.size() ? head[k + 1] : g.seg[j + 1]) - head[k] == all.count(v));
                k++;
            }
        }
    }
    CHECK(next == Q.size());
    return G.size();
}

int main()
{
    const char* what = "lists";
    std::mt19937_64 rng(4321);
    // 40 lists over a small universe: short ones, lengths around the tile, two of equal length, one empty, one with a
    // repeated id; 24..39 of a few ids each for the long queries
    const u32 sizes[24] = { 1, 2, 63, 64, 65, 100, 100, 333, 500, 500, 777, 1000, 1023, 1024, 1025, 1500, 2000, 2049, 2500, 3000,
        3500, 4000, 5000, 0 };
    std::vector<std::vector<u32>> ids(40);
    std::vector<u64> n(40);
    for (u32 r = 0; r < 40; r++) {
        const u32 size = r < 24 ? sizes[r] : 3 + r % 7;
        std::set<u32> s;
        while (s.size() < size) s.insert((u32)(rng() % 20000));
        ids[r].assign(s.begin(), s.end());
        if (r == 8) ids[r][10] = ids[r][9];  // (a repeated id: it counts twice)
        n[r] = ids[r].size();
        CHECK(n[r] == size);
    }

    what = "shapes";
    Queries S;
    S.add({ 7 });                          // one term: a copy
    S.add({ 5, 6 });
    S.add({ 9, 8, 22 });                   // three: a run without a partner
    S.add({ 4, 4 });                       // a list twice
    S.add({ 12, 3, 12, 0, 1 });            // five, a list twice around others
    S.add({ 20, 19, 18, 17, 16, 15, 14, 13 });
    S.add({ 20, 19, 18, 17, 16, 15, 14, 13, 2 });  // nine: the ninth passes through three rounds
    S.add({ 23 });                         // an empty list alone
    S.add({ 23, 11 });                     // ... as A, as B, in the middle
    S.add({ 11, 23 });
    S.add({ 10, 23, 11 });
    S.add({ 23, 23, 23 });
    std::vector<u32> long33;
    for (u32 r = 7; r < 40; r++) long33.push_back(r);
    S.add(long33);                         // 33 terms: six rounds
    S.add({ 0, 1 });
    CHECK(check_plan(what, n, S, ANSX_ISECT_BATCH_INTS_DEFAULT, &ids) == 1);
    CHECK(check_plan(what, n, S, 0, &ids) == S.size());  // a group per query: every query's rounds start at 0

    what = "random";
    Queries R;
    for (u32 q = 0; q < 60; q++) {
        std::vector<u32> t(1 + rng() % 6);
        for (u32& r : t) r = (u32)(rng() % 40);
        R.add(t);
    }
    u64 all = 0, most = 0;
    {
        std::set<u32> seen(R.rid.begin(), R.rid.end());
        for (const u32 r : seen) all += n[r];
        for (const u32 r : R.rid) all += 2 * n[r];
        for (size_t q = 0; q < R.size(); q++)
            most = std::max(most, query_ints(n, R.rid.data() + R.qoff[q], (size_t)(R.qoff[q + 1] - R.qoff[q])));
    }
    CHECK(check_plan(what, n, R, all, &ids) == 1);        // the budget just holds everything
    CHECK(check_plan(what, n, R, all - 1, &ids) == 2);    // ... and just does not
    const size_t some = check_plan(what, n, R, all / 3, &ids);  // (a list several groups name counts in each)
    CHECK(some > 2 && some < R.size() / 2);
    CHECK(check_plan(what, n, R, most, &ids) > 2);        // every query fits alone
    CHECK(check_plan(what, n, R, 1, &ids) == R.size());   // every query over the budget alone: a group each
    CHECK(check_plan(what, n, R, 0, &ids) == R.size());

    what = "one over the budget";
    Queries O;
    O.add({ 1, 2 });
    O.add({ 0, 1 });
    O.add({ 22, 21, 20 });  // 3 * (3500 + 4000 + 5000): alone above 30000
    O.add({ 2, 1 });
    O.add({ 0, 2 });
    CHECK(query_ints(n, O.rid.data() + O.qoff[2], 3) > 30000);
    CHECK(check_plan(what, n, O, 30000, &ids) == 3);

    what = "2^32 ints";
    const std::vector<u64> big = { 1ull << 31, (1ull << 31) - 1, 0xFFFFFFFFull, 1ull << 32, 5 };
    Queries B;
    B.add({ 0 });
    B.add({ 1 });     // 2^32 - 1 with the first: still one merge buffer
    B.add({ 4 });     // ... and 5 more are too many
    B.add({ 2 });     // alone at the limit
    B.add({ 0, 1 });  // a query of 2^32 - 1 ints
    B.add({ 4, 4 });  // every one of these closes the group in front of it
    CHECK(check_plan(what, big, B, ~0ull, nullptr) == 5);
    std::vector<UnbGroup> G;
    size_t bad = 99;
    B.add({ 0, 1, 4 });  // together 2^32 + 4
    B.add({ 3 });
    CHECK(unb_plan(big.data(), big.size(), B.rid.data(), B.qoff.data(), B.size(), ~0ull, TILE, &G, &bad) == ANSX_ERR_ARG);
    CHECK(bad == 6);
    Queries B2;
    B2.add({ 4 });
    B2.add({ 3 });  // a list of 2^32 ints
    bad = 99;
    CHECK(unb_plan(big.data(), big.size(), B2.rid.data(), B2.qoff.data(), B2.size(), ~0ull, TILE, &G, &bad) == ANSX_ERR_ARG);
    CHECK(bad == 1);

    printf("ok: %ld checks\n", checks);
    return 0;
}
