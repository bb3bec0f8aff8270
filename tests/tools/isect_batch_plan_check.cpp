// The host's plan of ansx_intersect_batch_dev (ans_large_alphabet_amd/csrc/ansx_plan.h, isb_plan) on the CPU, over
// synthetic headers: lists of given lengths whose ids are made up here.  The plan's own statements are checked -- every
// query in exactly one group, in order; the budget; drivers and round order, ties and repeats included; tables that
// name only what the group decodes; candidate totals below 2^32 -- and then each group is RUN the way the kernels run it
// (the buffer of its lists back to back, the gather, a lower bound per candidate and round, the compaction with its
// segment bounds) and every query's survivors are compared with the intersection computed directly.
// Built with -fsanitize=address,undefined and run by tests/test_intersect_batch_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

using namespace ansx_plan;

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

// what a query costs alone: its distinct lists once, its driver twice more
static u64 query_ints(const std::vector<u64>& n, const u32* t, size_t m)
{
    std::set<u32> seen(t, t + m);
    u64 a = 0, nd = ~0ull;
    for (const u32 r : seen) a += n[r];
    for (size_t j = 0; j < m; j++) nd = std::min(nd, n[t[j]]);
    return a + 2 * nd;
}

// The statements of the plan; -> the number of groups.  ids: every list's ids (null: the lengths only, nothing is run).
static size_t check_plan(const char* what, const std::vector<u64>& n, const Queries& Q, u64 budget,
    const std::vector<std::vector<u32>>* ids)
{
    std::vector<IsbGroup> G;
    size_t bad = ~(size_t)0;
    CHECK(isb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, &G, &bad) == ANSX_OK);
    CHECK(bad == ~(size_t)0);
    size_t next = 0;
    for (size_t gi = 0; gi < G.size(); gi++) {
        const IsbGroup& g = G[gi];
        CHECK(g.q0 == next && g.q1 > g.q0 && g.q1 <= Q.size());  // every query once, in order
        next = g.q1;
        const size_t nq = g.q1 - g.q0;
        CHECK(g.G.size() == nq + 1 && g.rt_off.size() == nq + 1 && g.drv.size() == nq && g.rt.size() == g.rt_list.size());
        // its lists: the non-empty ones its queries name, ascending, back to back
        std::set<u32> named;
        for (u64 j = Q.qoff[g.q0]; j < Q.qoff[g.q1]; j++) named.insert(Q.rid[j]);
        u64 buf = 0, cand = 0;
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
        u32 rounds = 0;
        for (size_t j = 0; j < nq; j++) {
            const u32* t = Q.rid.data() + Q.qoff[g.q0 + j];
            const size_t m = (size_t)(Q.qoff[g.q0 + j + 1] - Q.qoff[g.q0 + j]);
            // the driver: fewest ints, the earliest position; the others by (n, position)
            size_t d = 0;
            for (size_t k = 1; k < m; k++)
                if (n[t[k]] < n[t[d]]) d = k;
            std::vector<std::pair<u64, size_t>> rest;
            for (size_t k = 0; k < m; k++)
                if (k != d) rest.push_back({ n[t[k]], k });
            std::sort(rest.begin(), rest.end());
            CHECK(g.drv[j] == t[d] && g.G[j].dst == cand);
            CHECK(n[t[d]] == 0 || g.G[j].src == place(t[d]));
            CHECK(g.G[j].src + n[t[d]] <= buf);  // the gather stays inside the buffer
            cand += n[t[d]];
            CHECK(g.rt_off[j + 1] - g.rt_off[j] == m - 1 && g.rt_off[j + 1] <= g.rt.size());
            for (size_t k = 0; k + 1 < m; k++) {
                const u32 r = t[rest[k].second], e = g.rt_off[j] + (u32)k;
                CHECK(g.rt_list[e] == r && g.rt[e].n == n[r]);
                CHECK(n[r] == 0 || (g.rt[e].at == place(r) && std::binary_search(want.begin(), want.end(), r)));
                CHECK(g.rt[e].at + g.rt[e].n <= buf);  // the match stays inside the buffer
            }
            rounds = std::max(rounds, (u32)(m - 1));
        }
        CHECK(g.rt_off[0] == 0 && g.rt_off[nq] == g.rt.size() && g.rounds == rounds);
        CHECK(g.G[nq].dst == cand && cand <= 0xFFFFFFFFull);
        CHECK(g.ints == buf + 2 * cand);
        CHECK(nq == 1 || g.ints <= budget);
        if (gi + 1 < G.size()) {  // it ended because the next query did not fit
            const u32* t = Q.rid.data() + Q.qoff[g.q1];
            const size_t m = (size_t)(Q.qoff[g.q1 + 1] - Q.qoff[g.q1]);
            u64 add = 0, nd = ~0ull;
            std::set<u32> seen;
            for (size_t k = 0; k < m; k++) {
                if (!named.count(t[k]) && seen.insert(t[k]).second) add += n[t[k]];
                nd = std::min(nd, n[t[k]]);
            }
            CHECK(g.ints + add + 2 * nd > budget || cand + nd > 0xFFFFFFFFull);
        }
        if (!ids) continue;

        // run it
        std::vector<u32> ws;
        for (const u32 r : want) ws.insert(ws.end(), (*ids)[r].begin(), (*ids)[r].end());
        CHECK(ws.size() == buf);
        std::vector<u32> cur(cand), seg(nq + 1);
        for (u64 i = 0; i < cand; i++) {  // k_isectb_gather
            size_t q = 0;
            for (size_t j = 0; j < nq; j++)
                if (g.G[j].dst <= i) q = j;  // the LAST one: empty segments are passed over
            cur[i] = ws[g.G[q].src + (i - g.G[q].dst)];
        }
        for (size_t j = 0; j <= nq; j++) seg[j] = (u32)g.G[j].dst;
        for (u32 r = 0; r < g.rounds; r++) {
            std::vector<u32> nxt, nseg(nq + 1);
            std::vector<char> member(cur.size());
            for (size_t i = 0; i < cur.size(); i++) {  // k_isectb_match
                size_t q = 0;
                for (size_t j = 0; j < nq; j++)
                    if (seg[j] <= i) q = j;
                CHECK(seg[q] <= i && i < seg[q + 1]);
                const u32 e = g.rt_off[q] + r;
                if (e >= g.rt_off[q + 1]) {
                    member[i] = 1;
                    continue;
                }
                const u32* list = ws.data() + g.rt[e].at;
                const u32* lb = std::lower_bound(list, list + g.rt[e].n, cur[i]);
                member[i] = lb != list + g.rt[e].n && *lb == cur[i];
            }
            for (size_t j = 0; j <= nq; j++) {  // k_isectb_bounds
                u32 a = 0;
                for (size_t i = 0; i < seg[j]; i++) a += member[i];
                nseg[j] = a;
            }
            for (size_t i = 0; i < cur.size(); i++)
                if (member[i]) nxt.push_back(cur[i]);
            CHECK(nseg[nq] == nxt.size());
            cur.swap(nxt), seg.swap(nseg);
        }
        for (size_t j = 0; j < nq; j++) {  // against the intersection, computed directly
            const u32* t = Q.rid.data() + Q.qoff[g.q0 + j];
            const size_t m = (size_t)(Q.qoff[g.q0 + j + 1] - Q.qoff[g.q0 + j]);
            std::vector<u32> exp;
            for (const u32 v : (*ids)[g.drv[j]]) {
                size_t in = 0;  // (the driver's own place counts: v is one of its ids)
                for (size_t k = 0; k < m; k++) in += std::binary_search((*ids)[t[k]].begin(), (*ids)[t[k]].end(), v);
                if (in == m) exp.push_back(v);
            }
            CHECK(std::vector<u32>(cur.begin() + seg[j], cur.begin() + seg[j + 1]) == exp);
        }
    }
    CHECK(next == Q.size());
    return G.size();
}

int main()
{
    const char* what = "lists";
    std::mt19937_64 rng(12345);
    // 24 lists over a small universe, a planted core in all the non-empty ones; two pairs of equal length, one empty list
    const u32 sizes[24] = { 1, 2, 63, 64, 65, 100, 100, 333, 500, 500, 777, 1000, 1023, 1024, 1025, 1500, 2000, 2049, 2500, 3000,
        3500, 4000, 5000, 0 };
    std::vector<std::vector<u32>> ids(24);
    std::vector<u64> n(24);
    for (u32 r = 0; r < 24; r++) {
        std::set<u32> s;
        if (sizes[r] >= 63)
            for (u32 c = 0; c < 40; c++) s.insert(c * 401 + 7);
        while (s.size() < sizes[r]) s.insert((u32)(rng() % 20000));
        ids[r].assign(s.begin(), s.end());
        if (r == 8) ids[r][10] = ids[r][9];  // (a repeated id: the driver's multiplicities)
        n[r] = ids[r].size();
        CHECK(n[r] == sizes[r]);
    }

    what = "shapes";
    Queries S;
    S.add({ 5, 6 });        // a tie: the earlier position drives
    S.add({ 6, 5 });
    S.add({ 9, 8, 22 });    // a tie between the two short ones, the long one last
    S.add({ 22, 9, 8 });
    S.add({ 4, 4 });        // a list twice
    S.add({ 12, 3, 12 });   // ... around its driver
    S.add({ 7 });           // one term: no round
    S.add({ 0, 21 });       // a driver of one id
    S.add({ 23, 11 });      // an empty driver
    S.add({ 11, 23, 10 });  // an empty list behind the driver's place: it drives
    S.add({ 20, 19, 18, 17, 16 });
    S.add({ 1, 2 });
    CHECK(check_plan(what, n, S, ANSX_ISECT_BATCH_INTS_DEFAULT, &ids) == 1);

    what = "random";
    Queries R;
    for (u32 q = 0; q < 60; q++) {
        std::vector<u32> t(1 + rng() % 5);
        for (u32& r : t) r = (u32)(rng() % 24);
        R.add(t);
    }
    u64 all = 0, most = 0, least = ~0ull;
    {
        std::set<u32> seen(R.rid.begin(), R.rid.end());
        for (const u32 r : seen) all += n[r];
        for (size_t q = 0; q < R.size(); q++) {
            const u32* t = R.rid.data() + R.qoff[q];
            const size_t m = (size_t)(R.qoff[q + 1] - R.qoff[q]);
            const u64 own = query_ints(n, t, m);
            most = std::max(most, own), least = std::min(least, own);
            u64 nd = ~0ull;
            for (size_t k = 0; k < m; k++) nd = std::min(nd, n[t[k]]);
            all += 2 * nd;
        }
    }
    CHECK(check_plan(what, n, R, all, &ids) == 1);        // the budget just holds everything
    CHECK(check_plan(what, n, R, all - 1, &ids) == 2);    // ... and just does not
    const size_t some = check_plan(what, n, R, all / 2, &ids);  // (a list several groups name counts in each)
    CHECK(some > 2 && some < R.size() / 2);
    CHECK(check_plan(what, n, R, most, &ids) > 2);        // every query fits alone
    CHECK(check_plan(what, n, R, 1, &ids) == R.size());   // every query over the budget alone: a group each
    CHECK(check_plan(what, n, R, 0, &ids) == R.size());
    (void)least;

    what = "one over the budget";
    Queries O;
    O.add({ 1, 2 });
    O.add({ 0, 1 });
    O.add({ 22, 21, 20 });  // 3500 + 4000 + 5000 + 2 * 3500: alone above 10000
    O.add({ 2, 1 });
    O.add({ 0, 2 });
    CHECK(query_ints(n, O.rid.data() + O.qoff[2], 3) > 10000);
    CHECK(check_plan(what, n, O, 10000, &ids) == 3);

    what = "2^32 candidates";
    const std::vector<u64> big = { 1ull << 31, (1ull << 31) - 1, 0xFFFFFFFFull, 1ull << 32, 5 };
    Queries B;
    B.add({ 0 });
    B.add({ 1 });  // 2^32 - 1 with the first: still one group
    B.add({ 4 });  // ... and 5 more are too many
    B.add({ 2 });  // alone at the limit
    B.add({ 2, 3 });
    B.add({ 4, 3 });  // every one of these closes the group in front of it
    CHECK(check_plan(what, big, B, ~0ull, nullptr) == 5);
    B.add({ 3 });  // a driver of 2^32 ints
    std::vector<IsbGroup> G;
    size_t bad = 99;
    CHECK(isb_plan(big.data(), big.size(), B.rid.data(), B.qoff.data(), B.size(), ~0ull, &G, &bad) == ANSX_ERR_ARG);
    CHECK(bad == 6);

    printf("ok: %ld checks\n", checks);
    return 0;
}
