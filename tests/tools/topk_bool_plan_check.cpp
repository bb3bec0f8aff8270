// The host side of ansx_topk_bool_batch_dev under ANSX_BOOL_ALL on the CPU (ans_large_alphabet_amd/csrc/ansx_plan.h,
// isb_plan with want_terms; ansx_plan_types.h, topk_sat32 and topk_sat_add), over synthetic headers: lists of given
// lengths -- empty ones among them, which no container can hold -- whose ids and payloads are made up here.
//   1. The terms behind drivers and rounds.  With want_terms the plan is the plan without -- groups, lists, tables,
//      rounds, ints bit for bit -- plus dterm and rterm: one entry per query and one per entry of rt, each a term of ITS
//      query whose list is the one the table names (drv / rt_list); a query's driver and rounds together name each of
//      its terms exactly once, ties and a list named twice included.
//   2. Every group RUN the way the kernels run it (ansx_topk_bool.h): the drivers gathered into candidates; round 0
//      seeds -- the first of a run of equal ids inside its segment stays, with the saturating sum of sat32(weight *
//      payload) over the run; every round with a list takes the lower bound, whole-list and bounded to the part of the
//      list a tile of 1024 candidates inside one query can meet, member = found and equal, and adds the list's postings
//      of the id with topk_sat_add; the members are compacted, ids and scores alike; at least one round runs; then the
//      exclusion step drops what an excluded list holds; then the overflow rule: a SURVIVOR with score 0xFFFFFFFF names
//      its query, the smallest such.  Against a brute-force scorer: per query the set logic with std::set, 64-bit sums
//      of saturated products over all postings of the terms as named, the overflow rule on the ids of the result only.
//   3. The source list of the ranked calls with payloads (query_sources, query_sources_first_bad) over synthetic term and
//      exclusion sets, small and large batches (both ways of br_refs): with nothing excluded it is the layout written
//      out here on its own -- the referenced lists ascending, list u at entry 2u and its payload at 2u + 1, a term at
//      2 * (its list's rank); a list that is only excluded gets no payload entry; rid maps every name to the id entry
//      of its list; and the first bad entry names the smallest batch index, for a failing header and for a payload
//      whose n differs alike.
// Built with -fsanitize=address,undefined and run by tests/test_topk_bool_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

using namespace ansx_plan;

static const u32 TILE = 1024;  // ANSX_ISECT_TILE
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
    std::vector<u32> rid, w, xrid;
    std::vector<u64> qoff = { 0 }, xqoff = { 0 };
    void add(const std::vector<u32>& t, const std::vector<u32>& weights, const std::vector<u32>& x = {})
    {
        rid.insert(rid.end(), t.begin(), t.end());
        w.insert(w.end(), weights.begin(), weights.end());
        xrid.insert(xrid.end(), x.begin(), x.end());
        qoff.push_back(rid.size()), xqoff.push_back(xrid.size());
    }
    size_t size() const { return qoff.size() - 1; }
};

typedef std::vector<std::vector<u32>> Lists;

// what the call answers for query q: overflow, or (id, score) of every id of R(q)
static bool brute(const Queries& Q, size_t q, const Lists& ids, const Lists& pay, std::map<u32, u64>* out)
{
    std::map<u32, u64> score;
    std::map<u32, u32> in;  // the terms (as named) that hold the id
    for (u64 t = Q.qoff[q]; t < Q.qoff[q + 1]; t++) {
        const std::vector<u32>& l = ids[Q.rid[t]];
        std::set<u32> distinct(l.begin(), l.end());
        for (const u32 d : distinct) in[d]++;
        for (size_t x = 0; x < l.size(); x++) score[l[x]] += topk_sat32(Q.w[t], pay[Q.rid[t]][x]);
    }
    std::set<u32> X;
    for (u64 t = Q.xqoff[q]; t < Q.xqoff[q + 1]; t++) X.insert(ids[Q.xrid[t]].begin(), ids[Q.xrid[t]].end());
    bool over = false;
    out->clear();
    for (const auto& e : score) {
        if (in[e.first] != Q.qoff[q + 1] - Q.qoff[q] || X.count(e.first)) continue;
        if (e.second >= 0xFFFFFFFFull) over = true;
        (*out)[e.first] = e.second;
    }
    return over;
}

// -> the groups; *oflow: the first query of the batch with an overflowing result, ~0 where there is none
static size_t check_plan(const char* what, const std::vector<u64>& n, const Queries& Q, u64 budget, const Lists& ids, const Lists& pay,
    bool bounded, size_t* oflow)
{
    std::vector<IsbGroup> G0, G;
    size_t bad = ~(size_t)0;
    const bool x = !Q.xrid.empty();
    const u32* xr = x ? Q.xrid.data() : nullptr;
    const u64* xq = x ? Q.xqoff.data() : nullptr;
    CHECK(isb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, &G0, &bad, xr, xq) == ANSX_OK);
    CHECK(isb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, &G, &bad, xr, xq, true) == ANSX_OK);
    CHECK(bad == ~(size_t)0 && G.size() == G0.size());
    *oflow = ~(size_t)0;
    for (size_t gi = 0; gi < G.size(); gi++) {
        const IsbGroup &g = G[gi], &g0 = G0[gi];
        const size_t nq = g.q1 - g.q0;
        // nothing else differs
        CHECK(g0.dterm.empty() && g0.rterm.empty() && g.q0 == g0.q0 && g.q1 == g0.q1 && g.lists == g0.lists && g.at == g0.at);
        CHECK(g.rt_off == g0.rt_off && g.rt_list == g0.rt_list && g.drv == g0.drv && g.xt_off == g0.xt_off && g.xt_list == g0.xt_list);
        CHECK(g.ints == g0.ints && g.rounds == g0.rounds && g.G.size() == g0.G.size() && g.rt.size() == g0.rt.size() && g.xt.size() == g0.xt.size());
        CHECK(memcmp(g.G.data(), g0.G.data(), sizeof(ansx_isb_query) * g.G.size()) == 0);
        CHECK(g.rt.empty() || memcmp(g.rt.data(), g0.rt.data(), sizeof(ansx_isb_list) * g.rt.size()) == 0);
        CHECK(g.xt.empty() || memcmp(g.xt.data(), g0.xt.data(), sizeof(ansx_isb_list) * g.xt.size()) == 0);
        // the terms: of the query, of the list the table names, each once
        CHECK(g.dterm.size() == nq && g.rterm.size() == g.rt.size());
        std::vector<u32> seen(Q.rid.size(), 0);
        for (size_t j = 0; j < nq; j++) {
            const u64 t0 = Q.qoff[g.q0 + j], t1 = Q.qoff[g.q0 + j + 1];
            CHECK(g.dterm[j] >= t0 && g.dterm[j] < t1 && Q.rid[g.dterm[j]] == g.drv[j]);
            seen[g.dterm[j]]++;
            CHECK(g.rt_off[j + 1] - g.rt_off[j] == t1 - t0 - 1);
            u64 before = n[g.drv[j]];
            for (u32 e = g.rt_off[j]; e < g.rt_off[j + 1]; e++) {
                CHECK(g.rterm[e] >= t0 && g.rterm[e] < t1 && Q.rid[g.rterm[e]] == g.rt_list[e] && g.rt[e].n == n[g.rt_list[e]]);
                CHECK(before <= g.rt[e].n);  // ascending n from the driver on
                before = g.rt[e].n, seen[g.rterm[e]]++;
            }
        }
        for (u64 t = Q.qoff[g.q0]; t < Q.qoff[g.q1]; t++) CHECK(seen[t] == 1);

        // run it
        const u64 L = g.at.back(), nc0 = g.G[nq].dst;
        std::vector<u32> lists(L), vlists(L);
        for (size_t i = 0; i < g.lists.size(); i++) {
            std::copy(ids[g.lists[i]].begin(), ids[g.lists[i]].end(), lists.begin() + g.at[i]);
            std::copy(pay[g.lists[i]].begin(), pay[g.lists[i]].end(), vlists.begin() + g.at[i]);
        }
        std::vector<u32> cand(nc0), score(nc0), seg(nq + 1);
        for (size_t j = 0; j <= nq; j++) seg[j] = (u32)g.G[j].dst;
        for (size_t j = 0; j < nq; j++)
            for (u64 i = g.G[j].dst; i < g.G[j + 1].dst; i++) {
                CHECK(g.G[j].src + (i - g.G[j].dst) < L);
                cand[i] = lists[g.G[j].src + (i - g.G[j].dst)];
            }
        auto query_of = [&](u32 i) {  // the LAST j with seg[j] <= i
            size_t j = nq - 1;
            while (seg[j] > i) j--;
            return j;
        };
        const u32 rounds = std::max<u32>(g.rounds, 1u);
        for (u32 r = 0; r < rounds && !cand.empty(); r++) {
            const u32 nc = (u32)cand.size();
            std::vector<char> member(nc, 0);
            for (u32 i0 = 0; i0 < nc; i0 += TILE) {
                const u32 last = std::min(i0 + TILE, nc) - 1;
                const size_t qa = query_of(i0), qz = query_of(last);
                u64 blo = 0, bhi = 0;
                bool b = false;
                if (bounded && qa == qz && g.rt_off[qa] + r < g.rt_off[qa + 1]) {
                    const ansx_isb_list Ls = g.rt[g.rt_off[qa] + r];
                    const u32* l = lists.data() + Ls.at;
                    blo = (u64)(std::lower_bound(l, l + Ls.n, cand[i0]) - l), bhi = (u64)(std::upper_bound(l, l + Ls.n, cand[last]) - l);
                    bhi = std::max(bhi, blo), b = true;
                }
                for (u32 i = i0; i <= last; i++) {
                    const size_t q = query_of(i);
                    const u32 t = cand[i];
                    u32 sc = 0;
                    bool m = true;
                    if (r == 0) {
                        m = i == seg[q] || cand[i - 1] != t;
                        if (m)
                            for (u32 e = i; e < seg[q + 1] && cand[e] == t; e++) {
                                CHECK(g.G[q].src + (e - g.G[q].dst) < L);
                                sc = topk_sat_add(sc, topk_sat32(Q.w[g.dterm[q]], vlists[g.G[q].src + (e - g.G[q].dst)]));
                            }
                    } else {
                        sc = score[i];
                    }
                    const u32 e = g.rt_off[q] + r;
                    if (m && e < g.rt_off[q + 1]) {
                        const ansx_isb_list Ls = g.rt[e];
                        CHECK(Ls.at + Ls.n <= L);
                        const u32* l = lists.data() + Ls.at;
                        const u64 hi = b ? bhi : Ls.n;
                        u64 p = (u64)(std::lower_bound(l + (b ? blo : 0), l + hi, t) - l);
                        m = p < hi && l[p] == t;
                        if (m)
                            for (; p < Ls.n && l[p] == t; p++) sc = topk_sat_add(sc, topk_sat32(Q.w[g.rterm[e]], vlists[Ls.at + p]));
                    }
                    member[i] = m;
                    if (m) score[i] = sc;
                }
            }
            // the compaction, ids and scores by the same ballots, and the bounds
            std::vector<u32> nc_, ns_, nseg(nq + 1);
            size_t j = 0;
            for (u32 i = 0; i < nc; i++) {
                for (; j <= nq && seg[j] <= i; j++) nseg[j] = (u32)nc_.size();
                if (member[i]) nc_.push_back(cand[i]), ns_.push_back(score[i]);
            }
            for (; j <= nq; j++) nseg[j] = (u32)nc_.size();
            cand.swap(nc_), score.swap(ns_), seg.swap(nseg);
        }
        if (cand.empty()) std::fill(seg.begin(), seg.end(), 0u);
        if (!g.xt.empty() && !cand.empty()) {  // the exclusion step
            std::vector<u32> nc_, ns_, nseg(nq + 1);
            for (size_t j = 0; j < nq; j++) {
                nseg[j] = (u32)nc_.size();
                for (u32 i = seg[j]; i < seg[j + 1]; i++) {
                    bool keep = true;
                    for (u32 e = g.xt_off[j]; e < g.xt_off[j + 1] && keep; e++) {
                        CHECK(g.xt[e].at + g.xt[e].n <= L);
                        const u32* l = lists.data() + g.xt[e].at;
                        keep = !std::binary_search(l, l + g.xt[e].n, cand[i]);
                    }
                    if (keep) nc_.push_back(cand[i]), ns_.push_back(score[i]);
                }
            }
            nseg[nq] = (u32)nc_.size();
            cand.swap(nc_), score.swap(ns_), seg.swap(nseg);
        }
        // the overflow rule and the results
        for (size_t j = 0; j < nq; j++) {
            std::map<u32, u64> want;
            const bool over = brute(Q, g.q0 + j, ids, pay, &want);
            bool got_over = false;
            CHECK(seg[j + 1] - seg[j] == want.size());
            for (u32 i = seg[j]; i < seg[j + 1]; i++) {
                CHECK(i == seg[j] || cand[i - 1] < cand[i]);  // distinct, ascending
                CHECK(want.count(cand[i]));
                got_over |= score[i] == 0xFFFFFFFFu;
                CHECK(score[i] == (u32)std::min<u64>(want[cand[i]], 0xFFFFFFFFull));  // (saturated exactly from 2^32 - 1 on)
            }
            CHECK(got_over == over);
            if (got_over && *oflow == ~(size_t)0) *oflow = g.q0 + j;
        }
    }
    return G.size();
}

static void sat_cases()
{
    const char* what = "saturating add";
    CHECK(topk_sat_add(0, 0) == 0 && topk_sat_add(0xFFFFFFFEu, 0) == 0xFFFFFFFEu && topk_sat_add(0xFFFFFFFDu, 1) == 0xFFFFFFFEu);
    CHECK(topk_sat_add(0xFFFFFFFEu, 1) == 0xFFFFFFFFu && topk_sat_add(0xFFFFFFFEu, 2) == 0xFFFFFFFFu);
    CHECK(topk_sat_add(0xFFFFFFFFu, 0) == 0xFFFFFFFFu && topk_sat_add(0xFFFFFFFFu, 0xFFFFFFFFu) == 0xFFFFFFFFu);
    CHECK(topk_sat_add(0x80000000u, 0x7FFFFFFFu) == 0xFFFFFFFFu && topk_sat_add(0x80000000u, 0x7FFFFFFEu) == 0xFFFFFFFEu);
    std::mt19937_64 rng(3);
    for (int i = 0; i < 2000; i++) {  // 0xFFFFFFFF exactly when the 64-bit sum reaches 2^32 - 1, in any order of the terms
        u64 sum = 0;
        u32 acc = 0;
        const int m = 1 + (int)(rng() % 6);
        for (int j = 0; j < m; j++) {
            const u32 v = (rng() & 1) ? (u32)(rng() >> (32 + rng() % 8)) : (u32)(rng() % 3);
            sum += v, acc = topk_sat_add(acc, v);
        }
        CHECK((acc == 0xFFFFFFFFu) == (sum >= 0xFFFFFFFFull) && (acc == 0xFFFFFFFFu || acc == sum));
    }
}

static void plan_cases()
{
    std::mt19937_64 rng(9);
    // lists 0..12 of these lengths (two empty ones, two ties), ascending ids with repeats, payloads 0..3
    const std::vector<u64> n = { 5, 0, 1, 100, 4096, 4097, 0, 333, 1000, 64, 100, 3000, 2500 };
    Lists ids(n.size()), pay(n.size());
    for (size_t i = 0; i < n.size(); i++) {
        u32 at = 0;
        for (u64 x = 0; x < n[i]; x++) ids[i].push_back(at += (u32)(rng() % 3)), pay[i].push_back((u32)(rng() % 4));
    }
    ids[2][0] = ids[4][100];
    // the overflow lists: 13 holds id 7 with payloads that reach 2^32 - 2 under weight 4, 14 adds 1 or 2, 15 lacks id 7,
    // 16 excludes it
    Lists oi = { { 7, 9, 11 }, { 7 }, { 9, 11, 12, 13 }, { 7, 100 }, { 7, 7, 9 } }, op = { { 0x3FFFFFFFu, 5, 6 }, { 1 }, { 1, 1, 1, 1 }, { 0, 0 }, { 0x3FFFFFFFu, 0x3FFFFFFFu, 1 } };
    std::vector<u64> n2 = n;
    for (size_t i = 0; i < oi.size(); i++) ids.push_back(oi[i]), pay.push_back(op[i]), n2.push_back(oi[i].size());
    {
        Queries Q;
        Q.add({ 3 }, { 2 });                                       // 1 term: the seed round alone
        Q.add({ 0, 7 }, { 1, 3 }, { 9 });                          // 2
        Q.add({ 4, 1, 5 }, { 1, 1, 1 });                           // an empty list as a term: nothing
        Q.add({ 8, 9, 0, 3, 7 }, { 1, 2, 3, 4, 0 }, { 2, 6 });     // 5, a weight 0, an empty excluded list
        Q.add({ 7, 7 }, { 2, 5 });                                 // a list named twice, different weights: a driver tie
        Q.add({ 3, 10 }, { 1, 1 });                                // a tie of two lists: the earlier drives
        Q.add({ 10, 3 }, { 1, 1 }, { 3 });                         // ... and a term that is excluded as well: nothing
        Q.add({ 1 }, { 1 });                                       // nothing but an empty list
        Q.add({ 11, 12, 5, 4 }, { 1, 2, 3, 1 }, { 8, 7 });         // long lists: tiles inside one query, two excluded lists
        Q.add({ 4, 5 }, { 3, 3 });
        Q.add({ 2, 4 }, { 1, 1 });                                 // a driver of one id that the list holds
        Q.add({ 4, 4, 4 }, { 1, 2, 3 }, { 0 });                    // the driver's own repeats, three times
        u64 all = 0;
        for (size_t q = 0; q < Q.size(); q++)
            for (u64 t = Q.qoff[q]; t < Q.qoff[q + 1]; t++) all += 3 * n2[Q.rid[t]];
        for (const bool bounded : { false, true }) {
            size_t of = 0;
            const char* what = "one group";
            CHECK(check_plan(what, n2, Q, 4 * all, ids, pay, bounded, &of) == 1 && of == ~(size_t)0);
            what = "a group per query";
            const size_t most = check_plan(what, n2, Q, 0, ids, pay, bounded, &of);
            CHECK(most >= Q.size() - 3 && most <= Q.size() && of == ~(size_t)0);
            what = "several groups";
            const size_t some = check_plan(what, n2, Q, all / 4, ids, pay, bounded, &of);
            CHECK(some > 1 && some < most && of == ~(size_t)0);
        }
    }
    {
        Queries Q;
        Q.add({ 13, 14 }, { 4, 2 });              // 2^32 - 2: a result
        Q.add({ 13 }, { 5 }, { 16 });             // a product that saturates, of an excluded id: no error
        Q.add({ 13, 13, 15 }, { 4, 4, 1 });       // a partial sum that saturates, of an id a later list lacks: no error
        Q.add({ 13, 14 }, { 4, 3 });              // 2^32 - 1: the error
        Q.add({ 3 }, { 1 });
        Q.add({ 17, 17 }, { 2, 2 });              // the driver's own repeats pass 2^32: the error again, not the first
        Q.add({ 13, 14 }, { 4, 3 }, { 14 });      // ... excluded
        for (const bool bounded : { false, true })
            for (const u64 budget : { (u64)1 << 20, (u64)0, (u64)40 }) {
                size_t of = 0;
                const char* what = "overflow";
                check_plan(what, n2, Q, budget, ids, pay, bounded, &of);
                CHECK(of == 3);
            }
    }
}

// the smallest batch index at fault, found the slow way: a list whose id or payload header fails, or whose two differ in n
static size_t slow_first_bad(const std::vector<u32>& named, size_t nt, const std::set<u32>& fails_id, const std::set<u32>& fails_pay,
    const std::set<u32>& differs)
{
    std::set<u32> terms(named.begin(), named.begin() + nt), all(named.begin(), named.end());
    for (const u32 i : all) {  // (ascending)
        if (fails_id.count(i)) return i;
        if (terms.count(i) && (fails_pay.count(i) || differs.count(i))) return i;
    }
    return ~(size_t)0;
}

static void source_cases()
{
    std::mt19937_64 rng(21);
    const char* what = "source list";
    for (int round = 0; round < 300; round++) {
        const size_t count = round % 3 == 0 ? 40 : round % 3 == 1 ? 5000 : 1 + rng() % 9;  // (5000 > 4 * names + 1024: br_refs sorts)
        const size_t nt = 1 + rng() % 30, nx = round % 4 == 0 ? 0 : rng() % 12;
        std::vector<u32> named(nt + nx);
        for (u32& t : named) t = (u32)(rng() % count);
        QuerySources S;
        query_sources(named.data(), nt, named.size(), count, &S);
        const std::set<u32> terms(named.begin(), named.begin() + nt), all(named.begin(), named.end());
        // every referenced list once, ascending; its id entry, then its payload's where it is a term and only there
        CHECK(S.uniq == std::vector<u32>(all.begin(), all.end()) && S.idpos.size() == S.uniq.size());
        CHECK(S.owner.size() == all.size() + terms.size() && S.pay.size() == S.owner.size() && S.payof.size() == S.owner.size());
        size_t e = 0;
        for (size_t u = 0; u < S.uniq.size(); u++) {
            const bool term = terms.count(S.uniq[u]) != 0;
            CHECK(S.idpos[u] == e && S.owner[e] == u && !S.pay[e] && S.batch_index(e) == S.uniq[u]);
            CHECK(S.payof[e] == (term ? (u32)e + 1 : ANSX_TOPK_NONE));
            e++;
            if (!term) continue;  // (only excluded: no payload entry)
            CHECK(S.owner[e] == u && S.pay[e] == 1 && S.payof[e] == ANSX_TOPK_NONE && S.batch_index(e) == S.uniq[u]);
            e++;
        }
        CHECK(e == S.owner.size() && S.rid.size() == named.size());
        for (size_t j = 0; j < named.size(); j++) CHECK(!S.pay[S.rid[j]] && S.batch_index(S.rid[j]) == named[j]);
        if (nx == 0) {  // the layout of ansx_topk_batch_dev, written out on its own
            std::vector<u32> sorted(named.begin(), named.end());
            std::sort(sorted.begin(), sorted.end());
            sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
            CHECK(S.owner.size() == 2 * sorted.size());
            for (size_t u = 0; u < sorted.size(); u++) {
                CHECK(S.batch_index(2 * u) == sorted[u] && S.batch_index(2 * u + 1) == sorted[u] && !S.pay[2 * u] && S.pay[2 * u + 1]);
                CHECK(S.payof[2 * u] == 2 * u + 1);
            }
            for (size_t j = 0; j < nt; j++)
                CHECK(S.rid[j] == 2 * (u32)(std::lower_bound(sorted.begin(), sorted.end(), named[j]) - sorted.begin()));
        }
        // the first bad list: headers with n = 100 + the batch index; some fail, some payloads differ in n
        std::set<u32> fails_id, fails_pay, differs;
        for (int k = (int)(rng() % 3); k > 0; k--) ((rng() & 1) ? fails_id : fails_pay).insert(named[rng() % named.size()]);
        for (int k = (int)(rng() % 3); k > 0; k--) differs.insert(named[rng() % named.size()]);
        std::vector<BatchSrc> rs(S.owner.size());
        size_t failed = rs.size();
        for (size_t i = 0; i < rs.size(); i++) {
            const u32 b = (u32)S.batch_index(i);
            memset(&rs[i], 0, sizeof rs[i]);
            rs[i].H.n = 100 + b + (S.pay[i] && differs.count(b) ? 1 : 0);
            if (failed == rs.size() && (S.pay[i] ? fails_pay : fails_id).count(b)) failed = i;
        }
        for (size_t i = failed; i < rs.size(); i++) rs[i].H.n = 0xDEAD;  // (behind the first failure nothing is looked at)
        const size_t bad = query_sources_first_bad(S, rs, failed), want = slow_first_bad(named, nt, fails_id, fails_pay, differs);
        CHECK(bad <= failed && (bad == rs.size()) == (want == ~(size_t)0));
        if (bad < rs.size()) CHECK(S.batch_index(bad) == want);
    }
}

int main()
{
    sat_cases();
    plan_cases();
    source_cases();
    printf("ok: %ld checks\n", checks);
    return 0;
}
