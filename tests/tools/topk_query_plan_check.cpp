// The host side of ansx_topk_query_batch_dev on the CPU (ans_large_alphabet_amd/csrc/ansx_plan.h: query_split,
// query_runs, isb_plan with the optional terms as orid / oqoff, unb_plan; ansx_plan_types.h, topk_sat32 and
// topk_sat_add), over synthetic headers: lists of given lengths -- empty ones among them, which no container can hold --
// whose ids and payloads are made up here.
//   1. With the new inputs null, isb_plan's outputs are what they are with the inputs absent, bit for bit, and the
//      optional tables stay empty; unb_plan has no new input, and a run planned at an offset is the plan of the run's
//      queries alone.
//   2. The optional tables against the terms as named: per query of a group one entry per optional term, in order, its
//      list (ot_list), its place in orid (oterm), n the list's and at where the group decodes it; an optional list counts
//      once in the group's budget and joins its decoded lists.
//   3. The split and the runs: every term lands once, in order, on its side with its place in `terms`; the threshold as it
//      applies; maximal runs of one kind that cover the batch in order.
//   4. Every group of every run RUN the way the kernels run it.  Kind R (ansx_topk_bool.h, ansx_topk_query.h): the
//      drivers gathered, round 0 seeds, every required round takes the lower bound and adds the postings, the members
//      compacted; then the optional step over tiles of 1024 candidates -- a tile inside one query bounds [lo, hi) per
//      list and searches there (staged: at most 4096 ints; else in place), a tile that spans queries searches whole
//      lists -- with topk_sat_add per posting and a match count, the ballot "matches >= m"; then the exclusion step; then
//      the overflow rule over the survivors.  Kind O (ansx_topk.h): the terms merged, the heads, the 64-bit sums, the
//      entries per head against m, the exclusion, the overflow rule.  Against a brute-force scorer of the definition:
//      per query std::map / std::set over all postings of the terms as named.
//   5. The plans' limits name the first query in batch order whatever its kind.
// The plan of a call is query_plan's, the function ansx_topk_query_batch_dev calls: nothing of it is written again here.
// Built with -fsanitize=address,undefined and run by tests/test_topk_query_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

using namespace ansx_plan;

static const u32 TILE = 1024;   // ANSX_ISECT_TILE
static const u32 STAGE = 4096;  // ANSX_BOOL_STAGE
static const u32 UTILE = 4096;  // ANSX_UNION_TILE
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
    std::vector<u32> rid, w, xrid, msm;
    std::vector<u8> occ;
    std::vector<u64> qoff = { 0 }, xqoff = { 0 };
    void add(const std::vector<u32>& t, const std::vector<u8>& o, const std::vector<u32>& weights, u32 m, const std::vector<u32>& x = {})
    {
        rid.insert(rid.end(), t.begin(), t.end());
        occ.insert(occ.end(), o.begin(), o.end());
        w.insert(w.end(), weights.begin(), weights.end());
        xrid.insert(xrid.end(), x.begin(), x.end());
        qoff.push_back(rid.size()), xqoff.push_back(xrid.size()), msm.push_back(m);
    }
    size_t size() const { return qoff.size() - 1; }
};

typedef std::vector<std::vector<u32>> Lists;

// the definition: overflow among R(q), and (id, 64-bit score) of every id of R(q)
static bool brute(const Queries& Q, size_t q, const Lists& ids, const Lists& pay, std::map<u32, u64>* out)
{
    std::map<u32, u64> score, matches;
    std::map<u32, u32> in;  // the required terms (as named) that hold the id
    u32 nreq = 0;
    for (u64 t = Q.qoff[q]; t < Q.qoff[q + 1]; t++) {
        const std::vector<u32>& l = ids[Q.rid[t]];
        for (size_t x = 0; x < l.size(); x++) score[l[x]] += topk_sat32(Q.w[t], pay[Q.rid[t]][x]);
        if (Q.occ[t]) {
            std::set<u32> distinct(l.begin(), l.end());
            for (const u32 d : distinct) in[d]++;
            nreq++;
        } else {
            for (const u32 d : l) matches[d]++;
        }
    }
    const u64 m = nreq ? Q.msm[q] : std::max<u32>(Q.msm[q], 1u);
    std::set<u32> X;
    for (u64 t = Q.xqoff[q]; t < Q.xqoff[q + 1]; t++) X.insert(ids[Q.xrid[t]].begin(), ids[Q.xrid[t]].end());
    bool over = false;
    out->clear();
    for (const auto& e : score) {
        if (in[e.first] != nreq || matches[e.first] < m || X.count(e.first)) continue;
        if (e.second >= 0xFFFFFFFFull) over = true;
        (*out)[e.first] = e.second;
    }
    return over;
}

// what a group leaves: the survivors of its queries back to back
struct Left {
    std::vector<u32> cand, score, seg;
};

static void compact(const std::vector<char>& member, size_t nq, Left* S)
{
    std::vector<u32> nc_, ns_, nseg(nq + 1);
    size_t j = 0;
    for (u32 i = 0; i < (u32)S->cand.size(); i++) {
        for (; j <= nq && S->seg[j] <= i; j++) nseg[j] = (u32)nc_.size();
        if (member[i]) nc_.push_back(S->cand[i]), ns_.push_back(S->score[i]);
    }
    for (; j <= nq; j++) nseg[j] = (u32)nc_.size();
    S->cand.swap(nc_), S->score.swap(ns_), S->seg.swap(nseg);
}

static void exclude(const char* what, const std::vector<u32>& xt_off, const std::vector<ansx_isb_list>& xt, const std::vector<u32>& lists,
    size_t nq, Left* S)
{
    std::vector<char> keep(S->cand.size(), 1);
    for (size_t j = 0; j < nq; j++)
        for (u32 i = S->seg[j]; i < S->seg[j + 1]; i++)
            for (u32 e = xt_off[j]; e < xt_off[j + 1] && keep[i]; e++) {
                CHECK(xt[e].at + xt[e].n <= lists.size());
                const u32* l = lists.data() + xt[e].at;
                keep[i] = !std::binary_search(l, l + xt[e].n, S->cand[i]);
            }
    compact(keep, nq, S);
}

// a group of kind R the way topkb_group runs it; form: 0 the default rule, 1 "search", 2 "staged"
static void run_required(const char* what, const IsbGroup& g, const QuerySplit& P, const std::vector<u32>& w, const Lists& ids,
    const Lists& pay, u32 form, Left* S)
{
    const size_t nq = g.q1 - g.q0;
    const u64 L = g.at.back(), nc0 = g.G[nq].dst;
    std::vector<u32> lists(L), vlists(L);
    for (size_t i = 0; i < g.lists.size(); i++) {
        std::copy(ids[g.lists[i]].begin(), ids[g.lists[i]].end(), lists.begin() + g.at[i]);
        std::copy(pay[g.lists[i]].begin(), pay[g.lists[i]].end(), vlists.begin() + g.at[i]);
    }
    std::vector<u32>&cand = S->cand, &score = S->score, &seg = S->seg;
    cand.assign(nc0, 0), score.assign(nc0, 0), seg.assign(nq + 1, 0);
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
        for (u32 i = 0; i < nc; i++) {
            const size_t q = query_of(i);
            const u32 t = cand[i];
            u32 sc = 0;
            bool m = true;
            if (r == 0) {
                m = i == seg[q] || cand[i - 1] != t;
                if (m)
                    for (u32 e = i; e < seg[q + 1] && cand[e] == t; e++)
                        sc = topk_sat_add(sc, topk_sat32(w[P.rpos[g.dterm[q]]], vlists[g.G[q].src + (e - g.G[q].dst)]));
            } else {
                sc = score[i];
            }
            const u32 e = g.rt_off[q] + r;
            if (m && e < g.rt_off[q + 1]) {
                const ansx_isb_list Ls = g.rt[e];
                CHECK(Ls.at + Ls.n <= L);
                const u32* l = lists.data() + Ls.at;
                u64 p = (u64)(std::lower_bound(l, l + Ls.n, t) - l);
                m = p < Ls.n && l[p] == t;
                if (m)
                    for (; p < Ls.n && l[p] == t; p++) sc = topk_sat_add(sc, topk_sat32(w[P.rpos[g.rterm[e]]], vlists[Ls.at + p]));
            }
            member[i] = m;
            if (m) score[i] = sc;
        }
        compact(member, nq, S);
    }
    if (cand.empty()) {
        std::fill(seg.begin(), seg.end(), 0u);
        return;
    }
    // the optional step: where the group has an optional term or a threshold
    bool should = !g.ot.empty();
    for (size_t j = 0; j < nq; j++) should |= P.m[g.q0 + j] != 0;
    if (should) {
        const u32 nc = (u32)cand.size();
        std::vector<char> member(nc, 0);
        for (u32 i0 = 0; i0 < nc; i0 += TILE) {
            const u32 last = std::min(i0 + TILE, nc) - 1;
            const size_t qa = query_of(i0), qz = query_of(last);
            std::vector<u32> cnt(last - i0 + 1, 0);
            auto take = [&](const u32* l, u64 p, u64 end, u64 base, u32 i, u32 wt) {  // l[p ..) while equal; payloads at base + p
                for (; p < end && l[p] == cand[i]; p++) {
                    CHECK(base + p < L);
                    score[i] = topk_sat_add(score[i], topk_sat32(wt, vlists[base + p]));
                    cnt[i - i0]++;
                }
            };
            if (qa == qz) {
                for (u32 e = g.ot_off[qa]; e < g.ot_off[qa + 1]; e++) {
                    const ansx_isb_list Ls = g.ot[e];
                    CHECK(Ls.at + Ls.n <= L);
                    const u32* l = lists.data() + Ls.at;
                    const u64 lo = (u64)(std::lower_bound(l, l + Ls.n, cand[i0]) - l);
                    const u64 hi = std::max(lo, (u64)(std::upper_bound(l, l + Ls.n, cand[last]) - l));
                    if (lo == hi) continue;
                    const u32 wt = w[P.opos[g.oterm[e]]];
                    if (form != 1 && hi - lo <= STAGE) {
                        const std::vector<u32> stage(l + lo, l + hi);  // (its own memory: a read past the part is a finding)
                        for (u32 i = i0; i <= last; i++)
                            take(stage.data(), (u64)(std::lower_bound(stage.begin(), stage.end(), cand[i]) - stage.begin()), stage.size(),
                                Ls.at + lo, i, wt);
                    } else {
                        for (u32 i = i0; i <= last; i++) take(l, (u64)(std::lower_bound(l + lo, l + hi, cand[i]) - l), hi, Ls.at, i, wt);
                    }
                }
                for (u32 i = i0; i <= last; i++) member[i] = cnt[i - i0] >= P.m[g.q0 + qa];
            } else {
                for (u32 i = i0; i <= last; i++) {
                    const size_t q = query_of(i);
                    for (u32 e = g.ot_off[q]; e < g.ot_off[q + 1]; e++) {
                        const ansx_isb_list Ls = g.ot[e];
                        CHECK(Ls.at + Ls.n <= L);
                        const u32* l = lists.data() + Ls.at;
                        take(l, (u64)(std::lower_bound(l, l + Ls.n, cand[i]) - l), Ls.n, Ls.at, i, w[P.opos[g.oterm[e]]]);
                    }
                    member[i] = cnt[i - i0] >= P.m[g.q0 + q];
                }
            }
        }
        compact(member, nq, S);
    }
    if (!g.xt.empty() && !cand.empty()) exclude(what, g.xt_off, g.xt, lists, nq, S);
}

// a group of kind O the way topk_group runs it
static void run_optional(const char* what, const UnbGroup& g, const Queries& Q, const std::vector<u32>& m, const Lists& ids,
    const Lists& pay, Left* S)
{
    const size_t nq = g.q1 - g.q0;
    const u64 L = g.at.back();
    std::vector<u32> lists(L);
    for (size_t i = 0; i < g.lists.size(); i++) std::copy(ids[g.lists[i]].begin(), ids[g.lists[i]].end(), lists.begin() + g.at[i]);
    S->cand.clear(), S->score.clear(), S->seg.assign(nq + 1, 0);
    bool least = false;
    for (size_t j = 0; j < nq; j++) least |= m[g.q0 + j] >= 2;
    for (size_t j = 0; j < nq; j++) {
        const size_t q = g.q0 + j;
        std::vector<std::pair<u32, u32>> merged;  // the query's span of the merge buffers: (id, saturated product)
        for (u64 t = Q.qoff[q]; t < Q.qoff[q + 1]; t++)
            for (size_t x = 0; x < ids[Q.rid[t]].size(); x++) merged.push_back({ ids[Q.rid[t]][x], topk_sat32(Q.w[t], pay[Q.rid[t]][x]) });
        CHECK(g.seg[j + 1] - g.seg[j] == merged.size());
        std::stable_sort(merged.begin(), merged.end(), [](const std::pair<u32, u32>& a, const std::pair<u32, u32>& b) { return a.first < b.first; });
        S->seg[j] = (u32)S->cand.size();
        for (size_t h = 0; h < merged.size();) {  // a head, the end of its run, its 64-bit sum
            size_t end = h;
            u64 sum = 0;
            for (; end < merged.size() && merged[end].first == merged[h].first; end++) sum += merged[end].second;
            // (without the filter a head is kept whatever m: m is at most 1 and a head has an entry)
            if (!least || end - h >= m[q]) S->cand.push_back(merged[h].first), S->score.push_back((u32)std::min<u64>(sum, 0xFFFFFFFFull));
            h = end;
        }
    }
    S->seg[nq] = (u32)S->cand.size();
    if (!g.xt.empty() && !S->cand.empty()) exclude(what, g.xt_off, g.xt, lists, nq, S);
}

// the whole call -> its groups; *oflow: the first query of the batch with an overflowing result, ~0 where there is none
static size_t check_call(const char* what, const std::vector<u64>& n, const Queries& Q, u64 budget, const Lists& ids, const Lists& pay,
    u32 form, size_t* oflow, size_t* nruns = nullptr)
{
    const size_t nq = Q.size();
    const bool x = !Q.xrid.empty();
    const u32* xr = x ? Q.xrid.data() : nullptr;
    // the plan of the whole call, by the function the library calls
    QueryPlan QP;
    size_t bad_call = ~(size_t)0;
    CHECK(query_plan(n.data(), n.size(), Q.rid.data(), Q.occ.data(), Q.qoff.data(), Q.msm.data(), xr, x ? Q.xqoff.data() : nullptr, nq,
              budget, UTILE, &QP, &bad_call) == ANSX_OK);
    CHECK(bad_call == ~(size_t)0);
    const QuerySplit& P = QP.split;
    // 3. the split
    CHECK(P.rqoff.size() == nq + 1 && P.oqoff.size() == nq + 1 && P.m.size() == nq && P.rrid.size() + P.orid.size() == Q.rid.size());
    for (size_t q = 0; q < nq; q++) {
        u64 r = P.rqoff[q], o = P.oqoff[q];
        for (u64 t = Q.qoff[q]; t < Q.qoff[q + 1]; t++)
            if (Q.occ[t]) {
                CHECK(r < P.rqoff[q + 1] && P.rpos[r] == t && P.rrid[r] == Q.rid[t]);
                r++;
            } else {
                CHECK(o < P.oqoff[q + 1] && P.opos[o] == t && P.orid[o] == Q.rid[t]);
                o++;
            }
        CHECK(r == P.rqoff[q + 1] && o == P.oqoff[q + 1]);
        CHECK(P.m[q] == (P.rqoff[q + 1] > P.rqoff[q] ? Q.msm[q] : std::max<u32>(Q.msm[q], 1u)));
    }
    // ... and the runs: maximal, of one kind, the batch in order
    const std::vector<QueryRun>& runs = QP.runs;
    CHECK(QP.plans.size() == runs.size());
    size_t at = 0;
    for (size_t r = 0; r < runs.size(); r++) {
        CHECK(runs[r].a == at && runs[r].b > runs[r].a && (r == 0 || runs[r].req != runs[r - 1].req));
        for (size_t q = runs[r].a; q < runs[r].b; q++) CHECK((P.rqoff[q + 1] > P.rqoff[q]) == runs[r].req);
        at = runs[r].b;
    }
    CHECK(at == nq);
    if (nruns) *nruns = runs.size();

    *oflow = ~(size_t)0;
    size_t ngroups = 0;
    for (size_t ri = 0; ri < runs.size(); ri++) {
        const QueryRun& run = runs[ri];
        const size_t a = run.a, cnt = run.b - run.a;
        const u64* xq = x ? Q.xqoff.data() + a : nullptr;
        size_t bad = ~(size_t)0;
        std::vector<Left> left;
        std::vector<std::pair<size_t, size_t>> span;
        if (run.req) {
            std::vector<IsbGroup> G = QP.plans[ri].req, G0;  // (q0 / q1: the call's query numbers)
            CHECK(QP.plans[ri].opt.empty());
            // the same run without its optional terms: the drivers, the rounds and the excluded tables of every query
            CHECK(isb_plan(n.data(), n.size(), P.rrid.data(), P.rqoff.data() + a, cnt, ~(u64)0 >> 2, &G0, &bad, xr, xq, true) == ANSX_OK);
            CHECK(bad == ~(size_t)0 && G0.size() == 1);
            size_t e0 = 0, x0 = 0;
            for (IsbGroup& g : G) {
                const size_t Qn = g.q1 - g.q0;
                // 2. the optional tables
                CHECK(g.ot_off.size() == Qn + 1 && g.ot.size() == g.ot_list.size() && g.ot.size() == g.oterm.size());
                std::set<u32> named;
                u64 ints = 0;
                for (size_t j = 0; j < Qn; j++) {
                    const size_t q = g.q0 + j;
                    CHECK(g.ot_off[j + 1] - g.ot_off[j] == P.oqoff[q + 1] - P.oqoff[q]);
                    for (u32 e = g.ot_off[j]; e < g.ot_off[j + 1]; e++) {
                        const u64 t = P.oqoff[q] + (e - g.ot_off[j]);
                        CHECK(g.oterm[e] == t && g.ot_list[e] == P.orid[t] && g.ot[e].n == n[P.orid[t]]);
                        const size_t k = (size_t)(std::lower_bound(g.lists.begin(), g.lists.end(), P.orid[t]) - g.lists.begin());
                        if (g.ot[e].n) CHECK(k < g.lists.size() && g.lists[k] == P.orid[t] && g.ot[e].at == g.at[k]);
                    }
                    for (u64 t = P.rqoff[q]; t < P.rqoff[q + 1]; t++) named.insert(P.rrid[t]);
                    for (u64 t = P.oqoff[q]; t < P.oqoff[q + 1]; t++) named.insert(P.orid[t]);
                    if (x)
                        for (u64 t = Q.xqoff[q]; t < Q.xqoff[q + 1]; t++) named.insert(Q.xrid[t]);
                    ints += 2 * (g.G[j + 1].dst - g.G[j].dst);
                    // the driver and the rounds: the required terms', whatever the optional ones
                    CHECK(g.drv[j] == G0[0].drv[q - a] && g.dterm[j] == G0[0].dterm[q - a]);
                    CHECK(g.rt_off[j + 1] - g.rt_off[j] == P.rqoff[q + 1] - P.rqoff[q] - 1);
                    for (u32 e = g.rt_off[j]; e < g.rt_off[j + 1]; e++, e0++)
                        CHECK(g.rt_list[e] == G0[0].rt_list[e0] && g.rterm[e] == G0[0].rterm[e0] && g.rt[e].n == G0[0].rt[e0].n);
                    if (x)
                        for (u32 e = g.xt_off[j]; e < g.xt_off[j + 1]; e++, x0++) CHECK(g.xt_list[e] == G0[0].xt_list[x0]);
                }
                std::vector<u32> want;  // every named list once, the empty ones left out
                for (const u32 r : named) {
                    ints += n[r];
                    if (n[r]) want.push_back(r);
                }
                CHECK(g.lists == want && g.ints == ints);
                left.emplace_back();
                run_required(what, g, P, Q.w, ids, pay, form, &left.back());
                span.push_back({ g.q0, g.q1 });
            }
        } else {
            std::vector<UnbGroup> G = QP.plans[ri].opt;
            CHECK(QP.plans[ri].req.empty());
            for (UnbGroup& g : G) {
                left.emplace_back();
                run_optional(what, g, Q, P.m, ids, pay, &left.back());
                span.push_back({ g.q0, g.q1 });
            }
        }
        CHECK(!span.empty() && span.front().first == run.a && span.back().second == run.b);
        for (size_t gi = 0; gi < left.size(); gi++) {
            const Left& S = left[gi];
            CHECK(gi == 0 || span[gi].first == span[gi - 1].second);
            for (size_t q = span[gi].first; q < span[gi].second; q++) {
                const size_t j = q - span[gi].first;
                std::map<u32, u64> want;
                const bool over = brute(Q, q, ids, pay, &want);
                bool got_over = false;
                CHECK(S.seg[j + 1] - S.seg[j] == want.size());
                for (u32 i = S.seg[j]; i < S.seg[j + 1]; i++) {
                    CHECK(i == S.seg[j] || S.cand[i - 1] < S.cand[i]);  // distinct, ascending
                    CHECK(want.count(S.cand[i]));
                    got_over |= S.score[i] == 0xFFFFFFFFu;
                    CHECK(S.score[i] == (u32)std::min<u64>(want[S.cand[i]], 0xFFFFFFFFull));  // (saturated exactly from 2^32 - 1 on)
                }
                CHECK(got_over == over);
                if (got_over && *oflow == ~(size_t)0) *oflow = q;
            }
        }
        ngroups += left.size();
    }
    return ngroups;
}

// 1. the new inputs null against the inputs absent
static void same_plans(const std::vector<u64>& n, const Queries& Q, u64 budget)
{
    const char* what = "null against absent";
    for (const bool terms : { false, true })
        for (const bool x : { false, true }) {
            std::vector<IsbGroup> G0, G;
            size_t b0 = 77, b1 = 77;
            const u32* xr = x ? Q.xrid.data() : nullptr;
            const u64* xq = x ? Q.xqoff.data() : nullptr;
            const int r0 = isb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, &G0, &b0, xr, xq, terms);
            const int r1 = isb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, &G, &b1, xr, xq, terms, nullptr, nullptr);
            CHECK(r0 == r1 && b0 == b1 && G.size() == G0.size());
            for (size_t gi = 0; gi < G.size(); gi++) {
                const IsbGroup &g = G[gi], &g0 = G0[gi];
                CHECK(g.q0 == g0.q0 && g.q1 == g0.q1 && g.lists == g0.lists && g.at == g0.at && g.rt_off == g0.rt_off);
                CHECK(g.rt_list == g0.rt_list && g.drv == g0.drv && g.xt_off == g0.xt_off && g.xt_list == g0.xt_list);
                CHECK(g.dterm == g0.dterm && g.rterm == g0.rterm && g.ints == g0.ints && g.rounds == g0.rounds);
                CHECK(g.G.size() == g0.G.size() && g.rt.size() == g0.rt.size() && g.xt.size() == g0.xt.size());
                CHECK(memcmp(g.G.data(), g0.G.data(), sizeof(ansx_isb_query) * g.G.size()) == 0);
                CHECK(g.rt.empty() || memcmp(g.rt.data(), g0.rt.data(), sizeof(ansx_isb_list) * g.rt.size()) == 0);
                CHECK(g.xt.empty() || memcmp(g.xt.data(), g0.xt.data(), sizeof(ansx_isb_list) * g.xt.size()) == 0);
                CHECK(g.ot_off.empty() && g.ot.empty() && g.ot_list.empty() && g.oterm.empty());
                CHECK(g0.ot_off.empty() && g0.ot.empty() && g0.ot_list.empty() && g0.oterm.empty());
            }
            // unb_plan has no new input: a run planned at an offset is the plan of its queries alone
            const size_t a = Q.size() / 3, cnt = Q.size() - a - 1;
            std::vector<u64> own(Q.qoff.begin() + a, Q.qoff.begin() + a + cnt + 1), xown(Q.xqoff.begin() + a, Q.xqoff.begin() + a + cnt + 1);
            std::vector<UnbGroup> U0, U;
            const int u0 = unb_plan(n.data(), n.size(), Q.rid.data(), own.data(), cnt, budget, UTILE, &U0, &b0, xr, x ? xown.data() : nullptr, terms);
            const int u1 = unb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data() + a, cnt, budget, UTILE, &U, &b1, xr, x ? xq + a : nullptr, terms);
            CHECK(u0 == ANSX_OK && u1 == ANSX_OK && U.size() == U0.size());
            for (size_t gi = 0; gi < U.size(); gi++) {
                const UnbGroup &g = U[gi], &g0 = U0[gi];
                CHECK(g.q0 == g0.q0 && g.q1 == g0.q1 && g.lists == g0.lists && g.at == g0.at && g.seg == g0.seg && g.roff == g0.roff);
                CHECK(g.tiles == g0.tiles && g.xt_off == g0.xt_off && g.xt_list == g0.xt_list && g.pterm == g0.pterm && g.ints == g0.ints);
                CHECK(g.rounds == g0.rounds && g.pairs.size() == g0.pairs.size());
                CHECK(g.pairs.empty() || memcmp(g.pairs.data(), g0.pairs.data(), sizeof(ansx_unb_pair) * g.pairs.size()) == 0);
            }
        }
}

static void cases()
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
    // the overflow lists: 13 holds id 7 with payloads that reach 2^32 - 4 under weight 4, 14 adds 2 or 3, 15 lacks id 7,
    // 16 excludes it, 17 holds it twice
    Lists oi = { { 7, 9, 11 }, { 7 }, { 9, 11, 12, 13 }, { 7, 100 }, { 7, 7, 9 } }, op = { { 0x3FFFFFFFu, 5, 6 }, { 1 }, { 1, 1, 1, 1 }, { 0, 0 }, { 0x3FFFFFFFu, 0x3FFFFFFFu, 1 } };
    std::vector<u64> n2 = n;
    for (size_t i = 0; i < oi.size(); i++) ids.push_back(oi[i]), pay.push_back(op[i]), n2.push_back(oi[i].size());
    const u8 M = 1, S = 0;
    {
        Queries Q;
        Q.add({ 3, 7 }, { M, S }, { 2, 3 }, 0);                                  // R  +a b
        Q.add({ 3, 7, 8 }, { M, S, S }, { 2, 3, 1 }, 1);                          // R  +a b c, at least one
        Q.add({ 4, 5, 11, 12 }, { S, S, S, S }, { 1, 2, 3, 4 }, 2, { 9 });        // O  at least two, tiles of many heads
        Q.add({ 4, 1, 5 }, { M, M, S }, { 1, 1, 1 }, 0);                          // R  an empty required list: nothing
        Q.add({ 4, 1, 6, 5 }, { M, S, S, S }, { 1, 1, 1, 1 }, 1, { 6, 2 });       // R  empty optional and excluded lists
        Q.add({ 1, 6 }, { S, S }, { 1, 1 }, 0);                                   // O  nothing but empty lists
        Q.add({ 1, 3 }, { S, S }, { 1, 4 }, 1, { 1 });                            // O  an empty optional list, an empty excluded one
        Q.add({ 4, 5, 11, 12 }, { M, S, S, S }, { 1, 2, 3, 1 }, 2, { 8, 7 });     // R  long lists: tiles inside one query
        Q.add({ 5, 4, 11, 12 }, { M, M, S, S }, { 1, 2, 3, 1 }, 3);               // R  two required lists, two rounds
        Q.add({ 7, 7, 7 }, { M, S, S }, { 2, 5, 1 }, 2);                          // R  required and twice optional
        Q.add({ 7, 7, 3 }, { S, S, S }, { 2, 5, 1 }, 3);                          // O  a list named twice counts twice
        Q.add({ 2, 4 }, { M, S }, { 1, 1 }, 1);                                   // R  a driver of one id that the list holds
        Q.add({ 3 }, { M }, { 1 }, 1);                                            // R  a threshold and no optional term: nothing
        Q.add({ 3 }, { M }, { 1 }, 0);                                            // R  one term
        Q.add({ 3 }, { S }, { 1 }, 2);                                            // O  one term, two entries asked for: its repeats
        Q.add({ 10, 3, 9 }, { M, S, S }, { 1, 1, 2 }, 1, { 3 });                  // R  optional and excluded
        Q.add({ 10, 3 }, { M, M }, { 1, 1 }, 0, { 3 });                           // R  required and excluded: nothing
        u64 all = 0;
        for (size_t q = 0; q < Q.size(); q++)
            for (u64 t = Q.qoff[q]; t < Q.qoff[q + 1]; t++) all += 3 * n2[Q.rid[t]];
        same_plans(n2, Q, 4 * all), same_plans(n2, Q, 0), same_plans(n2, Q, all / 4);
        for (const u32 form : { 0u, 1u, 2u }) {
            size_t of = 0, nruns = 0;
            const char* what = "a group per run";
            CHECK(check_call(what, n2, Q, 4 * all, ids, pay, form, &of, &nruns) == nruns && of == ~(size_t)0);
            CHECK(nruns == 9);  // RR O RR OO RRR O RRR O RR
            what = "a group per query";
            const size_t most = check_call(what, n2, Q, 0, ids, pay, form, &of);
            CHECK(most == Q.size() && of == ~(size_t)0);
            what = "several groups";
            const size_t some = check_call(what, n2, Q, all / 4, ids, pay, form, &of);
            CHECK(some >= nruns && some < most && of == ~(size_t)0);
        }
        // thresholds from 0 to terms + 1 on every query
        for (u32 m = 0; m <= 5; m++) {
            Queries T = Q;
            for (size_t q = 0; q < T.size(); q++) T.msm[q] = std::min<u32>(m, (u32)(T.qoff[q + 1] - T.qoff[q]) + 1);
            size_t of = 0;
            const char* what = "threshold sweep";
            check_call(what, n2, T, 4 * all, ids, pay, m % 3, &of);
            CHECK(of == ~(size_t)0);
            check_call(what, n2, T, 0, ids, pay, (m + 1) % 3, &of);
        }
        // random roles over the same lists
        for (int round = 0; round < 60; round++) {
            Queries T;
            const size_t nq = 1 + rng() % 12;
            for (size_t q = 0; q < nq; q++) {
                const size_t m = 1 + rng() % 5;
                std::vector<u32> t(m), wt(m), xx(rng() % 3);
                std::vector<u8> o(m);
                for (size_t k = 0; k < m; k++) t[k] = (u32)(rng() % 13), wt[k] = (u32)(rng() % 4), o[k] = (u8)(rng() % 3 == 0);
                for (u32& e : xx) e = (u32)(rng() % 13);
                T.add(t, o, wt, (u32)(rng() % (m + 2)), xx);
            }
            size_t of = 0;
            const char* what = "random roles";
            check_call(what, n2, T, round % 3 == 0 ? 0 : round % 3 == 1 ? 4 * all : 9000, ids, pay, (u32)round % 3, &of);
            CHECK(of == ~(size_t)0);
        }
    }
    {
        Queries Q;
        Q.add({ 13, 14 }, { M, S }, { 4, 2 }, 0);                 // 2^32 - 2: a result
        Q.add({ 13, 13 }, { M, S }, { 4, 4 }, 1, { 16 });         // a sum that saturates, of an excluded id: no error
        Q.add({ 13, 13, 15 }, { M, S, S }, { 4, 4, 1 }, 2);       // ... of an id that fails the threshold: no error
        Q.add({ 13, 13, 15 }, { S, S, S }, { 4, 4, 1 }, 3);       // ... the same without a required term
        Q.add({ 13, 13, 15 }, { M, S, M }, { 4, 4, 1 }, 0);       // ... of an id a required list lacks: no error
        Q.add({ 13, 14 }, { M, S }, { 4, 3 }, 1);                 // 2^32 - 1: the error
        Q.add({ 3 }, { M }, { 1 }, 0);
        Q.add({ 17, 17 }, { S, S }, { 2, 2 }, 2);                 // a later query overflows as well, of the other kind
        Q.add({ 13, 14 }, { M, S }, { 4, 3 }, 0, { 14 });         // ... excluded
        for (const u32 form : { 0u, 1u, 2u })
            for (const u64 budget : { (u64)1 << 20, (u64)0, (u64)40 }) {
                size_t of = 0;
                const char* what = "overflow";
                check_call(what, n2, Q, budget, ids, pay, form, &of);
                CHECK(of == 5);
            }
    }
}

// 5. the limits: the first failing query in batch order, whatever its kind -- planned run by run as the call plans
static void limit_cases()
{
    const char* what = "limits";
    const std::vector<u64> n = { 10, (u64)1 << 32, 20, ((u64)1 << 32) - 5 };
    auto first_bad = [&](const Queries& Q, size_t* where) {  // (the function the library calls)
        QueryPlan QP;
        return query_plan(n.data(), n.size(), Q.rid.data(), Q.occ.data(), Q.qoff.data(), Q.msm.data(), nullptr, nullptr, Q.size(), 1000,
            UTILE, &QP, where);
    };
    const u8 M = 1, S = 0;
    size_t where = 99;
    {
        Queries Q;  // the shortest REQUIRED list decides: a long optional list is no limit, a long required one beside a short one neither
        Q.add({ 0, 2 }, { M, S }, { 1, 1 }, 0);
        Q.add({ 2, 0 }, { S, S }, { 1, 1 }, 0);
        Q.add({ 0, 1 }, { M, M }, { 1, 1 }, 0);
        CHECK(first_bad(Q, &where) == ANSX_OK);
    }
    {
        Queries Q;  // R, O, R(bad), O(bad): the third
        Q.add({ 0 }, { M }, { 1 }, 0);
        Q.add({ 2 }, { S }, { 1 }, 0);
        Q.add({ 1, 0 }, { M, S }, { 1, 1 }, 0);
        Q.add({ 3, 0 }, { S, S }, { 1, 1 }, 0);
        CHECK(first_bad(Q, &where) == ANSX_ERR_ARG && where == 2);
    }
    {
        Queries Q;  // R, O(bad: its lists together reach 2^32), R(bad): the second
        Q.add({ 0 }, { M }, { 1 }, 0);
        Q.add({ 3, 0 }, { S, S }, { 1, 1 }, 0);
        Q.add({ 1 }, { M }, { 1 }, 0);
        CHECK(first_bad(Q, &where) == ANSX_ERR_ARG && where == 1);
    }
    {
        Queries Q;  // O, R, R(bad), R(bad): the second query of the second run, and a null bad_query is left alone
        Q.add({ 2 }, { S }, { 1 }, 0);
        Q.add({ 0 }, { M }, { 1 }, 0);
        Q.add({ 1 }, { M }, { 1 }, 0);
        Q.add({ 1, 2 }, { M, S }, { 1, 1 }, 0);
        where = 99;
        CHECK(first_bad(Q, &where) == ANSX_ERR_ARG && where == 2);
        CHECK(first_bad(Q, nullptr) == ANSX_ERR_ARG);
    }
    {
        Queries Q;  // nothing fails: *bad_query is not written
        Q.add({ 2 }, { S }, { 1 }, 0);
        Q.add({ 0 }, { M }, { 1 }, 0);
        where = 99;
        CHECK(first_bad(Q, &where) == ANSX_OK && where == 99);
    }
}

int main()
{
    cases();
    limit_cases();
    printf("ok: %ld checks\n", checks);
    return 0;
}
