// The host's plan of ansx_bool_batch_dev (ans_large_alphabet_amd/csrc/ansx_plan.h: isb_plan and unb_plan with excluded
// lists, plan_excl_tables) on the CPU, over synthetic headers: lists of given lengths whose ids are made up here.
// Checked for both ops: every query in exactly one group, in order; the budget with a list counted once however it is
// named, as a term, as an excluded list or as both; that xt / xt_off have the shape the kernel walks -- Q + 1 ascending
// offsets, every query's excluded lists in order, {at, n} inside the buffer that was laid out, an empty list as n = 0;
// the 2^32 limits, which an excluded list of any length does not meet.  Then every group is RUN: the positive result
// of each query is computed directly (ALL: the driver's ids that are in every other term; ANY: the distinct ids), laid
// out in segments as the positive phase leaves them, and a CPU model of k_bool_exclude -- tiles of 1024 candidates, the
// staged range, the bounded range in the buffer, the whole-list search of a tile that spans queries -- runs on the
// plan's tables under each form and two stage sizes; what it keeps is compared with the set difference.
// Built with -fsanitize=address,undefined and run by tests/test_bool_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

using namespace ansx_plan;

static const u32 TILE = 1024, UTILE = 4096;
static long checks = 0, paths[3] = { 0, 0, 0 };  // lists met staged, in a bounded range, by a whole-list search
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
    void add(const std::vector<u32>& t)
    {
        rid.insert(rid.end(), t.begin(), t.end());
        qoff.push_back(rid.size());
    }
    size_t size() const { return qoff.size() - 1; }
    const u32* at(size_t q) const { return rid.data() + qoff[q]; }
    size_t len(size_t q) const { return (size_t)(qoff[q + 1] - qoff[q]); }
};

// isb_query_of
static u32 query_of(const std::vector<u32>& seg, u32 lo, u32 hi, u32 i)
{
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (seg[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

static u64 lower(const u32* list, u64 lo, u64 hi, u32 t)
{
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (list[mid] >= t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

static u64 upper(const u32* list, u64 lo, u64 hi, u32 t)
{
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (list[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// k_bool_exclude over cand / seg with the tables xt_off / xt into ws -> the kept, per query.  form: 0 default, 1 search,
// 2 staged; stage: ANSX_BOOL_STAGE.  Every read of ws is bounds-checked against the list it belongs to.
static std::vector<std::vector<u32>> model_exclude(const char* what, const std::vector<u32>& ws, const std::vector<u32>& cand,
    const std::vector<u32>& seg, const std::vector<u32>& xt_off, const std::vector<ansx_isb_list>& xt, u32 form, u32 stage)
{
    const u32 Q = (u32)seg.size() - 1, nc = (u32)cand.size();
    std::vector<std::vector<u32>> kept(Q);
    std::vector<u32> st(stage);
    for (u64 i0 = 0; i0 < nc; i0 += TILE) {
        const u64 last = std::min<u64>(i0 + TILE, nc) - 1;
        const u32 q0 = query_of(seg, 0, Q - 1, (u32)i0), q1 = query_of(seg, q0, Q - 1, (u32)last);
        std::vector<char> keep(last - i0 + 1, 1);
        if (q0 == q1) {
            const u32 tf = cand[i0], tl = cand[last];
            for (u32 e = xt_off[q0]; e < xt_off[q0 + 1]; e++) {
                const ansx_isb_list L = xt[e];
                CHECK(L.at + L.n <= ws.size());
                const u32* list = ws.data() + L.at;
                const u64 lo = lower(list, 0, L.n, tf);
                u64 hi = upper(list, 0, L.n, tl);
                hi = hi < lo ? lo : hi;
                CHECK(lo <= hi && hi <= L.n);
                if (lo == hi) continue;
                const u64 len = hi - lo;
                if (form != 1 && len <= stage) {
                    paths[0]++;
                    for (u64 j = 0; j < len; j++) st[j] = list[lo + j];
                    for (u64 i = i0; i <= last; i++) {
                        if (!keep[i - i0]) continue;
                        const u64 p = lower(st.data(), 0, len, cand[i]);
                        if (p < len && st[p] == cand[i]) keep[i - i0] = 0;
                    }
                } else {
                    paths[1]++;
                    for (u64 i = i0; i <= last; i++) {
                        if (!keep[i - i0]) continue;
                        const u64 p = lower(list, lo, hi, cand[i]);
                        CHECK(p >= lo && p <= hi);
                        if (p < hi && list[p] == cand[i]) keep[i - i0] = 0;
                    }
                }
            }
        } else {
            for (u64 i = i0; i <= last; i++) {
                const u32 q = query_of(seg, q0, q1, (u32)i);
                for (u32 e = xt_off[q]; e < xt_off[q + 1]; e++) {
                    const ansx_isb_list L = xt[e];
                    CHECK(L.at + L.n <= ws.size());
                    paths[2]++;
                    const u64 p = lower(ws.data() + L.at, 0, L.n, cand[i]);
                    if (p < L.n && ws[L.at + p] == cand[i]) {
                        keep[i - i0] = 0;
                        break;
                    }
                }
            }
        }
        for (u64 i = i0; i <= last; i++)
            if (keep[i - i0]) kept[query_of(seg, q0, q1, (u32)i)].push_back(cand[i]);
    }
    return kept;
}

// The statements of the plan for one op (all: isb_plan, else unb_plan); -> the number of groups.  ids: every list's ids
// (null: the lengths only, nothing is run).
static size_t check_plan(const char* what, bool all, const std::vector<u64>& n, const Queries& T, const Queries& X, u64 budget,
    const std::vector<std::vector<u32>>* ids)
{
    CHECK(T.size() == X.size());
    std::vector<IsbGroup> GI;
    std::vector<UnbGroup> GU;
    size_t bad = ~(size_t)0;
    if (all) CHECK(isb_plan(n.data(), n.size(), T.rid.data(), T.qoff.data(), T.size(), budget, &GI, &bad, X.rid.data(), X.qoff.data()) == ANSX_OK);
    else CHECK(unb_plan(n.data(), n.size(), T.rid.data(), T.qoff.data(), T.size(), budget, UTILE, &GU, &bad, X.rid.data(), X.qoff.data()) == ANSX_OK);
    CHECK(bad == ~(size_t)0);
    const size_t ng = all ? GI.size() : GU.size();
    // what a query takes twice: its driver's ints (ALL), the ints of its lists as named (ANY)
    auto twice = [&](size_t q) {
        u64 a = all ? ~0ull : 0;
        for (size_t k = 0; k < T.len(q); k++) a = all ? std::min(a, n[T.at(q)[k]]) : a + n[T.at(q)[k]];
        return a;
    };
    size_t next = 0;
    for (size_t gi = 0; gi < ng; gi++) {
        const size_t q0 = all ? GI[gi].q0 : GU[gi].q0, q1 = all ? GI[gi].q1 : GU[gi].q1;
        const std::vector<u32>& lists = all ? GI[gi].lists : GU[gi].lists;
        const std::vector<u64>& at = all ? GI[gi].at : GU[gi].at;
        const std::vector<u32>& xt_off = all ? GI[gi].xt_off : GU[gi].xt_off;
        const std::vector<ansx_isb_list>& xt = all ? GI[gi].xt : GU[gi].xt;
        const std::vector<u32>& xt_list = all ? GI[gi].xt_list : GU[gi].xt_list;
        const u64 ints = all ? GI[gi].ints : GU[gi].ints;
        CHECK(q0 == next && q1 > q0 && q1 <= T.size());  // every query once, in order
        next = q1;
        const size_t nq = q1 - q0;
        // its lists: the non-empty ones a term or an exclusion names, ascending, back to back, each ONCE
        std::set<u32> named;
        for (u64 j = T.qoff[q0]; j < T.qoff[q1]; j++) named.insert(T.rid[j]);
        for (u64 j = X.qoff[q0]; j < X.qoff[q1]; j++) named.insert(X.rid[j]);
        u64 buf = 0, dbl = 0;
        std::vector<u32> want;
        for (const u32 r : named) {
            buf += n[r];
            if (n[r]) want.push_back(r);
        }
        CHECK(lists == want && at.size() == want.size() + 1);
        u64 a = 0;
        for (size_t k = 0; k < want.size(); k++) {
            CHECK(at[k] == a);
            a += n[want[k]];
        }
        CHECK(at.back() == buf && a == buf);
        for (size_t q = q0; q < q1; q++) dbl += twice(q);
        CHECK(ints == buf + 2 * dbl);  // (a list that is term and excluded: once)
        CHECK(nq == 1 || ints <= budget);
        if (gi + 1 < ng) {  // it ended because the next query did not fit
            u64 add = 0;
            std::set<u32> seen;
            for (size_t k = 0; k < T.len(q1); k++)
                if (!named.count(T.at(q1)[k]) && seen.insert(T.at(q1)[k]).second) add += n[T.at(q1)[k]];
            for (size_t k = 0; k < X.len(q1); k++)
                if (!named.count(X.at(q1)[k]) && seen.insert(X.at(q1)[k]).second) add += n[X.at(q1)[k]];
            CHECK(ints + add + 2 * twice(q1) > budget || dbl + twice(q1) > 0xFFFFFFFFull);
        }
        auto place = [&](u32 r) { return at[(size_t)(std::lower_bound(want.begin(), want.end(), r) - want.begin())]; };
        // the second table
        CHECK(xt_off.size() == nq + 1 && xt_off[0] == 0 && xt_off[nq] == xt.size() && xt_list.size() == xt.size());
        CHECK(xt.size() == X.qoff[q1] - X.qoff[q0]);
        for (size_t j = 0; j < nq; j++) {
            CHECK(xt_off[j + 1] - xt_off[j] == X.len(q0 + j));
            for (size_t k = 0; k < X.len(q0 + j); k++) {
                const u32 r = X.at(q0 + j)[k];
                const ansx_isb_list L = xt[xt_off[j] + k];
                CHECK(xt_list[xt_off[j] + k] == r && L.n == n[r]);
                CHECK(L.n == 0 ? L.at == 0 : L.at == place(r));  // (an empty list: kept, n = 0)
                CHECK(L.at + L.n <= buf);
            }
        }
        if (!ids) continue;

        // run it: the positive phase directly, then the model of the kernel on the plan's tables
        std::vector<u32> ws;
        for (const u32 r : want) ws.insert(ws.end(), (*ids)[r].begin(), (*ids)[r].end());
        CHECK(ws.size() == buf);
        std::vector<u32> cand, seg;
        std::vector<std::vector<u32>> expect(nq);
        for (size_t j = 0; j < nq; j++) {
            const u32* t = T.at(q0 + j);
            const size_t m = T.len(q0 + j);
            std::vector<u32> P;
            if (all) {
                size_t d = 0;  // the driver: fewest ints, the earliest of equal ones
                for (size_t k = 1; k < m; k++)
                    if (n[t[k]] < n[t[d]]) d = k;
                CHECK(GI[gi].drv[j] == t[d]);
                for (const u32 v : (*ids)[t[d]]) {
                    bool in = true;
                    for (size_t k = 0; k < m && in; k++) in = k == d || std::binary_search((*ids)[t[k]].begin(), (*ids)[t[k]].end(), v);
                    if (in) P.push_back(v);
                }
            } else {
                std::set<u32> u;
                for (size_t k = 0; k < m; k++) u.insert((*ids)[t[k]].begin(), (*ids)[t[k]].end());
                P.assign(u.begin(), u.end());
            }
            std::set<u32> ex;
            for (size_t k = 0; k < X.len(q0 + j); k++) ex.insert((*ids)[X.at(q0 + j)[k]].begin(), (*ids)[X.at(q0 + j)[k]].end());
            seg.push_back((u32)cand.size());
            cand.insert(cand.end(), P.begin(), P.end());
            for (const u32 v : P)
                if (!ex.count(v)) expect[j].push_back(v);
        }
        seg.push_back((u32)cand.size());
        if (cand.empty()) continue;
        for (const u32 stage : { 64u, 4096u })
            for (u32 form = 0; form < 3; form++) CHECK(model_exclude(what, ws, cand, seg, xt_off, xt, form, stage) == expect);
    }
    CHECK(next == T.size());
    return ng;
}

int main()
{
    const char* what = "lists";
    std::mt19937_64 rng(8765);
    // 40 lists over a small universe: lengths around the tile and the stage, one empty (23), one with a repeated id (8),
    // one that ends in 0xFFFFFFFF (19); 24..39 of a few ids each
    const u32 sizes[24] = { 1, 2, 63, 64, 65, 100, 100, 333, 500, 500, 777, 1000, 1023, 1024, 1025, 1500, 2000, 2049, 2500, 3000,
        3500, 4000, 5000, 0 };
    std::vector<std::vector<u32>> ids(40);
    std::vector<u64> n(40);
    for (u32 r = 0; r < 40; r++) {
        const u32 size = r < 24 ? sizes[r] : 3 + r % 7;
        std::set<u32> s;
        while (s.size() < size) s.insert((u32)(rng() % 9000));
        ids[r].assign(s.begin(), s.end());
        if (r == 8) ids[r][10] = ids[r][9];
        if (r == 19) ids[r].back() = 0xFFFFFFFFu;
        n[r] = ids[r].size();
        CHECK(n[r] == size);
    }

    what = "shapes";
    Queries S, E;
    auto q = [&](std::vector<u32> t, std::vector<u32> x) { S.add(t), E.add(x); };
    q({ 22 }, { 21 });                  // whole tiles inside one query, a range that is staged
    q({ 22, 21 }, {});                  // excludes nothing
    q({ 22 }, { 22 });                  // term and excluded: nothing is left
    q({ 20, 21 }, { 20 });
    q({ 19 }, { 19, 18 });              // 0xFFFFFFFF excluded
    q({ 19, 18 }, { 17 });              // ... and kept
    q({ 8 }, { 9 });                    // a repeated id
    q({ 9 }, { 8, 8 });                 // ... in the excluded list, which is named twice
    q({ 22 }, { 23 });                  // an empty excluded list
    q({ 23 }, { 22 });                  // an empty positive side
    q({ 22 }, { 0, 1, 2, 3, 23, 20 });  // many lists, an empty one among them
    q({ 24 }, { 25 });                  // small queries: tiles that span them
    q({ 26, 27 }, { 28, 29 });
    q({ 30 }, {});
    q({ 31 }, { 31 });
    q({ 32, 33, 34 }, { 35 });
    q({ 21, 22 }, { 36, 19 });
    CHECK(check_plan(what, true, n, S, E, ANSX_ISECT_BATCH_INTS_DEFAULT, &ids) == 1);
    CHECK(check_plan(what, false, n, S, E, ANSX_ISECT_BATCH_INTS_DEFAULT, &ids) == 1);
    CHECK(check_plan(what, true, n, S, E, 0, &ids) == S.size());  // a group per query
    CHECK(check_plan(what, false, n, S, E, 0, &ids) == S.size());

    what = "random";
    Queries R, RX;
    for (u32 k = 0; k < 80; k++) {
        std::vector<u32> t(1 + rng() % 4), x(rng() % 4);
        for (u32& r : t) r = (u32)(rng() % 40);
        for (u32& r : x) r = (u32)(rng() % 40);
        R.add(t), RX.add(x);
    }
    for (const bool all : { true, false }) {
        const size_t one = check_plan(what, all, n, R, RX, ANSX_ISECT_BATCH_INTS_DEFAULT, &ids);
        CHECK(one == 1);
        const size_t some = check_plan(what, all, n, R, RX, 40000, &ids);  // (a list several groups name counts in each)
        CHECK(some > 2 && some < R.size());
        CHECK(check_plan(what, all, n, R, RX, 1, &ids) == R.size());
    }

    what = "counted once";
    {  // lists 21 (4000) and 22 (5000): term and excluded in one query, then excluded again by the next
        Queries T, X;
        T.add({ 21, 22 }), X.add({ 22, 21 });
        T.add({ 0 }), X.add({ 22 });
        const u64 both = 4000 + 5000 + 2 * 4000 + 1 + 2 * 1;  // ALL: the drivers twice
        CHECK(check_plan(what, true, n, T, X, both, &ids) == 1);
        CHECK(check_plan(what, true, n, T, X, both - 1, &ids) == 2);
        const u64 any = 4000 + 5000 + 2 * 9000 + 1 + 2 * 1;   // ANY: the terms as named twice
        CHECK(check_plan(what, false, n, T, X, any, &ids) == 1);
        CHECK(check_plan(what, false, n, T, X, any - 1, &ids) == 2);
    }

    what = "2^32 ints";
    const std::vector<u64> big = { 1ull << 31, (1ull << 31) - 1, 0xFFFFFFFFull, 1ull << 32, 5, 1ull << 40 };
    {
        Queries T, X;
        T.add({ 0 }), X.add({ 5 });     // an excluded list of 2^40 ints: any length
        T.add({ 4, 3 }), X.add({ 3 });  // ALL: the driver is the short one
        T.add({ 2 }), X.add({ 3, 5 });
        CHECK(check_plan(what, true, big, T, X, ~0ull, nullptr) >= 1);
        std::vector<IsbGroup> G;
        size_t bad = 99;
        T.add({ 3, 3 }), X.add({});     // a driver of 2^32 ints
        CHECK(isb_plan(big.data(), big.size(), T.rid.data(), T.qoff.data(), T.size(), ~0ull, &G, &bad, X.rid.data(), X.qoff.data()) == ANSX_ERR_ARG);
        CHECK(bad == 3);
    }
    {
        Queries T, X;
        T.add({ 0 }), X.add({ 5 });
        T.add({ 1 }), X.add({ 3 });
        T.add({ 4 }), X.add({ 3, 5 });  // the merge buffer would pass 2^32: a new group
        T.add({ 0, 1 }), X.add({ 2 });  // a query of 2^32 - 1 ints
        CHECK(check_plan(what, false, big, T, X, ~0ull, nullptr) == 3);
        std::vector<UnbGroup> G;
        size_t bad = 99;
        T.add({ 0, 1, 4 }), X.add({});  // together 2^32 + 4
        CHECK(unb_plan(big.data(), big.size(), T.rid.data(), T.qoff.data(), T.size(), ~0ull, UTILE, &G, &bad, X.rid.data(), X.qoff.data()) == ANSX_ERR_ARG);
        CHECK(bad == 4);
    }

    what = "without exclusions";
    {  // the parents' calls: no second table
        std::vector<IsbGroup> GI;
        std::vector<UnbGroup> GU;
        size_t bad = 99;
        CHECK(isb_plan(n.data(), n.size(), S.rid.data(), S.qoff.data(), S.size(), 0, &GI, &bad) == ANSX_OK);
        CHECK(unb_plan(n.data(), n.size(), S.rid.data(), S.qoff.data(), S.size(), 0, UTILE, &GU, &bad) == ANSX_OK);
        for (const IsbGroup& g : GI) CHECK(g.xt_off.empty() && g.xt.empty());
        for (const UnbGroup& g : GU) CHECK(g.xt_off.empty() && g.xt.empty());
    }
    CHECK(paths[0] > 0 && paths[1] > 0 && paths[2] > 0);  // every search path of the kernel ran
    printf("ok: %ld checks; lists met staged %ld, in a bounded range %ld, whole %ld\n", checks, paths[0], paths[1], paths[2]);
    return 0;
}
