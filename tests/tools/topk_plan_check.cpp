// The host side of ansx_topk_batch_dev on the CPU (ans_large_alphabet_amd/csrc/ansx_plan.h, unb_plan with want_terms;
// ansx_plan_types.h, the arithmetic of the selection), over synthetic headers: lists of given lengths whose ids and
// payloads are made up here.
//   1. The terms behind the pairs.  With want_terms the plan is the plan without -- groups, pairs, rounds, tiles bit for
//      bit -- plus pterm: two entries per pair; a side of a first-round pair with ints names a term of ITS query whose
//      list is the one the side reads (same place in the buffer, same length); every other side names none; every named
//      term of a non-empty list stands behind exactly one side.  Then each group is RUN the way the kernels run it:
//      values sat32(weight of the side's term * payload) beside the keys, a stable merge per pair and round (ties: A
//      first), heads and 64-bit sums per run of equal ids, the select below, the sort -- and every query's ranked ids
//      and scores are compared with the sums per id computed directly from the terms as named.
//   2. The select.  An emulation of k_topk_hist / k_topk_pick / k_topk_gather built from topk_digit, topk_candidate,
//      topk_pick and topk_with_digit -- 256 bins, eight rounds -- against std::sort: random and adversarial keys, all
//      scores equal, all keys in one bin of every round but the last, k = 1, n - 1, n, n + 1 and 1024.
// Built with -fsanitize=address,undefined and run by tests/test_topk_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

using namespace ansx_plan;

static const u32 TILE = 4096;
static long checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        checks++;                                                                    \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: %s -- %s\n", __FILE__, __LINE__, #cond, what);   \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

// ---------------------------------------------------------------------------------------------------- the select
// -> the keys >= the want-th largest, want = min(k, n), in any order: what k_topk_gather leaves in a query's slot
static std::vector<u64> select_emulated(const char* what, const std::vector<u64>& keys, u32 k)
{
    std::vector<u64> out;
    if (keys.empty()) return out;
    u32 want = (u32)std::min<size_t>(k, keys.size());
    const u32 want0 = want;
    u64 prefix = 0;
    for (u32 r = 0; r < ANSX_TOPK_ROUNDS; r++) {
        u32 hist[ANSX_TOPK_BINS] = { 0 };
        for (const u64 x : keys)
            if (topk_candidate(x, prefix, r)) hist[topk_digit(x, r)]++;
        u32 above = 0;
        const u32 d = topk_pick(hist, ANSX_TOPK_BINS, want, &above);
        CHECK(above < want && hist[d] >= want - above);
        prefix = topk_with_digit(prefix, r, d);
        want -= above;
        // the kernel's form of the same pick: four bins a lane, the lane whose bins hold the want-th
        u32 incl = 0;
        bool found = false;
        for (u32 lane = 64; lane-- > 0;) {
            const u32 own = hist[4 * lane] + hist[4 * lane + 1] + hist[4 * lane + 2] + hist[4 * lane + 3], ab = incl;
            incl += own;
            if (ab < want + above && want + above <= incl) {
                u32 a = 0;
                const u32 dl = topk_pick(hist + 4 * lane, 4, want + above - ab, &a);
                CHECK(!found && 4 * lane + dl == d && ab + a == above);
                found = true;
            }
        }
        CHECK(found);
    }
    CHECK(want == 1);  // distinct keys: the last digit's bin holds the one key that is the prefix
    for (const u64 x : keys)
        if (x >= prefix) out.push_back(x);
    CHECK(out.size() == want0);
    return out;
}

static void check_select(const char* what, std::vector<u64> keys, u32 k)
{
    std::vector<u64> got = select_emulated(what, keys, k);
    std::sort(got.begin(), got.end(), std::greater<u64>());
    std::sort(keys.begin(), keys.end(), std::greater<u64>());
    keys.resize(std::min<size_t>(k, keys.size()));
    CHECK(got == keys);
}

static void select_cases()
{
    std::mt19937_64 rng(5);
    const char* what = "pack";
    CHECK(topk_key(5, 7) > topk_key(5, 8) && topk_key(6, 8) > topk_key(5, 7) && topk_key(0, 0xFFFFFFFFu) == 0);
    CHECK(topk_key_id(topk_key(9, 0xFFFFFFFEu)) == 0xFFFFFFFEu && topk_key_score(topk_key(0xFFFFFFFEu, 3)) == 0xFFFFFFFEu);
    CHECK(topk_sat32(0xFFFFFFFFu, 1) == 0xFFFFFFFFu && topk_sat32(65536, 65536) == 0xFFFFFFFFu && topk_sat32(65535, 65537) == 0xFFFFFFFFu);
    CHECK(topk_sat32(0xFFFFFFFEu, 1) == 0xFFFFFFFEu && topk_sat32(0, 0xFFFFFFFFu) == 0 && topk_sat32(3, 5) == 15);
    CHECK(topk_digit(0xAB00000000000000ull, 0) == 0xAB && topk_digit(0xCDull, 7) == 0xCD);
    for (const size_t n : { (size_t)1, (size_t)2, (size_t)5, (size_t)255, (size_t)256, (size_t)257, (size_t)1023, (size_t)1024,
             (size_t)1025, (size_t)5000 }) {
        std::vector<std::pair<const char*, std::vector<u64>>> sets;
        std::vector<u64> v(n);
        for (size_t i = 0; i < n; i++) v[i] = topk_key((u32)(rng() % 1000), (u32)i * 3u);  // many ties in the score
        sets.push_back({ "random scores, ties", v });
        for (size_t i = 0; i < n; i++) v[i] = topk_key(77, (u32)(rng() >> 40) * 4096u + (u32)i);  // all scores equal
        sets.push_back({ "all scores equal", v });
        for (size_t i = 0; i < n; i++) v[i] = topk_key(0x12345678u, 0x9ABCDE00u ^ (u32)(i & 255u) ^ ((u32)(i >> 8) << 8));
        if (n <= 256) sets.push_back({ "one bin in every round but the last", v });
        for (size_t i = 0; i < n; i++) v[i] = 0xFFFFFFFFFFFFFFFFull - i;  // the top of the key space
        sets.push_back({ "top of the key space", v });
        for (size_t i = 0; i < n; i++) v[i] = i;  // ... and its bottom, key 0 included
        sets.push_back({ "bottom of the key space", v });
        for (size_t i = 0; i < n; i++) v[i] = topk_key((u32)(i % 7) << 24, (u32)(i % 2 ? 0x80000000u : 0u) + (u32)i);  // high byte, top bit of the id
        sets.push_back({ "scores in the high byte, ids across the top bit", v });
        for (auto& s : sets)
            for (const size_t k : { (size_t)1, (size_t)2, n > 1 ? n - 1 : 1, n, n + 1, (size_t)64, (size_t)1000, (size_t)1024 })
                check_select(s.first, s.second, (u32)k);
    }
}

// ---------------------------------------------------------------------------------------------------- the plan
struct Queries {
    std::vector<u32> rid, w;
    std::vector<u64> qoff{ 0 };
    void add(const std::vector<u32>& t, std::mt19937_64& rng)
    {
        rid.insert(rid.end(), t.begin(), t.end());
        for (size_t i = 0; i < t.size(); i++) w.push_back((u32)(rng() % 5));  // (weight 0 among them)
        qoff.push_back(rid.size());
    }
    size_t size() const { return qoff.size() - 1; }
};

struct KV {
    u32 key, val;
};

static size_t check_plan(const char* what, const std::vector<u64>& n, const Queries& Q, u64 budget, u32 k,
    const std::vector<std::vector<u32>>& ids, const std::vector<std::vector<u32>>& pay)
{
    std::vector<UnbGroup> G0, G;
    size_t bad = ~(size_t)0;
    CHECK(unb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, TILE, &G0, &bad) == ANSX_OK);
    CHECK(unb_plan(n.data(), n.size(), Q.rid.data(), Q.qoff.data(), Q.size(), budget, TILE, &G, &bad, nullptr, nullptr, true) == ANSX_OK);
    CHECK(bad == ~(size_t)0 && G.size() == G0.size());
    for (size_t gi = 0; gi < G.size(); gi++) {
        const UnbGroup &g = G[gi], &g0 = G0[gi];
        // nothing else differs
        CHECK(g0.pterm.empty() && g.q0 == g0.q0 && g.q1 == g0.q1 && g.lists == g0.lists && g.at == g0.at && g.seg == g0.seg);
        CHECK(g.roff == g0.roff && g.tiles == g0.tiles && g.ints == g0.ints && g.rounds == g0.rounds && g.pairs.size() == g0.pairs.size());
        CHECK(g.pairs.empty() || memcmp(g.pairs.data(), g0.pairs.data(), sizeof(ansx_unb_pair) * g.pairs.size()) == 0);
        CHECK(g.pterm.size() == 2 * g.pairs.size());
        std::map<u32, u64> at_of;  // list -> its place in the buffer
        for (size_t i = 0; i < g.lists.size(); i++) at_of[g.lists[i]] = g.at[i];
        const size_t nq = g.q1 - g.q0;
        std::vector<u32> seen(Q.rid.size(), 0);
        for (size_t i = 0; i < g.pairs.size(); i++) {
            const ansx_unb_pair& p = g.pairs[i];
            // its query: the one whose span holds dst
            size_t j = 0;
            while (j + 1 < nq && g.seg[j + 1] <= p.dst) j++;
            for (u32 side = 0; side < 2; side++) {
                const u32 t = g.pterm[2 * i + side], len = side ? p.nb : p.na;
                const u64 from = side ? p.b : p.a;
                if (!p.from_lists || len == 0) {
                    CHECK(t == ANSX_TOPK_NONE);
                    continue;
                }
                CHECK(t != ANSX_TOPK_NONE && t >= Q.qoff[g.q0 + j] && t < Q.qoff[g.q0 + j + 1]);
                CHECK(n[Q.rid[t]] == len && at_of.count(Q.rid[t]) && at_of[Q.rid[t]] == from);
                seen[t]++;
            }
        }
        for (u64 t = Q.qoff[g.q0]; t < Q.qoff[g.q1]; t++) CHECK(seen[t] == (n[Q.rid[t]] ? 1u : 0u));

        // run it: the buffers of ids and payloads, the rounds with values, heads, scores, select, sort
        const u64 L = g.at.back(), M = g.seg[nq];
        std::vector<u32> lists(L), vlists(L);
        for (size_t i = 0; i < g.lists.size(); i++) {
            std::copy(ids[g.lists[i]].begin(), ids[g.lists[i]].end(), lists.begin() + g.at[i]);
            std::copy(pay[g.lists[i]].begin(), pay[g.lists[i]].end(), vlists.begin() + g.at[i]);
        }
        std::vector<KV> buf[2] = { std::vector<KV>(M), std::vector<KV>(M) };
        for (u32 r = 0; r < g.rounds; r++)
            for (u32 i = g.roff[r]; i < g.roff[r + 1]; i++) {
                const ansx_unb_pair& p = g.pairs[i];
                std::vector<KV> A(p.na), B(p.nb);
                for (u32 side = 0; side < 2; side++) {
                    std::vector<KV>& S = side ? B : A;
                    const u64 from = side ? p.b : p.a;
                    for (size_t x = 0; x < S.size(); x++) {
                        CHECK(from + x < (p.from_lists ? L : M));
                        if (p.from_lists) S[x] = { lists[from + x], topk_sat32(Q.w[g.pterm[2 * i + side]], vlists[from + x]) };
                        else S[x] = buf[1 - (r & 1u)][from + x];
                    }
                }
                CHECK((u64)p.dst + p.na + p.nb <= M);
                std::merge(A.begin(), A.end(), B.begin(), B.end(), buf[r & 1u].begin() + p.dst,
                    [](const KV& x, const KV& y) { return x.key < y.key; });  // (stable: A first among equals)
            }
        const std::vector<KV>& fin = buf[(g.rounds - 1u) & 1u];
        for (size_t j = 0; j < nq; j++) {
            std::vector<u64> keys;
            for (u32 x = g.seg[j]; x < g.seg[j + 1];) {
                u32 y = x;
                u64 sum = 0;
                for (; y < g.seg[j + 1] && fin[y].key == fin[x].key; y++) sum += fin[y].val;
                CHECK(sum < 0xFFFFFFFFull);
                keys.push_back(topk_key((u32)sum, fin[x].key));
                x = y;
            }
            std::vector<u64> got = select_emulated(what, keys, k);
            std::sort(got.begin(), got.end(), std::greater<u64>());
            // directly: the sums per id over the terms as named
            std::map<u32, u64> score;
            for (u64 t = Q.qoff[g.q0 + j]; t < Q.qoff[g.q0 + j + 1]; t++)
                for (size_t x = 0; x < ids[Q.rid[t]].size(); x++) score[ids[Q.rid[t]][x]] += (u64)Q.w[t] * pay[Q.rid[t]][x];
            std::vector<std::pair<u64, u32>> ranked;  // (score, id)
            for (const auto& e : score) ranked.push_back({ e.second, e.first });
            std::sort(ranked.begin(), ranked.end(), [](const std::pair<u64, u32>& x, const std::pair<u64, u32>& y) {
                return x.first != y.first ? x.first > y.first : x.second < y.second;
            });
            ranked.resize(std::min<size_t>(k, ranked.size()));
            CHECK(got.size() == ranked.size());
            for (size_t x = 0; x < got.size(); x++)
                CHECK(topk_key_id(got[x]) == ranked[x].second && topk_key_score(got[x]) == ranked[x].first);
        }
    }
    return G.size();
}

static void plan_cases()
{
    std::mt19937_64 rng(9);
    // lists 0..11 of these lengths (two empty ones), ascending ids with repeats, payloads 0..3
    const std::vector<u64> n = { 5, 0, 1, 100, 4096, 4097, 0, 333, 1000, 64, 2, 8193 };
    std::vector<std::vector<u32>> ids(n.size()), pay(n.size());
    for (size_t i = 0; i < n.size(); i++) {
        u32 at = 0;
        for (u64 x = 0; x < n[i]; x++) ids[i].push_back(at += (u32)(rng() % 4)), pay[i].push_back((u32)(rng() % 4));
    }
    ids[2][0] = 0xFFFFFFFFu, ids[10] = { 0xFFFFFFFEu, 0xFFFFFFFFu };
    Queries Q;
    Q.add({ 3 }, rng);                              // 1 term
    Q.add({ 0, 7 }, rng);                           // 2
    Q.add({ 4, 1, 5 }, rng);                        // 3, an empty list among them
    Q.add({ 8, 9, 0, 3, 7 }, rng);                  // 5
    Q.add({ 0, 2, 3, 4, 5, 7, 8, 9, 10 }, rng);     // 9
    Q.add({ 7, 7 }, rng);                           // a list named twice
    Q.add({ 3, 6, 3, 1, 3 }, rng);                  // ... three times, between empty ones
    Q.add({ 1 }, rng);                              // nothing but an empty list
    Q.add({ 6, 1 }, rng);
    Q.add({ 11, 2, 10 }, rng);                      // the top of the id space
    Q.add({ 1, 9 }, rng);                           // an empty FIRST side
    u64 all = 0;
    for (size_t q = 0; q < Q.size(); q++)
        for (u64 t = Q.qoff[q]; t < Q.qoff[q + 1]; t++) all += 3 * n[Q.rid[t]];
    for (const u32 k : { 1u, 10u, 1024u }) {
        const char* what = "one group";
        CHECK(check_plan(what, n, Q, all, k, ids, pay) == 1);
        what = "a group per query";  // (but a query of empty lists, which costs nothing, joins the one in front)
        const size_t most = check_plan(what, n, Q, 0, k, ids, pay);
        CHECK(most >= Q.size() - 3 && most < Q.size());
        what = "several groups";
        const size_t some = check_plan(what, n, Q, all / 4, k, ids, pay);
        CHECK(some > 1 && some < most);
    }
}

int main()
{
    select_cases();
    plan_cases();
    printf("ok: %ld checks\n", checks);
    return 0;
}
