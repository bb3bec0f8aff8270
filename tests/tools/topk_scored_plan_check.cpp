// The host side of ansx_topk_scored_batch_dev's impact step on the CPU (ans_large_alphabet_amd/csrc/ansx_plan.h:
// impact_plan; ansx_plan_types.h: impact_tiles, impact_list_of, impact_tile_start, impact_mask, impact_bad_id,
// impact_word -- the arithmetic k_topk_impacts runs), over made-up buffers of ids and payloads.
//   1. impact_plan: an entry per list that has ints and a payload, in the buffer's order, with its place in the group
//      and the tiles in front of it; lists of no ints and lists without a payload get none; the tile limit.
//   2. The kernel RUN over the plan the way k_topk_impacts runs it, for tiles of 1024, 2048 and 4096 postings, in both
//      forms (a stage of S rows, S below, at and above tf_rows) and with a grid of one workgroup, a few, or one per tile:
//      per tile the list by the binary search, per lane and round the uint4's mask, whole uint4 or single ints, the bound
//      check before the norm is read, the clamped row, the flag's minimum.  Every read of an id or a payload and every
//      write goes through a checked accessor: inside the list of the tile, a posting written at most once, a whole
//      uint4 only at a multiple of four ints; the norms are a function that refuses an id of ndocs or more; the stage is
//      a vector of exactly S rows.
//   3. The judge: a brute-force rewrite of the buffer, list by list -- the payloads of lists without one, and of the
//      postings with an id of ndocs or more, must come out untouched, every other payload as its impact, and the flag
//      word as the smallest place of a list with such an id (or what the scan left, if that is smaller).
// Cases: lists of 0, 1, 3, 4, 5, 1023, 1024 and 1025 ints (and 4097, 9000) at every alignment modulo 4; lists without
// a payload between lists with one; the groups of isb_plan and unb_plan over queries that share lists, where a list
// several queries name is rewritten once and a list that is only excluded not at all; payloads of 0, tf_rows - 1,
// tf_rows and 2^30 - 1; tf_rows of 1, 2, 64 and 256; ids at ndocs - 1 and at ndocs in the first and in a later list;
// ndocs = 2^32 with the id 0xFFFFFFFF; the tile limit.
// Built with -fsanitize=address,undefined and run by tests/test_topk_scored_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace ansx_plan;

static const u32 NT = 256;           // ANSX_IMPACT_NT
static const u32 NONE = 0xFFFFFFFFu;  // ANSX_SS_NONE
static long checks = 0;
static const char* what = "";
#define CHECK(cond)                                                                  \
    do {                                                                             \
        checks++;                                                                    \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: %s -- %s\n", __FILE__, __LINE__, #cond, what);   \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

static u32 norm_fn(u32 id) { return (u32)(((u64)id * 2654435761ull) >> 13) & 255u; }

struct Scorer {
    u64 ndocs;
    u32 rows;
    std::vector<u32> table;  // rows * 256
    u32 norm(u32 id) const
    {
        CHECK((u64)id < ndocs);  // (the kernel compares before it reads)
        return norm_fn(id);
    }
};

static Scorer make_scorer(u64 ndocs, u32 rows, u32 seed)
{
    Scorer s = { ndocs, rows, std::vector<u32>((size_t)rows * 256) };
    std::mt19937 rng(seed);
    for (u32& w : s.table) w = rng();
    return s;
}

struct Group {  // a group's buffers as group_decode leaves them: list k at [at[k], at[k + 1])
    std::vector<u32> lists;   // the referenced list of every slot
    std::vector<u64> at;
    std::vector<u32> payof;   // per referenced list
    std::vector<u32> ids, pay;
    void add(u32 n, bool has_pay)
    {
        if (at.empty()) at.push_back(0);
        lists.push_back((u32)payof.size());
        payof.push_back(has_pay ? 1u : ANSX_TOPK_NONE);
        at.push_back(at.back() + n);
        ids.resize((size_t)at.back()), pay.resize((size_t)at.back());
    }
};

// the definition, list by list -> the expected payloads and flag word
static void brute(const Group& g, const Scorer& sc, u32 flag0, std::vector<u32>* pay, u32* flag)
{
    *pay = g.pay, *flag = flag0;
    for (size_t k = 0; k < g.lists.size(); k++) {
        if (g.payof[g.lists[k]] == ANSX_TOPK_NONE) continue;
        for (u64 i = g.at[k]; i < g.at[k + 1]; i++) {
            if ((u64)g.ids[i] >= sc.ndocs) {
                *flag = std::min(*flag, (u32)k);
                continue;
            }
            const u32 row = std::min(g.pay[i], sc.rows - 1);
            (*pay)[i] = sc.table[(size_t)row * 256 + norm_fn(g.ids[i])];
        }
    }
}

// k_topk_impacts over the plan: `wgs` workgroups walk the tiles with a grid stride; staged: srows rows in LDS
static void run_kernel(const Group& g, const Scorer& sc, const std::vector<ansx_impact_list>& P, u64 tiles, u32 rounds, u32 wgs, bool staged,
    u32 srows, std::vector<u32>* pay, u32* flag)
{
    const u32 TILE = rounds * NT * 4, np = (u32)P.size(), ntiles = (u32)tiles;
    std::vector<u32> stage(sc.table.begin(), sc.table.begin() + (staged ? (size_t)srows * 256 : 0));
    const u32 swords = (u32)stage.size();
    std::vector<u8> written(pay->size(), 0);
    for (u32 b = 0; b < wgs; b++)
        for (u32 t = b; t < ntiles; t += wgs) {
            const u32 e = impact_list_of(P.data(), np, t);
            CHECK(e < np && P[e].tile <= t && (e + 1 == np || P[e + 1].tile > t));
            const ansx_impact_list L = P[e];
            const u64 s0 = impact_tile_start(L, t, TILE), end = L.at + L.n;
            CHECK(s0 % 4 == 0 && s0 < end && s0 + TILE > L.at);  // (every tile of the host's table holds an int of its list)
            auto rd = [&](const std::vector<u32>& v, u64 i) {
                CHECK(i >= L.at && i < end && i < v.size());
                return v[(size_t)i];
            };
            auto wr = [&](u64 i, u32 v) {
                CHECK(i >= L.at && i < end && !written[(size_t)i]);
                written[(size_t)i] = 1, (*pay)[(size_t)i] = v;
            };
            for (u32 tid = 0; tid < NT; tid++) {
                bool bad = false;
                for (u32 r = 0; r < rounds; r++) {
                    const u64 i = s0 + (u64)(r * NT + tid) * 4;
                    u32 m = i < end ? impact_mask(L, i) : 0u;
                    if (m == 15u) CHECK(i % 4 == 0 && i >= L.at && i + 4 <= end);  // the whole uint4, loaded and stored
                    u32 v[4] = { 0, 0, 0, 0 };
                    for (u32 j = 0; j < 4; j++) {
                        if (!((m >> j) & 1u)) continue;
                        const u32 id = rd(g.ids, i + j), tf = rd(g.pay, i + j);
                        if (impact_bad_id(id, sc.ndocs)) {
                            bad = true, m &= ~(1u << j);
                            continue;
                        }
                        const u32 w = impact_word(tf, sc.norm(id), sc.rows);
                        CHECK(w < sc.rows * 256u);
                        v[j] = staged && w < swords ? stage[w] : sc.table[w];
                    }
                    for (u32 j = 0; j < 4; j++)
                        if ((m >> j) & 1u) wr(i + j, v[j]);
                }
                if (bad && L.pos < *flag) *flag = std::min(*flag, L.pos);
            }
        }
    // every posting of a planned list was looked at once: written, or an id the norms have no entry for
    for (const ansx_impact_list& L : P)
        for (u64 i = L.at; i < L.at + L.n; i++) CHECK(written[(size_t)i] || (u64)g.ids[(size_t)i] >= sc.ndocs);
}

static void check_plan(const Group& g, u32 tile, const std::vector<ansx_impact_list>& P, u64 tiles)
{
    size_t e = 0;
    u64 t = 0;
    for (size_t k = 0; k < g.lists.size(); k++) {
        const u64 n = g.at[k + 1] - g.at[k];
        if (n == 0 || g.payof[g.lists[k]] == ANSX_TOPK_NONE) continue;
        CHECK(e < P.size() && P[e].at == g.at[k] && P[e].n == n && P[e].pos == k && P[e].tile == t);
        t += ((g.at[k] & 3) + n + tile - 1) / tile;
        e++;
    }
    CHECK(e == P.size() && t == tiles);
}

// the group under every tile, form, stage and grid, against the judge
static void check_group(Group& g, const Scorer& sc, u32 flag0 = NONE)
{
    if (g.at.empty()) g.at.push_back(0);
    std::vector<u32> want;
    u32 want_flag;
    brute(g, sc, flag0, &want, &want_flag);
    for (const u32 rounds : { 1u, 2u, 4u }) {
        std::vector<ansx_impact_list> P;
        u64 tiles = 0;
        CHECK(impact_plan(g.lists, g.at, &g.payof, rounds * NT * 4, &P, &tiles) == ANSX_OK);
        check_plan(g, rounds * NT * 4, P, tiles);
        if (P.empty()) continue;  // (the host launches nothing)
        const u32 stages[] = { 0, 1, sc.rows > 1 ? sc.rows - 1 : 1, sc.rows };
        for (const u32 srows : stages)
            for (const u32 wgs : { 1u, 3u, (u32)tiles }) {
                std::vector<u32> pay = g.pay;
                u32 flag = flag0;
                run_kernel(g, sc, P, tiles, rounds, std::min<u32>(wgs, (u32)tiles), srows != 0, std::min(srows, sc.rows), &pay, &flag);
                CHECK(pay == want);
                CHECK(flag == want_flag);
            }
    }
    std::vector<ansx_impact_list> P;  // without payloads at all: no entry
    u64 tiles = 7;
    CHECK(impact_plan(g.lists, g.at, nullptr, 1024, &P, &tiles) == ANSX_OK && P.empty() && tiles == 0);
}

static void fill(Group& g, const Scorer& sc, std::mt19937& rng)
{
    const u32 edge[] = { 0u, sc.rows - 1, sc.rows, (1u << 30) - 1, 1u, 2u, 63u, 64u, 255u, 256u };
    const u64 top = std::min<u64>(sc.ndocs, (u64)1 << 32);
    for (size_t i = 0; i < g.ids.size(); i++) {
        g.ids[i] = (u32)(rng() % top);  // (ids of a list ascend in a real group; the kernel does not depend on it)
        g.pay[i] = rng() % 3 ? edge[rng() % 10] : rng() % (2 * sc.rows + 2);
    }
}

int main()
{
    std::mt19937 rng(20240);
    const u32 lens[] = { 0, 1, 3, 4, 5, 1023, 1024, 1025, 4097, 9000 };
    // ---- every length at every alignment: a list without a payload of `a` ints in front, one of 2 behind, then a short one
    what = "lengths and alignments";
    for (const u32 rows : { 1u, 2u, 64u, 256u }) {
        const Scorer sc = make_scorer(1u << 20, rows, rows);
        for (const u32 n : lens)
            for (u32 a = 0; a < 4; a++) {
                if (rows != 64 && n > 1025) continue;
                Group g;
                g.add(a, false), g.add(n, true), g.add(2, false), g.add(7, true), g.add(0, true), g.add(n ? n - 1 : 3, true);
                fill(g, sc, rng);
                check_group(g, sc);
            }
    }
    // ---- ids at ndocs - 1 and at ndocs, in the first and in a later list; the scan's own flag
    what = "the bound";
    {
        const Scorer sc = make_scorer(1000, 64, 5);
        for (u32 where = 0; where < 8; where++) {
            Group g;
            g.add(3, false), g.add(2000, true), g.add(5, false), g.add(1030, true), g.add(6, true);
            fill(g, sc, rng);
            // (the list without a payload holds ids far above ndocs: never looked up)
            g.ids[0] = 0xFFFFFFFFu, g.ids[2004] = 5000;
            const u64 l1 = g.at[1], l3 = g.at[3], l4 = g.at[4];
            g.ids[l1] = 999, g.ids[l1 + 1999] = 999, g.ids[l3 + 1029] = 999;  // ndocs - 1: fine
            if (where & 1u) g.ids[l1 + 1024] = 1000;                           // the first list with a payload
            if (where & 2u) g.ids[l3] = 1000, g.ids[l3 + 1029] = 0xFFFFFFFFu;  // a later one
            if (where & 4u) g.ids[l4 + 5] = 1000;
            for (const u32 flag0 : { NONE, 0u, 2u, 4u }) check_group(g, sc, flag0);
            std::vector<u32> want;
            u32 flag;
            brute(g, sc, NONE, &want, &flag);
            CHECK(flag == ((where & 1u) ? 1u : (where & 2u) ? 3u : (where & 4u) ? 4u : NONE));
        }
    }
    // ---- ndocs = 2^32 admits 0xFFFFFFFF
    what = "ndocs = 2^32";
    {
        const Scorer sc = make_scorer((u64)1 << 32, 16, 9);
        Group g;
        g.add(1, false), g.add(1500, true);
        fill(g, sc, rng);
        g.ids[1] = 0xFFFFFFFFu, g.ids[1500] = 0xFFFFFFFFu, g.ids[700] = 0xFFFFFFFEu;
        check_group(g, sc);
        std::vector<u32> want;
        u32 flag;
        brute(g, sc, NONE, &want, &flag);
        CHECK(flag == NONE && want[1] == sc.table[(size_t)std::min(g.pay[1], 15u) * 256 + norm_fn(0xFFFFFFFFu)]);
        CHECK(!impact_bad_id(0xFFFFFFFFu, (u64)1 << 32) && impact_bad_id(0xFFFFFFFFu, 0xFFFFFFFFull) && !impact_bad_id(0, 1) && impact_bad_id(1, 1));
    }
    // ---- the groups of the real planners: lists several queries name, a list that is only excluded
    what = "isb_plan / unb_plan groups";
    {
        const std::vector<u64> n = { 1500, 3, 0, 1024, 2049, 5, 777 };  // list 2 is empty, list 5 only ever excluded
        const std::vector<u32> rid = { 0, 1, 3, 0, 4, 0, 3, 3, 6, 2, 4 };  // queries (0 1 3) (0 4) (0 3 3) (6 2 4)
        const std::vector<u64> qoff = { 0, 3, 5, 8, 11 };
        const std::vector<u32> xrid = { 5, 5, 1 };
        const std::vector<u64> xqoff = { 0, 1, 1, 2, 3 };
        std::vector<u32> payof(n.size(), 1u);
        payof[5] = ANSX_TOPK_NONE;
        const Scorer sc = make_scorer(1u << 20, 64, 77);
        for (const u64 budget : { (u64)1 << 28, (u64)1 }) {
            std::vector<IsbGroup> ig;
            std::vector<UnbGroup> ug;
            size_t bad = 0;
            CHECK(isb_plan(n.data(), n.size(), rid.data(), qoff.data(), 4, budget, &ig, &bad, xrid.data(), xqoff.data(), true) == ANSX_OK);
            CHECK(unb_plan(n.data(), n.size(), rid.data(), qoff.data(), 4, budget, 4096, &ug, &bad, xrid.data(), xqoff.data(), true) == ANSX_OK);
            CHECK(ig.size() == (budget == 1 ? 4u : 1u) && ug.size() == ig.size());
            auto one = [&](const std::vector<u32>& lists, const std::vector<u64>& at) {
                Group g;
                g.lists = lists, g.at = at, g.payof = payof;
                g.ids.resize((size_t)at.back()), g.pay.resize((size_t)at.back());
                fill(g, sc, rng);
                for (size_t k = 0; k < lists.size(); k++)
                    if (lists[k] == 5) g.ids[(size_t)at[k]] = 0xFFFFFFFFu;  // (above ndocs, and no error)
                std::vector<ansx_impact_list> P;
                u64 tiles;
                CHECK(impact_plan(lists, at, &payof, 2048, &P, &tiles) == ANSX_OK);
                size_t with = 0;
                for (const u32 l : lists) with += l != 5 && n[l] > 0;
                CHECK(P.size() == with);  // a list several queries name has ONE entry
                check_group(g, sc);
            };
            for (const IsbGroup& g : ig) one(g.lists, g.at);
            for (const UnbGroup& g : ug) one(g.lists, g.at);
        }
    }
    // ---- the tile limit: 2^31 - 1 tiles pass, one more does not, wherever it is crossed
    what = "the tile limit";
    {
        std::vector<ansx_impact_list> P;
        u64 tiles = 0;
        const std::vector<u32> payof = { 1, 1, 1 };
        const u64 most = 0x7FFFFFFFull * 1024;
        CHECK(impact_plan({ 0 }, { 0, most }, &payof, 1024, &P, &tiles) == ANSX_OK && tiles == 0x7FFFFFFFull && P.size() == 1);
        CHECK(impact_plan({ 0 }, { 0, most + 1 }, &payof, 1024, &P, &tiles) == ANSX_ERR_ARG);
        CHECK(impact_plan({ 0, 1 }, { 0, 1, most + 1 }, &payof, 1024, &P, &tiles) == ANSX_ERR_ARG);  // (the second list starts at int 1: a tile more)
        CHECK(impact_plan({ 0, 1 }, { 0, 4, most - 1020 }, &payof, 1024, &P, &tiles) == ANSX_OK && tiles == 0x7FFFFFFFull && P[1].tile == 1);
        CHECK(impact_plan({ 0, 1, 2 }, { 0, (u64)1 << 42, (u64)1 << 43, ((u64)1 << 43) + 5 }, &payof, 1024, &P, &tiles) == ANSX_ERR_ARG);
        CHECK(impact_plan({ 0 }, { 0, most * 4 }, &payof, 4096, &P, &tiles) == ANSX_OK && tiles == 0x7FFFFFFFull);
        CHECK(impact_tiles(3, 1, 1024) == 1 && impact_tiles(3, 1022, 1024) == 2 && impact_tiles(0, 1024, 1024) == 1 && impact_tiles(1, 1024, 1024) == 2);
    }
    printf("ok: %ld checks\n", checks);
    return 0;
}
