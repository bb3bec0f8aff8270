// The arithmetic of the query kernels' frame on the CPU (ans_large_alphabet_amd/csrc/ansx_query_tile.h: isb_query_of,
// qt_last_le, bx_lower, bx_upper, qt_clamp, qt_limit, qt_elem, qt_tile_last, qt_tile_queries, qt_tile_queries_by -- the
// code the kernels inline), built with the host compiler alone.  Every array lives in a heap block of exactly its length.
//   1. isb_query_of against a linear scan: every seg of Q = 1 .. 6 queries over totals 0 .. 12 (empty queries at the
//      front, in the middle, at the end); every i below the total; an empty query is never returned; every enclosing
//      pair (the queries of an a <= i and a b >= i, what a tile hands it) gives what the whole [0, Q - 1] gives.  The
//      accessor form qt_last_le over the 64-bit bounds of an array of ansx_isb_query (k_isectb_gather's key) gives
//      the same.
//   2. bx_lower / bx_upper against std::lower_bound / std::upper_bound: every ascending list of 0 .. 9 ints over four
//      values (runs of equal ids), every sub-range [lo, hi), every t from below the first value to above the last;
//      once over the heap block, once through an accessor that refuses a read at mid outside [lo, hi).
//   3. qt_clamp / qt_limit: the device total below, at and above n, and absent.
//   4. A whole tile emulated as the kernels run it: n in {1, 63, 64, 65, 1023, 1024, 1025, 2049}; one query, two
//      queries with the bound on, one before and one after every tile edge and every 64-element edge, three with an
//      empty one there, and all those bounds at once; the device total absent, 0, n / 2, n - 1, n, n + 1.  Per tile
//      below the limit the prologue's qb by both forms, per element qt_elem and its query inside [qb[0], qb[1]]; the
//      elements of a tile are those of its sixteen 64-element words, each once, and none at or beyond the grid's end.
// Built with -fsanitize=address,undefined and run by tests/test_query_tile_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_query_tile.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static long checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        checks++;                                                        \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                     \
        }                                                                \
    } while (0)

// a heap block of exactly v.size() entries
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v)
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// every ascending seg[0 .. Q] from 0 to total
template <class F> static void every_seg(u32 Q, u32 total, F f)
{
    std::vector<u32> seg(Q + 1, 0);
    seg[Q] = total;
    std::vector<u32> cut(Q > 0 ? Q - 1 : 0, 0);  // seg[1 .. Q - 1]
    for (;;) {
        for (u32 j = 1; j < Q; j++) seg[j] = cut[j - 1];
        f(seg);
        int j = (int)cut.size() - 1;
        while (j >= 0 && cut[j] == total) j--;
        if (j < 0) return;
        const u32 v = cut[j] + 1;
        for (size_t k = j; k < cut.size(); k++) cut[k] = v;
    }
}

// the query of element i by a linear scan: the one whose span holds it
static u32 query_scan(const std::vector<u32>& seg, u32 i)
{
    for (u32 j = 0; j + 1 < seg.size(); j++)
        if (seg[j] <= i && i < seg[j + 1]) return j;
    CHECK(false);  // (an element below the total lies in a query)
    return 0;
}

static void check_query_of()
{
    for (u32 Q = 1; Q <= 6; Q++)
        for (u32 total = 0; total <= 12; total++)
            every_seg(Q, total, [&](const std::vector<u32>& sv) {
                const auto seg = exact(sv);
                std::vector<u32> ref(total);
                for (u32 i = 0; i < total; i++) {
                    ref[i] = query_scan(sv, i);
                    CHECK(sv[ref[i]] < sv[ref[i] + 1]);  // never an empty one
                    CHECK(isb_query_of(seg.get(), 0, Q - 1, i) == ref[i]);
                }
                std::vector<ansx_isb_query> gv(Q + 1);
                for (u32 j = 0; j <= Q; j++) gv[j] = { 0, sv[j] };
                const auto G = exact(gv);
                const ansx_isb_query* g = G.get();
                const auto dst = [g](u32 j) { return g[j].dst; };
                for (u32 a = 0; a < total; a++)
                    for (u32 b = a; b < total; b++)
                        for (u32 i = a; i <= b; i++) {
                            CHECK(isb_query_of(seg.get(), ref[a], ref[b], i) == ref[i]);
                            CHECK(qt_last_le(dst, ref[a], ref[b], (u64)i) == ref[i]);
                        }
            });
}

struct Window {  // list[mid] for lo <= mid < hi only
    const u32* list;
    u64 lo, hi;
    u32 operator[](u64 mid) const
    {
        CHECK(lo <= mid && mid < hi);
        return list[mid];
    }
};

static void check_bounds()
{
    for (u32 len = 0; len <= 9; len++) {
        std::vector<u32> lv(len, 1);  // values 1, 3, 5, 7, ascending
        for (;;) {
            const auto list = exact(lv);
            for (u64 lo = 0; lo <= len; lo++)
                for (u64 hi = lo; hi <= len; hi++)
                    for (u32 t = 0; t <= 8; t++) {
                        const u64 el = std::lower_bound(lv.begin() + lo, lv.begin() + hi, t) - lv.begin();
                        const u64 eu = std::upper_bound(lv.begin() + lo, lv.begin() + hi, t) - lv.begin();
                        CHECK(bx_lower((const u32*)list.get(), lo, hi, t) == el);
                        CHECK(bx_upper((const u32*)list.get(), lo, hi, t) == eu);
                        CHECK(bx_lower(Window{ list.get(), lo, hi }, lo, hi, t) == el);
                        CHECK(bx_upper(Window{ list.get(), lo, hi }, lo, hi, t) == eu);
                    }
            int j = (int)len - 1;
            while (j >= 0 && lv[j] == 7) j--;
            if (j < 0) break;
            const u32 v = lv[j] + 2;
            for (u32 k = j; k < len; k++) lv[k] = v;
        }
    }
}

static void check_limit()
{
    for (u32 n = 0; n <= 5; n++) {
        CHECK(qt_limit(nullptr, n) == n);
        for (u64 total = 0; total <= 7; total++) {
            CHECK(qt_clamp(total, n) == std::min<u64>(total, n));
            CHECK(qt_limit(&total, n) == std::min<u64>(total, n));
        }
        const u64 big = (1ull << 32) + n;  // (a count that does not fit 32 bits)
        CHECK(qt_clamp(big, n) == n && qt_limit(&big, n) == n);
    }
}

static void tile_case(const std::vector<u32>& sv, u32 n, const u64* total)
{
    const u32 Q = (u32)sv.size() - 1, nc = (u32)qt_limit(total, n);
    CHECK(nc <= n && (!total || nc <= *total));
    const u32 ntiles = (n + ANSX_ISECT_TILE - 1u) / ANSX_ISECT_TILE;  // (the grid covers n)
    const auto seg = exact(sv);
    std::vector<ansx_isb_query> gv(Q + 1);
    for (u32 j = 0; j <= Q; j++) gv[j] = { 0, sv[j] };
    const auto G = exact(gv);
    const ansx_isb_query* g = G.get();
    const auto dst = [g](u32 j) { return g[j].dst; };
    std::vector<u32> ref(nc);
    for (u32 j = 0, i = 0; i < nc; i++) {
        while (sv[j + 1] <= i) j++;
        ref[i] = j;
    }
    std::vector<u32> seen((size_t)ntiles * ANSX_ISECT_TILE, 0);
    for (u32 tile = 0; tile < ntiles; tile++) {
        const u64 i0 = (u64)tile * ANSX_ISECT_TILE;
        u32 qb[2] = { 0, 0 }, qg[2] = { 0, 0 };
        if (i0 < nc) {  // (a tile at or beyond the limit leaves before its prologue)
            CHECK(qt_tile_last(i0, nc) == std::min<u64>(i0 + ANSX_ISECT_TILE, nc) - 1);
            qt_tile_queries(seg.get(), Q, i0, nc, qb);  // qt_prologue's thread 0
            qt_tile_queries_by(dst, Q, i0, nc, qg);     // qt_prologue_by's
            CHECK(qb[0] == ref[i0] && qb[1] == ref[qt_tile_last(i0, nc)] && qg[0] == qb[0] && qg[1] == qb[1]);
        }
        for (u32 k = 0; k < ANSX_ISECT_CPT; k++)
            for (u32 tid = 0; tid < ANSX_ISECT_NT; tid++) {
                const u64 i = qt_elem(i0, k, tid);
                CHECK(i >= i0 && i < i0 + ANSX_ISECT_TILE);
                // (its ballot word and bit, as the kernels hand them to isect_ballot)
                CHECK((i - i0) / 64u == k * (ANSX_ISECT_NT / 64u) + (tid >> 6) && i % 64u == (tid & 63u));
                seen[i]++;
                if (i < nc) {
                    CHECK(isb_query_of(seg.get(), qb[0], qb[1], (u32)i) == ref[i]);
                    CHECK(qt_last_le(dst, qg[0], qg[1], i) == ref[i]);
                }
            }
    }
    for (u32 c : seen) CHECK(c == 1);
}

static void check_tiles()
{
    const u32 ns[] = { 1, 63, 64, 65, 1023, 1024, 1025, 2049 };
    for (u32 n : ns) {
        std::vector<u32> bounds;  // on, one before and one after every 64-element edge (the tile edges are among them)
        for (u32 e = 0; e <= n + 64u; e += 64u)
            for (int d = -1; d <= 1; d++) {
                const i64 b = (i64)e + d;
                if (b >= 0 && b <= (i64)n && (bounds.empty() || bounds.back() < (u32)b)) bounds.push_back((u32)b);
            }
        std::vector<std::vector<u32>> segs;
        segs.push_back({ 0, n });
        for (u32 b : bounds) segs.push_back({ 0, b, n }), segs.push_back({ 0, b, b, n });
        std::vector<u32> all = { 0 };
        all.insert(all.end(), bounds.begin(), bounds.end());
        all.push_back(n);
        segs.push_back(all);
        const u64 totals[] = { 0, n / 2u, n - 1u, n, (u64)n + 1u };
        for (const auto& sv : segs) {
            tile_case(sv, n, nullptr);
            for (u64 t : totals) tile_case(sv, n, &t);
        }
    }
}

int main()
{
    check_query_of();
    check_bounds();
    check_limit();
    check_tiles();
    printf("ok: %ld checks\n", checks);
    return 0;
}
