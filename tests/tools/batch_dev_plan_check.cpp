// The device plan of ansx_decode_batch_device_ranges_dev on the CPU.  The arithmetic its kernels run per item lives in
// ans_large_alphabet_amd/csrc/ansx_plan_types.h (bdr_span, bdr_ref_of, bdr_block_ints, bdr_pass_of, bdr_pass_first,
// bdr_lower_bound, bdr_src_bound, bdr_piece, bdr_rup4); here it is driven in plain loops, step for step as
// ansx_batchdevranges.h drives it -- spans of global blocks, a stable sort by first block, the union by running
// maximum, tb, every group's first entry, the pass scalars summed entry by entry and range by range, a pass's tables
// and pieces -- over seeded random batches of many tiny containers in several geometries, lengths that are no multiple
// of 4 or of the block size, and passes of 1, 3, 7 and 16384 blocks.  Per pass the resulting B, O, work-list ints,
// payload bound and the multiset of (src, dst, count) pieces are compared with what the host-array call plans for the
// same ranges (ansx_plan.h: br_runs, br_pieces, Pass::take_runs).
// Built with -fsanitize=address,undefined and run by tests/test_batch_device_ranges_plan_cpu.py; exit status 0 and "ok".
#include "../../ans_large_alphabet_amd/csrc/ansx_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <tuple>

using namespace ansx_plan;

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

typedef std::tuple<u64, u64, u64> Piece;  // src, dst, count

static void run_case(u64 seed, u32 nref, u32 ngeo, u32 max_blocks, size_t nranges, u32 PB)
{
    std::mt19937_64 rng(seed);
    auto below = [&](u64 m) { return (u64)(rng() % m); };
    static const u32 BIS[] = { 4, 16, 32, 64, 8 };  // (a block size is a multiple of 4)
    // the referenced containers in batch order
    std::vector<BatchSrc> rs(nref);
    std::vector<u32> geo(nref);
    for (u32 j = 0; j < nref; j++) {
        geo[j] = (u32)below(ngeo);
        const u32 bi = BIS[geo[j]];
        const u64 n = below(4) == 0 ? 1 + below(bi) : 1 + below((u64)max_blocks * bi);
        rs[j] = {};
        rs[j].H.n = n, rs[j].H.block_ints = bi, rs[j].H.ckpt_interval = 1;
        rs[j].nblocks = (u32)((n + bi - 1) / bi);
        rs[j].H.payload_bytes = 1 + below(3 * n + 8);  // (some below, some above blocks x bbound)
        rs[j].base = 4096 * (u64)(j + 1);
    }
    // ranges: points, short and long ones, empty ones, whole containers; unsorted, repeated
    std::vector<u32> rid(nranges), cnt(nranges);
    std::vector<u64> first(nranges), off(nranges + 1);
    u64 total = 0;
    for (size_t i = 0; i < nranges; i++) {
        const u32 j = (u32)below(nref);
        const u64 n = rs[j].H.n, f = below(n + 1);
        u64 c = 0;
        switch (below(6)) {
        case 0: c = 0; break;
        case 1: c = n - f; break;
        case 2: c = std::min<u64>(n - f, 1); break;
        default: c = below(std::min<u64>(n - f, 3 * rs[j].H.block_ints) + 1);
        }
        if (i > 0 && below(10) == 0) rid[i] = rid[i - 1], first[i] = first[i - 1], cnt[i] = cnt[i - 1];
        else rid[i] = j, first[i] = f, cnt[i] = (u32)c;
        off[i] = total, total += cnt[i];
    }
    off[nranges] = total;

    // ---- the host-array call's plan, per geometry group
    std::map<Geometry, std::vector<u32>> members, ids;
    for (u32 j = 0; j < nref; j++) members[br_geometry(rs[j].H)].push_back(j);
    for (size_t i = 0; i < nranges; i++)
        if (cnt[i]) ids[br_geometry(rs[rid[i]].H)].push_back((u32)i);

    // ---- the device plan: the host's part
    BdrTables Tb;
    CHECK(bdr_tables(rs, PB, [](const ansx_container_header& H0) { return (u64)(2 * H0.block_ints + 3); }, &Tb));
    const std::vector<u32>& rmap = Tb.rmap;
    const std::vector<ansx_bdr_ref>& R = Tb.R;
    const std::vector<ansx_bdr_group>& G = Tb.G;
    const u32 nslots = (u32)Tb.nslots;
    std::vector<u32> inv(nref);
    for (u32 j = 0; j < nref; j++) inv[rmap[j]] = j;
    CHECK(R.size() == nref && Tb.S.size() == nref && Tb.Hs.size() == G.size());
    for (u32 r = 0; r < nref; r++) {  // the order of the global blocks: by group, batch order inside; bases ascend strictly
        CHECK(Tb.S[r].base == rs[inv[r]].base && R[r].n == rs[inv[r]].H.n && G[R[r].group].bi == rs[inv[r]].H.block_ints);
        if (r) CHECK(R[r].gbase == R[r - 1].gbase + R[r - 1].nblocks && R[r].group >= R[r - 1].group);
        if (r && R[r].group == R[r - 1].group) CHECK(inv[r] > inv[r - 1]);
        if (!r || R[r].group != R[r - 1].group) CHECK(G[R[r].group].gbase == R[r].gbase);
    }
    const u32 ng = (u32)G.size();
    // ---- ... and the kernels', item by item
    std::vector<ansx_bdr_range> rg;
    std::vector<std::pair<u32, u32>> span;  // (first global block, last + 1)
    for (size_t i = 0; i < nranges; i++) {
        if (!cnt[i]) continue;
        const ansx_bdr_ref& rec = R[rmap[rid[i]]];
        u32 a, b;
        bdr_span(first[i], cnt[i], G[rec.group].bi, rec.gbase, &a, &b);
        CHECK(a >= rec.gbase && b <= rec.gbase + rec.nblocks && a < b);
        span.push_back({ a, b });
        rg.push_back({ first[i], off[i], cnt[i], rmap[rid[i]], 0, 0 });
    }
    std::stable_sort(span.begin(), span.end(), [](const std::pair<u32, u32>& x, const std::pair<u32, u32>& y) { return x.first < y.first; });
    const size_t nne = span.size();
    std::vector<u32> S(nne), offl(nne), tb;
    u32 cover = 0;
    for (size_t i = 0; i < nne; i++) {  // the union by running maximum (ansx_ranges.h, dr_union)
        S[i] = std::max(span[i].first, cover);
        offl[i] = (u32)tb.size();
        for (u32 b = S[i]; b < span[i].second; b++) tb.push_back(b);
        cover = std::max(cover, span[i].second);
    }
    const u32 T = (u32)tb.size();
    for (u32 k = 1; k < T; k++) CHECK(tb[k - 1] < tb[k]);
    for (ansx_bdr_range& g : rg) {  // k_bdr_k0
        const ansx_bdr_ref& rec = R[g.r];
        const u32 gb0 = rec.gbase + (u32)(g.first / G[rec.group].bi);
        size_t i = 0;
        while (i + 1 < nne && S[i + 1] <= gb0) i++;
        g.k0 = offl[i] + (gb0 - S[i]);
        CHECK(g.k0 < T && tb[g.k0] == gb0);
    }
    std::vector<u64> tg(ng + 1, T);  // k_bdr_groups
    for (u32 g = 0; g < ng; g++) {
        size_t lo = 0;
        while (lo < nne && span[lo].first < G[g].gbase) lo++;
        tg[g] = lo < nne ? offl[lo] : T;
        CHECK(tg[g] == bdr_lower_bound(tb.data(), T, G[g].gbase));
    }
    std::vector<ansx_bdr_pass> ps(nslots, ansx_bdr_pass{});
    for (u32 k = 0; k < T; k++) {  // k_bdr_pass_blocks
        const u32 gb = tb[k];
        const ansx_bdr_ref rec = R[bdr_ref_of(R.data(), (u32)R.size(), gb)];
        CHECK(rec.gbase <= gb && gb < rec.gbase + rec.nblocks);
        const ansx_bdr_group grp = G[rec.group];
        const u32 t0 = (u32)tg[rec.group], t1 = (u32)tg[rec.group + 1];
        CHECK(t0 <= k && k < t1);
        const u32 p = bdr_pass_of(k, t0, PB), ka = bdr_pass_first(p, t0, PB);
        const u32 kb = (u64)ka + PB < t1 ? ka + PB : t1;
        const u32 nk = bdr_block_ints(rec.n, grp.bi, gb - rec.gbase), slot = grp.pslot + p;
        CHECK(slot < nslots && nk >= 1 && nk <= grp.bi);
        ps[slot].wl += bdr_rup4(nk);
        if (k + 1 == kb) ps[slot].last_n = nk;
        if (k == ka || tb[k - 1] < rec.gbase) {
            u32 e = bdr_lower_bound(tb.data(), T, rec.gbase + rec.nblocks);
            if (e > kb) e = kb;
            ps[slot].cap_pay += bdr_src_bound(rec.payload_bytes, e - k, grp.bbound);
        }
    }
    for (const ansx_bdr_range& g : rg) {  // k_bdr_pass_pieces
        const ansx_bdr_group grp = G[R[g.r].group];
        const u32 t0 = (u32)tg[R[g.r].group], t1 = (u32)tg[R[g.r].group + 1];
        const u32 k1 = g.k0 + ((u32)((g.first + g.count - 1) / grp.bi) - (u32)(g.first / grp.bi));
        CHECK(k1 < t1);
        u64 sum = 0;
        for (u32 p = bdr_pass_of(g.k0, t0, PB); p <= bdr_pass_of(k1, t0, PB); p++) {
            const u32 ka = bdr_pass_first(p, t0, PB), kb = (u64)ka + PB < t1 ? ka + PB : t1;
            u64 start;
            u32 k, b;
            const u32 m = bdr_piece(g, grp.bi, ka, kb, &start, &k, &b);
            CHECK(m > 0);
            ps[grp.pslot + p].np++, ps[grp.pslot + p].ints += m, sum += m;
        }
        CHECK(sum == g.count);
    }

    // ---- pass by pass against the host-array call's plan
    u32 g = 0;
    for (const auto& gr : members) {
        const Geometry geo_g = gr.first;
        const u32 bi = G[g].bi;
        const u64 bbound = G[g].bbound;
        if (!ids.count(geo_g)) {
            CHECK(tg[g] == tg[g + 1]);
            g++;
            continue;
        }
        std::vector<BrRun> runs;
        br_runs(rs, rid, first.data(), cnt.data(), ids[geo_g], bi, PB, &runs);
        std::vector<ansx_piece> PP;
        std::vector<u64> PC, pfirst;
        br_pieces(rs, rid, first.data(), cnt.data(), off, ids[geo_g], bi, runs, &PP, &PC, &pfirst);
        const u32 npass = runs.back().pass + 1;
        CHECK((tg[g + 1] - tg[g] + PB - 1) / PB == npass);
        Pass P;
        size_t kr = 0;
        for (u32 p = 0; p < npass; p++) {
            kr = P.take_runs(rs[gr.second[0]].H, rs, runs, kr, p, bi, bbound);
            const u32 ka = bdr_pass_first(p, (u32)tg[g], PB), kb = (u32)std::min<u64>((u64)ka + PB, tg[g + 1]);
            const ansx_bdr_pass& q = ps[G[g].pslot + p];
            CHECK(P.B.size() == kb - ka);
            CHECK(q.wl == P.wl);
            CHECK(q.cap_pay == P.cap_pay);
            CHECK(q.last_n == P.O.back().n);
            CHECK(q.np == pfirst[p + 1] - pfirst[p]);
            // k_bdr_pass_table
            std::vector<ansx_blk_out> O(kb - ka);
            u64 run = 0;
            for (u32 k = ka; k < kb; k++) {
                const u32 r = bdr_ref_of(R.data(), (u32)R.size(), tb[k]), b = tb[k] - R[r].gbase;
                const u32 nk = bdr_block_ints(R[r].n, bi, b);
                O[k - ka] = { run, nk, 0 };
                run += bdr_rup4(nk);
                CHECK(P.cont[P.B[k - ka].src] == inv[r] && P.B[k - ka].b == b);
                CHECK(P.O[k - ka].off == O[k - ka].off && P.O[k - ka].n == nk);
            }
            CHECK(run == P.wl);
            // k_bdr_piece_part / k_bdr_piece_put over every non-empty range, whichever its group
            std::multiset<Piece> mine, host;
            u64 ints = 0;
            for (const ansx_bdr_range& x : rg) {
                u64 start;
                u32 k, b;
                const u32 xbi = G[R[x.r].group].bi;
                const u32 m = bdr_piece(x, xbi, ka, kb, &start, &k, &b);
                if (!m) continue;
                CHECK(R[x.r].group == g && k >= ka && k < kb);
                mine.insert(Piece{ O[k - ka].off + (start - (u64)b * xbi), x.dst + (start - x.first), m });
                ints += m;
            }
            for (u64 i = pfirst[p]; i < pfirst[p + 1]; i++) host.insert(Piece{ PP[i].src, PP[i].dst, PC[i] });
            CHECK(mine == host);
            CHECK(ints == q.ints);
        }
        g++;
    }
}

int main()
{
    u64 seed = 1;
    for (const u32 PB : { 1u, 3u, 7u, 16384u }) {
        what = "many tiny containers";
        for (int rep = 0; rep < 12; rep++) run_case(seed++, 200, 3, 2, 1500, PB);
        what = "few containers of many blocks";
        for (int rep = 0; rep < 12; rep++) run_case(seed++, 9, 2, 40, 700, PB);
        what = "mixed";
        for (int rep = 0; rep < 12; rep++) run_case(seed++, 40, 5, 12, 3000, PB);
        what = "one container, one range";
        for (int rep = 0; rep < 8; rep++) run_case(seed++, 1, 1, 6, 1, PB);
        what = "sparse: most containers only hold empty ranges";
        for (int rep = 0; rep < 8; rep++) run_case(seed++, 120, 4, 3, 30, PB);
    }
    printf("ok: %ld checks\n", checks);
    return 0;
}
