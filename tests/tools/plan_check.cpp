// The host's plans of the random-access calls (ans_large_alphabet_amd/csrc/ansx_plan.h), executed on the CPU over
// identity data: int j of block b of a list is b * bi + j, of container r the pair (r, b * bi + j).  Nothing here
// restates a planner: a plan is run the way the kernels run it -- work list, pieces, chunks, the decoders' table -- and
// what comes out is compared with the slices the ranges name; beside that, the invariants the device side relies on.
// The steps and pass tables of ansx_encode_batch_dev are checked the same way: the steps partition the lists, and a pass's
// work list is walked block by block against the lists it came from.
// Built with -fsanitize=address,undefined and run by tests/test_range_plans_cpu.py; exit status 0 and "ok" on success.
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

typedef std::vector<std::pair<u64, u32>> Ranges;  // (first, count)

static void split(const Ranges& q, std::vector<u64>* first, std::vector<u32>* count)
{
    first->clear(), count->clear();
    for (const auto& r : q) first->push_back(r.first), count->push_back(r.second);
}

// ------------------------------------------------------------------------------- one container
// -> the number of stretches of consecutive touched blocks
static size_t check_single(const char* what, u64 n, u64 bi, const Ranges& q)
{
    std::vector<u64> first;
    std::vector<u32> count;
    split(q, &first, &count);
    u64 total = 0, chunks = 0;
    size_t nne = 0;
    const u64 nblocks = (n + bi - 1) / bi;
    std::vector<char> touched(nblocks, 0);
    for (const auto& r : q) {
        total += r.second, chunks += ((u64)r.second + ANSX_RANGE_CHUNK - 1) / ANSX_RANGE_CHUNK, nne += r.second != 0;
        for (u64 x = r.first; x < r.first + r.second; x += bi) touched[x / bi] = 1;
        if (r.second) touched[(r.first + r.second - 1) / bi] = 1;
    }
    RangePlan R;
    CHECK(range_plan(n, bi, first.data(), count.data(), q.size(), total, &R) == ANSX_OK);
    CHECK(R.total == total);
    if (!total) {
        CHECK(R.T == 0 && R.tb.empty() && R.pieces.empty());
        return 0;
    }
    // the touched blocks: ascending, unique, exactly the blocks some range touches
    CHECK(R.T == R.tb.size() && R.last_b == R.tb.back());
    size_t stretches = 1;
    for (size_t k = 0; k < R.tb.size(); k++) {
        CHECK(R.tb[k] < nblocks && touched[R.tb[k]]);
        if (k) CHECK(R.tb[k] > R.tb[k - 1]);
        if (k && R.tb[k] != R.tb[k - 1] + 1) stretches++;
    }
    u64 want_T = 0;
    for (const char t : touched) want_T += t;
    CHECK(R.T == want_T);
    // the gather, chunk by chunk through pstart as k_range_gather runs it; work-list int x is block tb[x / bi]'s x % bi
    CHECK(R.pieces.size() == nne && R.pstart.size() == nne + 1 && R.npieces == chunks && R.pstart.back() == chunks);
    const u64 n_sub = (R.T - 1) * bi + std::min<u64>(bi, n - R.last_b * bi);
    std::vector<u64> out(total, ~0ull);
    for (size_t p = 0; p < nne; p++) {
        const ansx_range_piece& pc = R.pieces[p];
        CHECK((u64)(R.pstart[p + 1] - R.pstart[p]) == (pc.count + ANSX_RANGE_CHUNK - 1) / ANSX_RANGE_CHUNK);
        for (u32 g = R.pstart[p]; g < R.pstart[p + 1]; g++) {
            const u64 o = (u64)(g - R.pstart[p]) * ANSX_RANGE_CHUNK, m = std::min<u64>(ANSX_RANGE_CHUNK, pc.count - o);
            for (u64 j = 0; j < m; j++) {
                const u64 x = pc.src + o + j;
                CHECK(x < n_sub && pc.dst + o + j < total && out[pc.dst + o + j] == ~0ull);
                out[pc.dst + o + j] = (u64)R.tb[x / bi] * bi + x % bi;
            }
        }
    }
    u64 at = 0;
    for (const auto& r : q)
        for (u64 j = 0; j < r.second; j++, at++) CHECK(out[at] == r.first + j);
    return stretches;
}

static void check_single_status(const char* what, u64 n, u64 bi, const Ranges& q, u64 cap, int want)
{
    std::vector<u64> first;
    std::vector<u32> count;
    split(q, &first, &count);
    RangePlan R;
    CHECK(range_plan(n, bi, first.data(), count.data(), q.size(), cap, &R) == want);
}

static Ranges random_ranges(std::mt19937_64& rng, u64 n, u64 bi)
{
    Ranges q;
    const size_t m = rng() % 9;
    for (size_t i = 0; i < m; i++) {
        const u64 f = rng() % (n + 1);
        u64 c = 0;
        switch (rng() % 4) {
        case 0: c = rng() % 3; break;
        case 1: c = rng() % (2 * bi + 1); break;
        case 2: c = rng() % (n + 1); break;
        default: c = 1; break;
        }
        q.push_back({ f, (u32)std::min<u64>(c, n - f) });
    }
    return q;
}

static void single_container(u64 bi, u64 n)
{
    const char* what = "single container";
    const u64 nblocks = (n + bi - 1) / bi;
    check_single("no ranges", n, bi, {});
    check_single("all counts zero", n, bi, { { 0, 0 }, { n, 0 }, { n / 2, 0 } });
    check_single("zero counts among others", n, bi, { { 0, 0 }, { 0, 1 }, { n, 0 }, { n - 1, 1 }, { n / 2, 0 } });
    CHECK(check_single("the whole list", n, bi, { { 0, (u32)n } }) == 1);
    check_single("the last int", n, bi, { { n - 1, 1 } });
    {
        Ranges q;
        for (u64 b = 1; b < nblocks; b++) q.push_back({ b * bi - 1, 2 });
        check_single("across every block boundary", n, bi, q);
    }
    check_single("duplicates", n, bi, { { n / 3, (u32)(n - n / 3) }, { n / 3, (u32)(n - n / 3) }, { 0, 1 }, { 0, 1 } });
    check_single("nested and overlapping", n, bi, { { 0, (u32)n }, { n / 4, (u32)(n / 2) }, { n / 2, (u32)(n - n / 2) }, { n / 3, 1 } });
    {
        Ranges q;
        for (u64 b = nblocks; b-- > 0;) q.push_back({ b * bi, 1 });
        CHECK(check_single("descending", n, bi, q) == 1);
    }
    if (nblocks >= 2) CHECK(check_single("adjacent blocks", n, bi, { { bi, 1 }, { bi - 1, 1 } }) == 1);
    if (nblocks >= 3) CHECK(check_single("a gap", n, bi, { { 2 * bi, 1 }, { bi - 1, 1 } }) == 2);

    check_single_status("first > n", n, bi, { { n + 1, 0 } }, 100, ANSX_ERR_ARG);
    check_single_status("first == n, count 1", n, bi, { { n, 1 } }, 100, ANSX_ERR_ARG);
    check_single_status("past the end by one", n, bi, { { n / 2, (u32)(n - n / 2 + 1) } }, 2 * n + 2, ANSX_ERR_ARG);
    check_single_status("first == n, count 0", n, bi, { { n, 0 } }, 0, ANSX_OK);
    check_single_status("capacity + 1", n, bi, { { 0, (u32)n }, { 0, 1 } }, n, ANSX_ERR_CAPACITY);
    check_single_status("exactly the capacity", n, bi, { { 0, (u32)n }, { 0, 1 } }, n + 1, ANSX_OK);
    check_single_status("both faults", n, bi, { { 0, (u32)n }, { 0, 1 }, { n, 1 } }, n, ANSX_ERR_ARG);

    std::mt19937_64 rng(20260000 + 31 * bi + n);
    for (int it = 0; it < 1000; it++) check_single("random", n, bi, random_ranges(rng, n, bi));
}

// ------------------------------------------------------------------------------- batches
struct Query {
    std::vector<u32> src;
    std::vector<u64> first;
    std::vector<u32> cnt;
    void add(u32 s, u64 f, u64 c) { src.push_back(s), first.push_back(f), cnt.push_back((u32)c); }
};

struct Batch {
    u64 bi;
    std::vector<BatchSrc> all;  // the batch: five containers over two geometries (the restart interval differs)
};

static Batch make_batch(u64 bi)
{
    Batch b;
    b.bi = bi;
    const u64 lens[5] = { 1, bi, bi + 1, 3 * bi + 1, 7 * bi };
    for (u32 i = 0; i < 5; i++) {
        BatchSrc s = {};
        s.H.n = lens[i], s.H.block_ints = (u32)bi, s.H.ckpt_interval = i % 2 ? 8 : 4, s.H.kind = 1;
        s.nblocks = s.H.nblocks = (u32)((lens[i] + bi - 1) / bi);
        s.H.max_nsyms = 100 + 7 * ((i * 3) % 5), s.H.max_log2_frame = 8 + (i * 2) % 5, s.H.max_present_m1 = (uint16_t)(50 - i * i);
        s.H.payload_bytes = i == 3 ? 10 : 1000 * (i + 1);  // (container 3: fewer bytes than the per-block bound allows)
        s.base = 0x1000 * (i + 1);
        s.lay = { 64, 100 + i, 200 + i, 300 + i, 400 + i };
        b.all.push_back(s);
    }
    return b;
}

// one of br_union's branches against a cover array
static void check_union(const char* what, std::vector<u64> sp, u32 nblocks)
{
    std::vector<char> cover((size_t)nblocks + 2, 0);
    for (const u64 s : sp)
        for (u32 b = (u32)(s >> 32); b <= (u32)s; b++) cover[b] = 1;
    std::vector<u32> diff;
    std::vector<std::pair<u32, u32>> out;
    br_union(sp.data(), sp.size(), nblocks, diff, out);
    std::vector<char> got((size_t)nblocks + 2, 0);
    for (size_t k = 0; k < out.size(); k++) {
        CHECK(out[k].first <= out[k].second && out[k].second < nblocks);
        if (k) CHECK(out[k].first > out[k - 1].second + 1);  // (ascending, a gap between any two)
        for (u32 b = out[k].first; b <= out[k].second; b++) got[b] = 1;
    }
    CHECK(got == cover);
}

// the referenced set, both branches (a batch barely larger than the query is marked, a far larger one sorted)
static void check_refs(const char* what, const Query& q, size_t count, std::vector<u32>* ref, std::vector<u32>* rid)
{
    std::vector<u32> ref2, rid2;
    const size_t nr = q.src.size();
    br_refs(q.src.data(), nr, count, ref, rid);
    br_refs(q.src.data(), nr, 4 * nr + 1025, &ref2, &rid2);
    const std::set<u32> names(q.src.begin(), q.src.end());
    CHECK(count <= 4 * nr + 1024 && *ref == std::vector<u32>(names.begin(), names.end()));
    CHECK(ref2 == *ref && rid2 == *rid && rid->size() == nr);
    for (size_t i = 0; i < nr; i++) CHECK((*rid)[i] < ref->size() && (*ref)[(*rid)[i]] == q.src[i]);
}

struct Wrote {  // a piece as it lands in the caller's buffer: ints [pos, pos + count) of container r at dst
    u64 dst, count, pos;
    u32 r;
    bool operator<(const Wrote& o) const { return dst < o.dst; }
};

// The ranges of a batch the way ansx_decode_batch_ranges_dev plans them: referenced set, groups by geometry, runs,
// pieces, passes.  with_pk: the search's PK beside the pieces.
static void check_batch(const char* what, const Batch& bt, const Query& q, u32 PB, bool with_pk)
{
    const u64 bi = bt.bi, bbound = 40;
    const size_t nr = q.src.size();
    std::vector<u32> ref, rid;
    check_refs(what, q, bt.all.size() + 3, &ref, &rid);  // (three more containers that no range names)
    std::vector<BatchSrc> rs;
    for (const u32 j : ref) rs.push_back(bt.all[j]);
    std::vector<u64> off(nr + 1);
    u64 total = 0;
    for (size_t i = 0; i < nr; i++) off[i] = total, total += q.cnt[i];
    off[nr] = total;
    std::vector<std::pair<Geometry, std::vector<u32>>> groups;
    for (size_t i = 0; i < nr; i++) {
        if (!q.cnt[i]) continue;
        const Geometry g = br_geometry(rs[rid[i]].H);
        size_t k = 0;
        while (k < groups.size() && groups[k].first != g) k++;
        if (k == groups.size()) groups.push_back({ g, {} });
        groups[k].second.push_back((u32)i);
    }
    CHECK(groups.size() <= 2);
    std::vector<Wrote> wrote;
    for (const auto& gr : groups) {
        const std::vector<u32>& ids = gr.second;
        std::vector<BrRun> runs;
        br_runs(rs, rid, q.first.data(), q.cnt.data(), ids, bi, PB, &runs);
        std::vector<ansx_piece> PP;
        std::vector<u64> PC, pfirst;
        std::vector<u32> PK;
        br_pieces(rs, rid, q.first.data(), q.cnt.data(), off, ids, bi, runs, &PP, &PC, &pfirst, with_pk ? &PK : nullptr);
        const u32 npass = runs.back().pass + 1;
        CHECK(pfirst.size() == (size_t)npass + 1 && pfirst[0] == 0 && pfirst[npass] == PP.size() && PC.size() == PP.size());
        // the touched (container, block) pairs: every one in exactly one run, in order
        std::set<std::pair<u32, u32>> want, got;
        for (const u32 i : ids)
            for (u64 b = q.first[i] / bi; b <= (q.first[i] + q.cnt[i] - 1) / bi; b++) want.insert({ rid[i], (u32)b });
        for (size_t k = 0; k < runs.size(); k++) {
            CHECK(runs[k].wl % 4 == 0 && runs[k].b0 <= runs[k].b1 && runs[k].b1 < rs[runs[k].r].nblocks);
            if (k) CHECK(runs[k].pass == runs[k - 1].pass || runs[k].pass == runs[k - 1].pass + 1);
            if (k) CHECK(std::make_pair(runs[k].r, runs[k].b0) > std::make_pair(runs[k - 1].r, runs[k - 1].b1));
            for (u32 b = runs[k].b0; b <= runs[k].b1; b++) CHECK(got.insert({ runs[k].r, b }).second);
        }
        CHECK(got == want);
        Pass P;
        size_t k = 0;
        for (u32 p = 0; p < npass; p++) {
            const size_t k_first = k;
            k = P.take_runs(rs[rid[ids[0]]].H, rs, runs, k, p, bi, bbound);
            const u32 T = (u32)P.B.size();
            CHECK(T >= 1 && T <= PB && P.O.size() == T && P.S.size() == P.cont.size());
            if (p + 1 < npass) CHECK(T == PB);  // (all passes but the last are full)
            // every run's k0 numbers its first block; the table follows the runs
            u32 kb = 0;
            for (size_t j = k_first; j < k; j++) {
                CHECK(runs[j].k0 == kb && P.O[kb].off == runs[j].wl && P.B[kb].b == runs[j].b0);
                kb += runs[j].b1 - runs[j].b0 + 1;
            }
            CHECK(kb == T);
            // every source once; the bound of the payload and the maxima over them
            u64 cap = 0;
            u32 mn = 0, mf = 0, mp = 0;
            for (size_t si = 0; si < P.S.size(); si++) {
                if (si) CHECK(P.cont[si] > P.cont[si - 1]);
                const BatchSrc& cs = rs[P.cont[si]];
                CHECK(P.S[si].base == cs.base && P.S[si].payload_off == cs.lay.payload_off && P.S[si].nblocks == cs.nblocks);
                u64 blocks = 0;
                for (u32 t = 0; t < T; t++) blocks += P.B[t].src == si;
                CHECK(blocks >= 1);
                cap += std::min<u64>(cs.H.payload_bytes, blocks * bbound);
                mn = std::max(mn, cs.H.max_nsyms), mf = std::max(mf, cs.H.max_log2_frame), mp = std::max<u32>(mp, cs.H.max_present_m1);
            }
            CHECK(P.cap_pay == cap && P.Hs.max_nsyms == mn && P.Hs.max_log2_frame == mf && P.Hs.max_present_m1 == mp);
            CHECK(P.Hs.block_ints == bi && P.Hs.ckpt_interval == gr.first[1]);
            // the table: blocks back to back inside a run, every block's own length, nothing past the work list
            for (u32 t = 0; t < T; t++) {
                const BatchSrc& cs = rs[P.cont[P.B[t].src]];
                CHECK(P.O[t].off % 4 == 0 && P.O[t].n == std::min<u64>(bi, cs.H.n - (u64)P.B[t].b * bi));
                CHECK(P.O[t].off + P.O[t].n <= P.wl);
                if (t) CHECK(P.O[t].off >= P.O[t - 1].off + P.O[t - 1].n);
            }
            // the pass's pieces over its table: work-list int x lies in the block t with O[t].off <= x < O[t].off + O[t].n
            for (u64 j = pfirst[p]; j < pfirst[p + 1]; j++) {
                u64 x = PP[j].src, dst = PP[j].dst, left = PC[j];
                CHECK(left > 0);
                bool head = true;
                while (left) {
                    u32 t = 0;
                    while (t < T && !(P.O[t].off <= x && x < P.O[t].off + P.O[t].n)) t++;
                    CHECK(t < T);
                    if (head && with_pk) CHECK(PK[j] == t);
                    head = false;
                    const u64 take = std::min<u64>(left, P.O[t].off + P.O[t].n - x);
                    wrote.push_back({ dst, take, (u64)P.B[t].b * bi + (x - P.O[t].off), P.cont[P.B[t].src] });
                    x += take, dst += take, left -= take;
                }
            }
        }
        CHECK(k == runs.size());
    }
    // what was written is the slices at off[i], once each
    std::sort(wrote.begin(), wrote.end());
    u64 at = 0;
    size_t i = 0;
    for (const Wrote& w : wrote) {
        CHECK(w.dst == at);
        while (i < nr && off[i + 1] <= at) i++;
        CHECK(i < nr && at + w.count <= off[i + 1] && w.r == rid[i] && w.pos == q.first[i] + (at - off[i]));
        at += w.count;
    }
    CHECK(at == total);
}

// ansx_decode_batch_dev's passes: every block of every container of a group exactly once, in order
static void check_whole_batch(const char* what, const Batch& bt, u32 PB)
{
    const u64 bi = bt.bi, bbound = 40;
    std::vector<u64> off(bt.all.size() + 1, 0);
    for (size_t i = 0; i < bt.all.size(); i++) off[i + 1] = off[i] + bt.all[i].H.n;
    for (u32 g = 0; g < 2; g++) {
        std::vector<u32> ids;
        for (u32 i = g; i < bt.all.size(); i += 2) ids.push_back(i);  // (make_batch: the geometries alternate)
        size_t ci = 0;
        u32 b0 = 0;
        std::vector<std::pair<u32, u32>> seen;
        std::vector<Wrote> wrote;
        bool straddled = false;
        while (ci < ids.size()) {
            Pass P;
            std::vector<ansx_range_piece> R;
            std::vector<u32> pstart;
            if (b0) straddled = true;
            const u64 npieces = batch_pass_plan(bt.all, off, ids, &ci, &b0, PB, bbound, &P, &R, &pstart);
            const u32 T = (u32)P.B.size();
            CHECK(T >= 1 && T <= PB && (ci == ids.size() || T == PB));
            CHECK(R.size() == P.S.size() && pstart.size() == R.size() + 1 && pstart.back() == npieces);
            u64 cap = 0, chunks = 0;
            for (size_t si = 0; si < P.S.size(); si++) {
                if (si) CHECK(P.cont[si] > P.cont[si - 1]);
                u64 blocks = 0, ints = 0;
                for (u32 t = 0; t < T; t++)
                    if (P.B[t].src == si) {
                        if (!blocks) CHECK(P.O[t].off == R[si].src && P.O[t].off % 4 == 0);
                        else CHECK(P.O[t].off == P.O[t - 1].off + bi);
                        blocks++, ints += P.O[t].n;
                        seen.push_back({ P.cont[si], P.B[t].b });
                    }
                CHECK(ints == R[si].count && pstart[si] == chunks);
                chunks += (ints + ANSX_RANGE_CHUNK - 1) / ANSX_RANGE_CHUNK;
                cap += std::min<u64>(bt.all[P.cont[si]].H.payload_bytes, blocks * bbound);
                const u32 first_b = P.B[(size_t)(std::find_if(P.B.begin(), P.B.end(), [&](const ansx_batch_blk& x) { return x.src == si; }) - P.B.begin())].b;
                wrote.push_back({ R[si].dst, ints, (u64)first_b * bi, P.cont[si] });
            }
            CHECK(P.cap_pay == cap && P.wl >= R.back().src + R.back().count);
        }
        size_t at = 0;
        for (const u32 i : ids)
            for (u32 b = 0; b < bt.all[i].nblocks; b++, at++) CHECK(at < seen.size() && seen[at] == std::make_pair(i, b));
        CHECK(at == seen.size());
        for (const Wrote& w : wrote) CHECK(w.dst == off[w.r] + w.pos && w.dst + w.count <= off[w.r + 1]);
        if (PB == 3) CHECK(straddled);
    }
}

static Query random_query(std::mt19937_64& rng, const Batch& bt)
{
    Query q;
    const size_t m = 1 + rng() % 12;
    const bool points = rng() % 3 == 0;  // (many single ints: more spans than blocks, br_union's counting branch)
    for (size_t i = 0; i < (points ? 4 * m : m); i++) {
        const u32 s = (u32)(rng() % bt.all.size());
        const u64 n = bt.all[s].H.n, f = rng() % (n + 1);
        u64 c = points ? 1 : rng() % 4 == 0 ? rng() % (n + 1) : rng() % (2 * bt.bi + 1);
        q.add(s, f, std::min<u64>(c, n - f));
    }
    return q;
}

static void batches(u64 bi)
{
    const char* what = "batch";
    const Batch bt = make_batch(bi);
    // br_union, both branches: more spans than blocks, and fewer
    std::mt19937_64 rng(777 + bi);
    for (int it = 0; it < 1000; it++) {
        const u32 nblocks = 1 + (u32)(rng() % 9);
        std::vector<u64> sp;
        const size_t m = it % 2 ? nblocks + 1 + rng() % 6 : 1 + rng() % nblocks;
        for (size_t i = 0; i < m; i++) {
            const u32 a = (u32)(rng() % nblocks), b = a + (u32)(rng() % (nblocks - a));
            sp.push_back((u64)a << 32 | b);
        }
        check_union(it % 2 ? "union, counted" : "union, sorted", sp, nblocks);
    }
    std::vector<std::pair<const char*, Query>> fixed;
    {
        Query q;
        for (u32 s = 0; s < 5; s++) q.add(s, 0, bt.all[s].H.n);
        fixed.push_back({ "every container whole", q });
    }
    {
        Query q;
        for (u32 s = 0; s < 5; s++) q.add(s, bt.all[s].H.n, 0), q.add(s, 0, 0);
        q.add(4, 0, 1);
        fixed.push_back({ "zero counts among one int", q });
    }
    {
        Query q;
        for (u32 s = 5; s-- > 0;) {
            const u64 n = bt.all[s].H.n;
            q.add(s, n - 1, 1);
            for (u64 b = 1; b * bi < n; b++) q.add(s, b * bi - 1, 2);
        }
        fixed.push_back({ "boundaries and last ints, descending", q });
    }
    {
        Query q;
        const u64 n = bt.all[4].H.n;
        q.add(4, 0, n), q.add(4, n / 4, n / 2), q.add(4, n / 4, n / 2), q.add(3, bi, 1), q.add(3, bi - 1, 1), q.add(4, n / 3, 1);
        q.add(3, 3 * bi, 1), q.add(3, 0, 1);  // (container 3: blocks 0, 1 adjacent; 3 behind a gap)
        fixed.push_back({ "duplicate, nested, overlapping, adjacent, gap", q });
    }
    {
        Query q;
        for (u64 x = 0; x < bt.all[3].H.n; x += 1 + x % 3) q.add(3, x, 1);
        q.add(1, 0, 1);
        fixed.push_back({ "point lookups: more spans than blocks", q });
    }
    for (const u32 PB : { 1u, 2u, 3u, 64u }) {
        check_whole_batch("whole batch", bt, PB);
        for (const bool pk : { false, true }) {
            for (const auto& fx : fixed) check_batch(fx.first, bt, fx.second, PB, pk);
            std::mt19937_64 r2(4242 + bi + PB);
            for (int it = 0; it < 1000; it++) check_batch("random", bt, random_query(r2, bt), PB, pk);
        }
    }
    (void)what;
}

// ------------------------------------------------------------------------------- batches of lists to encode
// Batches of 0..40 lists with lengths around every threshold (T: below it ANSrfold's remap is the identity; 1024: the
// small classes; the block; ANSX_ENCB_LONG_BLOCKS blocks), cut for passes of PB blocks.
static void encode_batches(u64 bi, u32 T)
{
    const char* what = "encode batch";
    const u64 lengths[] = { 1, T - 1, T, 1024, 1025, bi - 1, bi, bi + 1, 15 * bi, 16 * bi, 40 * bi };
    std::mt19937_64 rng(99 + bi + T);
    for (const u32 PB : { 1u, 2u, 7u, 16384u })
        for (size_t count = 0; count <= 40; count++)
            for (int remap = ENCB_REMAP_NONE; remap <= ENCB_REMAP_PA; remap++) {
                std::vector<u64> off(count + 1, 5);  // (the first list need not start at int 0)
                for (size_t i = 0; i < count; i++) off[i + 1] = off[i] + lengths[count == 11 ? i % 11 : rng() % 11];
                auto blocks_of = [&](size_t i) { return (off[i + 1] - off[i] + bi - 1) / bi; };
                // the steps partition the lists in order
                size_t at = 0;
                while (at < count) {
                    const EncStep st = encb_step(off.data(), count, at, bi, PB, true);
                    CHECK(st.l0 == at && st.l1 > st.l0 && st.l1 <= count);
                    at = st.l1;
                    const bool first_alone = blocks_of(st.l0) > PB || (off[st.l0 + 1] - off[st.l0]) / bi >= ANSX_ENCB_LONG_BLOCKS;
                    if (!st.NB) {  // alone: too long for a pass, or long enough to pay for itself
                        CHECK(st.l1 == st.l0 + 1 && first_alone);
                        continue;
                    }
                    CHECK(!first_alone && st.NB <= PB);
                    u64 nb = 0;
                    for (size_t i = st.l0; i < st.l1; i++) {
                        nb += blocks_of(i);
                        CHECK(blocks_of(i) <= PB && (off[i + 1] - off[i]) / bi < ANSX_ENCB_LONG_BLOCKS);
                    }
                    CHECK(nb == st.NB);
                    // (the pass is full: the next list would not fit, or goes alone)
                    if (st.l1 < count) CHECK(nb + blocks_of(st.l1) > PB || (off[st.l1 + 1] - off[st.l1]) / bi >= ANSX_ENCB_LONG_BLOCKS);
                    // the layout: sections in order, 16-byte aligned, none overlapping; the upload is what the host fills
                    const u32 nl = (u32)(st.l1 - st.l0);
                    const EncPassLayout L = encb_layout(st.NB, nl, remap != ENCB_REMAP_NONE);
                    const size_t sec[7] = { 0, L.o_l, L.o_i, L.o_m, L.o_r, L.o_s, L.plan_bytes };
                    const size_t need[6] = { sizeof(ansx_blk_in) * st.NB, sizeof(ansx_encb_list) * (nl + 1), remap != ENCB_REMAP_NONE ? 4 * (size_t)st.NB : 0,
                        sizeof(ansx_encb_max) * nl, sizeof(ansx_encb_res) * (nl + 1), 8 * ((size_t)st.NB + 1) };
                    for (int k = 0; k < 6; k++) CHECK(sec[k] % 16 == 0 && sec[k] + need[k] <= sec[k + 1]);
                    // the tables, written into an image of exactly the upload's size (the sanitizer sees any byte beyond it)
                    std::vector<u8> image(L.o_m);
                    EncPassTables Tb;
                    CHECK(encb_pass_tables(off.data(), st.l0, st.l1, bi, st.NB, remap, T, L, image.data(), &Tb));
                    CHECK(!encb_pass_tables(off.data(), st.l0, st.l1, bi, st.NB - 1, remap, T, L, image.data(), &Tb) || st.NB == 0);
                    CHECK(encb_pass_tables(off.data(), st.l0, st.l1, bi, st.NB, remap, T, L, image.data(), &Tb));
                    const ansx_blk_in* blk = (const ansx_blk_in*)image.data();
                    const ansx_encb_list* lists = (const ansx_encb_list*)(image.data() + L.o_l);
                    u32 k = 0, longest = 0;
                    for (size_t i = st.l0; i < st.l1; i++) {  // every int of every list exactly once, in order
                        CHECK(lists[i - st.l0].n == off[i + 1] - off[i] && lists[i - st.l0].fb == k);
                        for (u64 pos = off[i]; pos < off[i + 1]; k++) {
                            CHECK(k < st.NB && blk[k].off == pos && blk[k].list == i - st.l0 && blk[k].n >= 1 && blk[k].n <= bi);
                            CHECK(blk[k].n == bi || pos + blk[k].n == off[i + 1]);
                            pos += blk[k].n;
                            longest = std::max(longest, blk[k].n);
                        }
                    }
                    CHECK(k == st.NB && lists[nl].fb == st.NB && Tb.longest == longest);
                    if (remap == ENCB_REMAP_NONE) {
                        CHECK(Tb.ncls[0] + Tb.ncls[1] + Tb.ncls[2] == 0);
                        continue;
                    }
                    // the class ids: a permutation of the blocks, grouped by class, in block order inside a class
                    const u32* ids = (const u32*)(image.data() + L.o_i);
                    CHECK(Tb.ncls[0] + Tb.ncls[1] + Tb.ncls[2] == st.NB && (remap != ENCB_REMAP_PA || Tb.ncls[2] == 0));
                    std::vector<char> seen(st.NB, 0);
                    u32 j = 0;
                    for (u32 cls = 0; cls < 3; cls++)
                        for (u32 e = 0; e < Tb.ncls[cls]; e++, j++) {
                            const u32 b = ids[j];
                            CHECK(b < st.NB && !seen[b] && (e == 0 || ids[j - 1] < b));
                            seen[b] = 1;
                            const u32 n = blk[b].n;
                            const u32 want = remap == ENCB_REMAP_PA ? (n <= 1024 ? 0u : 1u) : (n < T ? 0u : (n <= 1024 ? 1u : 2u));
                            CHECK(want == cls);
                        }
                }
                // no batched form: every list alone
                for (size_t i = 0; i < count; i++) {
                    const EncStep st = encb_step(off.data(), count, i, bi, PB, false);
                    CHECK(st.l0 == i && st.l1 == i + 1 && st.NB == 0);
                }
            }
}

int main()
{
    for (const u64 bi : { (u64)4096, (u64)16384 })
        for (const u32 T : { 256u, 4096u }) encode_batches(bi, T);
    for (const u64 bi : { (u64)4, (u64)4096 }) {
        for (const u64 n : { (u64)1, bi, bi + 1, 3 * bi + 1 }) single_container(bi, n);
        batches(bi);
    }
    printf("ok: %ld checks\n", checks);
    return 0;
}
