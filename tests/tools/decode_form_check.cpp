// The form of a decode call (ans_large_alphabet_amd/csrc/ansx_decode_form.h) swept on the CPU: choose_decode_form is
// asked over geometries, header bounds and debug keys, and every answer is held against limits written down HERE --
// the chip's workgroup limits, the LDS every kernel carves (restated from the kernel source, the carve cited next to
// each formula), and the conditions under which a form may run at all.  A forced key must be honoured or refused for a
// reason named here; the refused combinations come out as a table (one row per key, value and reason) whose row count
// tests/test_decode_form_cpu.py pins.  Built with -fsanitize=address,undefined; exit status 0 and "ok" on success.
// The sweep is no full product (that would be some 10^11 queries).  Part 1 takes every codec, block size, restart interval
// and frame with the default keys and each parser key on its own: max_ns from a short list, max_ep in {1, max_ns},
// nblocks in {1, 65537}, max_block_bytes in {0, small on lean streams, the codec's bound on heavy ones} under the default
// keys and the bound alone under the parser keys; the counts on either side of every threshold, nblocks = 8 and the
// ANSX_PARSE_STAGE_WORDS values only on a dense subset (block_ints 1024 and 65536, fidelities 1 and 7, ANSmsb, ANSint).
// Part 2 crosses every combination of the decoder keys with nblocks in {1, 2, 3}, hinted or not, lean or heavy, on
// eight codecs, five block sizes, three frames and four counts.
#include "../../ans_large_alphabet_amd/csrc/ansx_decode_form.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace ansx_form;

static long checks = 0, queries = 0;
static void fail(const char* file, int line, const char* cond);  // prints the query at hand
#define CHECK(cond)                                \
    do {                                           \
        checks++;                                  \
        if (!(cond)) fail(__FILE__, __LINE__, #cond); \
    } while (0)

// ---------------------------------------------------------------------------------- the limits, independently
static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static const size_t WG_LDS = 160 * 1024;  // gfx950: LDS per workgroup
static const u32 CUS = 256;               // MI355X

// the codecs (include/ansx.h: ANSX_FOLD 0, ANSX_RFOLD 1, ANSX_MSB 2, ANSX_INT 3)
struct Codec {
    u32 kind, f, pa;
};
static u32 fold_threshold(u32 f) { return 1u << (f + 7); }  // ansx_dev.h fold_T
static size_t codec_bound(const Codec& c, size_t nb)        // ansx.hip block_bound, without the compaction layer
{
    const size_t hdr = c.kind == ANSX_RFOLD ? 4 + 4 * (size_t)fold_threshold(c.f) : 0;
    const size_t nsp = c.kind == ANSX_MSB ? 2048u : c.kind == ANSX_INT ? 16384u : (size_t)1 << (c.f + 9);
    return hdr + 8 + 4 * nsp + 7 * nb + 32;
}
static u32 segments(u32 nb, u32 ckpt)  // ansx_dev.h geo_nseg
{
    const u32 nfull = nb - (nb & 3u);
    if (ckpt == 0 || nfull == 0) return 1;
    return (nfull + ckpt - 1) / ckpt;
}

// k_decode_rank, "LDS carve: [bitmap+prefix][entries][symbol ids][most-frequent table][staged stream]":
//   off += (wmax * 8 + 15) & ~15;  off += 2 * ((max_ns * 4 + 15) & ~15);  off += ANSX_DEC_SCRATCH (96)
static size_t carve_rank_tables(u32 maxM, u32 max_ep)
{
    const size_t wmax = maxM >= 32 ? maxM / 32 : 1;
    return up16(wmax * 8) + 2 * up16((size_t)max_ep * 4) + 96;
}
// k_decode_rank, use_ring: "rings start at the next 16-byte boundary" (<= 15 bytes of slack), quad q's ring at
// rings + q * (ANSX_RING_STRIDE / 4), q < blockDim / 4; ring stride 128 * 4 + 16 = 528, small ring 256 + 16 = 272
static size_t carve_rings(u32 threads, size_t stride) { return 15 + (size_t)(threads / 4) * stride; }
// k_decode_rank2, "LDS carve: [interleaved bitmap + prefix entries][entries A][entries B][scratch][rings A][rings B]":
//   off += wmax * 16;  epb = 2 * ((max_ns * 4 + 15) & ~15), twice;  off += ANSX_DEC_SCRATCH;  ringsA aligned up,
//   ringsB = ringsA + (nt >> 2) * (ANSX_RING_STRIDE / 4)
static size_t carve_pair(u32 maxM, u32 max_ep, u32 threads)
{
    const size_t wmax = maxM >= 32 ? maxM / 32 : 1;
    return wmax * 16 + 4 * up16((size_t)max_ep * 4) + 96 + 15 + 2 * (size_t)(threads / 4) * 528;
}
// k_decode, "LDS carve: [cum][s2s][most-frequent table][staged stream]": cb = ((max_ns + 2) * 4 + 15) & ~15,
//   s2s_bytes = (maxM * 2 + 15) & ~15, RFOLD: 4 * T; without LDS_TAB only the most-frequent table and the stream.
//   (+ 4 bytes of static LDS: __shared__ u32 sh_bad)
static size_t carve_table(bool lds_tab, u32 maxM, u32 max_ns, size_t mf)
{
    return (lds_tab ? up16(((size_t)max_ns + 2) * 4) + up16((size_t)maxM * 2) : 0) + mf;
}
// dec_stage_stream: words [0, nw + 4) of the stream area, nw = (sbytes + 3) >> 2; a block is staged when
// sbytes + 24 <= stream_cap (k_decode_rank / k_decode: st_lds), so the staged bytes never pass stream_cap
static size_t staged_bytes(u32 sbytes) { return 4 * ((size_t)((sbytes + 3) >> 2) + 4); }

// k_parse_prelude_par: wave wv's slice at par_lds + wv * ((SW + 48) * 64) words, SW = 32; FORM 1 / 2: behind the SW
// staged rows, ANSX_PAR_STK = 11 stack rows and the value array, [element][64 lanes], of a depth-3 subtree
// (<= max_ns >> 3 items) + 2 sentinels, in the slice's remaining 48 rows
static size_t carve_par(u32 waves) { return (size_t)waves * (32 + 48) * 64 * 4; }
static bool par_array_fits(u32 max_ns, u32 elt) { return ((size_t)(max_ns >> 3) + 2) * 64 * elt + 11 * 64 * 4 <= 48 * 64 * 4; }
// k_parse_prelude_fast: E u16 [max_ns + 2][64] ("ebytes < 20480 ? 20480 : (ebytes + 15) & ~15"), stage
// [ANSX_PF_SW = 128][64] words, stack [21][64] words
static size_t carve_fast(u32 max_ns)
{
    const size_t e = ((size_t)max_ns + 2) * 128;
    return (e < 20480 ? 20480 : up16(e)) + 128 * 64 * 4 + 21 * 64 * 4;
}
// k_parse_prelude_win<SW>: stage [SW][64] + three stacks of [24][64] words
static size_t carve_win(u32 sw) { return ((size_t)sw + 72) * 64 * 4; }

// ---------------------------------------------------------------------------------- forced but refused
static std::map<std::pair<const char*, const char*>, long> refused_lit;  // (key=value, reason), both literals -> queries
static void refuse(const char* key, const char* reason) { refused_lit[{ key, reason }]++; }

static bool is_ring(int d) { return d == DEC_RING || d == DEC_SMALL_RING || d == DEC_PAIR; }
static bool is_rank(int d) { return d == DEC_STAGED || is_ring(d); }

struct Query {
    Codec c;
    u32 bi, ck, nblocks;
    DecodeBounds B;
    FormKeys K;
};

static const Query* at_hand = nullptr;
static const char* note = "";
static void fail(const char* file, int line, const char* cond)
{
    fprintf(stderr, "%s:%d: %s %s\n", file, line, cond, note);
    if (const Query* p = at_hand) {
        const Query& q = *p;
        fprintf(stderr,
            "kind %u f %u pa %u bi %u ck %u nblocks %u maxM %u max_ns %u max_ep %u hinted %d payload %llu mbb %u | generic %d win %d fast %d sw %u old %d "
            "table %d nostream %d mode %d pair %d small %d pair_lds %u\n",
            q.c.kind, q.c.f, q.c.pa, q.bi, q.ck, q.nblocks, q.B.maxM, q.B.max_ns, q.B.max_ep, (int)q.B.hinted, (unsigned long long)q.B.payload_bytes,
            q.B.max_block_bytes, (int)q.K.parse_generic, (int)q.K.parse_win, (int)q.K.parse_fast, q.K.parse_stage_words, (int)q.K.setup_old,
            (int)q.K.decode_table, (int)q.K.no_stream_lds, q.K.decode_mode, q.K.decode_pair, q.K.decode_small_ring, q.K.pair_lds_limit);
    }
    exit(1);
}

static FormGeo geo_of(const Query& q)
{
    FormGeo g;
    g.n = (u64)q.nblocks * q.bi;
    g.block_ints = q.bi, g.nblocks = q.nblocks, g.ckpt = q.ck;
    g.kind = q.c.kind, g.pa = q.c.pa;
    g.nseg = segments(q.bi, q.ck);
    g.mf_bytes = q.c.kind == ANSX_RFOLD ? 4 * fold_threshold(q.c.f) : 0;
    g.block_bound = codec_bound(q.c, q.bi);
    return g;
}

static void check_parser(const Query& q, const DecodeForm& F)
{
    const u32 maxM = q.B.maxM, ns = q.B.max_ns;
    const bool plain_int = q.c.kind == ANSX_INT && !q.c.pa;
    CHECK(F.p.lds <= WG_LDS);
    CHECK(F.p.threads != 0 && F.p.threads % 64 == 0 && F.p.threads <= 256);
    CHECK(F.p.grid != 0);
    CHECK((F.parser == PARSE_DONE) == plain_int);  // only k_int_sparse_parse fills the tables of plain ANSint, and only those
    switch (F.parser) {
    case PARSE_DONE: break;
    case PARSE_GENERIC:  // one lane per block, no dynamic LDS
        CHECK(F.p.threads == 64 && (u64)F.p.grid * 64 >= q.nblocks);
        break;
    case PARSE_PAR: {
        const u32 waves = F.p.threads / 64;
        CHECK(q.B.hinted);  // it reads the container's hints
        CHECK(F.p.lds >= carve_par(waves));
        CHECK((u64)F.p.grid * waves * 8 >= q.nblocks);  // eight lanes per block
        CHECK(F.p_variant <= 2);
        if (F.p_variant == 1) CHECK((u64)maxM + ns + 3 <= 65535u && par_array_fits(ns, 2));  // u16 elements hold every value
        if (F.p_variant == 2) CHECK(par_array_fits(ns, 4));
        break;
    }
    case PARSE_FAST:
        CHECK(F.p.threads == 64 && (u64)F.p.grid * 64 >= q.nblocks);
        CHECK(F.p.lds >= carve_fast(ns));
        CHECK((u64)maxM + ns + 3 <= 65535u);  // E is u16
        CHECK(F.p_variant >= 2 && F.p_variant <= 128 && F.p_variant % 2 == 0);
        break;
    case PARSE_WIN:
        CHECK(F.p.threads == 64 && (u64)F.p.grid * 64 >= q.nblocks);
        CHECK(F.p_variant == 128 || F.p_variant == 256);
        CHECK(F.p.lds >= carve_win(F.p_variant));
        break;
    default: CHECK(!"a parser");
    }
    // forced parser keys: honoured, or refused for a reason
    if (q.K.parse_generic && F.parser != PARSE_GENERIC) {
        CHECK(plain_int);
        refuse("ANSX_PARSE_GENERIC=1", "plain ANSint has no prelude parser");
    }
    if (q.K.parse_win && !q.K.parse_generic && !q.K.parse_fast && F.parser != PARSE_WIN) {
        CHECK(plain_int);
        refuse("ANSX_PARSE_WIN=1", "plain ANSint has no prelude parser");
    }
    if (q.K.parse_fast && !q.K.parse_generic && F.parser != PARSE_FAST) {
        if (plain_int) refuse("ANSX_PARSE_FAST=1", "plain ANSint has no prelude parser");
        else if ((u64)maxM + ns + 3 > 65535u) {
            CHECK(F.parser == PARSE_WIN);
            refuse("ANSX_PARSE_FAST=1", "frame + alphabet + 3 > 65535: windowed parser");
        } else {
            CHECK(F.parser == PARSE_WIN && carve_fast(ns) > 150 * 1024);
            refuse("ANSX_PARSE_FAST=1", "E array above 150 KiB: windowed parser");
        }
    }
    if (q.K.parse_stage_words && F.parser == PARSE_FAST) {
        if (q.K.parse_stage_words >= 2 && q.K.parse_stage_words <= 128) CHECK(F.p_variant == (q.K.parse_stage_words & ~1u));
        else {
            CHECK(F.p_variant == 128);
            refuse("ANSX_PARSE_STAGE_WORDS=n", "outside 2 .. 128: the default window");
        }
    }
    if (q.K.setup_old && F.parser == PARSE_PAR) CHECK(F.p_variant == 0);
}

// may a ring form run at all?  (geometry: dec_segments_ring takes nseg = block_ints / ckpt uniform segments of
// ckpt >> 2 steps; LDS: the chooser keeps ring workgroups within 60 KiB so that two and more share a CU)
static const char* ring_refusal(const Query& q, u32 threads)
{
    if (q.K.decode_table) return "ANSX_DECODE_TABLE is set";
    if (q.B.maxM > 65536u) return "frame above 2^16: table form";
    if (carve_rank_tables(q.B.maxM, q.B.max_ep) > 150 * 1024) return "rank tables above 150 KiB: table form";
    if (q.ck == 0 || q.bi % q.ck != 0 || q.ck % 4 != 0) return "segments of a block are not uniform";
    if (carve_rank_tables(q.B.maxM, q.B.max_ep) + (size_t)(threads / 4) * 528 + 16 > 60 * 1024) return "tables + rings above 60 KiB";
    return nullptr;
}

static void check_decoder(const Query& q, const DecodeForm& F, bool asked_again)
{
    const u32 maxM = q.B.maxM, ns = q.B.max_ns, ep = q.B.max_ep, mbb = q.B.max_block_bytes;
    const size_t mf = q.c.kind == ANSX_RFOLD ? 4 * (size_t)fold_threshold(q.c.f) : 0;
    const u32 nseg = segments(q.bi, q.ck);
    CHECK(F.d.lds + 4 <= WG_LDS);  // (+ k_decode's static word)
    CHECK(F.d.threads != 0 && F.d.threads % 64 == 0 && F.d.threads <= 256);
    CHECK(F.d.threads >= std::min<u32>(256u, nseg * 4) || F.d.threads == 256);  // a quad per segment while they fit
    CHECK(F.d.grid != 0);
    const char* no_ring = ring_refusal(q, F.d.threads);
    if (is_rank(F.decoder)) {
        CHECK(maxM <= 65536u);  // 16-bit slots
        CHECK(!q.K.decode_table);
    }
    if (is_ring(F.decoder)) {
        CHECK(q.ck != 0 && q.bi % q.ck == 0 && q.ck % 4 == 0);
        CHECK(no_ring == nullptr);
        CHECK(F.stream_cap == 0);
    }
    switch (F.decoder) {
    case DEC_STAGED:
        CHECK(F.d.grid == q.nblocks);
        CHECK(F.d.lds >= carve_rank_tables(maxM, ep) + F.stream_cap);
        break;
    case DEC_RING:
        CHECK(F.d.grid == q.nblocks);
        CHECK(F.d.lds >= carve_rank_tables(maxM, ep) + carve_rings(F.d.threads, 528));
        break;
    case DEC_SMALL_RING:
        CHECK(F.d.grid == q.nblocks);
        CHECK(F.d.lds >= carve_rank_tables(maxM, ep) + carve_rings(F.d.threads, 272));
        break;
    case DEC_PAIR:
        CHECK(q.nblocks >= 2);
        CHECK((u64)F.d.grid * 2 >= q.nblocks && (u64)(F.d.grid - 1) * 2 < q.nblocks);
        CHECK(F.d.lds >= carve_pair(maxM, ep, F.d.threads));
        break;
    case DEC_TABLE:
    case DEC_GTAB:
        CHECK(F.d.grid == q.nblocks);
        CHECK(F.d.lds >= carve_table(F.decoder == DEC_TABLE, maxM, ns, mf) + F.stream_cap);
        break;
    default: CHECK(!"a decoder");
    }
    if (F.stream_cap) {
        CHECK(F.stream_cap % 16 == 0);
        // every block of the container is staged, and what dec_stage_stream writes stays inside the area
        const size_t largest = mbb ? mbb : std::min<size_t>(0x7FFFFFFFu, codec_bound(q.c, q.bi));
        CHECK(largest + 24 <= F.stream_cap && staged_bytes((u32)largest) <= F.stream_cap);
    }
    // the index: not asked for exactly where a ring form could run without it
    const bool index_free = no_ring == nullptr && q.K.decode_mode != 2 && !q.c.pa;
    if (!asked_again) CHECK(mbb != 0 || index_free);
    if (mbb == 0) CHECK(!q.c.pa && (is_ring(F.decoder) || F.decoder == DEC_STAGED));

    // forced decoder keys
    if (q.K.decode_table) CHECK(F.decoder == DEC_TABLE || F.decoder == DEC_GTAB);
    if (q.K.decode_mode == 1 && !is_ring(F.decoder)) {
        CHECK(no_ring != nullptr);
        refuse("ANSX_DECODE_MODE=ring", no_ring);
    }
    if (q.K.decode_mode == 2 && F.decoder != DEC_STAGED) {
        CHECK(!is_rank(F.decoder));
        refuse("ANSX_DECODE_MODE=staged", q.K.decode_table ? "ANSX_DECODE_TABLE is set" : maxM > 65536u ? "frame above 2^16: table form" : "rank tables above 150 KiB: table form");
        if (!q.K.decode_table && maxM <= 65536u) CHECK(carve_rank_tables(maxM, ep) > 150 * 1024);
    }
    if (q.K.decode_pair == 1) CHECK(F.decoder != DEC_PAIR);
    if (q.K.decode_pair == 2 && F.decoder != DEC_PAIR) {
        if (!is_ring(F.decoder)) refuse("ANSX_DECODE_PAIR=always", "no ring form runs (forced staged, refused, or rings do not pay)");
        else if (q.nblocks < 2) refuse("ANSX_DECODE_PAIR=always", "a single block");
        else {
            CHECK(carve_pair(maxM, ep, F.d.threads) > 150 * 1024 - 32);
            refuse("ANSX_DECODE_PAIR=always", "two blocks' tables and rings above 150 KiB");
        }
    }
    if (q.K.decode_pair == 0 && q.K.pair_lds_limit == 0) CHECK(F.decoder != DEC_PAIR);  // the default never pairs
    if (q.K.decode_small_ring == 1) CHECK(F.decoder != DEC_SMALL_RING);
    if (q.K.decode_small_ring == 2 && F.decoder != DEC_SMALL_RING) {
        if (F.decoder == DEC_PAIR) refuse("ANSX_DECODE_SMALL_RING=always", "the pair kernel runs (512-byte rings only)");
        else {
            CHECK(!is_ring(F.decoder));
            refuse("ANSX_DECODE_SMALL_RING=always", "no ring form runs (forced staged, refused, or rings do not pay)");
        }
    }
    if (q.K.no_stream_lds && F.stream_cap != 0) {
        CHECK(!is_rank(F.decoder));
        refuse("ANSX_NO_STREAM_LDS=1", "the table forms stage by their own rule");
    }
    if (q.K.no_stream_lds && F.decoder == DEC_STAGED) CHECK(F.stream_cap == 0 && F.d.lds >= carve_rank_tables(maxM, ep));
}

static std::map<std::pair<int, int>, long> seen;  // (parser * 8 + variant class, decoder) -> queries

static void ask(const Query& q0)
{
    Query q = q0;
    queries++;
    at_hand = &q;
    DecodeForm F = choose_decode_form(geo_of(q), q.B, q.K, CUS);
    check_parser(q, F);
    bool again = false;
    if (F.needs_index) {
        CHECK(q.B.max_block_bytes == 0);
        // exactly where no ring form could run without it
        const u32 threads = std::min<u32>(256u, (u32)((segments(q.bi, q.ck) * 4 + 63) / 64 * 64));
        CHECK(ring_refusal(q, threads) != nullptr || q.K.decode_mode == 2 || q.c.pa);
        for (u32 mbb : { 38u, (u32)std::min<size_t>(0x7FFFFFFFu, codec_bound(q.c, q.bi) + (q.c.pa ? 16 + 4 * (size_t)q.bi : 0)) }) {
            q.B.max_block_bytes = mbb;
            const DecodeForm F2 = choose_decode_form(geo_of(q), q.B, q.K, CUS);
            CHECK(!F2.needs_index);
            CHECK(F2.parser == F.parser && F2.p_variant == F.p_variant && F2.p.lds == F.p.lds && F2.p.grid == F.p.grid && F2.p.threads == F.p.threads);
            check_decoder(q, F2, true);
            seen[{ F2.parser, F2.decoder }]++;
        }
        again = true;
    }
    if (!again) {
        check_decoder(q, F, false);
        seen[{ F.parser, F.decoder }]++;
    }
}

// ---------------------------------------------------------------------------------- the sweep
static std::vector<Codec> codecs(bool all)
{
    std::vector<Codec> v;
    if (all) {
        for (u32 f = 1; f <= 7; f++) v.push_back({ ANSX_FOLD, f, 0 }), v.push_back({ ANSX_RFOLD, f, 0 }), v.push_back({ ANSX_FOLD, f, 1 });
        v.push_back({ ANSX_MSB, 0, 0 }), v.push_back({ ANSX_MSB, 0, 1 }), v.push_back({ ANSX_INT, 0, 0 }), v.push_back({ ANSX_INT, 0, 1 });
    } else {
        v = { { ANSX_FOLD, 1, 0 }, { ANSX_FOLD, 7, 0 }, { ANSX_RFOLD, 1, 0 }, { ANSX_RFOLD, 7, 0 }, { ANSX_MSB, 0, 0 }, { ANSX_INT, 0, 0 },
            { ANSX_FOLD, 1, 1 }, { ANSX_INT, 0, 1 } };
    }
    return v;
}

static const u32 BLOCKS[] = { 4, 64, 1024, 1028, 2048, 4096, 16384, 32768, 65536 };

static std::vector<u32> ckpts(u32 bi)
{
    std::set<u32> s = { 0, 4, 64, 256, 1024, bi };
    std::vector<u32> v;
    for (u32 c : s)
        if (c <= bi) v.push_back(c);  // (make_plan drops a restart interval of block_ints and more: 0)
    return v;
}

// symbols present / symbol bound around every threshold that depends on them, for a frame of maxM:
//   the u32 and u16 value arrays of the subtree parser (max_ns >> 3 of 35 and 72), the windowed parser's 1024, the fast
//   loop's E array (max_ns + 2 <= 900) and its 16-bit values (maxM + max_ns + 3 <= 65535), the staged / ring limits of
//   52 and 60 KiB, the rank tables' 150 KiB (8 max_ep + bitmap + 96: max_ep = 16384 at a frame of 2^16 is 147 552 bytes,
//   the limit falls at 17 140), the table form's 150 KiB (4 (max_ns + 2) + 2 maxM)
static std::vector<u32> counts(u32 maxM, bool dense)
{
    std::set<long> s = { 1, 1025, 65536 };
    if (dense) s.insert({ 2, 256, 766, 1024, 16384, 17130, 32768, 65535 });
    if (dense) {
        for (long c : { 287l, 288l, 583l, 584l, 898l, 899l, 17130l })
            for (long d = -1; d <= 1; d++) s.insert(c + d);
        const long bitmap = (long)up16((maxM >= 32 ? maxM / 32 : 1) * 8);
        for (long lim : { 52l * 1024, 60l * 1024, 150l * 1024 })
            for (long rings : { 0l, 16l * 528 + 16, 64l * 528 + 16, 64l * 272 + 16 })
                for (long d = -4; d <= 4; d++) s.insert((lim - 96 - bitmap - rings) / 8 + d);
        for (long d = -4; d <= 4; d++) s.insert((150l * 1024 - 2 * (long)maxM) / 4 - 2 + d), s.insert(65535l - 3 - (long)maxM + d);
    }
    std::vector<u32> v;
    for (long c : s)
        if (c >= 1 && c <= 65536) v.push_back((u32)c);
    return v;
}

int main()
{
    Query q = {};
    // 1. Every geometry and every frame, default keys and each parser key on its own.
    std::vector<FormKeys> singles(1), windows;
    {
        FormKeys k;
        k = FormKeys(), k.parse_generic = true, singles.push_back(k);
        k = FormKeys(), k.parse_win = true, singles.push_back(k);
        k = FormKeys(), k.parse_fast = true, singles.push_back(k);
        k = FormKeys(), k.setup_old = true, singles.push_back(k);
        for (u32 sw : { 1u, 2u, 32u, 33u, 64u, 128u, 129u }) k = FormKeys(), k.parse_fast = true, k.parse_stage_words = sw, windows.push_back(k);
    }
    for (const Codec& c : codecs(true))
        for (u32 bi : BLOCKS)
            for (u32 ck : ckpts(bi)) {
                const bool dense = (bi == 1024 || bi == 65536) && (ck == 256 || ck == 0) && (c.f == 0 || c.f == 1 || c.f == 7);
                for (u32 nb : { 1u, 8u, 65537u }) {
                    if (nb == 8 && !dense) continue;
                    for (u32 lg = 0; lg <= 27; lg++)
                        for (u32 ns : counts(1u << lg, dense))
                            for (u32 ep : { 1u, ns }) {
                                if (ep > ns) continue;
                                q.c = c, q.bi = bi, q.ck = ck, q.nblocks = nb;
                                const u32 bound = (u32)std::min<size_t>(0x7FFFFFFFu, codec_bound(c, bi));
                                // default keys: no index, a small largest block on lean streams, the codec's bound on heavy ones
                                for (u32 mbb : { 0u, 38u, bound }) {
                                    q.B = { 1u << lg, ns, ep, (lg + ns) % 2 == 0, mbb == 38 ? (u64)nb * bi : (u64)nb * bi * 3, mbb };
                                    q.K = singles[0];
                                    ask(q);
                                }
                                // parser keys, hinted or not (the parser does not hang on the largest block)
                                for (int hinted = 0; hinted < 2; hinted++) {
                                    q.B = { 1u << lg, ns, ep, hinted != 0, (u64)nb * bi * 3, bound };
                                    for (size_t i = 1; i < singles.size(); i++) q.K = singles[i], ask(q);
                                    if (dense)
                                        for (const FormKeys& k : windows) q.K = k, ask(q);
                                }
                            }
                }
            }
    // 2. Every combination of the decoder keys, hinted or not, on fewer codecs and frames.
    for (const Codec& c : codecs(false))
        for (u32 bi : { 4u, 1024u, 1028u, 4096u, 65536u })
            for (u32 ck : ckpts(bi))
                for (u32 nb : { 1u, 2u, 3u })
                    for (u32 lg : { 12u, 16u, 17u })
                        for (u32 ns : { 1u, 17130u, 17150u, 65536u })
                            for (u32 ep : { 1u, ns }) {
                                if (ep > ns) continue;
                                q.c = c, q.bi = bi, q.ck = ck, q.nblocks = nb;
                                const u32 bound = (u32)std::min<size_t>(0x7FFFFFFFu, codec_bound(c, bi));
                                for (int combo = 0; combo < 4; combo++) {
                                    const u32 mbb = combo < 2 ? 0u : combo == 2 ? 38u : bound;
                                    const bool lean = combo == 0 || combo == 2;
                                    q.B = { 1u << lg, ns, ep, combo % 2 == 0, lean ? (u64)nb * bi : (u64)nb * bi * 3, mbb };
                                    for (int table = 0; table < 2; table++)
                                        for (int nostream = 0; nostream < 2; nostream++)
                                            for (int mode = 0; mode < 3; mode++)
                                                for (int pair = 0; pair < 3; pair++)
                                                    for (int small = 0; small < 3; small++)
                                                        for (u32 plim : { 0u, 150u * 1024 }) {
                                                            if (plim && pair) continue;  // (read only under "auto")
                                                            q.K = FormKeys();
                                                            q.K.decode_table = table, q.K.no_stream_lds = nostream, q.K.decode_mode = mode;
                                                            q.K.decode_pair = pair, q.K.decode_small_ring = small, q.K.pair_lds_limit = plim;
                                                            ask(q);
                                                        }
                                }
                            }
    // every parser and every decoder came up
    for (int p : { PARSE_DONE, PARSE_GENERIC, PARSE_PAR, PARSE_FAST, PARSE_WIN }) {
        long n = 0;
        for (const auto& kv : seen)
            if (kv.first.first == p) n += kv.second;
        at_hand = nullptr, note = "(a parser never chosen)";
        CHECK(n > 0);
    }
    for (int d : { DEC_STAGED, DEC_RING, DEC_SMALL_RING, DEC_PAIR, DEC_TABLE, DEC_GTAB }) {
        long n = 0;
        for (const auto& kv : seen)
            if (kv.first.second == d) n += kv.second;
        at_hand = nullptr, note = "(a decoder never chosen)";
        CHECK(n > 0);
    }
    printf("ok: %ld queries, %ld checks\n", queries, checks);
    std::set<std::pair<std::string, std::string>> refused;  // (the same literal may live at two addresses)
    for (const auto& kv : refused_lit) refused.insert({ kv.first.first, kv.first.second });
    printf("forced but refused: %zu rows\n", refused.size());
    for (const auto& r : refused) printf("  %-32s %s\n", r.first.c_str(), r.second.c_str());
    return 0;
}
