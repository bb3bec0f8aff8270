// The forms of an encode attempt (ans_large_alphabet_amd/csrc/ansx_encode_form.h) swept on the CPU: the four choosers
// are asked over geometries, attempts, the two mid-attempt values and the encode debug keys, and every answer is held
// against limits written down HERE -- the chip's workgroup limits, the LDS every kernel carves (restated from the
// kernel source, the carve cited next to each formula), grids that cover their blocks, and the conditions under which
// a form may run at all.  A forced key must be honoured or refused for a reason named here; the refused combinations
// come out as a table (one row per key, value and reason) whose row count tests/test_encode_form_cpu.py pins.  Built
// with -fsanitize=address,undefined; exit status 0 and "ok" on success.
// The sweep: every codec (fold and rfold 1..7, msb, int; fold, msb and int also compacted), block_ints in {128, 1000,
// 4096, 16384 (16380: compacted ANSint), 65536, 2^22}, restart interval {0, 32, 1024}, block counts on either side of
// every threshold a form reads, whole lists and lists with a partial last block, batch passes, discovery and hinted
// attempts with alphabets from a short list up to the row stride, nt in {0, 4..8}, frames 2^12, 2^16, 2^17 under the
// default keys; each key on its own over the same geometries with a thinner list of attempts.
// `encode_form_check --form` runs no sweep: it reads lines of name=value words from standard input -- one encode attempt
// each: geometry, attempt, keys, the two values the model phase finds, CU count -- and prints for each the report
// ansx_last_encode_form would give (the same report_* assignments the library makes), one line of name=value words.
// tests/test_encode_form_cpu.py holds the case table of tests/test_gpu_encode_forms.py against it.
#include "../../ans_large_alphabet_amd/csrc/ansx_encode_form.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <map>
#include <string>
#include <vector>

using namespace ansx_enc;

static long checks = 0, queries = 0;
static void fail(const char* file, int line, const char* cond);  // prints the query at hand
#define CHECK(cond)                                   \
    do {                                              \
        checks++;                                     \
        if (!(cond)) fail(__FILE__, __LINE__, #cond); \
    } while (0)

// ---------------------------------------------------------------------------------- the limits, independently
static const size_t WG_LDS = 160 * 1024;  // gfx950: LDS per workgroup
static const u32 WG_THREADS = 1024;
static const u32 CUS = 256;  // MI355X

static u32 fold_threshold(u32 f) { return 1u << (f + 7); }  // ansx_dev.h fold_T
static size_t slots_of(u32 kind, u32 f) { return kind == ANSX_MSB ? 2048u : kind == ANSX_INT ? 16384u : (size_t)1 << (f + 9); }  // fold_NSP
// the stream scratch: a block's worst-case stream (make_plan holds it below 2^31) + 16, slots 256 bytes apart
static u64 stride_of(u32 kind, u32 f, u32 pa, u64 nb)
{
    u64 hdr = kind == ANSX_RFOLD ? 4 + 4 * (u64)fold_threshold(f) : 0;
    if (pa) hdr += 8 + 4 * nb + 8;
    const u64 bound = hdr + 8 + 4 * slots_of(kind, f) + 7 * nb + 32;
    return (bound + 16 + 255) / 256 * 256;
}

// k_fold_hist: "Layout: [4][NSP + pad] u32 | [NSP + 8] f64 terms | max word" with sum_mode bit 0 (aux[2 * NSP + tid], tid < 17,
// behind hwords = 4 * (NSP + ANSX_HCOPY_PAD) words), no terms with bit 1 (tree sum); else hwords = PACKED ? NSP / 2 : NSP
static size_t carve_hist(bool packed, bool sum_here, bool tree_sum, u32 NSP)
{
    if (sum_here) return (size_t)4 * (NSP + 8) * 4 + (tree_sum ? 0 : ((size_t)2 * NSP + 17) * 4);
    return packed ? (size_t)NSP * 2 : (size_t)NSP * 4;
}
// k_sort_entropy: "[nbig_cap] big keys (freq << 16 | sym), then the staged row" [cap] of HT (STAGED), then "[512] terms,
// only allocated when the entropy is summed here"; 4.5 KB of static arrays (cnt, cnt0, vmask, wadj) beside it
static size_t carve_sort(u32 nbig_cap, bool staged, u32 cap, size_t elt, bool deferred)
{
    return (size_t)nbig_cap * 8 + (staged ? cap * elt : 0) + (deferred ? 0 : 512 * 8);
}
static const size_t SORT_STATIC = 256 * 4 + 256 * 2 + 256 * 8 + 256 * 4 + 4;
// k_candidates<NT, NCH>: "per wave: [2 BPW][ANSX_CAND_ROW] { freq, reciprocal of fs_rem }" double2, rows = NCH * BPW,
// BPW = 64 / NT, four waves per workgroup, ANSX_CAND_ROW = 65
static size_t carve_cand(u32 nt, u32 nch) { return (size_t)4 * nch * (64 / nt) * 65 * 16; }
// k_model_finish: off [cap] | bits [cap] | inc [cap] unless inc[] is the block's histogram row (IPT == 0 with incbuf), and
// a scratch word at frq + (inc_hbm ? cap + 8 : 2 cap + 8), frq = bits; 4.2 KB of static arrays (lut[512] f64, ...)
static size_t carve_finish(u32 cap, bool inc_hbm) { return (inc_hbm ? (size_t)2 * cap + 9 : (size_t)3 * cap + 9) * 4; }
static const size_t FIN_STATIC = 8 * 4 + 512 * 8 + 8 * 4 * 8 + 8 * 8;
// rfold_remap_hash_body: keys [slots] u32 | cnt32 [slots / 2] | sel [T] u64, "sel also holds a 1024-bin histogram" (512 u64)
static size_t carve_rf_hash(u32 slots, u32 T) { return 6 * (size_t)slots + 8 * (size_t)(T < 512 ? 512 : T); }
// k_rfg_select: "sel_g[]  // [T]" u64
static size_t carve_rfg_select(u32 T) { return (size_t)T * 8; }
// pa_remap_body: keys [slots] | uq [uqcap]
static size_t carve_pa_remap(u32 slots, u32 uqcap) { return ((size_t)slots + uqcap) * 4; }
// k_pa_header: off [cap] | bits [cap] | (cap < ANSX_PA_MAX_BLOCK) inc_lds at 2 cap + 16, [sigma <= cap]
static size_t carve_pa_header(u32 cap) { return cap < 16384u ? ((size_t)3 * cap + 16) * 4 : (size_t)2 * cap * 4; }
// k_write_prelude<IPT>: off [cap] | bits [cap] | SMALL (IPT > 0): inc at 2 cap, [cap]; with g_work nothing dynamic
static size_t carve_write_prelude(bool small, bool hbm, u32 cap) { return hbm ? 0 : (size_t)(small ? 3 : 2) * cap * 4; }
// k_int_sparse_prelude: off [sigma_cap] | bits [bits_cap]
static size_t carve_sparse_prelude(u32 sigma_cap, u32 bits_cap) { return ((size_t)sigma_cap + bits_cap) * 4; }
// k_encode<MODE>: "wtab = lds_tab + wv * 16 * lds_stride", one wave per 16 blocks; MODE 2: rows of ANSX_ENC_HOT = 577 words
static size_t carve_encode(u32 waves, u32 lds_stride) { return (size_t)waves * 16 * lds_stride * 4; }
// k_encode_pc<POW2, S>: "ptab = lds_pc + pair * 16 * rowwords", then per pair HANDW = 2 * S * 64 * 4 + (S == 8 ? 16 * 36 : 0)
// words; a row holds ns_cap + 1 running sums of 16 bits
static size_t carve_pc(u32 pairs, u32 S, u32 rowwords) { return ((size_t)pairs * 16 * rowwords + (size_t)pairs * (2 * S * 64 * 4 + (S == 8 ? 16 * 36 : 0))) * 4; }

// ---------------------------------------------------------------------------------- forced but refused
static std::map<std::pair<const char*, const char*>, long> refused_lit;  // (key=value, reason), both literals -> queries
static void refuse(const char* key, const char* reason) { refused_lit[{ key, reason }]++; }

struct Query {
    EncGeo g;
    EncAttempt a;
    EncKeys K;
    const char* key;  // the key that is set ("": none), as it appears in the table
    u32 max_logM, max_ns;
    bool serial;
};
static const Query* at_hand = nullptr;
static void fail(const char* file, int line, const char* cond)
{
    fprintf(stderr, "%s:%d: %s\n", file, line, cond);
    if (const Query* p = at_hand) {
        const Query& q = *p;
        fprintf(stderr, "kind %u f %u pa %u NSP %u bi %u ck %u nblocks %u n %llu plain %d pass %d longest %u pow2 %d | ns_cap %u nt %u rf_slots %u pa_distinct %u "
                        "sparse %d full %d | key '%s' | logM %u max_ns %u serial %d\n",
            q.g.kind, q.g.f, q.g.pa, q.g.NSP, q.g.block_ints, q.g.ckpt, q.g.nblocks, (unsigned long long)q.g.n, (int)q.g.plain, (int)q.g.batch_pass, q.g.longest,
            (int)q.g.map_pow2, q.a.ns_cap, q.a.nt, q.a.rf_slots, q.a.pa_distinct, (int)q.a.int_sparse, (int)q.a.sp_full_lds, q.key, q.max_logM, q.max_ns,
            (int)q.serial);
    }
    exit(1);
}

static void check_launch(const Launch& L, size_t statics, size_t attribute_from)
{
    CHECK(L.threads >= 64 && L.threads <= WG_THREADS && L.threads % 64 == 0);
    CHECK(L.lds + statics <= WG_LDS);
    CHECK(L.raise || L.lds <= attribute_from);  // (more dynamic LDS than the default limit is asked for first)
}

static void check(const Query& q)
{
    at_hand = &q;
    queries++;
    const EncGeo& g = q.g;
    const EncKeys& K = q.K;
    const u32 NSP = g.NSP, NB = g.nblocks;
    const u64 stride = stride_of(g.kind, g.f, g.pa, g.batch_pass ? g.longest : g.block_ints);
    CHECK(scratch_stride(g) == stride);
    const bool far_slots = stride * 16 >= 0x7FFFFF00ull;  // the f64 encoders' buffer view of 16 scratch slots: 31-bit offsets

    // ------------------------------------------------------------------ model
    const ModelForm M = choose_model_form(g, q.a, K, CUS, q.serial);
    CHECK(M.chunk % 4 == 0 && M.chunk <= 16384u && M.chunk >= 4);
    CHECK((u64)M.cpb * M.chunk >= g.block_ints && (u64)(M.cpb - 1) * M.chunk < g.block_ints);
    CHECK(M.hist.grid == M.cpb && M.sort.grid == 1 && M.fin.grid == 1);
    CHECK(M.h_deferred == (M.cpb == 1));
    CHECK(!M.h_in_hist || (M.h_deferred && NSP <= 2048));
    if (M.fast) {
        // k_candidates / k_model_finish: whole-block histograms with 16-bit counts, 16-bit frequencies (not ANSint), no
        // compaction, compact tables only, and the f64 encoder behind them (k_model_finish writes no 16-byte entries)
        CHECK(q.a.nt >= 4 && q.a.nt <= 8 && q.a.ns_cap != 0);
        CHECK(!g.pa && g.kind != ANSX_INT && M.h_deferred && g.block_ints <= 65535u && NSP <= 16384u);
        CHECK(!K.table16_fixup && !K.encode_gtab16 && !far_slots && !M.always16 == (NSP <= 4096));
        CHECK(M.bpw == 64 / q.a.nt);
    }
    const bool packed = M.hist.variant == HIST_PACKED;
    CHECK(!packed || (NSP % 2 == 0 && M.chunk <= 65535u && !M.h_in_hist));
    CHECK(M.hist.threads == 256 && M.hist.lds >= carve_hist(packed, M.h_in_hist, M.fast, NSP));
    check_launch(M.hist, 0, 48 * 1024);
    CHECK(M.sort_cap >= 64 && M.sort_cap <= NSP && M.nbig_cap >= 1 && M.nbig_cap <= NSP);
    CHECK((u64)M.nbig_cap * 256 > g.block_ints || M.nbig_cap == NSP);  // every symbol of frequency >= ANSX_VMAX = 256 has a slot
    const bool staged = M.sort.variant != SORT_U32_UNSTAGED;
    CHECK(M.sort.variant != SORT_U16 || g.block_ints <= 65535u);
    CHECK(M.sort.threads == 64 && M.sort.lds >= carve_sort(M.nbig_cap, staged, M.sort_cap, M.sort.variant == SORT_U16 ? 2 : 4, M.h_deferred));
    check_launch(M.sort, SORT_STATIC, 48 * 1024 - SORT_STATIC);
    CHECK(M.sort_cap == NSP || (q.a.ns_cap != 0 && M.sort_cap >= q.a.ns_cap));
    CHECK(M.fcap >= 64 && M.fcap <= NSP && (M.fcap >= q.a.ns_cap || M.fcap == NSP));
    {
        const int v = M.fin.variant;
        const bool one_wave = v == FIN_ONE_WAVE_5 || v == FIN_ONE_WAVE_8, generic = v == FIN_GENERIC_5 || v == FIN_GENERIC_8;
        CHECK(M.fin.threads == (one_wave ? 64u : 256u));
        // slots per thread: 4 x 256 (wave per candidate), 16 x 64 (one wave), 16 x 256, any (generic)
        CHECK(generic || NSP <= ((v == FIN_WAVES || one_wave) ? 1024u : 4096u));
        CHECK(generic == (NSP > 4096));  // (the launch hands k_model_finish the histogram row as inc[] exactly then)
        CHECK(q.a.nt <= 5 || (v != FIN_ONE_WAVE_5 && v != FIN_GENERIC_5 && v != FIN_16_5));  // NTC >= NT
        if (M.fast) {
            CHECK(M.fin.lds >= carve_finish(M.fcap, generic));
            check_launch(M.fin, FIN_STATIC, 48 * 1024);
        }
        if (K.fin_one_wave && !one_wave) {
            CHECK(NSP > 1024);
            refuse(q.key, "more than 1024 slots: 16 per lane do not hold the alphabet");
        }
    }
    if (M.fast) {
        const u32 sizes[3] = { NB, M.range_blocks, M.nranges ? NB - (M.nranges - 1) * M.range_blocks : NB };
        for (const u32 nblk : sizes) {
            const Launch C = cand_launch(M, nblk);
            CHECK(C.variant == 1 || C.variant == 2);
            CHECK(C.threads == 256 && C.lds >= carve_cand(q.a.nt, (u32)C.variant));
            check_launch(C, 0, 48 * 1024);
            const u64 per_wg = (u64)4 * C.variant * M.bpw;
            CHECK((u64)C.grid * per_wg >= nblk && (u64)(C.grid - 1) * per_wg < nblk);
            if (K.cand_chains) CHECK((u32)C.variant == K.cand_chains);
            // one chain while that leaves at most one wave per SIMD (four per CU)
            else CHECK((C.variant == 1) == ((nblk + M.bpw - 1) / M.bpw <= 4 * CUS));
        }
    }
    // the block-range split
    CHECK(M.nranges <= (u32)ANSX_PIPE_MAX_RANGES);
    if (M.nranges) {
        CHECK(M.fast && !q.serial && K.model_pipeline != ANSX_PIPE_NEVER);
        CHECK(M.range_blocks % 64 == 0 && (u64)M.nranges * M.range_blocks >= NB && (u64)(M.nranges - 1) * M.range_blocks < NB);
        CHECK(K.model_pipeline != 0 || (NB >= 8192u && g.n >= ((u64)1 << 27) && M.nranges <= 2));
    } else
        CHECK(M.range_blocks == NB);
    if (K.model_pipeline != 0 && K.model_pipeline != ANSX_PIPE_NEVER) {
        const u32 asked = K.model_pipeline == ANSX_PIPE_ALWAYS ? 2u : (u32)K.model_pipeline;
        if (!M.fast) refuse(q.key, "the exact model kernels run: nothing to overlap");
        else if (q.serial) refuse(q.key, "profile mode or a capturing stream: serial");
        else if (M.nranges != asked) {
            const u64 per = (((u64)NB + asked - 1) / asked + 63) / 64 * 64;  // a range's blocks, rounded up to 64
            CHECK(M.nranges >= 1 && M.nranges < asked && per * (asked - 1) >= NB);
            refuse(q.key, "fewer ranges: their boundaries are multiples of 64 blocks");
        }
    } else
        CHECK(K.model_pipeline != ANSX_PIPE_NEVER || M.nranges == 0);

    // ------------------------------------------------------------------ remap
    const RemapForm R = choose_remap_form(g, q.a);
    if (g.kind == ANSX_RFOLD) {
        const u32 T = fold_threshold(g.f);
        CHECK(R.rf != RF_NONE);
        if (R.rf == RF_HBM_HASH) {
            CHECK(g.block_ints > 16384u || T > 4096u);
            CHECK((R.rf_slots & (R.rf_slots - 1)) == 0 && ((u64)R.rf_slots >= 2ull * g.block_ints || R.rf_slots == (1u << 31)));
            CHECK(R.rf_select.threads == 256 && R.rf_select.lds >= carve_rfg_select(T));
            check_launch(R.rf_select, 256 * 4 + 8, 48 * 1024);
        } else {
            CHECK(R.rf == RF_LDS_OPT || R.rf == RF_LDS_FULL);  // (the sort form: no geometry reaches it)
            CHECK(g.block_ints <= 16384u && T <= 4096u && R.rf_slots % 4 == 0);
            CHECK(R.rf == RF_LDS_OPT ? (R.rf_slots == q.a.rf_slots && R.rf_slots < 20480u) : R.rf_slots == 20480u);
            CHECK(R.rf_slots * 4ull >= 5ull * g.block_ints || R.rf == RF_LDS_OPT);  // full size: >= 1.25 x the block's values
            CHECK(R.rf_remap.threads == 1024 && R.rf_remap.lds >= carve_rf_hash(R.rf_slots, T));
            check_launch(R.rf_remap, 12, 0);
            if (R.rf == RF_LDS_OPT) CHECK(2 * R.rf_remap.lds <= WG_LDS);  // two workgroups share a CU
        }
    } else
        CHECK(R.rf == RF_NONE);
    if (g.pa || q.a.int_sparse) {
        CHECK(R.pa_remap_lds >= carve_pa_remap(R.pa_slots, R.pa_uqcap) && R.pa_remap_lds + 12 + 160 <= WG_LDS);
        CHECK(R.pa_hdr_lds >= carve_pa_header(R.pa_hdr_cap) && R.pa_hdr_lds + 32 <= WG_LDS);
        CHECK((R.pa_uqcap & (R.pa_uqcap - 1)) == 0 && R.pa_uqcap >= 1024 && R.pa_uqcap <= 16384u);
        if (R.pa_small) {
            CHECK(q.a.pa_distinct != 0 && R.pa_uqcap >= q.a.pa_distinct && R.pa_slots >= 2 * q.a.pa_distinct && 2 * R.pa_remap_lds <= WG_LDS);
            CHECK(R.pa_hdr_cap == R.pa_uqcap);
        } else
            CHECK(R.pa_slots == 20480u && R.pa_uqcap == 16384u && R.pa_hdr_cap == 16384u && (!g.pa || g.block_ints <= 16384u));  // (rank space: pa_remap_body takes longer blocks in chunks)
        CHECK(!q.a.int_sparse || !R.pa_small);  // rank-space ANSint: "Always run with the full table sizes"
    }

    // ------------------------------------------------------------------ prelude writers (the exact model path only)
    bool entries16 = M.always16 != 0;  // the 16-byte table entries exist
    if (!M.fast) {
        const PreludeForm F = choose_prelude_form(g, q.a, K, M.always16, q.max_logM, q.max_ns);
        entries16 = entries16 || F.table16_first;
        const Launch& L = F.w;
        CHECK(F.pre_cap >= 64 && F.pre_cap <= NSP && (F.pre_cap >= q.max_ns || F.pre_cap == NSP || q.a.ns_cap != 0));
        CHECK(L.grid == NB && L.threads == 256);
        check_launch(L, 32, 48 * 1024);
        switch (L.variant) {
        case PRE_W4: CHECK(NSP <= 1024 && q.max_logM <= 16 && L.lds >= carve_write_prelude(true, false, F.pre_cap)); break;
        case PRE_W16: CHECK(NSP <= 4096 && q.max_logM <= 16 && L.lds >= carve_write_prelude(true, false, F.pre_cap)); break;
        case PRE_RANK_SPACE:
            CHECK(q.a.int_sparse && entries16);
            CHECK(F.sp_cap >= 64 && F.sp_cap <= 16384u && (F.sp_cap >= q.max_ns || F.sp_cap == 16384u) && F.sp_bits >= 1 && F.sp_bits <= 16384u);
            CHECK(L.lds >= carve_sparse_prelude(F.sp_cap, F.sp_bits));
            CHECK(!q.a.sp_full_lds || (F.sp_cap == 16384u && F.sp_bits == 16384u));
            break;
        case PRE_GENERIC: CHECK(entries16 && L.lds >= carve_write_prelude(false, false, F.pre_cap)); break;
        case PRE_GENERIC_HBM: CHECK(entries16 && carve_write_prelude(false, false, F.pre_cap) + 64 > 150 * 1024); break;
        default: CHECK(false);
        }
        if (K.test_sp_bits) {
            if (L.variant != PRE_RANK_SPACE) refuse(q.key, "no rank-space attempt");
            else if (q.a.sp_full_lds) refuse(q.key, "the repeat with the full-size writer");
            else CHECK(F.sp_bits == K.test_sp_bits);
        }
    } else
        CHECK(q.max_logM == 16);  // (k_model_finish writes compact entries only: the encoder behind it must be an f64 form, below)

    // ------------------------------------------------------------------ encoder
    const EncoderForm E = choose_encoder_form(g, K, CUS, q.max_logM, q.max_ns);
    CHECK(E.first % 16 == 0);
    if (!E.f64) {
        // integer state: frames above 2^16, scratch slots too far apart for 31-bit offsets, or on request -- and only
        // where the 16-byte entries were written
        CHECK(q.max_logM > 16 || far_slots || K.table16_fixup || K.encode_gtab16);
        CHECK(entries16 && !M.fast);
        CHECK(E.rest.variant == ENC_INT_STATE && E.pc.grid == 0 && E.first == 0 && E.rest.lds == 0 && E.rest.threads == 64);
        CHECK((u64)E.rest.grid * 64 >= (u64)NB * 4 && (u64)(E.rest.grid - 1) * 64 < (u64)NB * 4);  // four lanes per block
    } else {
        CHECK(q.max_logM <= 16 && !far_slots);
        const bool tables_fit = (size_t)16 * (q.max_ns | 1u) * 4 <= 40 * 1024;  // MODE 1: 16 rows of 4-byte entries per wave
        if (E.pc.grid) {
            // the pair kernel's own conditions ("Host-checked" at k_encode_pc)
            CHECK(!g.batch_pass && g.block_ints % 128 == 0 && g.block_ints <= (1u << 22));
            CHECK(g.ckpt == 0 || g.ckpt % (4 * E.S) == 0);
            CHECK(stride * 16 < 0x40000000ull);
            CHECK(E.criterion != PC_NONE && (E.S == 4 || E.S == 8) && E.pairs >= 1 && E.pairs <= 4 && E.pc.variant == (int)E.S);
            CHECK(E.pc.threads == 128 * E.pairs && E.pc.raise);
            CHECK(E.rowwords * 2 >= q.max_ns + 1 && E.pc.lds >= carve_pc(E.pairs, E.S, E.rowwords));
            check_launch(E.pc, 0, 0);
            CHECK(E.first % (16 * E.pairs) == 0 && E.first == E.pc.grid * 16 * E.pairs);
            CHECK(E.first >= NB && E.first - NB < 16 * E.pairs);  // all blocks, no idle workgroup
            CHECK(!K.no_pc && (!K.no_pc_auto || (K.use_pc && E.criterion == PC_A) || (K.force_pc && E.criterion == PC_A)));
            if (E.criterion == PC_A) CHECK(E.pairs == 4 && E.S == 8 && tables_fit && (((NB + 63) / 64) * 2 >= CUS || K.force_pc));
            if (E.criterion == PC_B) CHECK(E.S == 4 && (E.pairs == 2 || (K.pc_b_pairs == 1 && E.pairs == 1)) && (!tables_fit || K.encode_mode2));
            if (E.criterion == PC_C) CHECK(E.pairs == 1 && E.S == 8 && tables_fit && (NB + 15) / 16 <= 2 * CUS);
            if (!K.force_pc && E.criterion != PC_A) CHECK(g.n / g.block_ints >= (E.criterion == PC_B ? 32u : 16u));
        } else
            CHECK(E.first == 0);
        const u32 left = NB > E.first ? NB - E.first : 0;
        if (!left) CHECK(E.rest.grid == 0);
        else {
            const Launch& L = E.rest;
            const u32 wpw = L.threads / 64;
            CHECK(wpw >= 1 && wpw <= 4);
            CHECK((u64)L.grid * wpw * 16 >= left && (u64)(L.grid - 1) * wpw * 16 < left);
            CHECK(L.variant == ENC_MODE1 || L.variant == ENC_MODE2);
            if (L.variant == ENC_MODE1) CHECK(tables_fit && !K.encode_mode2 && E.lds_stride >= q.max_ns && (E.lds_stride & 1u));
            else CHECK((!tables_fit || K.encode_mode2) && E.lds_stride == 577);
            CHECK(L.lds >= carve_encode(wpw, E.lds_stride));
            check_launch(L, 0, 48 * 1024);
        }
    }
    // forced keys
    if (K.no_pc || (K.no_pc_auto && !K.use_pc && !K.force_pc)) CHECK(E.pc.grid == 0);
    if (K.encode_gtab16 || K.table16_fixup) CHECK(!E.f64);
    if (K.encode_mode2) {
        if (!E.f64) refuse(q.key, "the integer-state encoder runs");
        else CHECK(E.rest.variant != ENC_MODE1 && E.criterion != PC_A && E.criterion != PC_C);
    }
    if (K.pc_b_pairs == 1 && E.criterion != PC_B) refuse(q.key, "criterion (B) is not the one taken");
    if (K.force_pc && !E.pc.grid) {
        const size_t rw = ((q.max_ns + 2) / 2) | 1u;
        const bool mode1 = (size_t)16 * (q.max_ns | 1u) * 4 <= 40 * 1024;
        if (!E.f64) refuse(q.key, "the integer-state encoder runs");
        else if (g.batch_pass) refuse(q.key, "a batch pass: blocks through the per-block table");
        else if (g.block_ints % 128) refuse(q.key, "block_ints is no multiple of 128");
        else if (g.block_ints > (1u << 22)) refuse(q.key, "block_ints above 2^22");
        else if (stride * 16 >= 0x40000000ull) refuse(q.key, "scratch slots too far apart for the pair kernel");
        else if (!mode1 && carve_pc(2, 4, (u32)rw) > WG_LDS) refuse(q.key, "tables fit no pair form's LDS");
        else if (g.ckpt != 0 && g.ckpt % (mode1 ? 32 : 16) != 0) refuse(q.key, "restart interval no multiple of 4 S");
        else CHECK(false);
    }
    at_hand = nullptr;
}

// ---------------------------------------------------------------------------------- the sweep
struct Codec {
    u32 kind, f, pa;
};
struct KeySet {
    const char* name;
    EncKeys K;
};

// ---------------------------------------------------------------------------------- --form: one attempt per line
// words: kind f pa bi ck n (the geometry; nsp: a compacted pass's shorter row stride) batch longest | ns_cap nt rf_slots
// pa_distinct sparse full fused | the keys by their EncKeys names, no_big_geo | logM max_ns cus serial.  Unnamed words are 0
// (pc_b_pairs: 2; cus: 256).  An optimistic attempt (ns_cap != 0) is sized for frames of 2^16 and alphabets of ns_cap.
static int print_forms()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::map<std::string, unsigned long long> w;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "not name=value: %s\n", tok.c_str()); return 2; }
            w[tok.substr(0, eq)] = strtoull(tok.c_str() + eq + 1, nullptr, 0);
        }
        auto get = [&](const char* k, unsigned long long d = 0) { auto it = w.find(k); if (it == w.end()) return d; const unsigned long long v = it->second; w.erase(it); return v; };
        EncGeo g = {};
        g.kind = (u32)get("kind"), g.f = (u32)get("f"), g.pa = (u32)get("pa"), g.block_ints = (u32)get("bi"), g.ckpt = (u32)get("ck"), g.n = get("n");
        if (!g.block_ints || !g.n) { fprintf(stderr, "bi and n are needed: %s\n", line.c_str()); return 2; }
        g.nblocks = (u32)((g.n + g.block_ints - 1) / g.block_ints);
        g.NSP = (u32)get("nsp", slots_of(g.kind, g.f));
        g.batch_pass = get("batch") != 0, g.longest = (u32)get("longest"), g.map_pow2 = g.kind != ANSX_INT;
        EncAttempt a;
        a.ns_cap = (u32)get("ns_cap"), a.nt = (u32)get("nt"), a.rf_slots = (u32)get("rf_slots"), a.pa_distinct = (u32)get("pa_distinct");
        a.int_sparse = get("sparse") != 0, a.sp_full_lds = get("full") != 0;
        const bool fused = get("fused") != 0;
        EncKeys K;
        K.table16_fixup = get("table16_fixup"), K.encode_gtab16 = get("encode_gtab16"), K.fin_one_wave = get("fin_one_wave");
        K.use_pc = get("use_pc"), K.no_pc_auto = get("no_pc_auto"), K.force_pc = get("force_pc"), K.no_pc = get("no_pc"), K.encode_mode2 = get("encode_mode2");
        K.pc_b_pairs = (u32)get("pc_b_pairs", 2), K.test_sp_bits = (u32)get("test_sp_bits"), K.cand_chains = (u32)get("cand_chains");
        K.model_pipeline = (int)get("model_pipeline");
        const bool no_big_geo = get("no_big_geo") != 0;
        u32 logM = (u32)get("logM"), max_ns = (u32)get("max_ns");
        const u32 cus = (u32)get("cus", CUS);
        const bool serial = get("serial") != 0;
        if (!w.empty()) { fprintf(stderr, "unknown word %s\n", w.begin()->first.c_str()); return 2; }
        if (a.ns_cap) logM = 16, max_ns = a.ns_cap;
        ansx_encode_form_report r = {};
        report_remap(r, choose_remap_form(g, a), g.pa || a.int_sparse);
        report_attempt(r, g, a, fused);
        if (!fused) {
            const ModelForm M = choose_model_form(g, a, K, cus, serial);
            const u32 last = M.nranges ? g.nblocks - (M.nranges - 1) * M.range_blocks : g.nblocks;
            report_model(r, M, M.fast ? (u32)cand_launch(M, last).variant : 0u, M.fast && g.NSP > 4096 && !no_big_geo);
            if (!M.fast) report_prelude(r, choose_prelude_form(g, a, K, M.always16, logM, max_ns));
        }
        report_encoder(r, choose_encoder_form(g, K, cus, logM, max_ns));
        printf("attempt=%u ns_cap=%u nt=%u hist=%u cpb=%u h_deferred=%u h_in_hist=%u sort=%u fin=%u fcap=%u cand_chains=%u nranges=%u range_blocks=%u big_geo=%u "
               "rf=%u rf_slots=%u pa_small=%u pa_slots=%u pa_uqcap=%u prelude=%u table16_first=%u pre_cap=%u enc=%u enc_grid=%u enc_threads=%u enc_lds=%u "
               "criterion=%u pairs=%u S=%u pc_grid=%u first=%u nblocks=%u\n",
            r.attempt, r.ns_cap, r.nt, r.hist, r.cpb, r.h_deferred, r.h_in_hist, r.sort, r.fin, r.fcap, r.cand_chains, r.nranges, r.range_blocks, r.big_geo, r.rf,
            r.rf_slots, r.pa_small, r.pa_slots, r.pa_uqcap, r.prelude, r.table16_first, r.pre_cap, r.enc, r.enc_grid, r.enc_threads, r.enc_lds, r.criterion, r.pairs,
            r.S, r.pc_grid, r.first, r.nblocks);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--form")) return print_forms();
    std::vector<Codec> codecs;
    for (u32 f = 1; f <= 7; f++) codecs.push_back({ ANSX_FOLD, f, 0 }), codecs.push_back({ ANSX_RFOLD, f, 0 }), codecs.push_back({ ANSX_FOLD, f, 1 });
    codecs.push_back({ ANSX_MSB, 0, 0 }), codecs.push_back({ ANSX_MSB, 0, 1 }), codecs.push_back({ ANSX_INT, 0, 0 }), codecs.push_back({ ANSX_INT, 0, 1 });
    std::vector<KeySet> keys;
    {
        auto add = [&](const char* name, void (*set)(EncKeys&)) {
            KeySet k = { name, EncKeys() };
            set(k.K);
            keys.push_back(k);
        };
        add("", [](EncKeys&) {});
        add("ANSX_TEST_TABLE16_FIXUP=1", [](EncKeys& k) { k.table16_fixup = true; });
        add("ANSX_ENCODE_GTAB16=1", [](EncKeys& k) { k.encode_gtab16 = true; });
        add("ANSX_FIN_ONE_WAVE=1", [](EncKeys& k) { k.fin_one_wave = true; });
        add("ANSX_NO_PC=1", [](EncKeys& k) { k.no_pc = true; });
        add("ANSX_NO_PC_AUTO=1", [](EncKeys& k) { k.no_pc_auto = true; });
        add("ANSX_NO_PC_AUTO=1+ANSX_USE_PC=1", [](EncKeys& k) { k.no_pc_auto = k.use_pc = true; });
        add("ANSX_USE_PC=1", [](EncKeys& k) { k.use_pc = true; });
        add("ANSX_FORCE_PC=1", [](EncKeys& k) { k.force_pc = true; });
        add("ANSX_ENCODE_MODE2=1", [](EncKeys& k) { k.encode_mode2 = true; });
        add("ANSX_PC_B_PAIRS=1", [](EncKeys& k) { k.pc_b_pairs = 1; });
        add("ANSX_TEST_SP_BITS=100", [](EncKeys& k) { k.test_sp_bits = 100; });
        add("ANSX_CAND_CHAINS=1", [](EncKeys& k) { k.cand_chains = 1; });
        add("ANSX_CAND_CHAINS=2", [](EncKeys& k) { k.cand_chains = 2; });
        add("ANSX_MODEL_PIPELINE=never", [](EncKeys& k) { k.model_pipeline = ANSX_PIPE_NEVER; });
        add("ANSX_MODEL_PIPELINE=always", [](EncKeys& k) { k.model_pipeline = ANSX_PIPE_ALWAYS; });
        add("ANSX_MODEL_PIPELINE=3", [](EncKeys& k) { k.model_pipeline = 3; });
        add("ANSX_MODEL_PIPELINE=64", [](EncKeys& k) { k.model_pipeline = 64; });
    }
    const u32 block_ints[] = { 128, 1000, 4096, 16384, 65536, 1u << 22 };
    const u32 ckpts[] = { 0, 32, 1024 };
    const u32 counts[] = { 1, 15, 16, 17, 31, 32, 2 * CUS * 16 - 1, 2 * CUS * 16, 2 * CUS * 16 + 1, 65536, 65537 };
    const u32 alphabets[] = { 1, 64, 526, 640, 641, 1024, 2296, 2561, 4096, 8176, 16257, 65536 };
    for (const Codec& c : codecs)
        for (u32 bi : block_ints) {
            if (c.pa && bi > 16384u) continue;  // make_plan: the compaction layer takes blocks up to ANSX_PA_MAX_BLOCK ...
            if (c.pa && c.kind == ANSX_INT && bi == 16384u) bi = 16380u;  // ... ANSint up to 16380 (ranks are 1-based)
            for (const u32 ck0 : ckpts) {
                const u32 ck = ck0 >= bi ? 0 : ck0;  // (make_plan)
                for (const u32 nb : counts)
                    for (int shape = 0; shape < 3; shape++) {  // whole blocks | a partial last block | a batch pass
                        Query q = {};
                        q.g.kind = c.kind, q.g.f = c.f, q.g.pa = c.pa;
                        q.g.block_ints = bi, q.g.nblocks = nb, q.g.ckpt = ck;
                        q.g.n = shape == 0 ? (u64)nb * bi : (u64)(nb - 1) * bi + (shape == 1 ? 5 : 1);
                        q.g.batch_pass = shape == 2;
                        if (shape == 2 && (c.kind == ANSX_INT || c.f > 5 || (c.kind == ANSX_RFOLD && bi > 16384u))) continue;  // encode_batch_form
                        q.g.longest = shape == 2 ? std::min<u32>(bi, 1000u) : 0u;
                        q.g.NSP = (u32)slots_of(c.kind, c.f);
                        if (shape == 2 && c.pa) q.g.NSP = std::min<u32>(q.g.NSP, 256u);  // (a compacted pass: min_row_stride of its longest block)
                        q.g.map_pow2 = c.kind != ANSX_INT;
                        const u32 NSP = q.g.NSP;
                        for (const KeySet& ks : keys) {
                            const bool thin = ks.name[0] != 0;
                            q.K = ks.K, q.key = ks.name;
                            for (const u32 ns : alphabets) {
                                if (ns > NSP) continue;
                                for (int hinted = 0; hinted < 2; hinted++) {
                                    // make_plan / encode_dev_once: hints only with rows up to 4096 slots, or up to 16384 without ANSint / compaction
                                    if (hinted && !(NSP <= 4096 || (NSP <= 16384 && c.kind != ANSX_INT && !c.pa))) continue;
                                    if (hinted && (ks.K.encode_gtab16 || ks.K.table16_fixup)) continue;
                                    for (const u32 nt : { 0u, 4u, 5u, 6u, 7u, 8u }) {
                                        if (nt && (!hinted || (thin && nt != 5 && nt != 8))) continue;
                                        for (const u32 logM : { 12u, 16u, 17u }) {
                                            if (hinted && logM != 16) continue;  // (an optimistic attempt assumes frames up to 2^16)
                                            if (thin && logM == 12) continue;
                                            q.a = EncAttempt();
                                            q.a.ns_cap = hinted ? std::min<u32>(NSP, std::max<u32>(64u, (ns + 7u) & ~7u)) : 0u;
                                            q.a.nt = nt;
                                            q.max_logM = logM, q.max_ns = hinted ? q.a.ns_cap : ns;
                                            if (hinted && c.kind == ANSX_RFOLD) q.a.rf_slots = rf_opt_slots(ns, fold_threshold(c.f));
                                            if (hinted && c.pa) q.a.pa_distinct = ns;
                                            for (int serial = 0; serial < 2; serial++) {
                                                if (serial && (thin ? ks.K.model_pipeline == 0 : nb < 8192)) continue;
                                                q.serial = serial != 0;
                                                check(q);
                                                if (c.kind == ANSX_INT && !c.pa && !hinted && shape != 2) {  // rank space, and its repeat
                                                    q.a.int_sparse = true;
                                                    check(q);
                                                    q.a.sp_full_lds = true;
                                                    check(q);
                                                    q.a.int_sparse = q.a.sp_full_lds = false;
                                                }
                                            }
                                        }
                                    }
                                }
                            }
                        }
                    }
            }
        }
    // rf_opt_slots: 1.5 x the distinct values, and two tables with their selection buffers to a CU
    for (u32 f = 1; f <= 7; f++)
        for (u32 d = 0; d <= 20000; d += (d < 64 ? 1 : 37)) {
            const u32 s = rf_opt_slots(d, fold_threshold(f));
            checks++;
            if (s && !(d != 0 && s % 256 == 0 && s >= 1024 && 2ull * s >= 3ull * d && 2 * carve_rf_hash(s, fold_threshold(f)) <= WG_LDS)) fail(__FILE__, __LINE__, "rf_opt_slots");
        }
    printf("ok: %ld queries, %ld checks\n", queries, checks);
    std::map<std::pair<std::string, std::string>, long> refused;
    for (const auto& kv : refused_lit) refused[{ kv.first.first, kv.first.second }] += kv.second;
    printf("forced but refused: %zu rows\n", refused.size());
    for (const auto& kv : refused) printf("  %-34s %-62s %ld\n", kv.first.first.c_str(), kv.first.second.c_str(), kv.second);
    return 0;
}
