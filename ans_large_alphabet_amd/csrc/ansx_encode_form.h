// ansx -- the forms of one attempt of an encode call ("Host side of an encode call"): which
// instantiation of every templated kernel runs and in what launch shape, from the geometry, the attempt, the encode
// debug overrides, the chip's CU count and the two values the model phase finds (largest frame and alphabet).  Pure host
// arithmetic like ansx_decode_form.h: no context, no stream, no device pointer, so it builds with a plain host compiler
// and is swept on the CPU (tests/tools/encode_form_check.cpp) against the kernels' LDS carves.  The constants the
// kernels and this header share are in ansx_plan_types.h.
#pragma once
#include "../../include/ansx.h"
#include "ansx_plan_types.h"

#include <algorithm>

namespace ansx_enc {

static inline size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- LDS limits, each with the one reason it exists
constexpr size_t LDS_WORKGROUP = 160 * 1024;  // what one workgroup can have on gfx950: the pair encoder's carve is held against it
constexpr size_t LDS_BUDGET = 150 * 1024;     // ... and what a kernel with static arrays of its own may ask for beside them
constexpr size_t LDS_TWO_PER_CU = 78 * 1024;  // hint-sized hash tables: two workgroups of 1024 threads share a CU's 160 KB
constexpr size_t LDS_ENC_MODE1 = 40 * 1024;   // k_encode<1>: the 16 tables of a wave; four waves of a workgroup fill a CU
constexpr size_t LDS_NO_ATTRIBUTE = 48 * 1024;       // dynamic LDS up to here needs no hipFuncSetAttribute
constexpr size_t LDS_NO_ATTRIBUTE_SORT = 32 * 1024;  // ... k_sort_entropy, with 4.5 KB of static arrays beside its row, asks from here on

// The codec's symbol-array stride (the reference's MAX_SIGMA; the kernels' fold_NSP) and ANSrfold's T (their fold_T)
static inline size_t codec_nsp(int kind, u32 f) { return kind == ANSX_MSB ? 2048u : (kind == ANSX_INT ? 16384u : (size_t)1 << (f + 9)); }
static inline u32 rfold_T(u32 f) { return 1u << (f + 7); }

// worst-case bytes of one block's reference stream
static inline size_t block_bound(int kind, u32 f, size_t nb, bool pa = false)
{
    size_t hdr = kind == ANSX_RFOLD ? 4 + 4 * (size_t)rfold_T(f) : 0;
    size_t nsp = codec_nsp(kind, f);
    if (pa) hdr += 8 + 4 * nb + 8;  // alphabet header: at most 32 bits per distinct value
    return hdr + 8 + 4 * nsp + 7 * nb + 32;
}

// What the forms read of the call's geometry.
struct EncGeo {
    u64 n;
    u32 block_ints, nblocks, ckpt;
    u32 kind, f, pa;
    u32 NSP;          // symbol-row stride of the call (the codec's, or a compacted pass's shorter one)
    bool plain;       // a single reference stream
    bool batch_pass;  // a pass of ansx_encode_batch_dev: blocks through the per-block table ...
    u32 longest;      // ... and the ints of its longest block
    bool map_pow2;    // the map's thresholds are powers of two (the encoders' POW2 instantiations)
};
// bytes per block of the stream scratch (a batch pass: slots as long as its longest block needs, not as block_ints would)
static inline u64 scratch_stride(const EncGeo& g)
{
    return rup(block_bound((int)g.kind, g.f, g.batch_pass ? g.longest : g.block_ints, g.pa != 0) + 16, 256);
}

// What one attempt of an encode call may assume (EncodeAttempt of ansx.hip adds its one device pointer).
struct EncAttempt {
    // ns_cap == 0: discovery -- the largest alphabet / frame of the call are read back between the model kernels and
    // the encoder launch (one host round trip per candidate batch).
    // ns_cap != 0: optimistic -- the caller has seen this geometry before (alphabet hint): the first candidate batch is
    // assumed to settle every block, frames are assumed to stay within 2^16 and alphabets within ns_cap, so everything
    // is launched back to back; the assumptions are checked on the words that come back with the output size anyway,
    // and a miss returns ANSX_RETRY_GENERAL.  nt, rf_slots and pa_distinct are nonzero in optimistic attempts only.
    u32 ns_cap = 0;
    u32 nt = 0;                // candidates per block of the fast model path (4 .. 8), 0 = the exact model kernels
    u32 rf_slots = 0;          // ANSrfold: optimistic hash-table size (rf_opt_slots), 0 = the full-size table
    u32 pa_distinct = 0;       // compaction layer: the geometry's distinct-value hint (sizes k_pa_remap2), 0 = full size
    bool int_sparse = false;   // plain ANSint modelled in rank space (ansx_intsparse.h)
    bool sp_full_lds = false;  // ... and its prelude writer runs with the full-size LDS arrays (a block's code outgrew the hint-sized ones)
};

// The debug overrides that select a shape (the context's DebugOpts has them under the same names).
struct EncKeys {
    bool table16_fixup = false, encode_gtab16 = false, fin_one_wave = false;
    bool use_pc = false, no_pc_auto = false, force_pc = false, no_pc = false, encode_mode2 = false;
    u32 pc_b_pairs = 2, test_sp_bits = 0, cand_chains = 0;
    int model_pipeline = 0;
};

// A launch: which instantiation, and its shape.  raise: the dynamic LDS needs hipFuncSetAttribute first.
struct Launch {
    int variant;
    u32 grid, threads;
    size_t lds;
    bool raise;
};

// ------------------------------------------------------------------------------------------ the model phase
// (the variants have the values of the public enumerations, which ansx_last_encode_form reports)
enum { HIST_WORDS = ANSX_HIST_WORDS, HIST_PACKED = ANSX_HIST_PACKED };  // k_fold_hist<false / true>
enum { SORT_U16 = ANSX_SORT_U16, SORT_U32 = ANSX_SORT_U32, SORT_U32_UNSTAGED = ANSX_SORT_U32_UNSTAGED };  // k_sort_entropy<u16>, <u32>, <u32, false>
// k_model_finish<4, 8, 256> (wave per candidate), <16, NTC, 256>, <16, NTC, 64> (one wave per block), <0, NTC, 256> (generic)
enum { FIN_WAVES = ANSX_FIN_WAVES, FIN_16_5 = ANSX_FIN_16_5, FIN_16_8 = ANSX_FIN_16_8, FIN_ONE_WAVE_5 = ANSX_FIN_ONE_WAVE_5,
    FIN_ONE_WAVE_8 = ANSX_FIN_ONE_WAVE_8, FIN_GENERIC_5 = ANSX_FIN_GENERIC_5, FIN_GENERIC_8 = ANSX_FIN_GENERIC_8 };

// Launch shapes of the model kernels.  hist, sort and fin are launched per block range: their grid is workgroups PER BLOCK.
struct ModelForm {
    u32 chunk, cpb;    // K1: ints per histogram workgroup, workgroups per block
    bool h_deferred;   // blocks that fit one histogram workgroup (the normal case): entropy terms from K1, in-order sum from K2b (else both in K2a)
    bool h_in_hist;    // ... and alphabets up to 2048 slots are also summed in K1 (terms in LDS), larger ones through HBM in K2b
    bool fast;         // fast model path (ansx_fastmodel.h): k_candidates / k_model_finish instead of the candidate batches
    u32 nbig_cap, sort_cap;  // K2: "big" symbols have freq >= ANSX_VMAX; length of the staged row
    u32 always16;      // the 16-byte table entries have a certain consumer before the frames are known
    u32 bpw, fcap;     // fast model path: blocks per wave of k_candidates, alphabet capacity of k_model_finish
    Launch hist, sort, fin;
    // k_candidates: chains per lane forced by ANSX_CAND_CHAINS (0: by the launch's blocks, one chain up to cand_one_chain)
    u32 cand_forced, cand_one_chain;
    // the block-range pipeline: nranges == 0 is one launch of each kernel over all blocks on the caller's stream
    u32 range_blocks, nranges;
};

// chains per lane of k_candidates and its shape for a launch over nblk blocks: one chain while that leaves at most one
// wave per SIMD, else two (see the kernel); per launch, by its blocks.  variant: the chain count
static inline Launch cand_launch(const ModelForm& M, u32 nblk)
{
    const u32 nch = M.cand_forced ? M.cand_forced : (nblk <= M.cand_one_chain ? 1u : 2u);
    const u32 cwaves = (nblk + nch * M.bpw - 1) / (nch * M.bpw);
    const size_t lds = (size_t)ANSX_CAND_WAVES * nch * M.bpw * ANSX_CAND_ROW * 16;
    return { (int)nch, (cwaves + ANSX_CAND_WAVES - 1) / ANSX_CAND_WAVES, 64 * ANSX_CAND_WAVES, lds, lds > LDS_NO_ATTRIBUTE };
}

// serial: the call may not fork (profile mode would time overlapped kernels; a captured graph stays one chain)
static inline ModelForm choose_model_form(const EncGeo& g, const EncAttempt& a, const EncKeys& dbg, u32 num_cus, bool serial)
{
    ModelForm M = {};
    const u32 NSP = g.NSP;
    const u64 scr_stride = scratch_stride(g);
    M.chunk = g.block_ints < 16384u ? g.block_ints : 16384u;
    if (M.chunk & 3u) M.chunk = (M.chunk + 3u) & ~3u;
    M.cpb = (g.block_ints + M.chunk - 1) / M.chunk;
    M.h_deferred = (M.cpb == 1);
    M.h_in_hist = M.h_deferred && NSP <= 2048;
    // Fast model path: geometries seen before, whole-block histograms, 16-bit frequencies, compact tables; every
    // assumption is checked on the device and a miss repeats the call on the exact path.
    // (alphabets above 4096 slots -- f = 4, 5 -- take the generic form of k_model_finish as long as its three LDS arrays,
    // sized from the alphabet hint, fit a CU; ANSint has no u16 rule and 32-bit frequencies: exact path)
    M.fcap = std::min<u32>(NSP, std::max<u32>(64u, (a.ns_cap + 15u) & ~15u));
    M.fast = a.nt != 0 && !g.pa && M.h_deferred && g.block_ints <= 65535u && NSP <= 16384 && g.kind != ANSX_INT
        && (NSP <= 4096 || (size_t)M.fcap * 8 + 64 <= LDS_BUDGET) && !dbg.table16_fixup && !dbg.encode_gtab16
        && scr_stride * 16 < 0x7FFFFF00ull;
    // f >= 4: 16-bit counters, two per LDS word (a chunk holds at most 16384 values): half the LDS, twice the workgroups per CU
    const bool packed = NSP >= 8192u;
    // (fast path: H is a tree sum in registers, no LDS row of terms)
    const size_t hist_lds = packed ? (size_t)NSP * 2
        : !M.h_in_hist     ? (size_t)NSP * 4
                           : (size_t)4 * (NSP + ANSX_HCOPY_PAD) * 4 + (M.fast ? 0 : (size_t)NSP * 8 + 80);
    M.hist = { packed ? HIST_PACKED : HIST_WORDS, M.cpb, 256, hist_lds, hist_lds > LDS_NO_ATTRIBUTE };
    M.nbig_cap = (u32)std::min<size_t>(NSP, (size_t)g.block_ints / ANSX_VMAX + 2);
    // (optimistic calls with whole-block histograms: the staged row is as long as the alphabet hint, see the kernel)
    M.sort_cap = (a.ns_cap != 0 && M.h_deferred) ? std::min<u32>(NSP, std::max<u32>(64u, (a.ns_cap + 7u) & ~7u)) : NSP;
    const bool sort16 = g.block_ints <= 65535u;  // (a count fits 16 bits: half the staged row)
    size_t k2a_lds = (size_t)M.nbig_cap * 8 + (size_t)M.sort_cap * (sort16 ? 2 : 4) + (M.h_deferred ? 0 : 512 * 8);
    const bool staged = k2a_lds <= LDS_BUDGET;  // (f = 6, 7 with 32-bit counts: the row stays in HBM)
    if (!staged) k2a_lds = (size_t)M.nbig_cap * 8 + (M.h_deferred ? 0 : 512 * 8);
    M.sort = { !staged ? SORT_U32_UNSTAGED : (sort16 ? SORT_U16 : SORT_U32), 1, 64, k2a_lds, k2a_lds > LDS_NO_ATTRIBUTE_SORT };
    // consumers of the 16-byte table entries that are certain before the frames are known: the generic prelude writer (alphabets above
    // 4096 slots) and the integer-state encoder (forced, or scratch slots too far apart for the f64 encoder's 31-bit buffer offsets)
    M.always16 = (!dbg.table16_fixup && (NSP > 4096 || scr_stride * 16 >= 0x7FFFFF00ull || dbg.encode_gtab16)) ? 1u : 0u;
    M.bpw = M.fast ? 64u / a.nt : 1u;
    const size_t fin_lds = (size_t)M.fcap * (NSP > 4096 ? 8 : 12) + 64;  // (above 4096 slots: inc[] in the block's histogram row, two LDS arrays)
    const bool few = a.nt <= 5;
    // one wave per block (16 slots per lane, every candidate in every lane, no workgroup barriers): four times the blocks in flight
    if (NSP <= 1024 && dbg.fin_one_wave) M.fin = { few ? FIN_ONE_WAVE_5 : FIN_ONE_WAVE_8, 1, 64, fin_lds, false };
    else if (NSP <= 1024) M.fin = { FIN_WAVES, 1, 256, fin_lds, false };  // (wave-per-candidate form: NTC is not used)
    else if (NSP > 4096) M.fin = { few ? FIN_GENERIC_5 : FIN_GENERIC_8, 1, 256, fin_lds, false };
    else M.fin = { few ? FIN_16_5 : FIN_16_8, 1, 256, fin_lds, false };
    M.fin.raise = fin_lds > LDS_NO_ATTRIBUTE;
    M.cand_forced = dbg.cand_chains;
    M.cand_one_chain = (u32)std::min<u64>(0xFFFFFFFFu, (u64)4 * num_cus * M.bpw);
    // Block-range pipeline of the fast model path (ANSX_PIPE_* in ansx_plan_types.h): a range count on request, else
    // ANSX_PIPE_RANGES from the size rule on; range boundaries are multiples of 64 blocks
    M.range_blocks = g.nblocks, M.nranges = 0;
    const int mode = dbg.model_pipeline;
    const u32 want = mode > 0 ? (u32)mode
                              : ((mode == ANSX_PIPE_ALWAYS || (g.nblocks >= ANSX_PIPE_MIN_BLOCKS && g.n >= ANSX_PIPE_MIN_INTS)) ? ANSX_PIPE_RANGES : 0u);
    if (M.fast && !serial && mode != ANSX_PIPE_NEVER && want) {
        M.range_blocks = (u32)rup(((size_t)g.nblocks + want - 1) / want, 64);
        M.nranges = (g.nblocks + M.range_blocks - 1) / M.range_blocks;
    }
    return M;
}

// ------------------------------------------------------------------------------------------ the remap front
// Optimistic hash-table size for a geometry whose blocks had at most `distinct` different values so far: 1.5 x that,
// if two such tables (+ selection buffers) share a CU's LDS; 0 = use the full-size table.
static inline u32 rf_opt_slots(u32 distinct, u32 T)
{
    if (distinct == 0) return 0;
    u32 slots = (2 * distinct + distinct / 2 + 64 + 255) & ~255u;
    if (slots < 1024) slots = 1024;
    const size_t lds = 6 * (size_t)slots + 8 * (size_t)(T < 512 ? 512 : T);
    return lds <= LDS_TWO_PER_CU ? slots : 0u;
}

// ans_reorder_fold.hpp:70-106 on the device: LDS hash table per block for blocks <= 16384 ints (hint-sized on optimistic
// attempts), HBM hash table for longer blocks (incl. whole-list single-stream mode) and T > 4096 (f = 6, 7 -- the
// selection buffer alone is 64 / 128 KB); RF_SORT is what is left of the older sort form (T > 4096 in short blocks: no
// geometry reaches it while RF_HBM_HASH takes every T > 4096)
enum { RF_NONE = ANSX_RF_NONE, RF_HBM_HASH = ANSX_RF_HBM_HASH, RF_LDS_OPT = ANSX_RF_LDS_OPT, RF_LDS_FULL = ANSX_RF_LDS_FULL, RF_SORT = ANSX_RF_SORT };
struct RemapForm {
    int rf;
    u32 rf_slots;      // RF_HBM_HASH: slots per block in HBM; the LDS forms: table slots; RF_SORT: the sort's length
    Launch rf_select;  // RF_HBM_HASH: k_rfg_select (grid: per block)
    Launch rf_remap;   // the LDS forms and RF_SORT (grid: per block of the launch)
    // the compaction layer (k_pa_remap / k_pa_remap2 + k_pa_header over all blocks, or the large class of a pass): sizes
    // from the geometry's distinct-value hint on optimistic attempts -- hash set 2.5 x, value list the next power of two
    // above 1.25 x; both workgroups of a CU must fit its LDS
    bool pa_small;
    u32 pa_slots, pa_uqcap, pa_hdr_cap;
    size_t pa_remap_lds, pa_hdr_lds;
};
static inline RemapForm choose_remap_form(const EncGeo& g, const EncAttempt& a)
{
    RemapForm R = {};
    if (g.kind == ANSX_RFOLD) {
        const u32 T = rfold_T(g.f);
        if (g.block_ints > 16384u || T > 4096u) {
            R.rf = RF_HBM_HASH;
            R.rf_slots = 2;
            while ((u64)R.rf_slots < 2ull * g.block_ints && R.rf_slots < (1u << 31)) R.rf_slots <<= 1;
            R.rf_select = { 0, 1, 256, (size_t)T * 8, (size_t)T * 8 > LDS_NO_ATTRIBUTE };
        } else if (T <= 4096) {
            const size_t sel_bytes = 8 * (size_t)(T < 512 ? 512 : T);  // also holds a 1024-bin histogram
            const bool opt = a.rf_slots != 0 && a.rf_slots < ANSX_RF_SLOTS;
            R.rf = opt ? RF_LDS_OPT : RF_LDS_FULL;
            R.rf_slots = opt ? a.rf_slots : (u32)ANSX_RF_SLOTS;
            R.rf_remap = { 0, 1, 1024, 6 * (size_t)R.rf_slots + sel_bytes, true };
        } else {
            R.rf = RF_SORT;
            R.rf_slots = 2;
            while (R.rf_slots < g.block_ints) R.rf_slots <<= 1;
            const size_t lds = 6 * (size_t)R.rf_slots + 8 * (size_t)T + 16;
            R.rf_remap = { 0, 1, 256, lds, lds > LDS_NO_ATTRIBUTE };
        }
    }
    R.pa_slots = ANSX_PA_SLOTS, R.pa_uqcap = ANSX_PA_MAX_BLOCK;
    if (a.pa_distinct != 0) {
        const u32 d = a.pa_distinct;
        const u32 sl = (2 * d + d / 2 + 64 + 255) & ~255u;
        u32 uc = 1024;
        while (uc < d + d / 4 + 16) uc <<= 1;
        if (((size_t)sl + uc) * 4 <= LDS_TWO_PER_CU && uc <= ANSX_PA_MAX_BLOCK) R.pa_slots = sl, R.pa_uqcap = uc, R.pa_small = true;
    }
    R.pa_remap_lds = ((size_t)R.pa_slots + R.pa_uqcap) * 4;
    R.pa_hdr_cap = R.pa_small ? R.pa_uqcap : (u32)ANSX_PA_MAX_BLOCK;
    R.pa_hdr_lds = R.pa_small ? ((size_t)3 * R.pa_uqcap + 32) * 4 : ((size_t)2 * ANSX_PA_MAX_BLOCK + 16) * 4;
    return R;
}

// ------------------------------------------------------------------------------------------ the exact form's prelude writers
// k_write_prelude<4>, <16>, k_int_sparse_prelude, k_write_prelude<0> with its two arrays in LDS / in HBM (f = 6, 7)
enum { PRE_W4 = ANSX_PRE_W4, PRE_W16 = ANSX_PRE_W16, PRE_RANK_SPACE = ANSX_PRE_RANK_SPACE, PRE_GENERIC = ANSX_PRE_GENERIC,
    PRE_GENERIC_HBM = ANSX_PRE_GENERIC_HBM };
struct PreludeForm {
    bool table16_first;  // mixed call: a frame above 2^16 sends every block to the integer-state encoder (k_table16_from32)
    Launch w;            // variant: PRE_*
    u32 pre_cap;         // the writers' LDS arrays are as long as the call's largest alphabet, not as its slot count
    u32 sp_cap, sp_bits; // PRE_RANK_SPACE: distinct values and words of the bit buffer a block may have
};
static inline PreludeForm choose_prelude_form(const EncGeo& g, const EncAttempt& a, const EncKeys& dbg, u32 always16, u32 max_logM, u32 max_ns)
{
    PreludeForm F = {};
    const u32 NSP = g.NSP, NB = g.nblocks;
    F.table16_first = !always16 && (max_logM > 16 || dbg.table16_fixup);
    F.pre_cap = std::min<u32>(NSP, std::max<u32>(64u, ((a.ns_cap ? a.ns_cap : max_ns) + 7u) & ~7u));
    if (NSP <= 1024 && max_logM <= 16) {
        F.w = { PRE_W4, NB, 256, (size_t)F.pre_cap * 12 + 64, false };
    } else if (NSP <= 4096 && max_logM <= 16) {
        F.w = { PRE_W16, NB, 256, (size_t)F.pre_cap * 12 + 64, true };
    } else if (a.int_sparse) {
        // the reference's prelude over the VALUE range, from the rank-space model (16-byte entries: always16) and the block's values
        // LDS from the call's most distinct values per block (max_ns: read back by model_exact, the discovery path) unless a block's
        // code outgrew three words per value on the first attempt
        const bool full = a.sp_full_lds;
        F.sp_cap = full ? (u32)ANSX_SP_MAX_SIGMA : std::min<u32>(ANSX_SP_MAX_SIGMA, (std::max<u32>(max_ns, 64u) + 63u) & ~63u);
        F.sp_bits = full ? (u32)ANSX_SP_MAX_SIGMA
                         : (dbg.test_sp_bits ? dbg.test_sp_bits : std::min<u32>(ANSX_SP_MAX_SIGMA, 2u * F.sp_cap + 64u));
        F.w = { PRE_RANK_SPACE, NB, 256, (size_t)(F.sp_cap + F.sp_bits + 2) * 4, true };
    } else {
        const size_t gen_lds = (size_t)F.pre_cap * 8 + 64;
        if (gen_lds > LDS_BUDGET) F.w = { PRE_GENERIC_HBM, NB, 256, 64, false };  // f = 6, 7: the writer's two arrays in HBM
        else F.w = { PRE_GENERIC, NB, 256, gen_lds, gen_lds > LDS_NO_ATTRIBUTE };
    }
    return F;
}

// ------------------------------------------------------------------------------------------ the encoder
// K5.  The integer-state encoder (k_encode<0>, 16-byte table entries) takes frames above 2^16 and scratch slots too far
// apart for 31-bit buffer offsets.  The f64-state forms (frames <= 2^16, every block's alphabet <= max_ns) are three
// kernels that share the call's blocks:
//   k_encode_pc   producer / consumer wave pairs, 16 x pairs blocks per workgroup, where that form wins: (A) chip-filling calls
//                 whose tables fit 64 to a CU (four pairs, S = 8) -- BASELINE config 2; (B) alphabets too large for that whose
//                 tables fit at 32 (two pairs, S = 4: every entry in LDS, two rounds, each wave alone on its SIMD) -- BASELINE
//                 config 3; (C) short lists (one pair per workgroup, at most two per CU).  It takes ALL blocks of the call: the
//                 last workgroup pads itself with neutral steps (blocks that do not exist, the partial last block)
//   k_encode<1>   one wave per 16 blocks, 4-byte LDS entries: geometries the pair kernel does not take
//   k_encode<2>   compact tables in HBM with the hottest 1151 symbols per block in LDS: alphabets that fit neither
enum { ENC_INT_STATE = ANSX_ENC_INT_STATE, ENC_MODE1 = ANSX_ENC_MODE1, ENC_MODE2 = ANSX_ENC_MODE2 };
enum { PC_NONE = ANSX_PC_NONE, PC_A = ANSX_PC_A, PC_B = ANSX_PC_B, PC_C = ANSX_PC_C };
struct EncoderForm {
    bool f64;
    int criterion;      // PC_*: the criterion that chose the pair kernel; pc.grid == 0 where its restart rule then refused it
    u32 pairs, S, rowwords;
    Launch pc;          // variant: S
    u32 first;          // blocks the pair launch took
    Launch rest;        // variant: ENC_*; grid == 0: nothing left
    u32 lds_stride;     // words per table row of `rest`
};
static inline EncoderForm choose_encoder_form(const EncGeo& g, const EncKeys& dbg, u32 num_cus, u32 max_logM, u32 max_ns)
{
    EncoderForm E = {};
    const u32 NB = g.nblocks;
    const u64 scr_stride = scratch_stride(g);
    E.f64 = max_logM <= 16 && scr_stride * 16 < 0x7FFFFF00ull && !dbg.table16_fixup && !dbg.encode_gtab16;
    if (!E.f64) {
        E.rest = { ENC_INT_STATE, (u32)(((size_t)NB * 4 + 63) / 64), 64, 0, false };
        return E;
    }
    const u32 ns_entries = max_ns;
    const u32 lds_stride = ns_entries | 1u;  // odd stride spreads the 16 tables over the banks
    const size_t enc_lds = (size_t)16 * lds_stride * 4;
    const bool mode1 = enc_lds <= LDS_ENC_MODE1 && !dbg.encode_mode2;
    // ---- producer / consumer pairs
    E.rowwords = ((ns_entries + 2u) / 2u) | 1u;  // ns_entries + 1 running sums of 16 bits, an odd number of words per row
    const u32 full_blocks = (u32)(g.n / g.block_ints);
    const u32 enc_waves_all = (NB + 15) / 16;
    auto pc_lds = [&](u32 pairs, u32 S) { return (size_t)pairs * 16 * E.rowwords * 4 + (size_t)pairs * (2 * S * 1024 + (S == 8 ? 16 * 144 : 0)); };
    // (block_ints <= 2^22: the stand-in for a neutral step of a 2^16 frame lets the state creep by 2^-16 per step, see the kernel)
    // (a batch pass: its blocks are not block_ints apart in the input -- k_encode<MODE> reads them through the per-block table)
    const bool pc_geo = !dbg.no_pc && !g.batch_pass && g.block_ints % 128u == 0 && g.block_ints <= (1u << 22) && scr_stride * 16 < 0x40000000ull;
    if (pc_geo && (!dbg.no_pc_auto || dbg.use_pc || dbg.force_pc) && mode1 && pc_lds(4, 8) <= LDS_WORKGROUP
        && (((NB + 63) / 64) * 2 >= num_cus || dbg.force_pc))
        E.criterion = PC_A, E.pairs = 4, E.S = 8;  // (A) the chip-filling form: 0.66 against k_encode<1>'s 0.71 ms on the headline workload since the
                                                   // producer loads its inputs 16 bytes at a time (equal before that)
    else if (pc_geo && !mode1 && pc_lds(2, 4) <= LDS_WORKGROUP && (full_blocks >= 32 || dbg.force_pc) && !dbg.no_pc_auto)
        E.criterion = PC_B, E.pairs = dbg.pc_b_pairs, E.S = 4;  // (B) every table entry in LDS, two rounds
    else if (pc_geo && mode1 && enc_waves_all <= 2u * num_cus && (full_blocks >= 16 || dbg.force_pc) && !dbg.no_pc_auto)
        E.criterion = PC_C, E.pairs = 1, E.S = 8;  // (C) short lists: the call waits for one wave's state chain, and the consumer's is 20 % shorter.
                                                   // (Lists of fewer than 16 full blocks stay with k_encode<1>, which walks a short block's own steps only.)
    if (E.pairs && (g.ckpt == 0 || g.ckpt % (4u * E.S) == 0)) {
        const u32 wgs = (NB + 16 * E.pairs - 1) / (16 * E.pairs);
        E.pc = { (int)E.S, wgs, 128 * E.pairs, pc_lds(E.pairs, E.S), true };
        E.first = wgs * 16 * E.pairs;
        if (E.first >= NB) return E;
    }
    const u32 enc_waves = (NB - E.first + 15) / 16;
    u32 wpw = (enc_waves + num_cus - 1) / num_cus;
    wpw = wpw < 1 ? 1 : (wpw > 4 ? 4 : wpw);
    const u32 enc_grid = (enc_waves + wpw - 1) / wpw;
    if (mode1) {
        // ---- one wave per 16 blocks.  Waves of one workgroup run the main loop in step (a barrier per super-batch): up to four
        // waves per workgroup -- one per SIMD of a CU -- as soon as there are that many waves per CU (see k_encode)
        E.rest = { ENC_MODE1, enc_grid, 64 * wpw, wpw * enc_lds, wpw * enc_lds > LDS_NO_ATTRIBUTE };
        E.lds_stride = lds_stride;
    } else {
        // ---- alphabets too large for LDS: compact table entries from HBM, same branch-free f64 step
        const size_t lds2 = (size_t)wpw * 16 * ANSX_ENC_HOT * 4;
        E.rest = { ENC_MODE2, enc_grid, 64 * wpw, lds2, lds2 > LDS_NO_ATTRIBUTE };
        E.lds_stride = ANSX_ENC_HOT;
    }
    return E;
}

// ------------------------------------------------------------------------------------------ what the call reports
// ansx_last_encode_form: each phase copies the form it launched with into the attempt's report (ansx.hip: EncodeOutcome).
// Assignments only -- no chooser is asked here.
static inline void report_attempt(ansx_encode_form_report& r, const EncGeo& g, const EncAttempt& a, bool fused)
{
    r.attempt = (a.ns_cap ? ANSX_FORM_OPTIMISTIC : 0u) | (fused ? ANSX_FORM_FUSED : 0u) | (a.int_sparse ? ANSX_FORM_RANK_SPACE : 0u)
        | (a.int_sparse && a.sp_full_lds ? ANSX_FORM_SP_FULL_LDS : 0u) | (g.batch_pass ? ANSX_FORM_BATCH_PASS : 0u);
    r.ns_cap = a.ns_cap, r.nt = a.nt, r.nblocks = g.nblocks;
    // (until a phase says otherwise: the kernels of these stages did not run)
    r.hist = ANSX_HIST_NONE, r.sort = ANSX_SORT_NONE, r.fin = ANSX_FIN_NONE, r.prelude = ANSX_PRE_NONE, r.enc = ANSX_ENC_NONE;
}
// last_cand: the chain count of the last k_candidates launch (fast only); big_geo: the table for alphabets above 4096 slots
static inline void report_model(ansx_encode_form_report& r, const ModelForm& M, u32 last_cand, bool big_geo)
{
    if (M.fast) r.attempt |= ANSX_FORM_FAST_MODEL;
    r.hist = (u32)M.hist.variant, r.cpb = M.cpb, r.h_deferred = M.h_deferred, r.h_in_hist = M.h_in_hist;
    r.sort = (u32)M.sort.variant;
    r.fin = M.fast ? (u32)M.fin.variant : (u32)ANSX_FIN_NONE, r.fcap = M.fast ? M.fcap : 0u;
    r.cand_chains = M.fast ? last_cand : 0u;
    r.nranges = M.nranges, r.range_blocks = M.range_blocks, r.big_geo = big_geo;
}
static inline void report_remap(ansx_encode_form_report& r, const RemapForm& R, bool pa_ran)
{
    r.rf = (u32)R.rf, r.rf_slots = R.rf_slots;
    r.pa_small = pa_ran && R.pa_small, r.pa_slots = pa_ran ? R.pa_slots : 0u, r.pa_uqcap = pa_ran ? R.pa_uqcap : 0u;
}
static inline void report_prelude(ansx_encode_form_report& r, const PreludeForm& F)
{
    r.prelude = (u32)F.w.variant, r.table16_first = F.table16_first, r.pre_cap = F.pre_cap;
}
static inline void report_encoder(ansx_encode_form_report& r, const EncoderForm& E)
{
    r.enc = E.rest.grid ? (u32)E.rest.variant : (u32)ANSX_ENC_NONE;
    r.enc_grid = E.rest.grid, r.enc_threads = E.rest.threads, r.enc_lds = (u32)E.rest.lds;
    r.criterion = (u32)E.criterion, r.pairs = E.pairs, r.S = E.S, r.pc_grid = E.pc.grid, r.first = E.first;
}

}  // namespace ansx_enc
