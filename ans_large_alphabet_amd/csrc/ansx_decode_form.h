// ansx -- the form of a decode call ("Host path of decode"): which prelude parser and which block
// decoder run, and in what launch shape, from the container's header bounds, the geometry and the debug overrides.
// Pure host arithmetic like ansx_plan.h: no context, no stream, no device pointer, so it builds with a plain host
// compiler and is swept on the CPU (tests/tools/decode_form_check.cpp) against the kernels' LDS carves.  The LDS
// constants the kernels and this header share are in ansx_plan_types.h.
#pragma once
#include "../../include/ansx.h"
#include "ansx_plan_types.h"

#include <algorithm>

namespace ansx_form {

static inline size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What the chooser reads of the geometry, the codec-dependent sizes worked out by the caller (they hang on helpers the
// kernels share: geo_nseg, fold_T, block_bound).
struct FormGeo {
    u64 n;               // ints of the container
    u32 block_ints, nblocks, ckpt;
    u32 kind, pa;        // ANSX_FOLD .. ANSX_INT; 1: compacted
    u32 nseg;            // geo_nseg(block_ints, ckpt): decoder segments of a full block
    u32 mf_bytes;        // ANSrfold: bytes of a block's most-frequent table (4 fold_T), else 0
    size_t block_bound;  // the codec's worst-case block stream (block_bound without the compaction layer)
};

// The debug overrides the chooser reads (the context's DebugOpts has them under the same names).
struct FormKeys {
    bool parse_generic = false, parse_win = false, parse_fast = false;
    u32 parse_stage_words = 0;
    bool setup_old = false;
    bool decode_table = false, no_stream_lds = false;
    int decode_mode = 0;        // 0 auto, 1 "ring", 2 "staged"
    int decode_pair = 0;        // 0 auto, 1 "never", 2 "always"
    int decode_small_ring = 0;  // 0 auto, 1 "never", 2 "always"
    u32 pair_lds_limit = 0;
};

// Which subtree form k_parse_prelude_par runs, from header fields only: a depth-3 subtree has at most max_ns >> 3
// items; its value array (two sentinels more) and ANSX_PAR_STK stack rows must fit the 48 rows behind the staged words.
// 1: u16 elements (every value fits: frame + alphabet + 3 <= 65535), 2: u32 elements, 0: the windowed form.
static inline int ansx_par_form(u32 max_ns, u32 maxM)
{
    const size_t room = (size_t)(48 - ANSX_PAR_STK) * 64 * 4;
    const size_t elems = (size_t)(max_ns >> 3) + 2;
    if ((u64)maxM + max_ns + 3 <= 65535u && elems * 64 * 2 <= room) return 1;
    if (elems * 64 * 4 <= room) return 2;
    return 0;
}

// What the form of a decode depends on besides the geometry and the debug overrides: bounds from the container's header
// (for a single reference stream: from the peek at its first bytes).
struct DecodeBounds {
    u32 maxM, max_ns;     // the largest frame; the bound on a block's symbol indices
    u32 max_ep;           // the bound on the symbols PRESENT in a block (<= max_ns): the rank / select decoder keeps one
                          // 8-byte entry per present symbol, so this -- not max_ns -- sizes its LDS
    bool hinted;          // the container carries parse hints (a single stream has none)
    u64 payload_bytes;    // bytes of all block streams (per int of the list: how lean the streams are)
    u32 max_block_bytes;  // the largest block stream -- only the index knows it (k_validate_index) -- or 0: not looked up
};

// (the values of the public ansx_parser / ansx_decoder, which ansx_last_decode_stats reports)
enum { PARSE_DONE = ANSX_PARSER_DONE, PARSE_GENERIC = ANSX_PARSER_GENERIC, PARSE_PAR = ANSX_PARSER_PAR, PARSE_FAST = ANSX_PARSER_FAST,
    PARSE_WIN = ANSX_PARSER_WIN };  // PARSE_DONE: k_int_sparse_parse has filled the tables
// the k_decode_rank family (in the order of its RING parameter, then the pair kernel) and the two table forms of k_decode
enum { DEC_STAGED = ANSX_DECODER_STAGED, DEC_RING = ANSX_DECODER_RING, DEC_SMALL_RING = ANSX_DECODER_SMALL_RING, DEC_PAIR = ANSX_DECODER_PAIR,
    DEC_TABLE = ANSX_DECODER_TABLE, DEC_GTAB = ANSX_DECODER_GTAB };  // DEC_GTAB: needs the HBM slot table (dec_s2s)
struct LaunchShape {
    u32 grid, threads;
    size_t lds;
};
struct DecodeForm {
    bool needs_index;  // the decoder hangs on the largest block stream and the bounds do not have it: only the parser is
                       // filled in, ask again with max_block_bytes measured
    int parser;        // K7 ...
    u32 p_variant;     // ... PARSE_PAR: the subtree form (ansx_par_form), PARSE_WIN: staged words per lane, PARSE_FAST: stage_words
    int decoder;       // K8
    LaunchShape p, d;
    u32 stream_cap;  // DEC_STAGED and the table forms: bytes of LDS a block's stream is staged in, 0 = read from HBM
};

// The one place that decides which parser and which decoder a decode call runs, and in what launch shape.  Pure: no HIP
// call, nothing of the context but its overrides and the chip's CU count.
static inline DecodeForm choose_decode_form(const FormGeo& g, const DecodeBounds& B, const FormKeys& dbg, u32 num_cus)
{
    DecodeForm F = {};
    const u32 maxM = B.maxM, max_ns = B.max_ns;
    // K7.  Containers carry parse hints (bit offsets of the top subtrees of every block's interpolative code):
    // eight lanes per block, k_parse_prelude_par.  Without hints (single-stream mode) or on request one lane
    // per block: the windowed parser (any alphabet / frame size; ANSX_PARSE_WIN), the older E-array fast loop
    // (ANSX_PARSE_FAST: 16-bit values, up to ~880 symbols) or the generic kernel (ANSX_PARSE_GENERIC) --
    // all four are cross-checked in the tests.
    const size_t pf_lds = std::max<size_t>(20480, rup(((size_t)max_ns + 2) * 128, 16)) + (size_t)ANSX_PF_SW * 64 * 4 + 21 * 64 * 4;
    F.p = { (g.nblocks + 63) / 64, 64, 0 };
    if (g.kind == ANSX_INT && !g.pa) {
        F.parser = PARSE_DONE;
    } else if (dbg.parse_generic) {
        F.parser = PARSE_GENERIC;
    } else if (B.hinted && !dbg.parse_win && !dbg.parse_fast) {
        // Subtree form: value arrays (u16 / u32 elements) where a depth-3 subtree's array fits the slice the windowed
        // form needs anyway, from header fields only; otherwise, or with ANSX_DECODE_SETUP=old, the windowed form.
        F.parser = PARSE_PAR;
        F.p_variant = dbg.setup_old ? 0 : ansx_par_form(max_ns, maxM);
        // Waves per workgroup (each wave works alone on its own LDS slice): measured on MI355X at 16384 blocks,
        // windowed form: 530-symbol tables 1/2/3/4 waves -> 0.161/0.162/0.109/0.122 ms, 2300-symbol tables
        // 0.275/0.273/0.286/0.252; value-array form (event-timed, so ~0.005 above the kernel's own time): 526-symbol
        // tables 0.062/0.062/0.068/0.056, 257-symbol tables 0.045/0.042/0.048/0.039.
        const u32 par_waves = (g.nblocks + 7) / 8;
        const u32 pw_max = (F.p_variant != 0 || max_ns > 1024) ? 4u : 3u;
        const u32 pw = std::min<u32>(pw_max, std::max<u32>(1u, (par_waves + num_cus - 1) / num_cus));
        F.p = { (par_waves + pw - 1) / pw, 64 * pw, (size_t)pw * ANSX_PAR_SLICE_WORDS * 4 };
    } else if (dbg.parse_fast && (u64)maxM + max_ns + 3 <= 65535u && pf_lds <= 150 * 1024) {
        F.parser = PARSE_FAST;
        F.p_variant = ANSX_PF_SW;
        if (dbg.parse_stage_words >= 2 && dbg.parse_stage_words <= ANSX_PF_SW)  // tests: force the fast loop's in-kernel fallback
            F.p_variant = dbg.parse_stage_words & ~1u;
        F.p.lds = pf_lds;
    } else {
        F.parser = PARSE_WIN;
        F.p_variant = max_ns <= 1024 ? 128 : 256;  // (preludes of a few hundred bytes: 128 staged words per lane)
        F.p.lds = (size_t)(F.p_variant + 72) * 64 * 4;
    }
    // K8
    const u32 nseg = g.nseg;
    F.d.grid = g.nblocks;
    F.d.threads = std::min<u32>(256u, (u32)rup((size_t)nseg * 4, 64));
    const size_t LDS_LIMIT = 150 * 1024;
    // normal path: rank/select tables (frames up to 2^16), staged stream while >= 3 WGs/CU still fit
    const size_t rs_tables = rup((size_t)(maxM >= 32 ? maxM / 32 : 1) * 8, 16) + 2 * rup((size_t)B.max_ep * 4, 16) + ANSX_DEC_SCRATCH;
    const bool rank_form = maxM <= 65536u && rs_tables <= LDS_LIMIT && !dbg.decode_table;
    // per-quad stream rings when every segment of a full block has the same length; the (at
    // most one) partial block of the container then reads its stream straight from HBM
    // (measured on MI355X, 256 Mi ints: rings 0.73 vs 0.76 ms at 16 Ki / 1024, 0.73 vs 1.85 ms at
    // 64 Ki / 1024 where the stream no longer fits; staged 0.60 vs 0.69 ms at 16 Ki / 512 -- the
    // ring bookkeeping costs ~6 VALU per step, so it only pays when it frees a lot of LDS)
    const size_t ring_lds = (size_t)(F.d.threads / 4) * ANSX_RING_STRIDE + 16;  // + alignment slack
    const bool ring_ok = g.ckpt != 0 && g.block_ints % g.ckpt == 0 && g.ckpt % 4 == 0 && rs_tables + ring_lds <= 60 * 1024;
    const int force = dbg.decode_mode;  // tests: 1 "ring" | 2 "staged"
    // The ring decoder needs nothing from the index, so a container it could decode is never held up for one (no
    // validation kernel, no read-back): whether rings pay there, and the staging of the staged form if they do not, go
    // by the codec's worst-case block stream.  Every other form sizes its LDS from the largest block stream.
    const bool index_free = rank_form && ring_ok && force != 2 && !g.pa;
    if (!B.max_block_bytes && !index_free) {
        F.needs_index = true;
        return F;
    }
    const size_t block_bytes = B.max_block_bytes ? B.max_block_bytes : std::min<size_t>(0x7FFFFFFFu, g.block_bound);
    const size_t want_stream = rup(block_bytes + 32, 16);
    size_t tables = rs_tables;  // what the form keeps in LDS besides a staged stream
    if (rank_form) {
        // large tables (alphabets of thousands of symbols: one wave per block, a handful of waves per CU either
        // way): rings, 1.33 vs 2.08 ms on 2300-symbol alphabets -- the staging pass is pure latency there
        const bool staged_fits = rs_tables + want_stream <= 52 * 1024;
        const bool ring_pays = !staged_fits || rs_tables >= 12 * 1024 || 10 * (rs_tables + want_stream) > 16 * (rs_tables + ring_lds);
        if (ring_ok && (force ? force == 1 : ring_pays)) {
            // two blocks per workgroup, decoded in one instruction stream (k_decode_rank2): as long as four such workgroups
            // still fit a CU's LDS; the container's last one or two blocks take the single-block code inside that kernel
            const size_t lds2 = rup((size_t)(maxM >= 32 ? maxM / 32 : 1) * 16, 16) + 4 * rup((size_t)B.max_ep * 4, 16) + ANSX_DEC_SCRATCH + 2 * ring_lds;
            const int pair = dbg.decode_pair;  // tests / experiments: 1 never, 2 always (LDS permitting)
            // Streams of a few bytes per step (the container's bytes per int, header fields only): the 256-byte speculative
            // rings -- sixteen instead of ten blocks of the headline workload per CU; an interval that outran its window is
            // decoded again (dec_segments_ring_small), so a wrong guess here costs time, never correctness.
            const int small = dbg.decode_small_ring;  // tests: 1 never, 2 always
            const bool lean = g.n != 0 && (double)B.payload_bytes / (double)g.n <= 2.0 && g.ckpt % 16 == 0;
            if (pair != 1 && g.nblocks >= 2 && (pair == 2 ? lds2 <= 150 * 1024 : lds2 <= dbg.pair_lds_limit)) {
                F.decoder = DEC_PAIR;
                F.d.grid = (g.nblocks + 1) / 2;
                F.d.lds = lds2;
            } else if (small != 1 && (small == 2 || lean)) {
                F.decoder = DEC_SMALL_RING;
                F.d.lds = rs_tables + (size_t)(F.d.threads / 4) * ANSX_SRING_STRIDE + 16;
            } else {
                F.decoder = DEC_RING;
                F.d.lds = rs_tables + ring_lds;
            }
            return F;
        }
        F.decoder = DEC_STAGED;
        if (!staged_fits || dbg.no_stream_lds) {
            F.d.lds = rs_tables;
            return F;
        }
    } else {
        // frames above 2^16 (or forced): slot -> symbol table form, in LDS if it fits, else in HBM
        const size_t mfb = g.mf_bytes;
        tables = rup(((size_t)max_ns + 2) * 4, 16) + rup((size_t)maxM * 2, 16) + mfb;
        F.decoder = tables <= LDS_LIMIT ? DEC_TABLE : DEC_GTAB;
        if (F.decoder == DEC_GTAB) tables = mfb;
        if (tables + want_stream > 52 * 1024) {
            F.d.lds = std::max<size_t>(tables, 16);
            return F;
        }
    }
    F.d.lds = tables + want_stream;
    F.stream_cap = (u32)want_stream;
    return F;
}

}  // namespace ansx_form
