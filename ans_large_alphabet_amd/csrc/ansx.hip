// ansx — host side of the C-ABI (include/ansx.h): context, device workspace, launch sequences.
// Everything that computes runs in the HIP kernels of ansx_kernels.h / ansx_rfold.h; there is no
// CPU fallback: if no gfx950 device is usable, ansx_init fails with ANSX_ERR_NO_DEVICE.
#include "../../include/ansx.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the library itself is resolved at first use (ansx_gather_containers)

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "ansx_kernels.h"
#include "ansx_rfold.h"
#include "ansx_model.h"
#include "ansx_fastmodel.h"
#include "ansx_gen.h"
#include "ansx_pa.h"
#include "ansx_intsparse.h"
#include "ansx_ranges.h"
#include "ansx_batch.h"
#include "ansx_batchranges.h"
#include "ansx_encbatch.h"
#include "ansx_sums.h"
#include "ansx_rangesums.h"
#include "ansx_nextgeq.h"
#include "ansx_intersect.h"
#include "ansx_intersect_batch.h"
#include "ansx_union.h"
#include "ansx_bool.h"
#include "ansx_topk.h"
#include "ansx_topk_bool.h"
#include "ansx_topk_query.h"
#include "ansx_topk_scored.h"
#include "ansx_facet.h"
#include "ansx_filter.h"
#include "ansx_batchrangesums.h"
#include "ansx_batchnextgeq.h"
#include "ansx_batchdevranges.h"
#include "ansx_plan.h"  // the host's plans of the random-access calls, Layout, BatchSrc, rup
#include "ansx_decode_form.h"  // the form of a decode call: parser, decoder, launch shapes
#include "ansx_encode_form.h"  // the forms of an encode attempt: model, remap, prelude writer, encoder

using namespace ansx_plan;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct ProfRec {
    std::string name;
    hipEvent_t e0, e1;
};

}  // namespace

// Header of the last container decoded per shape (kind, fidelity, n, bytes): the next decode of that shape is launched
// on it without waiting for the header to come back, and a one-thread kernel compares it with the real one
// (k_check_header).  64 shapes; the OLDEST remembered one (insertion order) makes room, never the one being stored.
struct HeaderCache {
    typedef std::array<u64, 4> Key;
    const ansx_container_header* find(const Key& k) const { return map.count(k) ? &map.find(k)->second : nullptr; }
    void forget(const Key& k) { map.erase(k); }  // (its place in `order` lingers: remember() drops it)
    void remember(const Key& k, const ansx_container_header& H)
    {
        if (!map.count(k)) {
            order.erase(std::remove(order.begin(), order.end(), k), order.end());
            order.push_back(k);
            for (; order.size() > 64; order.pop_front()) map.erase(order.front());
        }
        map[k] = H;
    }
    void clear() { map.clear(), order.clear(); }

private:
    std::map<Key, ansx_container_header> map;
    std::deque<Key> order;  // keys of map, oldest first
};

// The pinned page every read-back of a few words lands in (ansx_ctx::pin).  The flag words serve every call; behind them
// each entry point has its own fields, at offsets that keep the fields of one call apart.
struct PinPage {
    u32 flags[16];  // bytes 0..63: the device's flag words (ANSX_G_*) with the result, a 64-bit payload size, in words 4, 5
    union {
        struct {  // a decode call
            union {
                ansx_container_header hdr;  // 64: the container's header (fetched or remembered; range_source: the source's)
                struct {     // 64: a single reference stream: its first bytes, those behind a most-frequent table,
                    u8 peek[16], peek_rf[16];  // and the two index entries of its one block (an upload)
                    u64 index[2];
                } plain;
            };
            u8 pad0[2048 - 64 - 64];
            u32 caller_flag;  // 2048: the flag word of decode_dev's caller (sub_decode), read back by its epilogue
            u8 pad1[1024 - 4];
            u64 planner[8];  // 3072: the scalars of the device planner (decode_device_ranges)
            u64 isect_total;  // 3136: the members an intersect step found, read back by the decode's epilogue
            u32 isect_sflag;  // 3144: the flag word of the scan behind a whole-list decode to ids (decode_ids)
        };
        u8 part_hdr[63][64];                       // 64: ansx_merge_containers_dev, the headers of up to 63 parts
        u64 rank_sizes[2 * ANSX_MERGE_MAX_PARTS];  // 64: ansx_gather_containers, (bytes, slot_bytes) of every rank
    };
};
static_assert(sizeof(PinPage) == 4096 && offsetof(PinPage, plain.index) == 96 && offsetof(PinPage, caller_flag) == 2048
        && offsetof(PinPage, planner) == 3072,
    "the pinned page is one 4096-byte allocation (ansx_init) and its fields keep their places");

struct ansx_ctx {
    u32 num_cus = 256;
    int device = 0;
    hipStream_t stream = nullptr;
    int last_hip = 0;
    bool profile = false;
    std::vector<ProfRec> recs;
    std::map<std::string, std::pair<double, u64>> acc;
    std::vector<std::string> order;
    DevBuf pre_work;  // f = 6, 7: off[] and bit buffer of the generic prelude writer
    DevBuf hist, hterm, sortF, sortSym, attS, prevS, attMeta, blk, table, tab32, scratch, misc, mapped, mostfreq,
        stage_in, stage_out, dec_s2s, dec_cum, dec_info, plain, rf_tmp, log2lut, pa_alpha, pa_info, pairs, lg2i, sizes, nearlist, force;
    DevBuf rng_plan, rng_cont, rng_list;  // ansx_decode_ranges_dev: flags + block list + range pieces, sub-container, its ints
    DevBuf rng_dev;                       // ansx_decode_device_ranges_dev: the device planner's workspace
    DevBuf bat_hdr;                       // ansx_decode_batch_dev: input addresses and headers of the batch
    DevBuf enb_plan, enb_wc;              // ansx_encode_batch_dev: a pass's plan and results; its restart points and hints (work area)
    DevBuf isect_ids;                     // ansx_intersect_dev: the driver's ids and the survivors of a step, two arrays of n_driver ints
    DevBuf isectb_ids, isectb_work;       // ansx_intersect_batch_dev, ansx_union_batch_dev: a group's ids and two candidate buffers; its tables, segments and IsectWork
    u8* isectb_pin = nullptr;             // ... and the pinned host image of its tables (rng_pin belongs to the decode's
    size_t isectb_pin_cap = 0;            //     passes and the scan, whose uploads are under way when the tables go up)
    DevBuf sums_plan, sums_ints;          // running sums and gaps: flag word + list starts + tile aggregates and carries; the gaps of a call (4 bytes per int)
    u8* rng_pin = nullptr;                // ... and the pinned host image of rng_plan (an asynchronous upload from
    size_t rng_pin_cap = 0;               //     pageable memory is staged by the runtime: 0.666 -> 0.618 ms at 4096 ranges)
    PinPage* pin = nullptr;
    // Largest alphabet (max_sym + 1) seen per (kind, fidelity, block_ints): sizes the LDS of the fused
    // model kernel and of the LDS-table encoder without a mid-call round trip (see encode_dev).
    std::map<u64, u32> ns_hint;
    std::map<u64, u32> rf_hint;  // rfold: most distinct values per block seen per geometry (optimistic hash-table size)
    HeaderCache hdrs;
    std::map<u32, DevBuf> geo;   // tree nodes of the interpolative code per alphabet size, tabulated per symbol-array size (<= 4096)
    DevBuf geo_big;              // the same for alphabets up to geo_big_cap symbols (symbol arrays above 4096 slots, fast model path:
    u32 geo_big_cap = 0;         //   sized from the geometry's alphabet hint, cap^2 * 4 bytes -- 284 MB for fidelity 5 on 2^20-valued lists)
    std::map<u32, u32> impact_wgs;  // k_topk_impacts, staged: the workgroups the chip holds, per (uint4 per lane, rows in LDS)
    std::map<u32, u32> facet_wgs;   // k_facet_count, lds: the workgroups the chip holds, per (values in LDS, combining or not)
    int last_gather_ranks = 0;   // ranks of the communicator the last ansx_gather_containers call ran on (ncclCommCount)
    std::set<u64> wide_hint;     // geometries that met a frame above 2^16: wide restart points from the start
    std::map<u64, u32> t_hint;   // largest chosen candidate index t (frame M0 * 2^t) + 1 seen per geometry: lanes per block of k_candidates
    std::set<u64> int_sparse_hint;  // plain-ANSint geometries whose values outgrew the dense 16384-symbol model: rank space from the start
    // ansx_encode_batch_dev learns in a slot of its own: the five hint sets above are exchanged with these for the
    // length of a batch call (EncBatchHints), so nothing a batch sees reaches a later ansx_encode_dev and vice versa
    struct {
        std::map<u64, u32> ns_hint, rf_hint, t_hint;
        std::set<u64> wide_hint, int_sparse_hint;
    } bat;
    ansx_encode_stats last = {};
    ansx_encode_form_report last_form = {};  // the forms of the most recent encode attempt whose container was returned (ansx_last_encode_form)
    ansx_decode_stats last_dec = {};  // the form of the most recent decode attempt that ran to its end (ansx_last_decode_stats)
    // Block-range pipeline of the fast model path (model_fast): two side streams and the events of its fork and join,
    // created by the first call that needs them (pipeline_prepare) and destroyed with the context, never per call.
    hipStream_t pipe_stream[2] = { nullptr, nullptr };
    std::vector<hipEvent_t> pipe_ev;  // [0], [1]: a side stream has finished its ranges; [2 + k]: the histogram of range k is done
    // Path-selection overrides for tests and experiments (every path must give identical bytes).
    // Taken from the environment ONCE in ansx_init, changed afterwards only through ansx_debug_set;
    // the per-call hot path never looks at the environment.
    struct Dbg {
        bool table16_fixup = false;   // ANSX_TEST_TABLE16_FIXUP: integer-state encoder fed by k_table16_from32
        bool encode_gtab16 = false;   // ANSX_ENCODE_GTAB16: force the 16-byte-entry integer-state encoder
        bool parse_generic = false;   // ANSX_PARSE_GENERIC: generic prelude parser kernel
        bool parse_win = false;       // ANSX_PARSE_WIN: one lane per block, windowed parser (ignores the parse hints)
        bool parse_fast = false;      // ANSX_PARSE_FAST: one lane per block, E-array fast loop where it applies
        bool decode_table = false;    // ANSX_DECODE_TABLE: slot -> symbol decoder tables
        bool no_stream_lds = false;   // ANSX_NO_STREAM_LDS: staged decoder reads the stream from HBM
        int decode_mode = 0;          // ANSX_DECODE_MODE: 0 auto, 1 "ring", 2 "staged"
        u32 parse_stage_words = 0;    // ANSX_PARSE_STAGE_WORDS: 0 = default
        bool model_fused = false;     // ANSX_MODEL_FUSED: the single LDS-resident model kernel instead of the five tailored ones
        bool model_sync = false;      // ANSX_MODEL_SYNC: always discover the alphabet with the mid-call read-back
        bool use_pc = false;          // ANSX_USE_PC: k_encode_pc's chip-filling shape even under ANSX_NO_PC_AUTO
        u32 pc_b_pairs = 2;           // ANSX_PC_B_PAIRS: pairs per workgroup of shape B (2: one workgroup per CU -- 1.04 ms on BASELINE config 3;
                                      // 1: two workgroups per CU, whose waves the dispatcher does not spread as evenly -- 1.21 ms)
        u32 test_sp_bits = 0;         // ANSX_TEST_SP_BITS: words of the sparse ANSint prelude writer's bit buffer on the first attempt (tests: forces its repeat)
        bool fin_one_wave = false;    // ANSX_FIN_ONE_WAVE: k_model_finish with one wave per block (alphabets up to 1024 slots)
        bool no_big_geo = false;      // ANSX_NO_BIG_GEO: no tabulated tree geometry for alphabets above 4096 slots
        bool no_pc_auto = false;      // ANSX_NO_PC_AUTO: never choose the pair kernel by itself (criteria A, B, C of choose_encoder_form)
        bool encode_mode2 = false;    // ANSX_ENCODE_MODE2: the compact-table encoder (k_encode<2>) even where the tables fit LDS (tests)
        bool force_pc = false;        // ANSX_FORCE_PC: the pair kernel for every workgroup of 64 full blocks, however few (tests)
        bool no_pc = false;           // ANSX_NO_PC: the LDS-table encoder as one wave per 16 blocks everywhere (k_encode<1>), no producer / consumer pairs
        int decode_small_ring = 0;    // ANSX_DECODE_SMALL_RING: "never" / "always" (default: by the container's bytes per int)
        bool chain_old = false;       // ANSX_MODEL_CHAIN=old: every block of k_model_finish reads and raises the call's running maxima itself (no k_model_maxima launch)
        bool setup_old = false;       // ANSX_DECODE_SETUP=old: windowed subtrees in k_parse_prelude_par, scan form of the decoder's table build
        int decode_pair = 0;          // ANSX_DECODE_PAIR: "0"/unset auto, "never", "always" (k_decode_rank2: two blocks per workgroup)
        u32 pair_lds_limit = 0;       // ANSX_DECODE_PAIR_LDS: auto uses the pair kernel up to this many bytes of LDS per workgroup (0: never --
                                      // measured SLOWER than one block per workgroup, 0.77-0.79 vs 0.72 ms on the headline workload)
        u32 wide_at = 16;             // ANSX_TEST_WIDE_AT: frames above 2^this need wide restart points (tests lower it to force the repeat)
        bool wide_restart = false;    // ANSX_WIDE_RESTART: 36-byte restart points (the v2 form) in every container
        u32 ns_hint = 0;              // ANSX_NS_HINT: alphabet hint for every call (0 = learn per geometry)
        u32 t_hint = 0;               // ANSX_T_HINT: candidates per block for every call (0 = learn per geometry)
        bool no_fast_model = false;   // ANSX_NO_FAST_MODEL: optimistic calls keep the exact model kernels
        double near_band = ANSX_NEAR_BAND;  // ANSX_NEAR_BAND: relative band around the stop-rule threshold inside which the host decides (tests widen it)
        bool near_flip = false;       // ANSX_TEST_NEAR_FLIP: the device decides close calls the wrong way (tests: the host must fix them)
        u32 cand_chains = 0;          // ANSX_CAND_CHAINS: 1 | 2 recurrences per lane in k_candidates (0 = by the call's size)
        double fast_guard = ANSX_FAST_GUARD;  // ANSX_FAST_GUARD: relative guard band of the fast model path's stop rule (tests widen it)
        int model_pipeline = 0;       // ANSX_MODEL_PIPELINE: 0 by the call's size, ANSX_PIPE_NEVER, ANSX_PIPE_ALWAYS, or a range count (1 .. ANSX_PIPE_MAX_RANGES)
        u32 batch_pass_blocks = 0;    // ANSX_BATCH_PASS_BLOCKS: blocks per pass of ansx_decode_batch_dev, ansx_decode_batch_ranges_dev and ansx_encode_batch_dev (0 = ANSX_BATCH_PASS_DEFAULT; tests force tiny passes)
        int bool_form = 0;            // ANSX_BOOL_FORM: 0 k_bool_exclude's own rule, 1 "search", 2 "staged" (ANSX_BOOL_FORM_*; tests and the bench tool force one)
        int topk_query_form = 0;      // ANSX_TOPK_QUERY_FORM: 0 k_topkq_should's own rule, 1 "search", 2 "staged" (ANSX_TOPKQ_FORM_*; tests and the bench tool force one)
        int topk_bool_form = 0;       // ANSX_TOPK_BOOL_FORM: 0 the default of k_topkb_match, 1 "search", 2 "bounded" (tests and the bench tool force one)
        int intersect_form = 0;       // ANSX_INTERSECT_FORM: 0 by ANSX_ISECT_FULL_PER_BLOCK, 1 "selective", 2 "full" (tests and the bench tool force one)
        int topk_impact_form = 0;     // ANSX_TOPK_IMPACT_FORM: 0 the default of k_topk_impacts (staged), 1 "global", 2 "staged" (ANSX_IMPACT_FORM_*; tests and the bench tool force one)
        u32 topk_impact_rounds = 0;   // ANSX_TOPK_IMPACT_TILE: 1024 | 2048 | 4096 postings per tile of k_topk_impacts, kept as uint4 per lane (0 = ANSX_IMPACT_ROUNDS_DEFAULT; the bench tool measures all three)
        u32 topk_impact_stage = 0;    // ANSX_TOPK_IMPACT_STAGE: the rows of the table its staged form keeps in LDS, 1 .. ANSX_IMPACT_STAGE_MAX (0 = ANSX_IMPACT_STAGE_ROWS)
        u32 topk_impact_grid = 0;     // ANSX_TOPK_IMPACT_GRID: the most workgroups of its staged form (0 = what the chip holds; tests force a few, so that one walks several tiles)
        int facet_form = 0;           // ANSX_FACET_FORM: 0 the default of k_facet_count (lds where nvalues allows), 1 "atomic", 2 "lds" (ANSX_FACET_FORM_*; tests and the bench tool force one)
        u32 facet_grid = 0;           // ANSX_FACET_GRID: the most workgroups of its lds form (0 = what the chip holds; tests force a few, so that one walks several tiles)
        int filter_form = 0;          // ANSX_FILTER_FORM: 0 the default of the filter step (fused where the group excludes something), 1 "own", 2 "fused" (ANSX_FILTER_FORM_*; tests and the bench tool force one)
        bool facet_no_combine = false;  // ANSX_FACET_NO_COMBINE: its lds form without the wave's combined add (the bench tool measures both)
        u64 isect_batch_ints = 0;     // ANSX_ISECT_BATCH_INTS: the ints a group of ansx_intersect_batch_dev or ansx_union_batch_dev may take (0 = ANSX_ISECT_BATCH_INTS_DEFAULT; tests force small groups)
        u32 range_sums_wg_max = 0;    // ANSX_RANGE_SUMS_WG_MAX: the largest block the one-kernel scan of the range sums takes (0 = ANSX_RS_WG_MAX; the bench tool measures both sides of the switch)
    } dbg;
};
typedef ansx_ctx::Dbg DebugOpts;

namespace {

#define HIPCHK(ctx, call)                                                                        \
    do {                                                                                         \
        hipError_t _e = (call);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            (ctx)->last_hip = (int)_e;                                                           \
            return ANSX_ERR_HIP;                                                                 \
        }                                                                                        \
    } while (0)

int ensure(ansx_ctx* c, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return ANSX_OK;
    if (b.p) {
        hipError_t e = hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
        if (e != hipSuccess) {
            c->last_hip = (int)e;
            return ANSX_ERR_HIP;
        }
    }
    size_t want = bytes + (bytes >> 3) + 4096;  // a little headroom against re-allocation
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        return ANSX_ERR_HIP;
    }
    b.cap = want;
    return ANSX_OK;
}

void prof_begin(ansx_ctx* c, const char* name, hipStream_t s)
{
    if (!c->profile) return;
    ProfRec r;
    r.name = name;
    (void)hipEventCreate(&r.e0);
    (void)hipEventCreate(&r.e1);
    (void)hipEventRecord(r.e0, s);
    c->recs.push_back(r);
}
void prof_end(ansx_ctx* c, hipStream_t s)
{
    if (!c->profile) return;
    (void)hipEventRecord(c->recs.back().e1, s);
}

#define LAUNCH(ctx, name, kern, grid, block, shmem, strm, ...)                                   \
    do {                                                                                         \
        prof_begin(ctx, name, strm);                                                             \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), (shmem), strm, __VA_ARGS__);           \
        prof_end(ctx, strm);                                                                     \
        HIPCHK(ctx, hipGetLastError());                                                          \
    } while (0)

// status of a stream / event call of the block-range pipeline (no early return: its caller still has to join)
int pipe_hip(ansx_ctx* c, hipError_t e)
{
    if (e == hipSuccess) return ANSX_OK;
    c->last_hip = (int)e;
    return ANSX_ERR_HIP;
}
// the side streams and events of a pipelined call of `nranges` ranges: made once per context, more events only when a
// later call has more ranges
int pipeline_prepare(ansx_ctx* c, u32 nranges)
{
    for (hipStream_t& st : c->pipe_stream)
        if (!st) HIPCHK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    while (c->pipe_ev.size() < 2 + (size_t)nranges) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->pipe_ev.push_back(e);
    }
    return ANSX_OK;
}

using ansx_enc::block_bound;  // worst-case bytes of one block's reference stream (ansx_encode_form.h)
using ansx_enc::codec_nsp;

// The shortest symbol-row stride (Plan::NSP) the encode kernels take when no int they see exceeds `vmax` (a compacted
// block's ranks: at most its length).  What a row must hold beyond the largest symbol `top` of 1..vmax, in one place:
//   - top + 1 entries, the block's alphabet;
//   - 8 more: k_scale_attempts and k_fold_hist read rows in chunks of 8 entries (ns rounded up to 8, plus a prefetch
//     that is clamped to stride - 8), and rows must start on 16-byte boundaries (u16 rows: a multiple of 8 entries);
//   - at least 64 entries: the floor of pre_cap, fcap and sort_cap (choose_model_form, choose_prelude_form), which are then cut
//     to min(stride, ...), and one full wave pass of k_sort_entropy / k_select_model;
//   - a power of two, as every codec's own stride is (ANSX_HCOPY_PAD's bank argument, hist_packed's NSP / 2 words).
// The stride selects launch shapes (ansx_encode_form.h) exactly as a codec's own slot count does, keys the
// interp-geo tables (ansx_ctx::geo, one per distinct stride) and is no part of any stream.
u32 min_row_stride(const ansx_map& m, u32 vmax)
{
    u32 top = 0;
    for (u32 x = 1; x <= vmax; x++) top = std::max(top, map_sym(m, x, map_nbytes(m, x)));
    u32 stride = 64;
    while (stride < top + 1u + 8u) stride <<= 1;
    return stride;
}

struct Plan {
    ansx_geo g;
    bool plain;
    Layout lay;
    u32 NSP;
    // decode of a batch pass (ansx_batch.h): the per-block table decode_dev puts into g after the header's checks
    // (make_plan has no part in it), and the ints of the output it lays out
    const ansx_blk_out* bout = nullptr;
    u64 bout_ints = 0;
    // encode of a batch pass (ansx_encbatch.h): the pass's work list and where its containers go; null everywhere else
    const struct EncBatchPass* bat = nullptr;
};

Layout layout_of(const ansx_geo& g, bool plain)
{
    Layout L;
    const u64 nck = (u64)g.nblocks * g.nckf;
    L.index_off = sizeof(ansx_container_header);
    L.ckoff_off = L.index_off + 8 * ((u64)g.nblocks + 1);
    if (g.ckw) {
        L.ckstate_off = rup(L.ckoff_off + 4 * nck, 8);
        L.hint_off = rup(L.ckstate_off + 32 * nck, 16);  // 8 x u32 parse hints per block
    } else {
        L.ckstate_off = L.ckoff_off;  // (one array of records)
        L.hint_off = rup(L.ckoff_off + (u64)ANSX_CK_RECORD * nck, 16);
    }
    L.payload_off = L.hint_off + 32 * (u64)g.nblocks;
    if (plain) L.index_off = L.ckoff_off = L.ckstate_off = L.hint_off = L.payload_off = 0;
    return L;
}

int make_plan(int kind, int f, size_t n, const ansx_opts* opts, Plan* P)
{
    if (kind != ANSX_FOLD && kind != ANSX_RFOLD && kind != ANSX_MSB && kind != ANSX_INT) return ANSX_ERR_ARG;
    if (kind == ANSX_MSB || kind == ANSX_INT) {
        if (f != 0) return ANSX_ERR_ARG;  // ANSmsb / ANSint have no fidelity parameter (methods.hpp:484-515)
    } else if (f < 1 || f > ANSX_MAX_FIDELITY) return ANSX_ERR_ARG;  // see include/ansx.h
    if (n == 0) return ANSX_ERR_ARG;
    u32 bi = opts ? opts->block_ints : 0;
    u32 ck = opts ? opts->ckpt_interval : 0;
    const u32 flags = opts ? opts->flags : 0;
    if (flags & ~(u32)ANSX_FLAG_COMPACT_ALPHABET) return ANSX_ERR_ARG;
    const bool pa = (flags & ANSX_FLAG_COMPACT_ALPHABET) != 0;
    // ANSint models every value up to the largest (ans_int.hpp:40-48).  Without the compaction layer the values
    // themselves must fit the 16384-symbol model (ANSX_ERR_DOMAIN otherwise: checked on the device); with it the
    // codec runs on a block's dense ranks.  ANSrfold brings its own remap.
    if (kind == ANSX_RFOLD && pa) return ANSX_ERR_ARG;
    if (pa) {
        if (bi == ANSX_SINGLE_STREAM) return ANSX_ERR_ARG;
        // ranks are 1-based (pseudo_adaptive.cpp:91-103): ANSint's alphabet is sigma + 1 <= 16384 symbols
        const u32 lim = kind == ANSX_INT ? 16380u : ANSX_PA_MAX_BLOCK;
        if (bi == 0) bi = kind == ANSX_INT ? 8192u : ANSX_DEFAULT_BLOCK_INTS;
        if (bi > lim) return ANSX_ERR_ARG;
    }
    P->plain = (bi == ANSX_SINGLE_STREAM);
    if (bi == 0) bi = ANSX_DEFAULT_BLOCK_INTS;
    if (ck == 0) ck = ANSX_DEFAULT_CKPT_INTERVAL;
    if (ck == ANSX_NO_CHECKPOINTS) ck = 0;
    if (P->plain) {
        if (n >= ((size_t)1 << 31)) return ANSX_ERR_ARG;  // reference limit
        bi = (u32)n;
        ck = 0;
    } else {
        if (bi & 3u) return ANSX_ERR_ARG;
        if (bi >= (1u << 31)) return ANSX_ERR_ARG;
    }
    if (ck & 3u) return ANSX_ERR_ARG;
    if (ck >= bi) ck = 0;
    // A block's worst-case stream (+ the 16 bytes of slack its scratch slot has) must stay below 2^31 bytes: the index
    // checks refuse a longer one (index_entry_ok, k_validate_index), and ansx_blk::stream_bytes and the wide restart
    // cursors are 32-bit.  Single-stream mode: the list is the block.
    if (block_bound(kind, (u32)f, bi, pa) + 16 >= ((size_t)1 << 31)) return ANSX_ERR_ARG;
    size_t nblocks = (n + bi - 1) / bi;
    if (nblocks > 0x7FFFFFFFull) return ANSX_ERR_ARG;
    ansx_geo g;
    g.n = n;
    g.block_ints = bi;
    g.nblocks = (u32)nblocks;
    g.ckpt = ck;
    g.nckf = geo_nseg(bi, ck) - 1;
    g.f = (u32)f;
    g.kind = (u32)kind;
    g.pa = pa ? 1u : 0u;
    g.ckw = 0;            // packed restart points unless set_restart_format() says otherwise
    g.payload_bytes = 0;  // (set by decode_dev from the container header)
    g.trusted_index = 0;  // (set by decode_dev on the single-stream path only, where the host writes the two entries)
    g.pad_ = 0;
    g.bout = nullptr;     // (set by decode_dev on a batch pass only)
    g.bin = nullptr;      // (set by encode_batch_pass only)
    g.map = kind == ANSX_MSB ? map_msb() : (kind == ANSX_INT ? map_int() : map_fold((u32)f));
    P->g = g;
    // symbol-array stride: the reference's MAX_SIGMA (ans_fold.hpp:70; ans_msb.hpp:28 has 1280)
    P->NSP = (u32)codec_nsp(kind, (u32)f);
    P->lay = layout_of(g, P->plain);
    return ANSX_OK;
}

// Restart points: packed 29-byte records (container v3 default) or the wide form (ansx_dev.h).  Wide is needed when a
// state can exceed 52 bits (frames above 2^16: ANSint always may, the others only with large alphabets in large
// blocks) or a cursor 24 bits; the encoder finds out about frames on the device and repeats the call (encode_dev).
void set_restart_format(Plan* P, bool wide)
{
    P->g.ckw = wide ? 1u : 0u;
    P->lay = layout_of(P->g, P->plain);
}

// fold maps have power-of-two thresholds 2^(f+7), 2^(f+15), 2^(f+23): the encoder derives the exception-byte
// count from the bit length instead of three comparisons
bool map_is_pow2(const ansx_map& m)
{
    return m.t1 >= 2 && (m.t1 & (m.t1 - 1)) == 0 && m.t1 < (1u << 15) && m.t2 == m.t1 << 8 && m.t3 == m.t1 << 16;
}
int flags_to_status(u32 fl)
{
    if (fl & (1u << 6)) return ANSX_ERR_DOMAIN;
    if (fl & (1u << 7)) return ANSX_ERR_MODEL;
    if (fl & (1u << 2)) return ANSX_ERR_CAPACITY;
    if (fl & (1u << 3)) return ANSX_ERR_FORMAT;
    return ANSX_OK;
}

// --------------------------------------------------------------------------------- rfold
// ans_reorder_fold.hpp:70-106 on the device, in the form R names (ansx_enc::choose_remap_form).
// ids != null (a batch pass, LDS forms only): the nids blocks of the pass listed there, addressed through g.bin
int rfold_remap(ansx_ctx* c, const ansx_geo& g, const ansx_enc::RemapForm& R, const u32* d_in, u32* mapped, u32* mostfreq,
    ansx_blk* blk, u32* gflags, hipStream_t s, const u32* ids = nullptr, u32 nids = 0)
{
    using namespace ansx_enc;
    const u32 grid = ids ? nids : g.nblocks;
    const Launch& L = R.rf_remap;
    if (R.rf == RF_HBM_HASH) {
        if (ids) return ANSX_ERR_ARG;  // (encode_batch_form keeps these off a pass)
        const u32 slots = R.rf_slots;
        int rc;
        if ((rc = ensure(c, c->rf_tmp, (size_t)g.nblocks * slots * 8 + (size_t)g.nblocks * 16))) return rc;
        u32* keys = (u32*)c->rf_tmp.p;
        u32* counts = keys + (size_t)g.nblocks * slots;
        u32* bstat = counts + (size_t)g.nblocks * slots;
        HIPCHK(c, hipMemsetAsync(keys, 0xFF, (size_t)g.nblocks * slots * 4, s));
        HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)g.nblocks * slots * 4 + (size_t)g.nblocks * 16, s));
        const size_t grid = (g.n + 255) / 256;
        LAUNCH(c, "k_rfg_insert", k_rfg_insert, grid, 256, 0, s, d_in, g, slots, keys, counts, bstat);
        if (R.rf_select.raise)
            HIPCHK(c, hipFuncSetAttribute((const void*)k_rfg_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.rf_select.lds));
        LAUNCH(c, "k_rfg_select", k_rfg_select, g.nblocks, R.rf_select.threads, R.rf_select.lds, s, g, slots, (const u32*)keys,
            counts, (const u32*)bstat, mostfreq, blk, gflags);
        LAUNCH(c, "k_rfg_map", k_rfg_map, grid, 256, 0, s, d_in, g, slots, (const u32*)keys, (const u32*)counts,
            (const ansx_blk*)blk, mapped);
        return ANSX_OK;
    }
    if (R.rf == RF_LDS_OPT) {
        HIPCHK(c, hipFuncSetAttribute((const void*)k_rfold_remap_hash2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
#ifdef ANSX_STAMPS_RF
        { static unsigned long long z[3] = { 0, 0, 0 }; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, 24, 4101 * 8); }
        hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, s);
#endif
        LAUNCH(c, "k_rfold_remap", k_rfold_remap_hash2, grid, L.threads, L.lds, s, d_in, g, R.rf_slots, mapped, mostfreq, blk, gflags, ids);
#ifdef ANSX_STAMPS_RF
        {
            (void)hipEventRecord(e1, s); (void)hipStreamSynchronize(s);
            float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
            unsigned long long z[3]; (void)hipMemcpyFromSymbol(z, HIP_SYMBOL(g_stamps), 24, 4101 * 8);
            fprintf(stderr, "[stamps] k_rfold_remap_hash2: events %.3f ms; workgroup lifetimes: max %llu ticks, mean %.0f ticks, %llu above 40 us\n", ms, z[0], (double)z[1] / g.nblocks, z[2]);
        }
#endif
        return ANSX_OK;
    }
    if (R.rf == RF_LDS_FULL) {
        HIPCHK(c, hipFuncSetAttribute((const void*)k_rfold_remap_hash, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
        LAUNCH(c, "k_rfold_remap", k_rfold_remap_hash, grid, L.threads, L.lds, s, d_in, g, R.rf_slots, mapped, mostfreq, blk, gflags, ids);
        return ANSX_OK;
    }
    if (L.raise) HIPCHK(c, hipFuncSetAttribute((const void*)k_rfold_remap, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    LAUNCH(c, "k_rfold_remap_sort", k_rfold_remap, g.nblocks, L.threads, L.lds, s, d_in, g, R.rf_slots, mapped, mostfreq, blk, gflags);
    return ANSX_OK;
}

// The remap of a batch pass (ansx_rfold.h): one launch per class of blocks that has any, over that class's block ids.
// `in` and `mapped` are addressed through g.bin, so both are pointers to where int 0 of the caller's input would be.
int rfold_remap_pass(ansx_ctx* c, const ansx_geo& g, const u32* d_in, u32* mapped, u32* mostfreq, ansx_blk* blk,
    u32* gflags, hipStream_t s, const ansx_enc::RemapForm& R, const u32* ids, const u32 ncls[3])
{
    const u32 n_id = ncls[RF_CLS_IDENTITY], n_small = ncls[RF_CLS_SMALL], n_large = ncls[RF_CLS_LARGE];
    if (n_id)
        LAUNCH(c, "k_rfold_remap_identity", k_rfold_remap_identity, std::min<u32>(2048u, (n_id + 3) / 4), 256, 0, s, d_in, g, ids,
            n_id, mapped, blk, gflags);
    if (n_small) {
        const size_t lds = 4 * (size_t)ANSX_RF_SMALL_LDS;  // two workgroups share a CU's 160 KB
        HIPCHK(c, hipFuncSetAttribute((const void*)k_rfold_remap_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        LAUNCH(c, "k_rfold_remap_small", k_rfold_remap_small, (n_small + 3) / 4, 256, lds, s, d_in, g, ids + n_id, n_small,
            mapped, mostfreq, blk, gflags);
    }
    if (n_large) return rfold_remap(c, g, R, d_in, mapped, mostfreq, blk, gflags, s, ids + n_id + n_small, n_large);
    return ANSX_OK;
}

// --------------------------------------------------------------------------------- encode
constexpr int ANSX_RETRY_GENERAL = -1;  // internal: an optimistic assumption did not hold, repeat without it
constexpr int ANSX_RETRY_WIDE = -2;     // internal: a frame above 2^16 in a call laid out for packed restart points, repeat with wide ones

// One attempt of an encode call: what it may assume.  The retry ladder (encode_dev -> encode_dev_once -> resolve_near)
// builds the attempts; inside an attempt the value is constant, and no function of the encode path learns a per-call
// fact from the context.
struct EncodeAttempt : ansx_enc::EncAttempt {  // (what it may assume: the part the forms read, ansx_encode_form.h)
    const u32* force = nullptr;  // per-block frames decided by the host (resolve_near), device array
};
// ... and what it found.  Every attempt starts it afresh, except sp_repeated, which only ever becomes true: a ladder
// that hands one outcome to all its attempts reads there whether any of them, at any depth, was repeated.
struct EncodeOutcome {
    u32 flags[16] = {};        // the words read back from `misc` (gflags, result): a copy, the pinned page is free again
    const u32* src = nullptr;  // the ints the model kernels saw (the input, or its remapped form)
    bool used_fast = false;    // the model came from k_candidates / k_model_finish
    bool used_pc = false;      // the producer / consumer encoder kernel ran
    bool sp_repeated = false;  // a rank-space attempt was repeated with the full-size prelude writer
    ansx_encode_form_report form = {};  // the forms the attempt's phases launched with (ansx_last_encode_form): written, never read
};

// What the phases of one attempt share: the call's arguments and the workspace pointers encode_begin carves.
struct EncodeWs {
    const Plan* P;  // (the first seven: set by the attempt's driver, the rest start as zero)
    const EncodeAttempt* a;
    EncodeOutcome* out;
    const u32* d_in;
    u8* d_out;
    size_t cap;
    hipStream_t s;
    u64 scr_stride;                 // bytes per block of the stream scratch
    u32 *gflags, *hist, *enc_sizes;
    u64 *result, *boff_ws;
    unsigned long long* enc_gsums;  // stream sizes summed per 64 blocks
    ansx_blk* blk;
    u32* hints;                     // the container's parse hints, or null
    const uint2* geo;               // tabulated tree nodes of the prelude's interpolative code, or null
    double* hterm;                  // entropy terms through HBM (model_prepare), or null
    const u32 *src, *mostfreq;      // encode_remap: the ints the model kernels and the encoder read; ANSrfold's selection
    u32 max_logM, max_ns;           // the model phase: largest frame / alphabet the later launches are sized for
    ansx_enc::EncGeo G;             // encode_begin: what the forms read of the plan ...
    ansx_enc::EncKeys K;            // ... and of the context's overrides
};

// A pass of ansx_encode_batch_dev (encode_batch_pass builds it; the phases reach it through Plan::bat)
struct EncBatchPass {
    const ansx_blk_in* hblk;  // the work list on the host (resolve_near reads a block back through it)
    u32 longest;              // ints of the pass's longest block: sizes the stream scratch stride
    ansx_encb_args A;         // device pointers of the plan, the results and the work area
    u64 in_base, in_ints;     // the pass's lists are ints [in_base, in_base + in_ints) of the caller's input
    const u32* remap_ids;     // block ids by remap class, device, class after class in the order of the form's enum below
    u32 remap_ncls[3];        // (null where the form has no remap front); remap_ncls: how many blocks each class has
    u8* d_out;                // the caller's buffer
    const ansx_encb_res* hres;  // pinned: the results, read back with the attempt's flag words
};

// The forms of an attempt -- ModelForm, RemapForm, PreludeForm, EncoderForm -- are host-only arithmetic in
// ansx_encode_form.h (swept on the CPU by tests/tools/encode_form_check.cpp).  Here: what they read of a plan and of
// the context's overrides.
using ansx_enc::EncoderForm;
using ansx_enc::ModelForm;
using ansx_enc::PreludeForm;
using ansx_enc::RemapForm;

ansx_enc::EncGeo enc_geo(const Plan& P)
{
    const ansx_geo& g = P.g;
    return { g.n, g.block_ints, g.nblocks, g.ckpt, g.kind, g.f, g.pa, P.NSP, P.plain, P.bat != nullptr, P.bat ? P.bat->longest : 0u,
        map_is_pow2(g.map) };
}

ansx_enc::EncKeys enc_keys(const DebugOpts& d)
{
    ansx_enc::EncKeys k;
    k.table16_fixup = d.table16_fixup, k.encode_gtab16 = d.encode_gtab16, k.fin_one_wave = d.fin_one_wave;
    k.use_pc = d.use_pc, k.no_pc_auto = d.no_pc_auto, k.force_pc = d.force_pc, k.no_pc = d.no_pc, k.encode_mode2 = d.encode_mode2;
    k.pc_b_pairs = d.pc_b_pairs, k.test_sp_bits = d.test_sp_bits, k.cand_chains = d.cand_chains;
    k.model_pipeline = d.model_pipeline;
    return k;
}

// the flag words (and the result behind them), read back into the attempt's outcome: a host wait
int read_flags(ansx_ctx* c, const EncodeWs& W, u32 words)
{
    HIPCHK(c, hipMemcpyAsync(c->pin->flags, c->misc.p, (size_t)words * 4, hipMemcpyDeviceToHost, W.s));
    HIPCHK(c, hipStreamSynchronize(W.s));
    memcpy(W.out->flags, c->pin->flags, (size_t)words * 4);
    return ANSX_OK;
}

// Phase 1: the workspace (grown on demand, kept by the context), the one-time tables, and k_begin_encode.
int encode_begin(ansx_ctx* c, EncodeWs& W)
{
    const Plan& P = *W.P;
    const ansx_geo& g = P.g;
    const u32 NB = g.nblocks, NSP = P.NSP;
    hipStream_t s = W.s;
    const bool sp = W.out->sp_repeated;
    *W.out = EncodeOutcome();
    W.out->sp_repeated = sp;
    W.G = enc_geo(P);
    W.K = enc_keys(c->dbg);
    W.scr_stride = ansx_enc::scratch_stride(W.G);
    if (!P.plain && W.cap < P.lay.payload_off) return ANSX_ERR_CAPACITY;
    int rc;
    if ((rc = ensure(c, c->hist, (size_t)NB * NSP * 4))) return rc;
    if ((rc = ensure(c, c->sortF, (size_t)NB * NSP * 4))) return rc;
    if ((rc = ensure(c, c->sortSym, (size_t)NB * NSP * 2))) return rc;
    const size_t fbytes = g.kind == ANSX_INT ? 4 : 2;  // candidate frequencies: u32 for ANSint (ans_int.hpp:30-34), u16 otherwise
    if ((rc = ensure(c, c->attS, (size_t)NB * ANSX_ATTEMPTS * NSP * fbytes))) return rc;
    if ((rc = ensure(c, c->prevS, (size_t)NB * NSP * fbytes))) return rc;
    if ((rc = ensure(c, c->attMeta, (size_t)NB * ANSX_ATTEMPTS * 16))) return rc;
    if (!c->log2lut.p) {  // stage-1 table of the portable log2, once per context (1.5 MB)
        if ((rc = ensure(c, c->log2lut, (size_t)65536 * sizeof(ansx_log2_ent)))) return rc;
        LAUNCH(c, "k_build_log2_lut", k_build_log2_lut, 256, 256, 0, s, (ansx_log2_ent*)c->log2lut.p);
    }
    if (NSP <= 4096) {  // tree nodes of the prelude's interpolative code for every alphabet size up to NSP, once per context
        DevBuf& gb = c->geo[NSP];
        if (!gb.p) {
            if ((rc = ensure(c, gb, ((size_t)NSP * (NSP + 1) / 2 + 8) * 8))) return rc;
            LAUNCH(c, "k_build_interp_geo", k_build_interp_geo, NSP, 256, 0, s, NSP, (uint2*)gb.p);
        }
        W.geo = (const uint2*)gb.p;
    }
    if ((rc = ensure(c, c->blk, (size_t)NB * sizeof(ansx_blk)))) return rc;
    if ((rc = ensure(c, c->table, (size_t)NB * NSP * sizeof(ansx_enc_entry)))) return rc;
    if ((rc = ensure(c, c->tab32, (size_t)NB * NSP * 4))) return rc;
    if ((rc = ensure(c, c->scratch, (size_t)NB * W.scr_stride))) return rc;
    if ((rc = ensure(c, c->misc, 64 + 8 * ((size_t)NB + 1)))) return rc;
    // per-block stream sizes + their sums per 64 blocks, published by the encoder for k_assemble
    const size_t ngroups = (((size_t)NB + 63) / 64 + 1) & ~(size_t)1;  // (an even count: the sums end on a 16-byte boundary)
    if ((rc = ensure(c, c->sizes, ngroups * 8 + (size_t)NB * 4))) return rc;
    W.enc_gsums = (unsigned long long*)c->sizes.p;
    W.enc_sizes = (u32*)((u8*)c->sizes.p + ngroups * 8);
    W.gflags = (u32*)c->misc.p;
    W.result = (u64*)((u8*)c->misc.p + 16);
    W.boff_ws = (u64*)((u8*)c->misc.p + 64);
    W.blk = (ansx_blk*)c->blk.p;
    W.hist = (u32*)c->hist.p;
    // (plain ANSint: no parse hints -- its decoder walks the value-range prelude sparsely, and the container must not depend on
    // which of the two models, dense or rank space, wrote it)
    W.hints = (P.plain || (g.kind == ANSX_INT && !g.pa)) ? nullptr : (u32*)(W.d_out + P.lay.hint_off);
    W.src = W.d_in;

    // flag words, size sums, block metadata, and the container's header / index / restart-point area: unused slots (short
    // last block) and alignment padding are defined to be zero, so equal inputs give byte-identical containers
    static_assert(sizeof(ansx_blk) % 16 == 0, "zeroed 16 bytes at a time");
    ansx_zero4 Z;
    Z.p[0] = (uint4*)c->misc.p, Z.n16[0] = 4;
    Z.p[1] = (uint4*)W.enc_gsums, Z.n16[1] = ngroups / 2;
    Z.p[2] = (uint4*)W.blk, Z.n16[2] = (u64)NB * (sizeof(ansx_blk) / 16);
    Z.p[3] = (uint4*)W.d_out, Z.n16[3] = P.plain ? 0 : (u64)P.lay.payload_off / 16;
    const u64 tot = Z.n16[0] + Z.n16[1] + Z.n16[2] + Z.n16[3];
    LAUNCH(c, "k_begin_encode", k_begin_encode, (u32)std::min<u64>(2048, (tot + 255) / 256), 256, 0, s, Z);
    return ensure(c, c->nearlist, (size_t)ANSX_NEAR_CAP * 4);
}

// Phase 2, the remap front: ANSrfold's most-frequent-value remap, the compaction layer, rank-space ANSint.  Leaves the
// ints the codec runs on in W.src (W.d_in itself where no front applies).
int encode_remap(ansx_ctx* c, EncodeWs& W)
{
    const ansx_geo& g = W.P->g;
    const EncodeAttempt& a = *W.a;
    const u32 NB = g.nblocks;
    hipStream_t s = W.s;
    const RemapForm R = ansx_enc::choose_remap_form(W.G, a);
    ansx_enc::report_remap(W.out->form, R, g.pa || a.int_sparse);
    int rc;
    if (g.kind == ANSX_RFOLD && W.P->bat) {
        // a batch pass (g.n is not its ints): `mapped` holds the pass's own stretch of the input's index space, and the
        // pointer handed on is biased by the stretch's start, so that the one work list g.bin addresses d_in and mapped
        // alike -- for the model kernels, the encoder and resolve_near's read-back
        const EncBatchPass& B = *W.P->bat;
        if ((rc = ensure(c, c->mapped, (size_t)std::max<u64>(B.in_ints, 1) * 4))) return rc;
        if ((rc = ensure(c, c->mostfreq, (size_t)NB * fold_T(g.f) * 4))) return rc;
        u32* biased = (u32*)((uintptr_t)c->mapped.p - (uintptr_t)B.in_base * 4);
        if ((rc = rfold_remap_pass(c, g, W.d_in, biased, (u32*)c->mostfreq.p, W.blk, W.gflags, s, R, B.remap_ids, B.remap_ncls)))
            return rc;
        W.src = biased;
        W.mostfreq = (const u32*)c->mostfreq.p;
    } else if (g.kind == ANSX_RFOLD) {
        if ((rc = ensure(c, c->mapped, (size_t)g.n * 4))) return rc;
        if ((rc = ensure(c, c->mostfreq, (size_t)NB * fold_T(g.f) * 4))) return rc;
        if ((rc = rfold_remap(c, g, R, W.d_in, (u32*)c->mapped.p, (u32*)c->mostfreq.p, W.blk, W.gflags, s))) return rc;
        W.src = (const u32*)c->mapped.p;
        W.mostfreq = (const u32*)c->mostfreq.p;
    }
    u32 *pa_mapped = nullptr, *pa_alpha = nullptr;  // ranks and running sums of the compaction layer / rank-space ANSint
    if (g.pa || a.int_sparse) {
        // (a batch pass: both in the input's own index space, biased like ANSrfold's `mapped` above -- the one work list
        // serves d_in, the ranks and the alphabets, and a block's alphabet, at most its ints, fits its own stretch)
        const EncBatchPass* B = W.P->bat;
        const size_t ints = B ? (size_t)std::max<u64>(B->in_ints, 1) : (size_t)NB * g.block_ints;
        const uintptr_t bias = B ? (uintptr_t)B->in_base * 4 : 0;
        if ((rc = ensure(c, c->mapped, ints * 4))) return rc;
        if ((rc = ensure(c, c->pa_alpha, ints * 4))) return rc;
        pa_mapped = (u32*)((uintptr_t)c->mapped.p - bias);
        pa_alpha = (u32*)((uintptr_t)c->pa_alpha.p - bias);
        W.src = pa_mapped;
    }
    // the blocks k_pa_remap / k_pa_header take: all of them, or the large class of a batch pass through its ids
    const u32* pa_ids = nullptr;
    u32 pa_large = NB;
    if (g.pa && W.P->bat) {
        // a batch pass: one launch pair per class of blocks that has any (ansx_pa.h); no table, no sizes for the small one
        const EncBatchPass& B = *W.P->bat;
        const u32 n_small = B.remap_ncls[PA_CLS_SMALL];
        if (n_small) {
            LAUNCH(c, "k_pa_remap_small", k_pa_remap_small, std::min<u32>(2048u, (n_small + 3) / 4), 256, 0, s, W.d_in, g, B.remap_ids,
                n_small, pa_mapped, pa_alpha, W.blk, W.gflags, 1u << 30);
            const u32 cap = ANSX_PA_SMALL_INTS;
            LAUNCH(c, "k_pa_header", k_pa_header, n_small, 256, ((size_t)3 * cap + 32) * 4, s, g, (const u32*)pa_alpha, W.blk,
                (u8*)c->scratch.p, W.scr_stride, cap, B.remap_ids);
        }
        pa_ids = B.remap_ids + n_small;
        pa_large = B.remap_ncls[PA_CLS_LARGE];
    }
    if (g.pa && pa_large) {
        // per-block alphabet compaction (src/pseudo_adaptive.cpp:85-130): alphabet header into the block's scratch slot, the
        // codec then runs on the 1-based ranks.  Hint-sized tables (R.pa_small) have a kernel of their own
        if (R.pa_small) {
            HIPCHK(c, hipFuncSetAttribute((const void*)k_pa_remap2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.pa_remap_lds));
            LAUNCH(c, "k_pa_remap", k_pa_remap2, pa_large, 1024, R.pa_remap_lds, s, W.d_in, g, R.pa_slots, R.pa_uqcap, pa_mapped, pa_alpha,
                W.blk, W.gflags, 1u << 30, pa_ids);
        } else {
            HIPCHK(c, hipFuncSetAttribute((const void*)k_pa_remap, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.pa_remap_lds));
            LAUNCH(c, "k_pa_remap", k_pa_remap, pa_large, 1024, R.pa_remap_lds, s, W.d_in, g, R.pa_slots, R.pa_uqcap, pa_mapped, pa_alpha,
                W.blk, W.gflags, 1u << 30, 0u, pa_ids);
        }
        HIPCHK(c, hipFuncSetAttribute((const void*)k_pa_header, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.pa_hdr_lds));
        LAUNCH(c, "k_pa_header", k_pa_header, pa_large, 256, R.pa_hdr_lds, s, g, (const u32*)pa_alpha, W.blk, (u8*)c->scratch.p,
            W.scr_stride, R.pa_hdr_cap, pa_ids);
    }
    if (a.int_sparse) {
        // plain ANSint on values beyond the dense model (ansx_intsparse.h): the codec runs on every block's 0-based ranks
        // (never hinted: R has the full-size tables)
        HIPCHK(c, hipFuncSetAttribute((const void*)k_pa_remap, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.pa_remap_lds));
        LAUNCH(c, "k_pa_remap", k_pa_remap, NB, 1024, R.pa_remap_lds, s, W.d_in, g, R.pa_slots, R.pa_uqcap, pa_mapped,
            pa_alpha, W.blk, W.gflags, (u32)ANSX_SP_VALUE_LIMIT, 1u, (const u32*)nullptr);
    }
    W.out->src = W.src;
    return ANSX_OK;
}

// ---- a form's variant -> the instantiation: the attribute call and the launch name the kernel through these
using hist_kernel_t = decltype(&k_fold_hist<false>);
using sort_kernel_t = decltype(&k_sort_entropy<u16>);
using cand_kernel_t = decltype(&k_candidates<4, 1>);
using fin_kernel_t = decltype(&k_model_finish<4, 8>);
hist_kernel_t hist_kernel(const ModelForm& M) { return M.hist.variant == ansx_enc::HIST_PACKED ? k_fold_hist<true> : k_fold_hist<false>; }
sort_kernel_t sort_kernel(const ModelForm& M)
{
    return M.sort.variant == ansx_enc::SORT_U32_UNSTAGED ? k_sort_entropy<u32, false>
        : (M.sort.variant == ansx_enc::SORT_U16 ? k_sort_entropy<u16> : k_sort_entropy<u32>);
}
cand_kernel_t cand_kernel(u32 NT, int nch)
{
    switch (NT) {
    case 4: return nch == 1 ? k_candidates<4, 1> : k_candidates<4, 2>;
    case 5: return nch == 1 ? k_candidates<5, 1> : k_candidates<5, 2>;
    case 6: return nch == 1 ? k_candidates<6, 1> : k_candidates<6, 2>;
    case 7: return nch == 1 ? k_candidates<7, 1> : k_candidates<7, 2>;
    default: return nch == 1 ? k_candidates<8, 1> : k_candidates<8, 2>;
    }
}
fin_kernel_t fin_kernel(const ModelForm& M)  // (its NTH is also the launch's workgroup size)
{
    switch (M.fin.variant) {
    case ansx_enc::FIN_ONE_WAVE_5: return k_model_finish<16, 5, 64>;
    case ansx_enc::FIN_ONE_WAVE_8: return k_model_finish<16, 8, 64>;
    case ansx_enc::FIN_WAVES: return k_model_finish<4, 8, 256>;
    case ansx_enc::FIN_GENERIC_5: return k_model_finish<0, 5, 256>;
    case ansx_enc::FIN_GENERIC_8: return k_model_finish<0, 8, 256>;
    case ansx_enc::FIN_16_5: return k_model_finish<16, 5, 256>;
    default: return k_model_finish<16, 8, 256>;
    }
}
template <class K>
int raise_lds(ansx_ctx* c, K kern, size_t lds)
{
    HIPCHK(c, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return ANSX_OK;
}

// ---- the launches of the model phase for the blocks [b0, be) on stream st
// K1
int launch_hist(ansx_ctx* c, const EncodeWs& W, const ModelForm& M, hipStream_t st, u32 b0, u32 be)
{
    const ansx_geo& g = W.P->g;
    const u32 NSP = W.P->NSP;
    // (sum_mode bit 1: on the fast model path H is the workgroup's tree sum and there is no hterm array to write)
    LAUNCH(c, "k_fold_hist", hist_kernel(M), (size_t)(be - b0) * M.hist.grid, M.hist.threads, M.hist.lds, st, W.src, g, M.chunk, M.cpb, NSP, W.hist, W.hterm,
        (M.h_in_hist ? 1u : 0u) | (M.fast ? 2u : 0u), W.blk, W.gflags, (g.kind == ANSX_INT && !g.pa) ? NSP : (1u << 30), b0, be);
    return ANSX_OK;
}
// K2
int launch_sort(ansx_ctx* c, const EncodeWs& W, const ModelForm& M, hipStream_t st, u32 b0, u32 be)
{
    LAUNCH(c, "k_sort_entropy", sort_kernel(M), be - b0, M.sort.threads, M.sort.lds, st, W.P->g, W.P->NSP, M.nbig_cap, M.h_deferred ? 1u : 0u, W.hist,
        (u32*)c->sortF.p, (u16*)c->sortSym.p, W.blk, M.sort_cap, M.fast ? (uint2*)c->pairs.p : (uint2*)nullptr, W.gflags, b0, be);
    return ANSX_OK;
}
// K2 and the two kernels of the fast model path behind it
int launch_fast_model(ansx_ctx* c, const EncodeWs& W, const ModelForm& M, hipStream_t st, u32 b0, u32 be)
{
    const ansx_geo& g = W.P->g;
    const u32 NSP = W.P->NSP, NT = W.a->nt;
    int rc;
    if ((rc = launch_sort(c, W, M, st, b0, be))) return rc;
    const ansx_enc::Launch cand = ansx_enc::cand_launch(M, be - b0);
    LAUNCH(c, "k_candidates", cand_kernel(NT, cand.variant), cand.grid, cand.threads, cand.lds, st,
        g, NSP, (const uint2*)c->pairs.p, (const ansx_blk*)W.blk, (uint4*)c->attS.p, (u32*)c->attMeta.p, b0, be);
    LAUNCH(c, "k_model_finish", fin_kernel(M), be - b0, M.fin.threads, M.fin.lds, st, g, NSP, NT, (const uint2*)c->pairs.p, (const uint4*)c->attS.p,
        (const u32*)c->attMeta.p, W.blk, (u32*)c->tab32.p, (u8*)c->scratch.p, W.scr_stride, W.mostfreq, W.hints, W.gflags, M.fcap,
        c->dbg.fast_guard, (const double*)c->lg2i.p, W.geo, NSP > 4096 ? W.hist : (u32*)nullptr, b0, be, c->dbg.chain_old ? 1u : 0u);
    if (!c->dbg.chain_old)  // (the call's running maxima: no longer every block's own business)
        LAUNCH(c, "k_model_maxima", k_model_maxima, (be - b0 + 255) / 256, 256, 0, st, (const ansx_blk*)W.blk, W.gflags, b0, be);
    return ANSX_OK;
}

// Phase 3a: what K1 and K2 need whichever model form follows
int model_prepare(ansx_ctx* c, EncodeWs& W, const ModelForm& M)
{
    const size_t NB = W.P->g.nblocks, NSP = W.P->NSP;
    int rc;
    if (M.cpb > 1) HIPCHK(c, hipMemsetAsync(W.hist, 0, NB * NSP * 4, W.s));
    if (M.h_deferred && !M.h_in_hist && !M.fast) {
        if ((rc = ensure(c, c->hterm, NB * NSP * 8))) return rc;
        W.hterm = (double*)c->hterm.p;
    }
    if (M.hist.raise && (rc = raise_lds(c, hist_kernel(M), M.hist.lds))) return rc;
    if (M.sort.raise && (rc = raise_lds(c, sort_kernel(M), M.sort.lds))) return rc;
    return ANSX_OK;
}

// Phase 3b, the model in its exact form: K1, K2, then frame sizes M0 * 2^t tried ANSX_ATTEMPTS at a time.  Almost every
// block settles in the first batch; the count of undecided blocks comes back with the words the encoder launch
// needs anyway (largest alphabet / frame), so further batches are launched only on demand.
int model_exact(ansx_ctx* c, EncodeWs& W, const ModelForm& M)
{
    const ansx_geo& g = W.P->g;
    const u32 NB = g.nblocks, NSP = W.P->NSP;
    const u32 nbatch = 24 / ANSX_ATTEMPTS;  // t < 24 (t <= 16 suffices)
    hipStream_t s = W.s;
    int rc;
    if ((rc = launch_hist(c, W, M, s, 0, NB))) return rc;
    if ((rc = launch_sort(c, W, M, s, 0, NB))) return rc;
    for (u32 batch = 0; batch < nbatch; batch++) {
        if (batch) HIPCHK(c, hipMemsetAsync(&W.gflags[ANSX_G_PAD], 0, 4, s));
        LAUNCH(c, "k_scale_attempts", k_scale_attempts, ((size_t)NB * ANSX_ATTEMPTS + 255) / 256, 256,
            0, s, g, NSP, batch, W.hist, (const u32*)c->sortF.p, (const u16*)c->sortSym.p, W.blk,
            (u16*)c->attS.p, (u32*)c->attMeta.p, (const double*)W.hterm, (const ansx_log2_ent*)c->log2lut.p,
            g.block_ints <= 65535u ? 1u : 0u);
        LAUNCH(c, "k_select_model", k_select_model, NB, 64, 0, s, g, NSP, batch, W.hist,
            (const u16*)c->attS.p, (const u32*)c->attMeta.p, (u16*)c->prevS.p, W.blk,
            (ansx_enc_entry*)c->table.p, (u32*)c->tab32.p, W.gflags, batch == nbatch - 1 ? 1u : 0u, M.always16,
            (u32*)c->nearlist.p, W.a->force, c->dbg.near_band, c->dbg.near_flip ? 1u : 0u);
        if (W.a->ns_cap != 0) {  // checked after the fact (blocks left undecided carry no model and are skipped)
            W.max_logM = 16;
            W.max_ns = W.a->ns_cap;
            break;
        }
        if ((rc = read_flags(c, W, 4))) return rc;
        const u32* fl = W.out->flags;
        if ((rc = flags_to_status(fl[ANSX_G_ERR]))) return rc;
        W.max_logM = fl[ANSX_G_MAXLOGM];
        W.max_ns = fl[ANSX_G_MAXNSYMS];
        if (fl[ANSX_G_PAD] == 0) break;
    }
    return ANSX_OK;
}

// Block-range pipeline of the fast model path: the call's blocks in `nranges` contiguous ranges,
// the histograms one after the other on the caller's stream, and k_sort_entropy -> k_candidates -> k_model_finish of
// every range but the last on one of the context's two side streams (alternating) behind that range's histogram -- a
// memory-bound kernel beside a VALU-bound one beside a latency chain.  The ranges meet in no workspace byte (every
// array is indexed by the absolute block number) and in `gflags` only through order-independent atomics.  Everything
// joins on the caller's stream in front of the encoder.  ModelForm::nranges == 0: one launch of each kernel over all
// blocks on the caller's stream.
// Phase 3b, the model in its fast form: K1, K2, k_candidates, k_model_finish (which also writes the preludes), serial
// or as the block-range pipeline.  Everything that is not a launch, an event record or a stream wait -- buffers, the
// one-time tables, the side streams, every function attribute -- comes first.
int model_fast(ansx_ctx* c, EncodeWs& W, ModelForm M)
{
    const u32 NB = W.P->g.nblocks, NSP = W.P->NSP;
    hipStream_t s = W.s;
    int rc;
    if (NSP > 4096 && !c->dbg.no_big_geo) {
        // k_model_finish<0>: a 14-level tree descent per item was two thirds of its prelude writer; the nodes of every alphabet
        // size up to the hint come from a table here too (built once per context, rebuilt when the hint grows)
        if (c->geo_big_cap < M.fcap) {
            if ((rc = ensure(c, c->geo_big, ((size_t)M.fcap * (M.fcap + 1) / 2 + 8) * 8))) return rc;
            LAUNCH(c, "k_build_interp_geo", k_build_interp_geo, M.fcap, 256, 0, s, M.fcap, (uint2*)c->geo_big.p);
            c->geo_big_cap = M.fcap;
        }
        W.geo = (const uint2*)c->geo_big.p;
    }
    if ((rc = ensure(c, c->pairs, (size_t)NB * NSP * 8))) return rc;
    if (!c->lg2i.p) {  // log2 of the integers below 2^16, once per context (512 KB)
        if ((rc = ensure(c, c->lg2i, (size_t)65536 * 8))) return rc;
        LAUNCH(c, "k_build_log2i_lut", k_build_log2i_lut, 256, 256, 0, s, (double*)c->lg2i.p);
    }
    if (M.nranges) {
        // (a captured graph with parallel branches: the call stays one chain of launches under capture -- the form again, serial)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) M = ansx_enc::choose_model_form(W.G, *W.a, W.K, c->num_cus, true);
        else if ((rc = pipeline_prepare(c, M.nranges))) return rc;
    }
    const u32 range_blocks = M.range_blocks, nranges = M.nranges;
    // k_candidates: the chain counts its launches will use (a full range and the last, shorter one)
    const ansx_enc::Launch cand[2] = { ansx_enc::cand_launch(M, range_blocks), ansx_enc::cand_launch(M, nranges ? NB - (nranges - 1) * range_blocks : NB) };
    ansx_enc::report_model(W.out->form, M, (u32)cand[1].variant, NSP > 4096 && !c->dbg.no_big_geo);
    for (int nch = 1; nch <= 2; nch++) {
        const ansx_enc::Launch& L = cand[0].variant == nch ? cand[0] : cand[1];
        if (L.variant == nch && L.raise && (rc = raise_lds(c, cand_kernel(W.a->nt, nch), L.lds))) return rc;
    }
    if (M.fin.raise && (rc = raise_lds(c, fin_kernel(M), M.fin.lds))) return rc;

    W.max_logM = 16;
    W.max_ns = W.a->ns_cap;
    if (nranges == 0) {
        if ((rc = launch_hist(c, W, M, s, 0, NB))) return rc;
        return launch_fast_model(c, W, M, s, 0, NB);
    }
    // fork: a range's model kernels wait for the event recorded on the caller's stream behind its histogram -- and with
    // it for everything the call, and the call before it, put on that stream (k_begin_encode, the remap, the previous
    // encoder's last read of the shared workspace)
    u32 used = 0;  // side streams with work of this call
    rc = ANSX_OK;
    for (u32 k = 0; k < nranges && !rc; k++) {
        const u32 b0 = k * range_blocks, be = std::min<u32>(NB, b0 + range_blocks);
        if ((rc = launch_hist(c, W, M, s, b0, be))) break;
        hipStream_t st = s;
        if (k + 1 < nranges) {
            const u32 side = k & 1u;
            st = c->pipe_stream[side];
            if ((rc = pipe_hip(c, hipEventRecord(c->pipe_ev[2 + k], s)))) break;
            if ((rc = pipe_hip(c, hipStreamWaitEvent(st, c->pipe_ev[2 + k], 0)))) break;
            used |= 1u << side;
        }  // (the last range stays on the caller's stream behind its histogram: nothing is left to overlap it with there,
           // and the encoder follows it without a cross-stream wait)
        rc = launch_fast_model(c, W, M, st, b0, be);
    }
    // join: always, whatever happened above -- when the call returns, all its work is ordered on the caller's stream
    for (u32 side = 0; side < 2; side++) {
        if (!(used & (1u << side))) continue;
        int rj = pipe_hip(c, hipEventRecord(c->pipe_ev[side], c->pipe_stream[side]));
        if (!rj) rj = pipe_hip(c, hipStreamWaitEvent(s, c->pipe_ev[side], 0));
        if (rj) {  // (the runtime refused the record or the wait: the host waits instead, so the promise still holds)
            (void)hipStreamSynchronize(c->pipe_stream[side]);
            if (!rc) rc = rj;
        }
    }
    return rc;
}

// Phase 4, the exact form's prelude writers (K3; they also fill the container's parse hints).  Their LDS arrays are as
// long as the call's largest alphabet (known here on the discovery path, assumed = the hint on the optimistic one), not
// as its slot count: workgroups per CU.
int write_preludes(ansx_ctx* c, EncodeWs& W, const PreludeForm& F)
{
    using namespace ansx_enc;
    const ansx_geo& g = W.P->g;
    const u32 NSP = W.P->NSP;
    hipStream_t s = W.s;
    const ansx_enc_entry* table = (const ansx_enc_entry*)c->table.p;
    const u32* tab32 = (const u32*)c->tab32.p;
    u8* scratch = (u8*)c->scratch.p;
    const Launch& L = F.w;
    int rc;
    report_prelude(W.out->form, F);
    if (F.table16_first)
        LAUNCH(c, "k_table16_from32", k_table16_from32, g.nblocks, 256, 0, s, g, NSP, (const ansx_blk*)W.blk, tab32, (ansx_enc_entry*)c->table.p);
    if (L.variant == PRE_RANK_SPACE) {
        if (L.raise && (rc = raise_lds(c, k_int_sparse_prelude, L.lds))) return rc;
        LAUNCH(c, "k_int_sparse_prelude", k_int_sparse_prelude, L.grid, L.threads, L.lds, s, g, NSP, (const u32*)c->pa_alpha.p, table, W.blk,
            scratch, W.scr_stride, F.sp_cap, F.sp_bits, (u32)(4 * NSP), W.gflags);
        return ANSX_OK;
    }
    const bool generic = L.variant == PRE_GENERIC || L.variant == PRE_GENERIC_HBM;  // (no tabulated tree nodes; HBM: f = 6, 7)
    u32* g_work = nullptr;
    if (L.variant == PRE_GENERIC_HBM) {
        if ((rc = ensure(c, c->pre_work, (size_t)g.nblocks * (2 * (size_t)F.pre_cap + 16) * 4))) return rc;
        g_work = (u32*)c->pre_work.p;
    }
    const auto kern = L.variant == PRE_W4 ? k_write_prelude<4> : (L.variant == PRE_W16 ? k_write_prelude<16> : k_write_prelude<0>);
    if (L.raise && (rc = raise_lds(c, kern, L.lds))) return rc;
    LAUNCH(c, "k_write_prelude", kern, L.grid, L.threads, L.lds, s, g, NSP, table, tab32, W.hist, W.blk, scratch, W.scr_stride, W.mostfreq,
        W.hints, F.pre_cap, generic ? (const uint2*)nullptr : W.geo, g_work);
    return ANSX_OK;
}

// Phase 5, the encoder (K5) in the form E names.  The f64-state forms keep their per-wave tables in LDS when they fit
// (sized from the largest alphabet / frame of the model phase); their emitted-byte stores go through a buffer
// descriptor spanning the wave's 16 scratch slots: 31-bit offsets.
int launch_encoder(ansx_ctx* c, EncodeWs& W, const EncoderForm& E)
{
    using namespace ansx_enc;
    const Plan& P = *W.P;
    const ansx_geo& g = P.g;
    hipStream_t s = W.s;
    u64* ck_state = P.plain ? nullptr : (u64*)(W.d_out + P.lay.ckstate_off);
    u32* ck_off = P.plain ? nullptr : (u32*)(W.d_out + P.lay.ckoff_off);
    const u32* tab32 = (const u32*)c->tab32.p;
    u8* scratch = (u8*)c->scratch.p;
    const bool pow2 = W.G.map_pow2;
    int rc;
    W.out->used_pc = false;  // (true below, once the pair kernel has taken blocks of this call)
    report_encoder(W.out->form, E);
    if (E.pc.grid) {  // producer / consumer pairs
        const auto kern = pow2 ? (E.S == 8 ? k_encode_pc<true, 8> : k_encode_pc<true, 4>) : (E.S == 8 ? k_encode_pc<false, 8> : k_encode_pc<false, 4>);
        if ((rc = raise_lds(c, kern, E.pc.lds))) return rc;
        LAUNCH(c, "k_encode", kern, E.pc.grid, E.pc.threads, E.pc.lds, s, W.src, g, P.NSP, tab32, W.max_ns, E.rowwords, W.blk, scratch,
            W.scr_stride, ck_state, ck_off, W.enc_sizes, W.enc_gsums);
        W.out->used_pc = true;
    }
    // one wave per 16 blocks (MODE 1: waves of one workgroup run the main loop in step, a barrier per super-batch), or
    // the integer-state encoder on the 16-byte entries
    const Launch& L = E.rest;
    if (!L.grid) return ANSX_OK;
    const bool int_state = L.variant == ENC_INT_STATE, mode1 = L.variant == ENC_MODE1;
    const auto kern = int_state ? k_encode<0> : (mode1 ? (pow2 ? k_encode<1, true> : k_encode<1, false>) : k_encode<2>);
    if (L.raise && (rc = raise_lds(c, kern, L.lds))) return rc;
    LAUNCH(c, E.first ? "k_encode_rest" : (mode1 ? "k_encode" : "k_encode_gtab"), kern, L.grid, L.threads, L.lds, s, W.src, g, P.NSP,
        int_state ? (const ansx_enc_entry*)c->table.p : (const ansx_enc_entry*)nullptr, tab32, E.lds_stride, W.blk, scratch, W.scr_stride,
        ck_state, ck_off, W.enc_sizes, W.enc_gsums, E.first);
    return ANSX_OK;
}

// Phase 6: assembly (K6), the attempt's one read-back of the flag words behind it, and their status.
int encode_finish(ansx_ctx* c, EncodeWs& W, size_t* out_bytes)
{
    const Plan& P = *W.P;
    const ansx_geo& g = P.g;
    const u32 NB = g.nblocks;
    hipStream_t s = W.s;
    u64* boff = P.plain ? W.boff_ws : (u64*)(W.d_out + P.lay.index_off);
    if (P.bat) {
        // a batch pass: every list's container straight from the stream scratch into the caller's buffer (ansx_encbatch.h);
        // the results ride on the read-back of the flag words
        ansx_encb_args A = P.bat->A;
        A.ns_cap = W.a->ns_cap;
        A.forced = W.a->force != nullptr ? 1u : 0u;
        // (the lists' maxima are gathered with atomics: every attempt of the pass starts them afresh)
        HIPCHK(c, hipMemsetAsync(A.mx, 0, sizeof(ansx_encb_max) * (size_t)A.nl, s));
        LAUNCH(c, "k_encb_scan", k_encb_scan, 1, 1024, 0, s, g, A, (const ansx_blk*)W.blk, (const u32*)W.enc_sizes, W.result, W.gflags);
        LAUNCH(c, "k_encb_write", k_encb_write, NB, 256, 0, s, g, A, (const u32*)W.enc_sizes, (const u8*)c->scratch.p, W.scr_stride,
            P.bat->d_out);
        HIPCHK(c, hipMemcpyAsync((void*)P.bat->hres, A.res, sizeof(ansx_encb_res) * ((size_t)A.nl + 1), hipMemcpyDeviceToHost, s));
    } else if (NB <= 65536u) {
        LAUNCH(c, "k_assemble", k_assemble, NB, 256, 0, s, g, (const u32*)W.enc_sizes, (const unsigned long long*)W.enc_gsums, boff, W.result,
            (const u8*)c->scratch.p, W.scr_stride, W.d_out, (u64)P.lay.payload_off, (u64)W.cap, W.gflags, P.plain ? 0u : 1u);
    } else {
        LAUNCH(c, "k_scan_sizes", k_scan_sizes, 1, 1024, 0, s, g, W.blk, boff, W.result, P.lay.payload_off,
            (u64)W.cap, W.gflags);
        LAUNCH(c, "k_compact", k_compact, NB, 256, 0, s, g, W.blk, boff, (const u8*)c->scratch.p,
            W.scr_stride, W.d_out + P.lay.payload_off, W.gflags);
        if (!P.plain)
            LAUNCH(c, "k_write_header", k_write_header, 1, 64, 0, s, g, W.d_out, W.gflags, W.result, P.lay.payload_off);
    }
    int rc;
    if ((rc = read_flags(c, W, 16))) return rc;
    const u32* fl = W.out->flags;
    if (W.a->ns_cap != 0) {
        if (fl[ANSX_G_ERR] & (1u << 6)) return ANSX_ERR_DOMAIN;
        if (fl[ANSX_G_ERR] & (1u << ANSX_G_VIOL_BIT)) return ANSX_RETRY_GENERAL;  // (rfold: optimistic hash table too small; the fused model: any assumption)
        if (fl[ANSX_G_PAD] != 0 || fl[ANSX_G_MAXLOGM] > 16 || fl[ANSX_G_MAXNSYMS] > W.a->ns_cap) return ANSX_RETRY_GENERAL;
        if (!g.ckw && g.nckf != 0 && fl[ANSX_G_MAXLOGM] > c->dbg.wide_at) return ANSX_RETRY_GENERAL;  // (tests only: wide_at < 16)
    }
    if ((rc = flags_to_status(fl[ANSX_G_ERR]))) return rc;
    u64 payload;
    memcpy(&payload, &fl[4], 8);
    *out_bytes = (size_t)(P.lay.payload_off + payload);
    return ANSX_OK;
}

// One attempt on the tailored model kernels: the phases in the order of DESIGN.md section 5.
int encode_general(ansx_ctx* c, const Plan& P, const u32* d_in, u8* d_out, size_t cap, size_t* out_bytes, hipStream_t s,
    const EncodeAttempt& a, EncodeOutcome* out)
{
    const ansx_geo& g = P.g;
    EncodeWs W = { &P, &a, out, d_in, d_out, cap, s };
    int rc;
    if ((rc = encode_begin(c, W))) return rc;                                  // workspace, k_begin_encode
    if ((rc = encode_remap(c, W))) return rc;                                  // rfold / compaction / rank-space ANSint
    // (profile mode: the event pairs of LAUNCH would time overlapped kernels -- serial there)
    const ModelForm M = ansx_enc::choose_model_form(W.G, a, W.K, c->num_cus, c->profile);
    out->used_fast = M.fast;
    ansx_enc::report_attempt(out->form, W.G, a, false);  // (behind encode_remap, which has noted its own form: neither touches the other's fields)
    ansx_enc::report_model(out->form, M, 0, false);      // (model_fast notes the form it ends up launching)
    if ((rc = model_prepare(c, W, M))) return rc;
    if ((rc = M.fast ? model_fast(c, W, M) : model_exact(c, W, M))) return rc;  // K1 .. K4
    if (!P.plain && !g.ckw && g.nckf != 0 && W.max_logM > c->dbg.wide_at) return ANSX_RETRY_WIDE;  // (discovery path: known before anything is encoded)
    if (!M.fast && (rc = write_preludes(c, W, ansx_enc::choose_prelude_form(W.G, a, W.K, M.always16, W.max_logM, W.max_ns)))) return rc;  // (k_model_finish wrote them)
    if ((rc = launch_encoder(c, W, ansx_enc::choose_encoder_form(W.G, W.K, c->num_cus, W.max_logM, W.max_ns)))) return rc;
    if ((rc = encode_finish(c, W, out_bytes))) return rc;
    if (a.int_sparse && !a.sp_full_lds && (out->flags[ANSX_G_ERR] & (1u << ANSX_G_VIOL_BIT))) {
        // (the value-range prelude of some block needs more than two words per distinct value)
        EncodeAttempt full = a;
        full.sp_full_lds = true;
        rc = encode_general(c, P, d_in, d_out, cap, out_bytes, s, full, out);
        out->sp_repeated = true;
    }
    return rc;
}

// LDS carve of k_model_fused for `cap` symbols (a multiple of 8), see ansx_model.h
ansx_model_lds model_layout(u32 cap)
{
    ansx_model_lds L;
    L.cap = cap;
    L.nc = cap <= 1024 ? 4u : (cap <= 2560 ? 2u : 1u);
    L.natt = cap <= 1024 ? 8u : 4u;  // candidate rows are the largest region: fewer per batch for big alphabets
    const u32 A = L.nc * (cap + 8) * 4;
    u32 off;
    if (L.nc == 4) {  // pairs | yF (12 cap bytes) live in histogram copies 1..3, dead once copy 0 holds the sums
        L.off_pairs = (cap + 8) * 4;
        off = A;
    } else {
        L.off_pairs = A;
        off = A + 12 * cap;
    }
    L.off_yF = L.off_pairs + 4 * cap;
    L.off_S = off;
    const u32 sbytes = L.natt * cap * 2;  // >= 8 cap: the entropy terms come first
    if (sbytes >= 8 * cap + ANSX_MODEL_SORT_BYTES) {
        L.off_E = off + 8 * cap;  // sort scratch behind the entropy terms
        off += sbytes;
    } else {
        L.off_E = off + sbytes;
        off += sbytes + (u32)rup(ANSX_MODEL_SORT_BYTES, 16);
    }
    L.off_pos = off;
    off += (u32)rup(2 * cap, 16);
    L.off_ffs = off;
    off += (u32)rup(4 * (cap + 4), 16);
    L.off_X = off;
    off += 256 * 8;
    if (4 * cap >= 256 * 8) L.off_X1 = L.off_pairs;  // pairs are dead once yF / ffs exist
    else {
        L.off_X1 = off;
        off += 256 * 8;
    }
    L.total = off;
    return L;
}

// Optimistic attempt, fused form (opt-in): ONE model kernel per block with everything in LDS (sized from the
// alphabet hint) between the shared front and tail.  Any block that does not fit the assumptions (alphabet above the
// hint, frame above 2^16) raises the violation flag and the caller repeats the call on the general path.
int encode_fast(ansx_ctx* c, const Plan& P, const u32* d_in, u8* d_out, size_t cap, size_t* out_bytes, hipStream_t s,
    const EncodeAttempt& a, EncodeOutcome* out)
{
    const ansx_model_lds ML = model_layout(a.ns_cap);
    if (ansx_enc::scratch_stride(enc_geo(P)) * 16 >= 0x7FFFFF00ull || ML.total > ansx_enc::LDS_BUDGET) return ANSX_RETRY_GENERAL;
    EncodeWs W = { &P, &a, out, d_in, d_out, cap, s };
    int rc;
    if ((rc = encode_begin(c, W))) return rc;
    if ((rc = encode_remap(c, W))) return rc;
    ansx_enc::report_attempt(out->form, W.G, a, true);
    const auto kern = a.ns_cap <= 1024 ? k_model_fused<4> : k_model_fused<16>;
    if (ML.total > ansx_enc::LDS_NO_ATTRIBUTE && (rc = raise_lds(c, kern, ML.total))) return rc;
    LAUNCH(c, "k_model_fused", kern, P.g.nblocks, 256, ML.total, s, W.src, P.g, P.NSP, ML, (const ansx_log2_ent*)c->log2lut.p, W.blk,
        (u32*)c->tab32.p, (u8*)c->scratch.p, W.scr_stride, W.mostfreq, W.gflags, 1u << 30, W.hints);
    W.max_logM = 16;
    W.max_ns = a.ns_cap;
    if ((rc = launch_encoder(c, W, ansx_enc::choose_encoder_form(W.G, W.K, c->num_cus, W.max_logM, W.max_ns)))) return rc;
    return encode_finish(c, W, out_bytes);
}

// ---------------------------------------------------------------------------------------------
// Close calls of the frame-size stop rule, decided again on the host.  The reference compares
// XH = -sum p log2(S/M) with 1.001 H (ans_util.hpp:127-128,149) using libm's log2; the device uses its own
// portable log2 (<= 1 ulp apart), so a comparison whose two sides agree to ~1e-12 is the one place where the
// two could part.  k_select_model lists the blocks with such a comparison; for each of them the host reads the
// block back, rebuilds its histogram and runs adjust_freqs as written (ans_util.hpp:100-157, util.hpp:271-298;
// this TU is compiled with -ffp-contract=off, log2 is the host libm's -- the function the reference itself
// would call here).  If any decision differs from the device's, the call is repeated on the exact path with
// the host's frames forced for those blocks.
// Returns log2 of the frame size, or -1 for the reference's degenerate exit.
int host_adjust_freqs(const std::vector<u32>& freqs, u32 largest_sym, bool require_u16)
{
    const u32 ns = largest_sym + 1;
    u64 n = 0;
    u32 sigma = 0;
    for (u32 i = 0; i < ns; i++) {
        n += freqs[i];
        sigma += freqs[i] != 0;
    }
    if (sigma == 0) return -1;
    u32 lg = (sigma & (sigma - 1)) == 0 ? 31u - (u32)__builtin_clz(sigma) : 32u - (u32)__builtin_clz(sigma);  // :109-112
    std::vector<u32> order;
    order.reserve(sigma);
    for (u32 i = 0; i < ns; i++)
        if (freqs[i]) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return freqs[a] < freqs[b]; });  // (freq, sym) ascending, :114-122
    double H;
    {  // util.hpp:271-282
        double acc = 0.0;
        for (u32 i = 0; i < ns; i++)
            if (freqs[i]) {
                const double p = (double)freqs[i] / (double)n;
                acc = acc + p * std::log2(p);
            }
        H = -acc;
    }
    const double thr = H * (1.0 + (double)1 / (double)1000);  // :124,127-128
    std::vector<u32> scaled(ns, 0u);
    int prev = -1;
    for (; lg <= 31; lg++) {
        i64 Mr = (i64)1 << lg;
        u64 fr = n;
        for (u32 j = 0; j < sigma; j++) {  // :77-95
            const u32 sym = order[j];
            const double a = (double)Mr / (double)fr;
            double v = a * (double)freqs[sym];
            v = 0.5 + v;
            u32 S = (u32)v;
            if (S == 0) S = 1;
            scaled[sym] = S;
            Mr -= S;
            fr -= freqs[sym];
            if (Mr < 0) break;
        }
        if (Mr != 0) continue;  // :131-135
        u32 maxS = 0;
        for (u32 i = 0; i < ns; i++)
            if (freqs[i] && scaled[i] > maxS) maxS = scaled[i];
        if (require_u16 && maxS >= ANSX_U16_LIMIT) return prev;  // :141-145
        double XH;
        {  // util.hpp:284-298 (note the int accumulators there)
            double acc = 0.0;
            const double nd = (double)(int)n, md = (double)(int)((i64)1 << lg);
            for (u32 i = 0; i < ns; i++)
                if (freqs[i] && scaled[i]) {
                    const double p = (double)freqs[i] / nd;
                    const double q = (double)scaled[i] / md;
                    acc = acc + p * std::log2(q);
                }
            XH = -acc;
        }
        if (XH < thr) return (int)lg;  // :149
        prev = (int)lg;
    }
    return -1;
}

// `last`: the attempt whose container stands in d_out, `out` its outcome.  A forced repeat assumes nothing but what
// the host decided, keeps the model space of that attempt, and leaves its own outcome in `out`.
int resolve_near(ansx_ctx* c, const Plan& P, const u32* d_in, u8* d_out, size_t cap, size_t* out_bytes, hipStream_t s,
    const EncodeAttempt& last, EncodeOutcome* out, u32* redecided)
{
    const ansx_geo& g = P.g;
    const u32 nn = out->flags[ANSX_G_NEAR];
    std::vector<u32> list;
    if (nn <= ANSX_NEAR_CAP) {
        list.resize(nn);
        HIPCHK(c, hipMemcpyAsync(list.data(), c->nearlist.p, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    } else {  // more close calls than the device lists: every block is looked at
        list.resize(g.nblocks);
        for (u32 b = 0; b < g.nblocks; b++) list[b] = b;
    }
    std::vector<u32> hin, hist, force;
    u32 nre = 0;
    for (const u32 b : list) {
        if (b >= g.nblocks) continue;
        // (g.bin is a device table: a batch pass keeps the host's copy)
        const u32 nb = P.bat ? P.bat->hblk[b].n : geo_block_n(g, b);
        const u64 first = P.bat ? P.bat->hblk[b].off : (u64)b * g.block_ints;
        ansx_blk hb;
        hin.resize(nb);
        HIPCHK(c, hipMemcpyAsync(hin.data(), out->src + first, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&hb, (const ansx_blk*)c->blk.p + b, sizeof(hb), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (hb.pa_sigma == 1) continue;  // (compaction: a one-value block has no model)
        hist.assign(P.NSP, 0u);
        u32 largest = 0;
        for (u32 i = 0; i < nb; i++) {
            const u32 x = hin[i];
            const u32 k = map_nbytes(g.map, x);
            const u32 sym = map_sym(g.map, x, k);
            if (sym >= P.NSP) return ANSX_ERR_DOMAIN;
            hist[sym]++;
            largest = sym > largest ? sym : largest;
        }
        const int lg = host_adjust_freqs(hist, largest, g.kind != ANSX_INT);
        const int dev = hb.status ? -1 : (int)hb.logM;
        if (lg != dev) {
            if (force.empty()) force.assign(g.nblocks, 0u);
            force[b] = lg < 0 ? 0xFFFFFFFFu : (u32)lg;
            nre++;
        }
    }
    *redecided = nre;
    // (a batch pass with close calls has written nothing yet -- k_encb_scan holds such an attempt back, so that a repeat
    // with other sizes leaves no stale byte behind the total: it is always repeated, with whatever the host decided)
    if (nre == 0 && !P.bat) return ANSX_OK;
    if (force.empty()) force.assign(g.nblocks, 0u);
    int rc;
    if ((rc = ensure(c, c->force, (size_t)g.nblocks * 4))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->force.p, force.data(), (size_t)g.nblocks * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));  // (force is a local)
    EncodeAttempt forced;
    forced.int_sparse = last.int_sparse;
    forced.force = (const u32*)c->force.p;
    return encode_general(c, P, d_in, d_out, cap, out_bytes, s, forced, out);
}

// (pa, kind, fidelity, block_ints): the key of the per-geometry hint maps
u64 geo_key(const ansx_geo& g) { return ((u64)g.pa << 48) | ((u64)g.kind << 40) | ((u64)g.f << 32) | g.block_ints; }

int encode_dev_once(ansx_ctx* c, const Plan& P, const u32* d_in, u8* d_out, size_t cap, size_t* out_bytes,
    hipStream_t s)
{
    // The first call of a geometry discovers its alphabet size with a mid-call read-back; later calls
    // are launched back to back on that hint and repeat (rarely) if the input outgrew it.
    const u64 key = geo_key(P.g);
    const bool int_plain = P.g.kind == ANSX_INT && !P.g.pa;
    const auto it = c->ns_hint.find(key);
    const u32 hint = c->dbg.ns_hint ? c->dbg.ns_hint : (it != c->ns_hint.end() ? it->second : 0u);
    const bool eligible = !P.plain && hint != 0 && (P.NSP <= 4096 || (P.NSP <= 16384 && P.g.kind != ANSX_INT && !P.g.pa)) && !c->dbg.encode_gtab16 && !c->dbg.table16_fixup
        && !c->dbg.model_sync;  // (with compaction too: the hint then describes the alphabets of the rank-remapped blocks)
    // (k_model_fused: the LDS-resident single-kernel model, measured slower than the five tailored
    // kernels -- DESIGN.md section 6 -- and therefore opt-in)
    const bool fused = eligible && c->dbg.model_fused && P.g.block_ints <= ANSX_MODEL_MAX_BLOCK && !P.g.pa && !P.bat;
    EncodeAttempt exact;  // discovery: nothing assumed
    exact.int_sparse = int_plain && c->int_sparse_hint.count(key) != 0;
    EncodeAttempt hinted = exact;  // ... and what the geometry's hints allow
    if (eligible) {
        hinted.ns_cap = std::min<u32>(P.NSP, std::max<u32>(64u, (hint + 7u) & ~7u));
        const auto rit = c->rf_hint.find(key);
        if (P.g.kind == ANSX_RFOLD && rit != c->rf_hint.end()) hinted.rf_slots = ansx_enc::rf_opt_slots(rit->second, fold_T(P.g.f));
        if (P.g.pa && rit != c->rf_hint.end()) hinted.pa_distinct = rit->second;
        // candidates per block for the fast model path: one more than the largest index chosen so far, 4..8 lanes
        // (fewer than 4 would leave the wave's lanes to more blocks than its LDS rows); above 8 the exact path stays
        const auto tit = c->t_hint.find(key);
        const u32 tcount = c->dbg.t_hint ? c->dbg.t_hint : (tit != c->t_hint.end() ? tit->second : 0u);
        if (!c->dbg.no_fast_model && tcount != 0 && tcount <= 8) hinted.nt = std::max<u32>(4u, tcount);
    }
    EncodeOutcome o;
    int rc = ANSX_RETRY_GENERAL;
    if (eligible) rc = (fused ? encode_fast : encode_general)(c, P, d_in, d_out, cap, out_bytes, s, hinted, &o);
    u32 path = !eligible ? 0u : (fused ? 2u : (o.used_fast ? 5u : 1u));
    const bool missed = eligible && rc == ANSX_RETRY_GENERAL;
    if (rc == ANSX_RETRY_GENERAL) {
        path = eligible ? path | 16u : 0u;
        rc = encode_general(c, P, d_in, d_out, cap, out_bytes, s, exact, &o);
    }
    // Plain ANSint: the dense model takes values below 16384; a call with larger ones is repeated in rank space, and so is
    // every later call of the geometry from the start -- unless its values turn out small, where the dense form (whose
    // containers carry parse hints) is the one a fresh context would have written: equal inputs, equal bytes.
    if (int_plain && !exact.int_sparse && rc == ANSX_ERR_DOMAIN) {
        exact.int_sparse = true;
        c->int_sparse_hint.insert(key);
        rc = encode_general(c, P, d_in, d_out, cap, out_bytes, s, exact, &o);
    } else if (int_plain && exact.int_sparse && rc == ANSX_OK && o.flags[ANSX_G_VMAX] < P.NSP) {
        exact.int_sparse = false;
        c->int_sparse_hint.erase(key);
        rc = encode_general(c, P, d_in, d_out, cap, out_bytes, s, exact, &o);
    }
    if (exact.int_sparse) path |= 256u;  // plain ANSint modelled in rank space
    // close calls of the stop rule (counted by the exact kernels only; the fast path repeats on them): the host decides
    u32 redecided = 0;
    const u32 near_blocks = o.flags[ANSX_G_NEAR];  // (a forced repeat skips the rule for the blocks it forces)
    if (rc == ANSX_OK && near_blocks != 0) rc = resolve_near(c, P, d_in, d_out, cap, out_bytes, s, exact, &o, &redecided);
    if (rc == ANSX_RETRY_WIDE) return rc;
    if (o.sp_repeated) path |= 512u;  // ... and repeated with the full-size prelude writer
    // (from here on `o` is the outcome of the attempt whose container is returned)
    c->last.host_redecided = redecided;
    c->last.path = path | (o.used_pc ? 128u : 0u);
    c->last.max_nsyms = o.flags[ANSX_G_MAXNSYMS];
    c->last.max_log2_frame = o.flags[ANSX_G_MAXLOGM];
    c->last.near_threshold_decisions = near_blocks;
    if (rc == ANSX_OK) c->last_form = o.form;
    if (rc == ANSX_OK && !P.plain) {
        // a miss raises the hint past what was seen, so inputs whose alphabets creep upwards do not
        // miss on every call
        const u32 seen = o.flags[ANSX_G_MAXNSYMS];
        const u32 want = missed ? seen + seen / 8 + 8 : seen;
        u32& h = c->ns_hint[key];
        if (want > h) h = want;
        u32& th = c->t_hint[key];
        const u32 wantt = o.flags[ANSX_G_MAXT] + 1u + (missed ? 1u : 0u);
        if (wantt > th) th = wantt;
        if (P.g.kind == ANSX_RFOLD || P.g.pa) {
            const u32 d = o.flags[ANSX_G_RFDIST];
            u32& r = c->rf_hint[key];
            const u32 wantd = missed ? d + d / 8 + 8 : d;
            if (wantd > r) r = wantd;
        }
    }
    return rc;
}

// Restart-point format of the call (see set_restart_format): packed unless the geometry rules it out or an earlier
// call of the geometry met a frame above 2^16; a call that meets one is repeated once with the wide form.
int encode_dev(ansx_ctx* c, const Plan& P0, const u32* d_in, u8* d_out, size_t cap, size_t* out_bytes, hipStream_t s)
{
    Plan P = P0;
    if (!P.plain) {
        const u64 key = geo_key(P.g);
        const size_t stream_bound = block_bound(P.g.kind, P.g.f, P.g.block_ints, P.g.pa != 0) + 16;
        const bool must = P.g.kind == ANSX_INT || stream_bound >= ((size_t)1 << ANSX_CK_CURSOR_BITS) || c->dbg.wide_restart;
        // The hint only picks which attempt runs FIRST; the format that is returned is a function of the input and the
        // options alone: wide if and only if this call's frames need it.
        const bool hinted = !must && c->wide_hint.count(key) != 0;
        set_restart_format(&P, must || hinted);
        int rc = encode_dev_once(c, P, d_in, d_out, cap, out_bytes, s);
        if (rc == ANSX_OK && hinted && c->last.max_log2_frame <= c->dbg.wide_at) {
            // an earlier call of this geometry needed wide restart points, this input does not: encode it again packed, so
            // that equal inputs give equal containers whatever the context encoded before (ranks of a multi-GPU job must
            // agree on the format, ansx_merge_containers_dev), and forget the hint
            c->wide_hint.erase(key);
            set_restart_format(&P, false);
            const u32 path0 = c->last.path;
            rc = encode_dev_once(c, P, d_in, d_out, cap, out_bytes, s);
            c->last.path |= (path0 & 16u) | 64u;  // 64: repeated with packed restart points
        }
        if (rc != ANSX_RETRY_WIDE) return rc;
        c->wide_hint.insert(key);
        set_restart_format(&P, true);
        const int rc2 = encode_dev_once(c, P, d_in, d_out, cap, out_bytes, s);
        c->last.path |= 32u;  // repeated with wide restart points
        return rc2;
    }
    return encode_dev_once(c, P, d_in, d_out, cap, out_bytes, s);
}

// --------------------------------------------------------------------------------- decode
// The form of a decode call -- DecodeBounds, DecodeForm, choose_decode_form -- is host-only arithmetic in
// ansx_decode_form.h (swept on the CPU by tests/tools/decode_form_check.cpp).  Here: what it reads of a plan's geometry
// and of the context's overrides.
using ansx_form::DecodeBounds;
using ansx_form::DecodeForm;
using ansx_form::LaunchShape;
using ansx_form::PARSE_DONE;
using ansx_form::PARSE_GENERIC;
using ansx_form::PARSE_PAR;
using ansx_form::PARSE_FAST;
using ansx_form::PARSE_WIN;
using ansx_form::DEC_STAGED;
using ansx_form::DEC_RING;
using ansx_form::DEC_SMALL_RING;
using ansx_form::DEC_PAIR;
using ansx_form::DEC_TABLE;
using ansx_form::DEC_GTAB;

ansx_form::FormGeo form_geo(const ansx_geo& g)
{
    return { g.n, g.block_ints, g.nblocks, g.ckpt, g.kind, g.pa, geo_nseg(g.block_ints, g.ckpt),
        g.kind == ANSX_RFOLD ? fold_T(g.f) * 4u : 0u, block_bound((int)g.kind, g.f, g.block_ints, false) };
}

ansx_form::FormKeys form_keys(const DebugOpts& d)
{
    ansx_form::FormKeys k;
    k.parse_generic = d.parse_generic, k.parse_win = d.parse_win, k.parse_fast = d.parse_fast;
    k.parse_stage_words = d.parse_stage_words;
    k.setup_old = d.setup_old;
    k.decode_table = d.decode_table, k.no_stream_lds = d.no_stream_lds;
    k.decode_mode = d.decode_mode, k.decode_pair = d.decode_pair, k.decode_small_ring = d.decode_small_ring;
    k.pair_lds_limit = d.pair_lds_limit;
    return k;
}

DecodeForm choose_decode_form(const ansx_geo& g, const DecodeBounds& B, const DebugOpts& dbg, u32 num_cus)
{
    return ansx_form::choose_decode_form(form_geo(g), B, form_keys(dbg), num_cus);
}

// What ansx_last_decode_stats reports of an attempt: its form, the bounds it was chosen from, how it came about
void note_decode_form(ansx_ctx* c, const ansx_geo& g, const DecodeBounds& B, const DecodeForm& F, u32 flags)
{
    ansx_decode_stats& d = c->last_dec;
    d.parser = (u32)F.parser, d.p_variant = F.p_variant, d.decoder = (u32)F.decoder;
    d.p_grid = F.p.grid, d.p_threads = F.p.threads, d.p_lds = (u32)F.p.lds;
    d.d_grid = F.d.grid, d.d_threads = F.d.threads, d.d_lds = (u32)F.d.lds;
    d.stream_cap = F.stream_cap;
    d.maxM = B.maxM, d.max_ns = B.max_ns, d.max_ep = B.max_ep, d.max_block_bytes = B.max_block_bytes;
    d.nblocks = g.nblocks;
    d.flags = flags;
}

// What the phases of a decode call share: where the pieces of its source are, its plan (the container's own, the
// caller's per-block table put in) and the bounds its form is chosen from.
struct DecodeSrc {
    Plan P;
    const u8* cont;
    const u64* boff;
    const u64* ck_state;
    const u32* ck_off;
    u64 payload_off;
    const u32* hints;  // the container's parse hints, or null
    DecodeBounds B;
};

// LAUNCH in the shape L, the kernel's limit on dynamic LDS raised first where the default does not do
template <class K, class... Args>
int launch_lds(ansx_ctx* c, const char* label, K kern, const LaunchShape& L, hipStream_t s, Args... args)
{
    int rc;
    if (L.lds > 48 * 1024 && (rc = raise_lds(c, kern, L.lds))) return rc;
    LAUNCH(c, label, kern, L.grid, L.threads, L.lds, s, args...);
    return ANSX_OK;
}

typedef void (*lane_parser_t)(const u8*, ansx_geo, u32, const u64*, u64, u32, u32, u32*, uint4*, u32*, const uint4*);
typedef void (*par_parser_t)(const u8*, ansx_geo, u32, const u64*, u64, u32, u32, const u32*, u32*, uint4*, u32*, const uint4*);
typedef void (*rank_decoder_t)(const u8*, ansx_geo, u32, const u64*, const u64*, const u32*, u64, u32*, u32, u32, u64,
    const u32*, const uint4*, u32*, u32);

// K7 and K8 as the form says: the parser fills dec_cum / dec_info, the decoder reads them
template <bool RF>
int launch_decode(ansx_ctx* c, const DecodeSrc& S, const DecodeForm& F, u32* d_out, hipStream_t s)
{
    const ansx_geo& g = S.P.g;
    const DecodeBounds& B = S.B;
    const u32 NSP = S.P.NSP;
    int rc;
    if ((rc = ensure(c, c->dec_cum, (size_t)g.nblocks * (NSP + 8) * 4))) return rc;
    if ((rc = ensure(c, c->dec_info, (size_t)g.nblocks * 16))) return rc;
    if (F.decoder == DEC_GTAB && (rc = ensure(c, c->dec_s2s, (size_t)g.nblocks * B.maxM * 2))) return rc;
    u32* cum = (u32*)c->dec_cum.p;
    uint4* info = (uint4*)c->dec_info.p;
    u32* gflags = (u32*)c->misc.p;
    const uint4* pa_info = g.pa ? (const uint4*)c->pa_info.p : nullptr;
    const par_parser_t par[3] = { k_parse_prelude_par<RF, ANSX_PAR_SW, 0>, k_parse_prelude_par<RF, ANSX_PAR_SW, 1>, k_parse_prelude_par<RF, ANSX_PAR_SW, 2> };
    const lane_parser_t lane = F.parser == PARSE_GENERIC ? k_parse_prelude<RF> : F.p_variant == 128 ? k_parse_prelude_win<RF, 128> : k_parse_prelude_win<RF, 256>;
    const rank_decoder_t rank[4] = { k_decode_rank<RF, 0>, k_decode_rank<RF, 1>, k_decode_rank<RF, 2>, k_decode_rank2<RF> };  // by DEC_*
    if (F.parser == PARSE_PAR)
        rc = launch_lds(c, F.p_variant ? "k_parse_prelude_arr" : "k_parse_prelude", par[F.p_variant], F.p, s,
            S.cont, g, NSP, S.boff, S.payload_off, B.max_ns, B.maxM, S.hints, cum, info, gflags, pa_info);
    else if (F.parser == PARSE_FAST)
        rc = launch_lds(c, "k_parse_prelude", k_parse_prelude_fast<RF>, F.p, s, S.cont, g, NSP,
            S.boff, S.payload_off, B.max_ns, B.maxM, cum, info, gflags, F.p_variant, pa_info);
    else if (F.parser != PARSE_DONE)
        rc = launch_lds(c, "k_parse_prelude", lane, F.p, s, S.cont, g, NSP, S.boff,
            S.payload_off, B.max_ns, B.maxM, cum, info, gflags, pa_info);
    if (rc) return rc;
    if (F.decoder == DEC_TABLE || F.decoder == DEC_GTAB) {
        const bool lds_tab = F.decoder == DEC_TABLE;
        return launch_lds(c, lds_tab ? "k_decode_table" : "k_decode_gtab", lds_tab ? k_decode<true, RF> : k_decode<false, RF>,
            F.d, s, S.cont, g, NSP, S.boff, S.ck_state, S.ck_off, S.payload_off, d_out, B.maxM,
            B.max_ns, F.stream_cap, lds_tab ? (u16*)nullptr : (u16*)c->dec_s2s.p, cum, (const uint4*)info, gflags);
    }
    // (the ring decoders bound their reads by the container's bytes where the staged one takes its staging size)
    const u64 cap = F.decoder == DEC_STAGED ? F.stream_cap : S.payload_off + B.payload_bytes;
    const u32 setup_old = c->dbg.setup_old ? 1u : 0u;  // the scan form of dec_build_rank_tables
    return launch_lds(c, "k_decode", rank[F.decoder], F.d, s, S.cont, g, NSP, S.boff, S.ck_state,
        S.ck_off, S.payload_off, d_out, B.maxM, B.max_ep, cap, (const u32*)cum, (const uint4*)info, gflags, setup_old);
}

__global__ void k_selftest_div(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out, u64 n)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = ansx_div_int31(a[i], b[i]);
}

__global__ void k_selftest_log2(const double* __restrict__ in, double* __restrict__ out, u64 n)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = ansx_log2_portable(in[i]);
}

#define ANSX_G_HDR_BIT 9u  // gflags[ANSX_G_ERR]: the container header is not the one this decode was launched on
__global__ void k_check_header(const u8* __restrict__ cont, ansx_container_header want, u32* __restrict__ gflags)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const u32* a = (const u32*)cont;
    const u32* w = (const u32*)&want;
    u32 diff = 0;
    for (int i = 0; i < 16; i++) diff |= a[i] ^ w[i];
    if (diff) atomicOr(&gflags[ANSX_G_ERR], 1u << ANSX_G_HDR_BIT);
}

__global__ void k_validate_index(ansx_geo g, const u64* __restrict__ boff, u64 payload_bytes,
    u32* __restrict__ gflags)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.nblocks) return;
    u64 a = boff[i], b = boff[i + 1];
    // a reference stream has at least 2 prelude bytes + one interpolative word + 32 state bytes; with
    // compaction a one-value block is just its alphabet header (8 bytes + code)
    const u64 min_bytes = g.pa ? 8 : 38;
    bool bad = (b < a) || (b - a) < min_bytes || (b - a) >= (1ull << 31) || b > payload_bytes;
    if (i == 0 && a != 0) bad = true;
    if (i == g.nblocks - 1 && b != payload_bytes) bad = true;
    if (bad) atomicOr(&gflags[ANSX_G_ERR], 1u << 3);
    else if (__hip_atomic_load(&gflags[ANSX_G_PAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (u32)(b - a))
        atomicMax(&gflags[ANSX_G_PAD], (u32)(b - a));  // largest block stream (sizes the LDS staging)
}

int parse_header(const u8* h, size_t bytes, ansx_container_header* out)
{
    if (bytes < sizeof(ansx_container_header)) return ANSX_ERR_FORMAT;
    ansx_container_header H;
    memcpy(&H, h, sizeof(H));
    static const char magic[6] = { 'A', 'N', 'S', 'X', 'v', '3' };
    if (memcmp(H.magic, magic, 6) != 0) return ANSX_ERR_FORMAT;
    const u32 k = H.kind & 0xFFu;  // bit 8: per-block alphabet compaction, bit 9: wide restart points
    if ((H.kind & ~0x3FFu) || k > 3 || H.n == 0 || H.block_ints == 0) return ANSX_ERR_FORMAT;
    if ((k == ANSX_MSB || k == ANSX_INT) ? H.fidelity != 0 : (H.fidelity < 1 || H.fidelity > ANSX_MAX_FIDELITY)) return ANSX_ERR_FORMAT;
    *out = H;
    return ANSX_OK;
}

// The options a container's header stands for
ansx_opts container_opts(const ansx_container_header& H)
{
    ansx_opts o;
    o.block_ints = H.block_ints;
    o.ckpt_interval = H.ckpt_interval ? H.ckpt_interval : ANSX_NO_CHECKPOINTS;
    o.flags = (H.kind & 0x100u) ? ANSX_FLAG_COMPACT_ALPHABET : 0;
    o.reserved = 0;
    return o;
}

// The checks every reader of a container applies to its header before it touches anything behind it: the codec the
// caller names, the layout the header's own geometry implies, every section inside the input, sane model bounds.
// P: the container's plan (the container, not the caller's options, defines the geometry).
int container_plan(const ansx_container_header& H, u32 kind, u32 f, size_t in_bytes, Plan* P)
{
    if ((H.kind & 0xFFu) != kind || H.fidelity != f) return ANSX_ERR_FORMAT;
    const ansx_opts o = container_opts(H);
    if (H.block_ints == ANSX_SINGLE_STREAM) return ANSX_ERR_FORMAT;
    if (make_plan((int)(H.kind & 0xFFu), (int)f, (size_t)H.n, &o, P)) return ANSX_ERR_FORMAT;
    set_restart_format(P, (H.kind & ANSX_KIND_WIDE_RESTART) != 0);
    if (P->g.nblocks != H.nblocks || P->g.nckf != H.ckpts_per_block || P->g.ckpt != H.ckpt_interval
        || P->lay.payload_off != H.payload_offset)
        return ANSX_ERR_FORMAT;
    // (written so that a crafted payload_bytes near 2^64 cannot wrap the sum; payload_offset covers
    // the index and the restart-point area, so this also places those inside the input)
    if (H.payload_offset > in_bytes || H.payload_bytes > in_bytes - H.payload_offset) return ANSX_ERR_FORMAT;
    // every block stream has a minimum length (index_entry_ok): a payload shorter than that for all blocks is malformed
    // whatever the index says (in particular payload_bytes == 0, which no parser may take for "no index")
    if (H.payload_bytes < (u64)P->g.nblocks * (P->g.pa ? 8u : 38u)) return ANSX_ERR_FORMAT;
    // (with compaction a list whose blocks all hold a single distinct value has no model at all)
    if (H.max_log2_frame > 31 || (H.max_nsyms == 0 && !P->g.pa) || H.max_nsyms > P->NSP) return ANSX_ERR_FORMAT;
    return ANSX_OK;
}

// One reference stream as the decoder's source: copied behind a 16-byte guard (the decoder reads 8 bytes below its
// cursor), max_sym / log2 M peeked on the host, the two index entries of its one block written here.
int source_plain(ansx_ctx* c, const Plan& Pin, const u8* d_in, size_t in_bytes, hipStream_t s, DecodeSrc* S)
{
    int rc;
    Plan P = Pin;
    if (in_bytes < 38) return ANSX_ERR_FORMAT;
    if ((rc = ensure(c, c->plain, in_bytes + 64))) return rc;
    HIPCHK(c, hipMemsetAsync(c->plain.p, 0, 16, s));
    HIPCHK(c, hipMemcpyAsync((u8*)c->plain.p + 16, d_in, in_bytes, hipMemcpyDeviceToDevice, s));
    // ONE host round trip: the first 16 bytes and, for ANSrfold, the 8 bytes behind a most-frequent table (where the
    // prelude starts if the block was reordered) are requested together
    const u8* hp = c->pin->plain.peek;
    const size_t pos_rf = 4 + 4 * (size_t)fold_T(P.g.f);
    HIPCHK(c, hipMemcpyAsync(c->pin->plain.peek, d_in, 16, hipMemcpyDeviceToHost, s));
    if (P.g.kind == ANSX_RFOLD && pos_rf + 8 <= in_bytes)
        HIPCHK(c, hipMemcpyAsync(c->pin->plain.peek_rf, d_in + pos_rf, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    size_t pos = 0;
    if (P.g.kind == ANSX_RFOLD) {
        u32 flag;
        memcpy(&flag, hp, 4);
        if (flag > 1) return ANSX_ERR_FORMAT;
        pos = flag ? pos_rf : 4;
        if (pos + 8 > in_bytes) return ANSX_ERR_FORMAT;
        if (flag) {
            hp = c->pin->plain.peek_rf;
            pos = 0;
        }
    }
    u32 ms = 0, sh = 0;
    for (int i = 0; i < 5; i++) {
        u8 cb = hp[pos++];
        ms += (u32)(cb & 127) << sh;
        if (!(cb & 128)) break;
        sh += 7;
    }
    const u32 lg = hp[pos];
    const bool int_sp = P.g.kind == ANSX_INT && !P.g.pa;  // (any max_sym below 2^30: the model is parsed in rank space)
    if ((int_sp ? ms >= ANSX_SP_VALUE_LIMIT : ms >= P.NSP) || lg > 31) return ANSX_ERR_FORMAT;
    // (the two index entries of the one block go up from pinned memory: no wait -- the page is next written by
    // this call's final read-back, which the stream orders behind this copy)
    u64* hb = c->pin->plain.index;
    hb[0] = 0, hb[1] = (u64)in_bytes;
    P.g.trusted_index = 1;  // the index of this one block is the pair written here, not container bytes
    u64* boff_ws = (u64*)((u8*)c->misc.p + 64);
    HIPCHK(c, hipMemcpyAsync(boff_ws, hb, 16, hipMemcpyHostToDevice, s));
    const u32 max_ns = std::min(ms + 1, P.NSP);
    *S = { P, (const u8*)c->plain.p, boff_ws, nullptr, nullptr, 16, nullptr, { 1u << lg, max_ns, max_ns, false, in_bytes, (u32)in_bytes } };
    return ANSX_OK;
}

// A container as the decoder's source: its header -- `spec` if given, else fetched (one host round trip) -- checked, the
// plan it implies and the bounds it states.  Every kernel treats header-derived sizes as untrusted anyway (index entries,
// restart points and hints are bounds-checked against them): that is what lets a call run on a remembered header.
int source_container(ansx_ctx* c, const Plan& Pin, const u8* d_in, size_t in_bytes, const ansx_container_header* spec,
    hipStream_t s, DecodeSrc* S)
{
    int rc;
    Plan P = Pin;
    if (in_bytes < sizeof(ansx_container_header)) return ANSX_ERR_FORMAT;
    if (spec) {
        c->pin->hdr = *spec;
    } else {
        HIPCHK(c, hipMemcpyAsync(&c->pin->hdr, d_in, sizeof(ansx_container_header), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    ansx_container_header H;
    if ((rc = parse_header((const u8*)&c->pin->hdr, in_bytes, &H))) return rc;
    if (H.n != P.g.n) return ANSX_ERR_FORMAT;
    if ((rc = container_plan(H, P.g.kind, P.g.f, in_bytes, &P))) return rc;
    P.g.payload_bytes = H.payload_bytes;  // every parser validates the two index entries of its own block (index_entry_ok)
    P.g.bout = Pin.bout;                  // (container_plan -> make_plan has reset it)
    const u32 max_ns = H.max_nsyms ? H.max_nsyms : 1u;
    *S = { P, d_in, (const u64*)(d_in + P.lay.index_off), (const u64*)(d_in + P.lay.ckstate_off), (const u32*)(d_in + P.lay.ckoff_off),
        H.payload_offset, (const u32*)(d_in + P.lay.hint_off),
        { 1u << H.max_log2_frame, max_ns, std::min<u32>(max_ns, (u32)H.max_present_m1 + 1u), true, H.payload_bytes, 0 } };
    return ANSX_OK;
}

// The steps ahead of the parser where the codec ran on a block's ranks (k_pa_unmap / k_int_unmap put the values back).
int decode_premap(ansx_ctx* c, const DecodeSrc& S, hipStream_t s)
{
    const Plan& P = S.P;
    const bool int_sparse = P.g.kind == ANSX_INT && !P.g.pa;
    if (!P.g.pa && !int_sparse) return ANSX_OK;
    int rc;
    u32* gflags = (u32*)c->misc.p;
    // alpha scratch: laid out like the output (geo_block_out)
    if ((rc = ensure(c, c->pa_alpha, 4 * (P.g.bout ? (size_t)P.bout_ints : (size_t)P.g.nblocks * P.g.block_ints)))) return rc;
    if ((rc = ensure(c, c->pa_info, (size_t)P.g.nblocks * 16))) return rc;
    if (P.g.pa) {  // alphabet headers first: they tell where every block's codec stream starts
        LAUNCH(c, "k_pa_parse", k_pa_parse, (P.g.nblocks + 63) / 64, 64, 0, s, S.cont, P.g, S.boff, S.payload_off,
            (u32*)c->pa_alpha.p, (uint4*)c->pa_info.p, gflags);
        return ANSX_OK;
    }
    // plain ANSint: the prelude ranges over the VALUES (any max_sym); its present symbols become the block's ranks
    // (ansx_intsparse.h) -- whichever model the encoder ran, the stream is the reference's
    if ((rc = ensure(c, c->dec_cum, (size_t)P.g.nblocks * (P.NSP + 8) * 4))) return rc;
    if ((rc = ensure(c, c->dec_info, (size_t)P.g.nblocks * 16))) return rc;
    LAUNCH(c, "k_parse_prelude", k_int_sparse_parse, (P.g.nblocks + 63) / 64, 64, 0, s, S.cont, P.g, P.NSP, S.boff, S.payload_off, S.B.maxM,
        (u32*)c->dec_cum.p, (uint4*)c->dec_info.p, (u32*)c->pa_alpha.p, (uint4*)c->pa_info.p, gflags);
    return ANSX_OK;
}

struct DecodeOpts {
    bool speculate = true;  // launch on the header remembered for the container's shape, if there is one
    bool remember = true;   // false: a sub-container must not stand in for the containers of ordinary calls of its shape
    // enqueued behind the decode's kernels and before its status read-back (the caller's gather: one host round trip less)
    const std::function<int(const u32* gflags)>* epilogue = nullptr;
};

// A decode call.  Where the call may (O.speculate) and a header is remembered for the container's shape, the first attempt
// runs on that header, `spec`, without waiting for the container's own; an attempt in vain is repeated once without.
int decode_dev(ansx_ctx* c, const Plan& Pin, const u8* d_in, size_t in_bytes, u32* d_out, hipStream_t s,
    const DecodeOpts& O = DecodeOpts())
{
    const HeaderCache::Key key = { (u64)Pin.g.kind, (u64)Pin.g.f, (u64)Pin.g.n, (u64)in_bytes };
    const ansx_container_header* spec = !Pin.plain && O.speculate ? c->hdrs.find(key) : nullptr;
    u32 how = 0;  // ANSX_DECODE_* flags of the attempt (ansx_last_decode_stats)
    for (;; c->hdrs.forget(key), spec = nullptr) {  // (at most twice: only an attempt on `spec` is repeated)
        int rc;
        if ((rc = ensure(c, c->misc, 64 + 8 * ((size_t)Pin.g.nblocks + 1)))) return rc;
        u32* gflags = (u32*)c->misc.p;
        HIPCHK(c, hipMemsetAsync(c->misc.p, 0, 64, s));
        DecodeSrc S;
        if ((rc = Pin.plain ? source_plain(c, Pin, d_in, in_bytes, s, &S) : source_container(c, Pin, d_in, in_bytes, spec, s, &S)))
            return rc;
        const ansx_geo& g = S.P.g;
        DecodeForm F = choose_decode_form(g, S.B, c->dbg, c->num_cus);
        if (F.needs_index) {
            if (spec) continue;  // (a read-back follows anyway: nothing to gain from the remembered header)
            LAUNCH(c, "k_validate_index", k_validate_index, (g.nblocks + 255) / 256, 256, 0, s, g, S.boff, S.B.payload_bytes, gflags);
            // the index must be sane before any block is touched
            HIPCHK(c, hipMemcpyAsync(c->pin->flags, c->misc.p, 16, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (c->pin->flags[ANSX_G_ERR]) return flags_to_status(c->pin->flags[ANSX_G_ERR]);
            S.B.max_block_bytes = c->pin->flags[ANSX_G_PAD];
            F = choose_decode_form(g, S.B, c->dbg, c->num_cus);
            how |= ANSX_DECODE_INDEX_VALIDATED;
        }
        note_decode_form(c, g, S.B, F, how | (spec ? ANSX_DECODE_ON_REMEMBERED : 0u));
        if ((rc = decode_premap(c, S, s))) return rc;
        if ((rc = g.kind == ANSX_RFOLD ? launch_decode<true>(c, S, F, d_out, s) : launch_decode<false>(c, S, F, d_out, s))) return rc;
        if (g.kind == ANSX_INT && !g.pa)
            LAUNCH(c, "k_int_unmap", k_int_unmap, g.nblocks, 256, 0, s, g, (const u32*)c->pa_alpha.p, (const uint4*)c->pa_info.p, d_out, gflags);
        if (g.pa)
            LAUNCH(c, "k_pa_unmap", k_pa_unmap, g.nblocks, 256, 0, s, g, (const u32*)c->pa_alpha.p, (const uint4*)c->pa_info.p, d_out, gflags);
        // the finish: the header the call ran on against the real one, the caller's epilogue, ONE read-back, the status
        if (spec) LAUNCH(c, "k_check_header", k_check_header, 1, 64, 0, s, d_in, *spec, gflags);
        if (O.epilogue && (rc = (*O.epilogue)(gflags))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->pin->flags, c->misc.p, 64, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (spec && (c->pin->flags[ANSX_G_ERR] & (1u << ANSX_G_HDR_BIT))) {  // another header: the slow way
            how = ANSX_DECODE_REPEATED;
            continue;
        }
        const int st = flags_to_status(c->pin->flags[ANSX_G_ERR]);
        if (!Pin.plain && !spec && st == ANSX_OK && O.remember) c->hdrs.remember(key, c->pin->hdr);
        return st;
    }
}

// --------------------------------------------------------------------------------- random access
// ansx_decode_ranges_dev / ansx_decode_device_ranges_dev, their ids variants and ansx_next_geq_dev (DESIGN.md sections
// 3a, 3f, 3g; the host path: section 5): a front builds the plan -- on the host (ansx_plan.h, range_plan; one upload) or
// on the device (the k_dr_* planner) -- and fills a RangeTail; range_tail prepares a sub-container of the touched blocks
// only (sub_prepare), builds it with k_range_index + k_range_copy, and decodes it (sub_decode: decode_dev, no cached
// header in or out) with the call's way out as the one epilogue: k_range_gather into the caller's buffer, the sums
// scan in front of it, the scan and k_ng_search, or the scan, k_isect_match and the compaction of an intersect step
// (RangeOut).

// the pinned buffer p of cap bytes holds at least `bytes` (its content is not kept)
int ensure_pinned(ansx_ctx* c, u8*& p, size_t& cap, size_t bytes)
{
    if (bytes <= cap) return ANSX_OK;
    if (p) HIPCHK(c, hipHostFree(p));
    p = nullptr;
    cap = 0;
    const size_t want = bytes + (bytes >> 3) + 4096;
    HIPCHK(c, hipHostMalloc((void**)&p, want, hipHostMallocDefault));
    cap = want;
    return ANSX_OK;
}

// ... rng_pin
int ensure_pin(ansx_ctx* c, size_t bytes) { return ensure_pinned(c, c->rng_pin, c->rng_pin_cap, bytes); }

// The source container's header, checked as decode_dev checks it, and its plan
int range_source(ansx_ctx* c, int kind, int f, const u8* d_in, size_t in_bytes, hipStream_t s, ansx_container_header* H,
    Plan* P)
{
    int rc;
    if (in_bytes < sizeof(ansx_container_header)) return ANSX_ERR_FORMAT;
    const u8* hp = (const u8*)&c->pin->hdr;
    HIPCHK(c, hipMemcpyAsync(&c->pin->hdr, d_in, sizeof(ansx_container_header), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = parse_header(hp, in_bytes, H))) return rc;  // (a single-stream stream has no magic: ANSX_ERR_FORMAT)
    if ((rc = container_plan(*H, (u32)kind, (u32)f, in_bytes, P))) return rc;
    P->g.payload_bytes = H->payload_bytes;  // (index_entry_ok on the source's entries)
    return ANSX_OK;
}

// The layout of a plan upload: 16-byte-aligned sections back to back in the pinned page, which go to the device in one
// copy.  add() places a section (none of the three a pass may do without: an empty one is nowhere); its handle gives its typed address on either side once upload_room has found room.
struct Upload {
    template <class T> struct Sec {
        size_t off, bytes;
    };
    size_t end = 0;
    u8 *host = nullptr, *devp = nullptr;
    template <class T> Sec<T> add(size_t n)
    {
        const size_t o = n ? rup(end, 16) : end;  // (an empty section takes no room, not even padding)
        end = o + sizeof(T) * n;
        return { o, sizeof(T) * n };
    }
    template <class T> T* pin(Sec<T> s) const { return (T*)(host + s.off); }
    template <class T> T* dev(Sec<T> s) const { return (T*)(devp + s.off); }
    template <class T> void put(Sec<T> s, const T* p) const { memcpy(host + s.off, p, s.bytes); }
};

// The pinned page and `buf` hold the sections (no copy out of the page is pending: every user ends in a synchronisation)
int upload_room(ansx_ctx* c, Upload& U, DevBuf& buf)
{
    int rc;
    if ((rc = ensure_pin(c, U.end)) || (rc = ensure(c, buf, U.end))) return rc;
    U.host = c->rng_pin, U.devp = (u8*)buf.p;
    return ANSX_OK;
}

// What the ranges and batch entries share: a container built on the device from blocks of other containers, decoded to
// a work list the caller's way out reads.  Three steps, the caller's launches between them:
//   sub_prepare  the sub-container's plan and header, room for it and for the work list.  T blocks and n_sub ints in
//                the geometry of header H (any n_sub that makes make_plan lay out exactly T blocks; bout / list_ints:
//                the decoders' table over a list of so many ints, or null / n_sub), a payload of at most cap_pay bytes;
//   the build    k_range_index + k_range_copy or k_batch_index + k_batch_copy write it (payload_bytes is theirs to
//                fill in), enqueued by the caller;
//   sub_decode   decode_dev on it -- no remembered header in or out -- with ONE epilogue: the caller's way out (given
//                the decode's flags: it skips when they hold an error) and the read-back of dflags, the build's own
//                flag word, both riding on the decode's final read-back.
struct Sub {
    Plan P;
    ansx_container_header H;
    u8* cont;
    u32* list;
    u64 bytes, cap_pay;
    ansx_range_lay lay() const { return { P.lay.ckoff_off, P.lay.ckstate_off, P.lay.hint_off, P.lay.payload_off }; }
};

int sub_prepare(ansx_ctx* c, int kind, int f, const ansx_container_header& H, u64 n_sub, u32 T, u64 cap_pay, u64 list_ints,
    const ansx_blk_out* bout, Sub* S)
{
    int rc;
    const ansx_opts o = container_opts(H);
    if (make_plan(kind, f, (size_t)n_sub, &o, &S->P)) return ANSX_ERR_FORMAT;
    set_restart_format(&S->P, (H.kind & ANSX_KIND_WIDE_RESTART) != 0);
    if (S->P.g.nblocks != T || S->P.g.nckf != H.ckpts_per_block) return ANSX_ERR_FORMAT;
    S->P.bout = bout, S->P.bout_ints = list_ints;
    S->H = H;
    S->H.n = n_sub, S->H.nblocks = T, S->H.payload_bytes = 0, S->H.payload_offset = S->P.lay.payload_off;
    S->bytes = S->P.lay.payload_off + cap_pay, S->cap_pay = cap_pay;
    if ((rc = ensure(c, c->rng_cont, S->bytes + 64))) return rc;
    if ((rc = ensure(c, c->rng_list, 4 * list_ints + 64))) return rc;
    S->cont = (u8*)c->rng_cont.p, S->list = (u32*)c->rng_list.p;
    return ANSX_OK;
}

template <class WayOut> int sub_decode(ansx_ctx* c, const Sub& S, const u32* dflags, const WayOut& way_out, hipStream_t s)
{
    u32* hflag = &c->pin->caller_flag;
    *hflag = 0;
    const std::function<int(const u32*)> epilogue = [&](const u32* gflags) -> int {
        int rc;
        if ((rc = way_out((u32*)gflags))) return rc;
        HIPCHK(c, hipMemcpyAsync(hflag, dflags, 4, hipMemcpyDeviceToHost, s));
        return ANSX_OK;
    };
    DecodeOpts O;
    O.speculate = O.remember = false, O.epilogue = &epilogue;
    const int rc = decode_dev(c, S.P, S.cont, (size_t)S.bytes, S.list, s, O);
    return *hflag ? ANSX_ERR_FORMAT : rc;  // (the flag: an index entry of one of its blocks was invalid)
}

// What becomes of the decoded work list on a call's way out
enum WayOutKind {
    OUT_GATHER,       // its ranges are copied to the caller's buffer
    OUT_SUMS_GATHER,  // it becomes running sums from the caller's block bases first, in place (DESIGN.md sections 3f, 3h)
    OUT_SUMS_SEARCH,  // ... and the targets are searched in them, in the gather's place (sections 3g, 3h)
    OUT_SUMS_MATCH,   // ... or matched against them and the members compacted (section 3i)
};

// The workspace of an intersect step's match and compaction (ansx_intersect.h) over nc candidates, 16-byte aligned:
// total u64[2] | tile counts u64[ntiles] | ballots u64[ceil(nc / 64)] | pos u64[nc] when positions are asked for.
// 8 bytes per 64 candidates, 8 per tile and, with positions, 8 per candidate.
struct IsectWork {
    u64 *total, *counts, *ballots, *wpos;
    u32 ntiles;
    static size_t bytes(u64 nc, bool pos)
    {
        return 16 + 8 * (size_t)((nc + ANSX_ISECT_TILE - 1) / ANSX_ISECT_TILE) + 8 * (size_t)((nc + 63) / 64) + (pos ? 8 * (size_t)nc : 0);
    }
    IsectWork() : total(nullptr), counts(nullptr), ballots(nullptr), wpos(nullptr), ntiles(0) {}
    IsectWork(u8* w, u64 nc, bool pos)
    {
        ntiles = (u32)((nc + ANSX_ISECT_TILE - 1) / ANSX_ISECT_TILE);
        total = (u64*)w, counts = total + 2, ballots = counts + ntiles, wpos = pos ? ballots + (nc + 63) / 64 : nullptr;
    }
};

// The outputs of an intersect step: device arrays of cap entries, any but not all of them null
struct IsectOut {
    u32 *ids, *idx;
    u64* pos;
    u64 cap;
};

// What both forms of the match end in, enqueued in the decode's epilogue behind k_isect_match / k_isect_match_full:
// the scan of the tile counts, the compaction, and the total on its way home with the decode's final read-back.
int isect_compact(ansx_ctx* c, const IsectWork& W, const u32* d_cand, u32 nc, const IsectOut& o, const u32* gflags,
    const u32* dflags, hipStream_t s);

// the largest block the one-kernel scan takes
u64 range_sums_wg_max(const ansx_ctx* c)
{
    return std::max<u64>(c->dbg.range_sums_wg_max ? c->dbg.range_sums_wg_max : ANSX_RS_WG_MAX, ANSX_RS_CHUNK);
}

// the aggregates of the three-phase scan, for the blocks it is used on: one per chunk of every touched block
int range_sums_workspace(ansx_ctx* c, u64 bi, u64 T, u64** agg)
{
    int rc;
    *agg = nullptr;
    if (bi <= range_sums_wg_max(c)) return ANSX_OK;
    const u64 tiles = T * ((bi + ANSX_RS_TILE - 1) / ANSX_RS_TILE);
    if (tiles > 0x7FFFFFFFull) return ANSX_ERR_ARG;
    if ((rc = ensure(c, c->sums_plan, 8 * (size_t)tiles * (ANSX_RS_NT / 64u)))) return rc;
    *agg = (u64*)c->sums_plan.p;
    return ANSX_OK;
}

// The work list of T touched blocks (n_sub ints, blocks of bi) -> its running sums from bases[tb[k]], in place, and the
// check of the bases into gflags.  Enqueued between the decode and the gather; no synchronisation.
int range_sums_scan(ansx_ctx* c, u32* list, u64 n_sub, u64 bi, u64 T, const u32* dtb, u32 nblocks, const u32* d_bases,
    u64* agg, u32* gflags, hipStream_t s)
{
    if (bi <= ANSX_RS_CHUNK) {
        LAUNCH(c, "k_rs_scan_small", k_rs_scan_small, (u32)((T + 3) / 4), ANSX_RS_NT, 0, s, list, n_sub, (u32)bi, (u32)T, dtb,
            nblocks, d_bases, gflags);
    } else if (bi <= range_sums_wg_max(c)) {
        LAUNCH(c, "k_rs_scan_block", k_rs_scan_block, (u32)T, ANSX_RS_NT, 0, s, list, n_sub, (u32)bi, dtb, nblocks, d_bases,
            gflags);
    } else {
        const u32 tpb = (u32)((bi + ANSX_RS_TILE - 1) / ANSX_RS_TILE), grid = (u32)(T * tpb);
        LAUNCH(c, "k_rs_reduce", k_rs_reduce, grid, ANSX_RS_NT, 0, s, (const u32*)list, n_sub, (u32)bi, (u32)T, tpb, agg,
            (const u32*)gflags);
        LAUNCH(c, "k_rs_carry", k_rs_carry, (u32)T, ANSX_RS_NT, 0, s, agg, tpb * (ANSX_RS_NT / 64u), dtb, nblocks, d_bases,
            gflags);
        LAUNCH(c, "k_rs_apply", k_rs_apply, grid, ANSX_RS_NT, 0, s, list, n_sub, (u32)bi, tpb, (const u64*)agg,
            (const u32*)gflags);
    }
    return ANSX_OK;
}

// The way out of a call on one container, with what each kind needs: the gathers' destination; for the sums the
// caller's block bases, nbases of them; for ansx_next_geq_dev (ansx_nextgeq.h) the nt targets and
// the outputs, and the ranges made of the targets -- first / count by k_ng_locate, offsets by the planner -- which the
// device front fills in in its own copy.
struct RangeOut {
    WayOutKind kind;
    u32* d_out;
    const u32* d_bases;
    size_t nbases;
    const u32* d_targets;
    u32 nt;
    u64* d_pos;
    u32* d_ids;
    const u64 *first, *offsets;
    const u32* count;
    IsectOut isect;  // OUT_SUMS_MATCH: the targets are the candidates; d_pos, d_ids are not used
    IsectWork iw;    // ... and its workspace, the device front's to fill in
};

// What both fronts hand to the tail, the plan on the device: the source container, its header and plan; tb[T] the
// touched blocks (ascending, unique; last_b the last); R the pieces of the nr non-empty ranges, pstart[nr + 1] their
// first gather pieces of npieces; dflags: a zeroed word.
struct RangeTail {
    const u8* d_in;
    ansx_container_header H;
    Plan P;
    u64 T, last_b;
    const u32 *dtb, *pstart;
    const ansx_range_piece* R;
    u32 nr;
    u64 npieces;
    u32* dflags;
};

// The tail both fronts share: prepare the sub-container of the touched blocks, build it, decode it, and out
int range_tail(ansx_ctx* c, int kind, int f, const RangeTail& t, const RangeOut& out, hipStream_t s)
{
    int rc;
    const Plan& P = t.P;
    const u64 n = t.H.n, bi = P.g.block_ints, T = t.T;
    const u64 n_sub = (T - 1) * bi + std::min<u64>(bi, n - t.last_b * bi);  // (only the source's last block can be short: it sorts last)
    u64* agg = nullptr;
    if (out.kind != OUT_GATHER && (rc = range_sums_workspace(c, bi, T, &agg))) return rc;  // (here: growing it may wait for the device)
    // (max_present_m1, max_nsyms, max_log2_frame are bounds over the blocks: they hold for any subset)
    const u64 cap_pay = std::min<u64>(t.H.payload_bytes, T * (u64)block_bound(kind, (u32)f, P.g.block_ints, P.g.pa != 0));
    Sub sub;
    if ((rc = sub_prepare(c, kind, f, t.H, n_sub, (u32)T, cap_pay, n_sub, nullptr, &sub))) return rc;
    const ansx_range_lay sl = { P.lay.ckoff_off, P.lay.ckstate_off, P.lay.hint_off, P.lay.payload_off };
    LAUNCH(c, "k_range_index", k_range_index, 1, 1024, 0, s, t.d_in, P.g, t.dtb, (u32)T, sub.H, sub.cont, cap_pay, t.dflags);
    LAUNCH(c, "k_range_copy", k_range_copy, (u32)T, 256, 0, s, t.d_in, P.g, sl, sub.lay(), t.dtb, sub.cont, cap_pay, t.dflags);
    return sub_decode(c, sub, t.dflags, [&](u32* gflags) -> int {
        // (the sums: the work list becomes ids first, in place; the scan reports foreign bases in gflags)
        if (out.kind != OUT_GATHER
            && (rc = range_sums_scan(c, sub.list, n_sub, bi, T, t.dtb, P.g.nblocks, out.d_bases, agg, gflags, s)))
            return rc;
        if (out.kind == OUT_SUMS_SEARCH) {
            LAUNCH(c, "k_ng_search", k_ng_search, (out.nt + ANSX_NG_NT - 1) / ANSX_NG_NT, ANSX_NG_NT, 0, s, (const u32*)sub.list,
                n_sub, bi, n, out.d_targets, out.nt, out.first, out.count, out.offsets, t.R, out.d_pos, out.d_ids,
                (const u32*)gflags, (const u32*)t.dflags);
            return ANSX_OK;
        }
        if (out.kind == OUT_SUMS_MATCH) {
            LAUNCH(c, "k_isect_match", k_isect_match, out.iw.ntiles, ANSX_ISECT_NT, 0, s, (const u32*)sub.list, n_sub, bi,
                out.d_targets, out.nt, out.first, out.count, out.offsets, t.R, out.iw.ballots, out.iw.counts, out.iw.wpos,
                (const u32*)gflags, (const u32*)t.dflags);
            return isect_compact(c, out.iw, out.d_targets, out.nt, out.isect, gflags, t.dflags, s);
        }
        const u32 grid = (u32)std::min<u64>(t.npieces, 1u << 20);
        LAUNCH(c, "k_range_gather", k_range_gather, grid, 256, 0, s, (const u32*)sub.list, t.R, t.pstart, t.nr, (u32)t.npieces,
            out.d_out, (const u32*)gflags);
        return ANSX_OK;
    }, s);
}

// ansx_decode_ranges_dev: the plan built on the host from host arrays (ansx_plan.h, range_plan), uploaded in one copy
int decode_ranges(ansx_ctx* c, int kind, int f, const u8* d_in, size_t in_bytes, const u64* first, const u32* count,
    size_t nranges, size_t cap, const RangeOut& out, hipStream_t s)
{
    int rc;
    RangeTail t = { d_in };
    if ((rc = range_source(c, kind, f, d_in, in_bytes, s, &t.H, &t.P))) return rc;
    if (out.kind != OUT_GATHER && out.nbases != (size_t)t.P.g.nblocks + 1) return ANSX_ERR_ARG;
    RangePlan R;
    if ((rc = range_plan(t.H.n, t.P.g.block_ints, first, count, nranges, cap, &R))) return rc;
    if (R.total == 0) return ANSX_OK;
    // the plan on the device, one upload: flags[4] | touched blocks u32[T] | range pieces | first piece per range u32[nr + 1]
    Upload U;
    const auto s_fl = U.add<u32>(4);
    const auto s_tb = U.add<u32>(R.tb.size());
    const auto s_pc = U.add<ansx_range_piece>(R.pieces.size());
    const auto s_ps = U.add<u32>(R.pstart.size());
    if ((rc = upload_room(c, U, c->rng_plan))) return rc;
    memset(U.pin(s_fl), 0, s_fl.bytes);
    U.put(s_tb, R.tb.data()), U.put(s_pc, R.pieces.data()), U.put(s_ps, R.pstart.data());
    HIPCHK(c, hipMemcpyAsync(U.devp, U.host, U.end, hipMemcpyHostToDevice, s));
    t.T = R.T, t.last_b = R.last_b, t.dtb = U.dev(s_tb), t.R = U.dev(s_pc), t.pstart = U.dev(s_ps);
    t.nr = (u32)R.pieces.size(), t.npieces = R.npieces, t.dflags = U.dev(s_fl);
    return range_tail(c, kind, f, t, out, s);
}

// ansx_decode_device_ranges_dev: the plan built on the device from first / count in device memory (ansx_ranges.h,
// "device plan"); one read-back of its scalars decides the errors and sizes the tail, no O(nranges) copy either way.
// The front serves ansx_next_geq_dev too (OUT_SUMS_SEARCH; nranges targets): the ranges are then k_ng_locate's, one int
// at the start of every target's block, made in front of the planner in workspace behind its own; the planner and its
// read-back are the same, *total_ints is the number of targets found, and the tail searches instead of gathering.
// An intersect step (OUT_SUMS_MATCH, section 3i) is that search with another way out, and its workspace behind.
// device_ranges_from: the call behind the source's header, for a caller that has it already (t.d_in, t.H, t.P).
int device_ranges_from(ansx_ctx* c, int kind, int f, RangeTail t, const u64* d_first, const u32* d_count, size_t nranges,
    size_t cap, u64* d_offsets, u64* total_ints, RangeOut out, hipStream_t s)
{
    int rc;
    if (out.kind != OUT_GATHER && out.nbases != (size_t)t.P.g.nblocks + 1) return ANSX_ERR_ARG;
    const bool match = out.kind == OUT_SUMS_MATCH, search = out.kind == OUT_SUMS_SEARCH || match;
    const u64 n = t.H.n, bi = t.P.g.block_ints, nr = nranges, nb = t.P.g.nblocks;
    u32 kb = 0;  // key bits of a block id
    while ((1ull << kb) < nb) kb++;
    const u64 nt = (nr + ANSX_DR_TILE - 1) / ANSX_DR_TILE;

    // workspace: scalars u64[8] | per-tile partials u64[6 nt] | radix histogram u32[16 nt] | pieces[nr] |
    // pstart u32[nr + 1] | spans (b0, b1 + 1) twice over u32[4 nr] | tb u32[nblocks]
    const size_t o_pt = 64, o_h = o_pt + 48 * nt, o_pc = rup(o_h + 64 * nt, 16), o_ps = o_pc + sizeof(ansx_range_piece) * nr;
    const size_t o_sp = rup(o_ps + 4 * (nr + 1), 16), o_tb = o_sp + 16 * nr;
    // (ansx_next_geq_dev, behind tb: first u64[nr] | offsets u64[nr + 1] | count u32[nr])
    const size_t o_nf = rup(o_tb + 4 * nb, 16), o_no = o_nf + 8 * nr, o_nc = o_no + 8 * (nr + 1);
    const size_t o_iw = rup(o_nc + 4 * nr, 16);  // (an intersect step, behind count: IsectWork)
    const size_t bytes = match ? o_iw + IsectWork::bytes(nr, out.isect.pos != nullptr) : search ? o_nc + 4 * nr : o_tb + 4 * nb;
    if ((rc = ensure(c, c->rng_dev, bytes))) return rc;
    u8* w = (u8*)c->rng_dev.p;
    if (match) out.iw = IsectWork(w + o_iw, nr, out.isect.pos != nullptr);
    if (search) {
        u64* nf = (u64*)(w + o_nf);
        u32* nc = (u32*)(w + o_nc);
        LAUNCH(c, "k_ng_locate", k_ng_locate, (u32)((nr + ANSX_NG_TILE - 1) / ANSX_NG_TILE), ANSX_NG_NT, 0, s, out.d_bases, (u32)nb,
            bi, out.d_targets, (u32)nr, nf, nc);
        d_first = out.first = nf, d_count = out.count = nc, d_offsets = (u64*)(w + o_no), out.offsets = d_offsets;
    }
    u64* sc = (u64*)w;
    u64* part = (u64*)(w + o_pt);
    u64* partm = part + 4 * nt;
    u64* parta = part + 5 * nt;
    u32* hist = (u32*)(w + o_h);
    ansx_range_piece* R = (ansx_range_piece*)(w + o_pc);
    u32* pstart = (u32*)(w + o_ps);
    u32* kv[4] = { (u32*)(w + o_sp), (u32*)(w + o_sp) + nr, (u32*)(w + o_sp) + 2 * nr, (u32*)(w + o_sp) + 3 * nr };
    u32* tb = (u32*)(w + o_tb);
    u32 cur = 0;  // the sorted spans are kv[cur], kv[cur + 1]; the union goes to the other pair
    if (nr <= ANSX_DR_TILE) {
        LAUNCH(c, "k_dr_plan_small", k_dr_plan_small, 1, ANSX_DR_NT, 0, s, d_first, d_count, (u32)nr, n, bi, kb, d_offsets,
            R, pstart, kv[2], kv[3], parta, sc);
    } else {
        const u32 g = (u32)nt;
        LAUNCH(c, "k_dr_spans", k_dr_spans, g, ANSX_DR_NT, 0, s, d_first, d_count, nr, n, part);
        LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, false>), 1, ANSX_DR_NT, 0, s, part, nt, 4u, nt, sc, (u32*)&sc[ANSX_DR_FLAGS]);
        LAUNCH(c, "k_dr_compact", k_dr_compact, g, ANSX_DR_NT, 0, s, d_first, d_count, nr, n, bi, (const u64*)part,
            (const u64*)sc, d_offsets, kv[0], kv[1], R, pstart);
        for (u32 sh = 0; sh < kb; sh += 4) {
            LAUNCH(c, "k_dr_digit_count", k_dr_digit_count, g, ANSX_DR_NT, 0, s, kv[cur], (const u64*)sc, sh, hist);
            LAUNCH(c, "k_dr_scan", (k_dr_scan<u32, false>), 1, ANSX_DR_NT, 0, s, hist, 16 * nt, 1u, 0ull, (u64*)nullptr,
                (u32*)nullptr);
            LAUNCH(c, "k_dr_digit_scatter", k_dr_digit_scatter, g, ANSX_DR_NT, 0, s, kv[cur], kv[cur + 1], kv[2 - cur],
                kv[3 - cur], (const u64*)sc, sh, (const u32*)hist);
            cur = 2 - cur;
        }
        LAUNCH(c, "k_dr_tile_max", k_dr_tile_max, g, ANSX_DR_NT, 0, s, kv[cur + 1], (const u64*)sc, partm);
        LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, true>), 1, ANSX_DR_NT, 0, s, partm, nt, 1u, 0ull, sc + ANSX_DR_LASTB1,
            (u32*)nullptr);
        LAUNCH(c, "k_dr_adds", k_dr_adds, g, ANSX_DR_NT, 0, s, kv[cur], kv[cur + 1], (const u64*)sc, (const u64*)partm,
            kv[2 - cur], kv[3 - cur], parta);
        LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, false>), 1, ANSX_DR_NT, 0, s, parta, nt, 1u, 0ull, sc + ANSX_DR_T,
            (u32*)nullptr);
        LAUNCH(c, "k_dr_pieces", k_dr_pieces, (u32)((nr + ANSX_DR_NT - 1) / ANSX_DR_NT), ANSX_DR_NT, 0, s, R,
            (const u64*)sc, bi, kv[2 - cur], kv[3 - cur], (const u64*)parta);
    }
    const u32* S = kv[2 - cur];
    const u32* offl = kv[3 - cur];
    u64* hs = c->pin->planner;
    HIPCHK(c, hipMemcpyAsync(hs, sc, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (hs[ANSX_DR_BAD]) return ANSX_ERR_ARG;
    const u64 total = hs[ANSX_DR_TOTAL], nne = hs[ANSX_DR_NNE], npieces = hs[ANSX_DR_NPIECES], T = hs[ANSX_DR_T];
    if (total_ints) *total_ints = total;
    if (total > cap) return ANSX_ERR_CAPACITY;
    if (total == 0) {
        if (search && !match) {  // (no target found and no tail: the outputs are filled here; the call returns with them written, as ever)
            LAUNCH(c, "k_ng_none", k_ng_none, (u32)((nr + ANSX_NG_NT - 1) / ANSX_NG_NT), ANSX_NG_NT, 0, s, n, (u32)nr, out.d_pos,
                out.d_ids);
            HIPCHK(c, hipStreamSynchronize(s));
        }
        return ANSX_OK;
    }
    if (npieces > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (T == 0 || T > nb || nne == 0 || hs[ANSX_DR_LASTB1] == 0) return ANSX_ERR_HIP;  // (cannot happen: a planner fault)
    LAUNCH(c, "k_dr_blocks", k_dr_blocks, (u32)((T + ANSX_DR_NT - 1) / ANSX_DR_NT), ANSX_DR_NT, 0, s, tb, (u32)T, (u32)nne,
        S, offl, (const u64*)parta);
    t.T = T, t.last_b = hs[ANSX_DR_LASTB1] - 1, t.dtb = tb, t.R = R, t.pstart = pstart, t.nr = (u32)nne, t.npieces = npieces;
    t.dflags = (u32*)&sc[ANSX_DR_FLAGS];
    return range_tail(c, kind, f, t, out, s);
}

int decode_device_ranges(ansx_ctx* c, int kind, int f, const u8* d_in, size_t in_bytes, const u64* d_first,
    const u32* d_count, size_t nranges, size_t cap, u64* d_offsets, u64* total_ints, const RangeOut& out, hipStream_t s)
{
    int rc;
    RangeTail t = { d_in };
    if ((rc = range_source(c, kind, f, d_in, in_bytes, s, &t.H, &t.P))) return rc;
    return device_ranges_from(c, kind, f, t, d_first, d_count, nranges, cap, d_offsets, total_ints, out, s);
}

// --------------------------------------------------------------------------------- batches of containers
// ansx_decode_batch_dev: every header in one round trip (batch_headers) -> the host's checks,
// offsets and capacity -> per geometry, passes of at most P blocks built by ansx_plan::Pass: one upload of the pass's
// plan, sub_prepare, k_batch_index + k_batch_copy build a sub-container of the pass's blocks, sub_decode on it with the
// per-block table and k_range_gather into the caller's buffer as the way out.
#define ANSX_BATCH_PASS_DEFAULT 16384u  // blocks per pass: the block count of the headline container

u32 batch_pass_blocks(const ansx_ctx* c) { return c->dbg.batch_pass_blocks ? c->dbg.batch_pass_blocks : ANSX_BATCH_PASS_DEFAULT; }

// The header round trip of the batch calls, over the m containers pos[0..m) of the batch (pos null: the first m): the
// addresses up (0 for an input too short to hold a header), k_batch_headers, the headers back; then decode_dev's
// checks on every one, in that order.  ANSX_ERR_FORMAT with *bad = the first j that fails them.
int batch_headers(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, const u32* pos, size_t m,
    std::vector<BatchSrc>* src, size_t* bad, hipStream_t s)
{
    int rc;
    Upload U;
    const auto s_addr = U.add<u64>(m);
    const auto s_hdr = U.add<uint4>(4 * m);  // (comes back: only the addresses go up)
    if ((rc = upload_room(c, U, c->bat_hdr))) return rc;
    u64* addr = U.pin(s_addr);
    for (size_t j = 0; j < m; j++) {
        const size_t i = pos ? pos[j] : j;
        addr[j] = in_bytes[i] >= sizeof(ansx_container_header) ? (u64)(uintptr_t)d_ins[i] : 0;
    }
    HIPCHK(c, hipMemcpyAsync(U.devp, U.host, s_addr.bytes, hipMemcpyHostToDevice, s));
    LAUNCH(c, "k_batch_headers", k_batch_headers, (u32)((4 * (u64)m + 255) / 256), 256, 0, s, (const u64*)U.dev(s_addr), (u64)m,
        U.dev(s_hdr));
    HIPCHK(c, hipMemcpyAsync(U.pin(s_hdr), U.dev(s_hdr), 64 * m, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    src->resize(m);
    for (size_t j = 0; j < m; j++) {
        const size_t i = pos ? pos[j] : j;
        BatchSrc& b = (*src)[j];
        Plan P;
        if (in_bytes[i] < sizeof(ansx_container_header) || parse_header((const u8*)U.pin(s_hdr) + 64 * j, in_bytes[i], &b.H)
            || container_plan(b.H, (u32)kind, (u32)f, in_bytes[i], &P)) {  // (a single-stream stream has no magic)
            *bad = j;
            return ANSX_ERR_FORMAT;
        }
        b.lay = P.lay;
        b.base = (u64)(uintptr_t)d_ins[i];
        b.nblocks = P.g.nblocks;
    }
    return ANSX_OK;
}

// The loop over the geometry groups every batch call ends in: fn on each group's members; a format error from in there
// was found on the device, which container it was is not known: *bad = count.
typedef std::map<Geometry, std::vector<u32>> GeometryGroups;
template <class F> int for_each_group(const GeometryGroups& groups, size_t count, size_t* bad, const F& fn)
{
    for (const auto& gr : groups) {
        const int rc = fn(gr.second);
        if (rc == ANSX_ERR_FORMAT && bad) *bad = count;
        if (rc) return rc;
    }
    return ANSX_OK;
}

// A pass's plan on the device, one upload: flags[4] | sources | blocks | table | the caller's own sections behind them
struct PassUp {
    Upload U;
    Upload::Sec<u32> flags = U.add<u32>(4);
    Upload::Sec<ansx_batch_src> S;
    Upload::Sec<ansx_batch_blk> B;
    Upload::Sec<ansx_blk_out> O;
    explicit PassUp(const Pass& P)
        : S(U.add<ansx_batch_src>(P.S.size())), B(U.add<ansx_batch_blk>(P.B.size())), O(U.add<ansx_blk_out>(P.O.size())) {}
};

// The part every pass shares, once the caller has found room for the plan (upload_room) and put its own sections: the
// plan goes up, the sub-container of the pass's T blocks is prepared and built.  Every buffer is bounded by the pass:
// its blocks, their ints and their bytes, and the caller's sections.
int pass_build(ansx_ctx* c, int kind, int f, const Pass& P, const PassUp& D, Sub* sub, hipStream_t s)
{
    int rc;
    const u32 T = (u32)P.B.size();
    memset(D.U.pin(D.flags), 0, D.flags.bytes);
    D.U.put(D.S, P.S.data()), D.U.put(D.B, P.B.data()), D.U.put(D.O, P.O.data());
    HIPCHK(c, hipMemcpyAsync(D.U.devp, D.U.host, D.U.end, hipMemcpyHostToDevice, s));
    // (any n that makes make_plan lay out exactly T blocks: the table says how long each is)
    if ((rc = sub_prepare(c, kind, f, P.Hs, (u64)(T - 1) * P.Hs.block_ints + P.O.back().n, T, P.cap_pay, P.wl, D.U.dev(D.O), sub)))
        return rc;
    u32* dflags = D.U.dev(D.flags);
    LAUNCH(c, "k_batch_index", k_batch_index, 1, 1024, 0, s, (const ansx_batch_src*)D.U.dev(D.S), (const ansx_batch_blk*)D.U.dev(D.B),
        sub->P.g, T, sub->H, sub->cont, P.cap_pay, dflags);
    LAUNCH(c, "k_batch_copy", k_batch_copy, T, 256, 0, s, (const ansx_batch_src*)D.U.dev(D.S), (const ansx_batch_blk*)D.U.dev(D.B),
        sub->P.g, sub->lay(), sub->cont, P.cap_pay, dflags);
    return ANSX_OK;
}

// One pass over containers ids[*ci..] of one geometry, from block *b0 of the first, up to PB blocks; moves *ci / *b0
// past them.
int batch_pass(ansx_ctx* c, int kind, int f, const std::vector<BatchSrc>& src, const std::vector<u64>& off,
    const std::vector<u32>& ids, size_t* ci, u32* b0, u32 PB, u32* d_out, hipStream_t s)
{
    int rc;
    const ansx_container_header& H0 = src[ids[*ci]].H;
    const u64 bbound = block_bound(kind, (u32)f, (size_t)H0.block_ints, (H0.kind & 0x100u) != 0);
    Pass P;
    std::vector<ansx_range_piece> R;
    std::vector<u32> pstart;
    const u64 npieces = batch_pass_plan(src, off, ids, ci, b0, PB, bbound, &P, &R, &pstart);
    if (npieces > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    const u32 nr = (u32)R.size();
    PassUp D(P);
    const auto s_r = D.U.add<ansx_range_piece>(nr);  // the gather's pieces | first piece per source
    const auto s_ps = D.U.add<u32>((size_t)nr + 1);
    if ((rc = upload_room(c, D.U, c->rng_plan))) return rc;
    D.U.put(s_r, R.data()), D.U.put(s_ps, pstart.data());
    Sub sub;
    if ((rc = pass_build(c, kind, f, P, D, &sub, s))) return rc;
    return sub_decode(c, sub, D.U.dev(D.flags), [&](u32* gflags) -> int {
        const u32 grid = (u32)std::min<u64>(npieces, 1u << 20);
        LAUNCH(c, "k_range_gather", k_range_gather, grid, 256, 0, s, (const u32*)sub.list, (const ansx_range_piece*)D.U.dev(s_r),
            (const u32*)D.U.dev(s_ps), nr, (u32)npieces, d_out, (const u32*)gflags);
        return ANSX_OK;
    }, s);
}

// The containers of `groups` (members of src, by geometry) whole, src[i] to off[i] of d_out, in passes of at most
// ANSX_BATCH_PASS_BLOCKS blocks.  A format error found on the device: *bad_index = count.
int batch_decode_groups(ansx_ctx* c, int kind, int f, const std::vector<BatchSrc>& src, const std::vector<u64>& off,
    const GeometryGroups& groups, size_t count, u32* d_out, size_t* bad_index, hipStream_t s)
{
    const u32 PB = batch_pass_blocks(c);
    return for_each_group(groups, count, bad_index, [&](const std::vector<u32>& ids) -> int {
        int rc;
        size_t ci = 0;
        u32 b0 = 0;
        while (ci < ids.size())
            if ((rc = batch_pass(c, kind, f, src, off, ids, &ci, &b0, PB, d_out, s))) return rc;
        return ANSX_OK;
    });
}

int decode_batch(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, size_t count,
    u32* d_out, size_t cap, u64* offsets, u64* total_ints, size_t* bad_index, hipStream_t s)
{
    int rc;
    std::vector<BatchSrc> src;
    size_t bad = count;
    if ((rc = batch_headers(c, kind, f, d_ins, in_bytes, nullptr, count, &src, &bad, s))) {
        if (rc == ANSX_ERR_FORMAT && bad_index) *bad_index = bad;
        return rc;
    }
    // the offsets and the total, in batch order
    std::vector<u64> off(count + 1);
    u64 total = 0;
    for (size_t i = 0; i < count; i++) {
        off[i] = total;
        total = src[i].H.n > ~0ull - total ? ~0ull : total + src[i].H.n;  // (saturated: no buffer holds that many)
    }
    off[count] = total;
    if (offsets) memcpy(offsets, off.data(), 8 * (count + 1));
    if (total_ints) *total_ints = total;
    if (total > cap) return ANSX_ERR_CAPACITY;

    // groups of one geometry, batch order inside each
    GeometryGroups groups;
    for (size_t i = 0; i < count; i++) groups[br_geometry(src[i].H)].push_back((u32)i);
    return batch_decode_groups(c, kind, f, src, off, groups, count, d_out, bad_index, s);
}

// --------------------------------------------------------------------------------- ranges of a batch
// ansx_decode_batch_ranges_dev: the REFERENCED containers (ansx_plan.h, br_refs) and their
// headers in one round trip (batch_headers) -> the host's checks, offsets and capacity -> per geometry, the touched
// (container, block) pairs, sorted and unique, in passes of at most P (br_runs, br_pieces, Pass): each pass as one of
// ansx_decode_batch_dev, with the way out the call names -- k_piece_gather, the scan in front of it, or the scan and
// k_ngb_search.

// The way out of a batch call, with what each kind needs: the gather's destination; for the sums (DESIGN.md section
// 3h, ansx_batchrangesums.h) the caller's bases of every referenced container; for ansx_next_geq_batch_dev the targets
// and the outputs.
struct BatchOut {
    WayOutKind kind;
    u32* d_out;
    std::vector<const u32*> bases;
    const u32* d_targets;
    u64* d_pos;
    u32* d_ids;
};

// The work list of a pass of T blocks (geometry bi; O, B: its table and blocks on the device, SB: its sources' bases) ->
// its running sums in place, every block from its own container's base, and the check of the bases into gflags.
// Enqueued between the pass's decode and its gather; no synchronisation.  range_sums_scan's shapes and switch.
int batch_sums_scan(ansx_ctx* c, u32* list, u64 bi, u32 T, const ansx_blk_out* O, const ansx_batch_blk* B,
    const ansx_brs_src* SB, u64* agg, u32* gflags, hipStream_t s)
{
    if (bi <= ANSX_RS_CHUNK) {
        LAUNCH(c, "k_brs_scan_small", k_brs_scan_small, (T + 3) / 4, ANSX_RS_NT, 0, s, list, O, B, SB, T, gflags);
    } else if (bi <= range_sums_wg_max(c)) {
        LAUNCH(c, "k_brs_scan_block", k_brs_scan_block, T, ANSX_RS_NT, 0, s, list, O, B, SB, gflags);
    } else {
        const u32 tpb = (u32)((bi + ANSX_RS_TILE - 1) / ANSX_RS_TILE), grid = T * tpb;
        LAUNCH(c, "k_brs_reduce", k_brs_reduce, grid, ANSX_RS_NT, 0, s, (const u32*)list, O, tpb, agg, (const u32*)gflags);
        LAUNCH(c, "k_brs_carry", k_brs_carry, T, ANSX_RS_NT, 0, s, agg, tpb * (ANSX_RS_NT / 64u), B, SB, gflags);
        LAUNCH(c, "k_brs_apply", k_brs_apply, grid, ANSX_RS_NT, 0, s, list, O, tpb, (const u64*)agg, (const u32*)gflags);
    }
    return ANSX_OK;
}

// The ranges `ids` (non-empty, in range order) of one geometry; rs: the referenced containers, rid[i] / off[i]: range
// i's container among them and its place in d_out (OUT_SUMS_SEARCH: the target's index).
int batch_ranges_group(ansx_ctx* c, int kind, int f, const std::vector<BatchSrc>& rs, const std::vector<u32>& rid,
    const u64* first, const u32* cnt, const std::vector<u64>& off, const std::vector<u32>& ids, u32 PB, const BatchOut& out,
    hipStream_t s)
{
    int rc;
    const ansx_container_header& H0 = rs[rid[ids[0]]].H;
    const u64 bi = H0.block_ints;
    const u64 bbound = block_bound(kind, (u32)f, (size_t)bi, (H0.kind & 0x100u) != 0);
    const bool sums = out.kind != OUT_GATHER, search = out.kind == OUT_SUMS_SEARCH;
    std::vector<BrRun> runs;
    br_runs(rs, rid, first, cnt, ids, bi, PB, &runs);
    std::vector<ansx_piece> PP;
    std::vector<u64> PC, pfirst;
    std::vector<u32> PK;  // (the search: every piece's block of its pass)
    br_pieces(rs, rid, first, cnt, off, ids, bi, runs, &PP, &PC, &pfirst, search ? &PK : nullptr);
    const u32 npass = runs.back().pass + 1;

    Pass P;
    size_t k = 0;
    for (u32 p = 0; p < npass; p++) {
        k = P.take_runs(H0, rs, runs, k, p, bi, bbound);
        const u64 np = pfirst[p + 1] - pfirst[p];
        if (np > 0xFFFFFFFFull) return ANSX_ERR_ARG;
        const u32 T = (u32)P.B.size();
        // behind the pass's own sections: pieces | their exclusive prefix over the pass -- or, for the search, where a
        // piece is one int at the start of a block, that block of the pass in the prefix's place | the sources' bases
        PassUp D(P);
        Upload& U = D.U;
        const auto s_pp = U.add<ansx_piece>(np);
        const auto s_pk = U.add<u32>(search ? np : 0);
        const auto s_wp = U.add<u64>(search ? 0 : np + 1);
        const auto s_sb = U.add<ansx_brs_src>(sums ? P.cont.size() : 0);
        u64* agg = nullptr;
        if (sums && (rc = range_sums_workspace(c, bi, T, &agg))) return rc;  // (here: growing it may wait for the device)
        if ((rc = upload_room(c, U, c->rng_plan))) return rc;
        U.put(s_pp, PP.data() + pfirst[p]);
        u64 ints = 0;
        if (search) U.put(s_pk, PK.data() + pfirst[p]);
        else {
            u64* wpos = U.pin(s_wp);
            for (u64 q = 0; q < np; q++) wpos[q] = ints, ints += PC[pfirst[p] + q];
            wpos[np] = ints;
        }
        for (size_t j = 0; sums && j < P.cont.size(); j++)
            U.pin(s_sb)[j] = { (u64)(uintptr_t)out.bases[P.cont[j]], rs[P.cont[j]].nblocks, 0 };
        Sub sub;
        if ((rc = pass_build(c, kind, f, P, D, &sub, s))) return rc;
        rc = sub_decode(c, sub, U.dev(D.flags), [&](u32* gflags) -> int {
            int st;
            // (the sums: the work list becomes ids first, in place; the scan reports foreign bases in gflags)
            if (sums && (st = batch_sums_scan(c, sub.list, bi, T, U.dev(D.O), U.dev(D.B), U.dev(s_sb), agg, gflags, s))) return st;
            if (search) {
                LAUNCH(c, "k_ngb_search", k_ngb_search, (u32)((np + ANSX_NGB_NT - 1) / ANSX_NGB_NT), ANSX_NGB_NT, 0, s,
                    (const u32*)sub.list, (const ansx_blk_out*)U.dev(D.O), (const ansx_batch_blk*)U.dev(D.B), T, bi,
                    (const ansx_piece*)U.dev(s_pp), (const u32*)U.dev(s_pk), (u32)np, out.d_targets, out.d_pos, out.d_ids,
                    (const u32*)gflags, (const u32*)U.dev(D.flags));
                return ANSX_OK;
            }
            const u32 grid = (u32)std::min<u64>((ints + ANSX_PIECE_CHUNK - 1) / ANSX_PIECE_CHUNK, 1u << 20);
            LAUNCH(c, "k_piece_gather", k_piece_gather, grid, 256, 0, s, (const u32*)sub.list, (const ansx_piece*)U.dev(s_pp),
                (const u64*)U.dev(s_wp), (u32)np, ints, out.d_out, (const u32*)gflags);
            return ANSX_OK;
        }, s);
        if (rc) return rc;
    }
    return ANSX_OK;
}

// The front half every call on ranges of a batch shares (src: the container every range or target names): the
// referenced containers `ref`, every range's place among them `rid`, and their checked headers `rs`.  nbases (the
// sums): every referenced container's count of bases against its blocks, behind the header checks.
struct BrFront {
    std::vector<u32> ref, rid;
    std::vector<BatchSrc> rs;
};
int batch_ranges_front(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, size_t count,
    const u32* src, size_t nranges, const size_t* nbases, BrFront* F, size_t* bad_container, hipStream_t s)
{
    int rc;
    br_refs(src, nranges, count, &F->ref, &F->rid);  // (nothing below looks at any other container)
    const std::vector<u32>& ref = F->ref;
    size_t bad = 0;
    if ((rc = batch_headers(c, kind, f, d_ins, in_bytes, ref.data(), ref.size(), &F->rs, &bad, s))) {
        if (rc == ANSX_ERR_FORMAT && bad_container) *bad_container = ref[bad];
        return rc;
    }
    if (nbases)
        for (size_t j = 0; j < ref.size(); j++)
            if (nbases[ref[j]] != (size_t)F->rs[j].nblocks + 1) {
                if (bad_container) *bad_container = ref[j];
                return ANSX_ERR_ARG;
            }
    return ANSX_OK;
}

// d_bases / nbases (the sums): those of every container of the batch, HOST arrays; null for the plain call
int decode_batch_ranges(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, size_t count,
    const u32* src, const u64* first, const u32* cnt, size_t nranges, u32* d_out, size_t cap, u64* offsets, u64* total_ints,
    size_t* bad_container, size_t* bad_range, const u32* const* d_bases, const size_t* nbases, hipStream_t s)
{
    int rc;
    BrFront F;
    if ((rc = batch_ranges_front(c, kind, f, d_ins, in_bytes, count, src, nranges, nbases, &F, bad_container, s))) return rc;
    const std::vector<u32>& rid = F.rid;
    const std::vector<BatchSrc>& rs = F.rs;
    // every range against its own container's n; the offsets and the total
    std::vector<u64> off(nranges + 1);
    u64 total = 0;
    for (size_t i = 0; i < nranges; i++) {
        const u64 n = rs[rid[i]].H.n;
        if (first[i] > n || (u64)cnt[i] > n - first[i]) {
            if (bad_range) *bad_range = i;
            return ANSX_ERR_ARG;
        }
        off[i] = total;
        total += cnt[i];  // (at most 2^32 - 1 per range, at most 2^32 - 1 ranges: no wrap)
    }
    off[nranges] = total;
    if (offsets) memcpy(offsets, off.data(), 8 * (nranges + 1));
    if (total_ints) *total_ints = total;
    if (total > cap) return ANSX_ERR_CAPACITY;
    if (total == 0) return ANSX_OK;

    // the non-empty ranges by geometry, range order inside
    GeometryGroups groups;
    for (size_t i = 0; i < nranges; i++)
        if (cnt[i]) groups[br_geometry(rs[rid[i]].H)].push_back((u32)i);
    BatchOut out = { d_bases ? OUT_SUMS_GATHER : OUT_GATHER, d_out, {}, nullptr, nullptr, nullptr };
    for (size_t j = 0; d_bases && j < F.ref.size(); j++) out.bases.push_back(d_bases[F.ref[j]]);  // (the referenced containers')
    const u32 PB = batch_pass_blocks(c);
    return for_each_group(groups, count, bad_container, [&](const std::vector<u32>& ids) -> int {
        return batch_ranges_group(c, kind, f, rs, rid, first, cnt, off, ids, PB, out, s);
    });
}

// ansx_decode_batch_device_ranges_dev ("device plan"; ansx_batchdevranges.h): src / first / cnt
// are device arrays, and nothing here is O(nranges).  Three waits before the passes: the front's scalars (how many
// containers are referenced), their headers, and the planner's scalars with every pass's.
//   front  the addresses and sizes of all `count` containers go up unjudged; k_bdr_mark, k_bdr_slots
//   host   batch_headers' checks on the referenced containers; the geometry groups; per referenced container its
//          ansx_bdr_ref, ansx_batch_src and (the sums) ansx_brs_src, in the order of the global blocks: one upload
//   plan   section 3a's planner over the global blocks, then the pass scalars
//   pass   k_bdr_pass_table and the pieces on the device in pass_build's place, then the pass of the host-array call
int decode_batch_device_ranges(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, size_t count,
    const u32* d_src, const u64* d_first, const u32* d_cnt, size_t nranges, u32* d_out, size_t cap, u64* d_offsets,
    u64* total_ints, size_t* bad_container, size_t* bad_range, const u32* const* d_bases, const size_t* nbases, hipStream_t s)
{
    int rc;
    const bool sums = d_bases != nullptr;
    const u64 nr = nranges, nt = (nr + ANSX_DR_TILE - 1) / ANSX_DR_TILE;
    const u32 g_nr = (u32)((nr + ANSX_DR_NT - 1) / ANSX_DR_NT);

    // ---- front: scalars | addresses | sizes | bases | marks go up; slots, the referenced list and its addresses stay
    const size_t mref = (size_t)std::min<u64>(count, nr);
    Upload F;
    const auto f_sc = F.add<u64>(ANSX_BDR_F_SCALARS);
    const auto f_addr = F.add<u64>(count);
    const auto f_inb = F.add<u64>(count);
    const auto f_bas = F.add<u64>(sums ? count : 0);
    const auto f_mark = F.add<u32>(count);
    const size_t f_up = F.end;
    const auto f_slot = F.add<u32>(count);
    const auto f_ref = F.add<u32>(mref);
    const auto f_ra = F.add<u64>(mref);
    if ((rc = ensure_pin(c, f_up)) || (rc = ensure(c, c->bat_hdr, F.end))) return rc;
    F.host = c->rng_pin, F.devp = (u8*)c->bat_hdr.p;
    memset(F.pin(f_sc), 0, f_sc.bytes);
    F.pin(f_sc)[ANSX_BDR_F_BADSRC] = F.pin(f_sc)[ANSX_BDR_F_BADPTR] = ~0ull;
    memcpy(F.pin(f_addr), d_ins, 8 * count);  // (unjudged: a container no range names may be null)
    memcpy(F.pin(f_inb), in_bytes, 8 * count);
    if (sums) memcpy(F.pin(f_bas), d_bases, 8 * count);
    memset(F.pin(f_mark), 0, f_mark.bytes);
    HIPCHK(c, hipMemcpyAsync(F.devp, F.host, f_up, hipMemcpyHostToDevice, s));
    LAUNCH(c, "k_bdr_mark", k_bdr_mark, g_nr, ANSX_DR_NT, 0, s, d_src, nr, (u32)count, (const u64*)F.dev(f_addr),
        (const u64*)(sums ? F.dev(f_bas) : nullptr), F.dev(f_mark), F.dev(f_sc));
    LAUNCH(c, "k_bdr_slots", k_bdr_slots, 1, ANSX_DR_NT, 0, s, (const u32*)F.dev(f_mark), (u32)count, (const u64*)F.dev(f_addr),
        (const u64*)F.dev(f_inb), F.dev(f_slot), F.dev(f_ref), F.dev(f_ra), F.dev(f_sc));
    u64* hs = c->pin->planner;
    HIPCHK(c, hipMemcpyAsync(hs, F.dev(f_sc), 64, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (hs[ANSX_BDR_F_BADSRC] != ~0ull || hs[ANSX_BDR_F_BADPTR] != ~0ull) {
        if (bad_range) *bad_range = (size_t)(hs[ANSX_BDR_F_BADSRC] != ~0ull ? hs[ANSX_BDR_F_BADSRC] : hs[ANSX_BDR_F_BADPTR]);
        return ANSX_ERR_ARG;
    }
    const size_t nref = (size_t)hs[ANSX_BDR_F_NREF];
    if (nref == 0 || nref > mref) return ANSX_ERR_HIP;  // (cannot happen: a front fault)

    // ---- the referenced containers' headers, and which they are
    std::vector<u32> ref(nref);
    std::vector<BatchSrc> rs(nref);
    {
        Upload U;
        const auto s_ref = U.add<u32>(nref);
        const auto s_hdr = U.add<uint4>(4 * nref);
        if ((rc = upload_room(c, U, c->rng_plan))) return rc;
        LAUNCH(c, "k_batch_headers", k_batch_headers, (u32)((4 * (u64)nref + 255) / 256), 256, 0, s, (const u64*)F.dev(f_ra), (u64)nref,
            U.dev(s_hdr));
        HIPCHK(c, hipMemcpyAsync(U.pin(s_hdr), U.dev(s_hdr), s_hdr.bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(U.pin(s_ref), F.dev(f_ref), s_ref.bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        memcpy(ref.data(), U.pin(s_ref), s_ref.bytes);
        for (size_t j = 0; j < nref; j++) {  // batch_headers' checks, in batch order
            const size_t i = ref[j];
            BatchSrc& b = rs[j];
            Plan P;
            if (i >= count) return ANSX_ERR_HIP;
            if (in_bytes[i] < sizeof(ansx_container_header) || parse_header((const u8*)U.pin(s_hdr) + 64 * j, in_bytes[i], &b.H)
                || container_plan(b.H, (u32)kind, (u32)f, in_bytes[i], &P) || P.g.nblocks == 0) {
                if (bad_container) *bad_container = i;
                return ANSX_ERR_FORMAT;
            }
            b.lay = P.lay, b.base = (u64)(uintptr_t)d_ins[i], b.nblocks = P.g.nblocks;
        }
    }
    for (size_t j = 0; sums && j < nref; j++)
        if (nbases[ref[j]] != (size_t)rs[j].nblocks + 1) {
            if (bad_container) *bad_container = ref[j];
            return ANSX_ERR_ARG;
        }

    // ---- the groups and the global blocks: group after group, batch order inside (ansx_plan.h, bdr_tables)
    const u32 PB = batch_pass_blocks(c);
    BdrTables Tb;
    if (!bdr_tables(rs, PB, [&](const ansx_container_header& H0) {
            return block_bound(kind, (u32)f, (size_t)H0.block_ints, (H0.kind & 0x100u) != 0);
        }, &Tb))
        return ANSX_ERR_ARG;
    const std::vector<u32>& rmap = Tb.rmap;
    const std::vector<ansx_bdr_ref>& recs = Tb.R;
    const std::vector<ansx_bdr_group>& grp = Tb.G;
    const std::vector<ansx_batch_src>& S = Tb.S;
    const std::vector<ansx_container_header>& Hs = Tb.Hs;
    const u32 ng = (u32)grp.size();
    const u64 nbtot = Tb.nbtot, nslots = Tb.nslots;
    std::vector<ansx_brs_src> SB;  // (the sums: every referenced container's bases, in the order of R)
    if (sums) {
        SB.resize(nref);
        for (size_t j = 0; j < nref; j++) SB[rmap[j]] = { (u64)(uintptr_t)d_bases[ref[j]], rs[j].nblocks, 0 };
    }
    u32 kb = 0;  // key bits of a global block
    while ((1ull << kb) < nbtot) kb++;

    // ---- the planner's workspace: what comes back | what goes up | what stays
    Upload W;
    const auto w_sc = W.add<u64>(ANSX_BDR_SCALARS);
    const auto w_tg = W.add<u64>((size_t)ng + 1);
    const auto w_ps = W.add<ansx_bdr_pass>(nslots);
    const size_t w_back = W.end;
    const auto w_rmap = W.add<u32>(nref);
    const auto w_rec = W.add<ansx_bdr_ref>(nref);
    const auto w_grp = W.add<ansx_bdr_group>(ng);
    const auto w_S = W.add<ansx_batch_src>(nref);
    const auto w_SB = W.add<ansx_brs_src>(SB.size());
    const size_t w_up = W.end;
    const auto w_part = W.add<u64>(4 * nt);
    const auto w_hist = W.add<u32>(16 * nt);
    const auto w_rng = W.add<ansx_bdr_range>(nr);
    const auto w_kv = W.add<u32>(4 * nr);
    const auto w_tb = W.add<u32>(nbtot);
    if ((rc = ensure_pin(c, w_up)) || (rc = ensure(c, c->rng_dev, W.end))) return rc;
    W.host = c->rng_pin, W.devp = (u8*)c->rng_dev.p;
    memset(W.host, 0, w_back);
    W.pin(w_sc)[ANSX_BDR_BADRANGE] = ~0ull;
    W.put(w_rmap, rmap.data()), W.put(w_rec, recs.data()), W.put(w_grp, grp.data()), W.put(w_S, S.data());
    if (sums) W.put(w_SB, SB.data());
    HIPCHK(c, hipMemcpyAsync(W.devp, W.host, w_up, hipMemcpyHostToDevice, s));
    u64* sc = W.dev(w_sc);
    u64* part = W.dev(w_part);
    u64* partm = part + 2 * nt;
    u64* parta = part + 3 * nt;
    u32* hist = W.dev(w_hist);
    u32* kv[4] = { W.dev(w_kv), W.dev(w_kv) + nr, W.dev(w_kv) + 2 * nr, W.dev(w_kv) + 3 * nr };
    const ansx_bdr_ref* dR = W.dev(w_rec);
    const ansx_bdr_group* dG = W.dev(w_grp);
    ansx_bdr_range* rng = W.dev(w_rng);
    u32* tb = W.dev(w_tb);
    u32 cur = 0;  // the sorted spans are kv[cur], kv[cur + 1]; the union goes to the other pair
    {
        const u32 g = (u32)nt;
        const u32* slot = F.dev(f_slot);
        LAUNCH(c, "k_bdr_spans", k_bdr_spans, g, ANSX_DR_NT, 0, s, d_src, d_first, d_cnt, nr, slot, (const u32*)W.dev(w_rmap), dR,
            part, sc);
        LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, false>), 1, ANSX_DR_NT, 0, s, part, nt, 2u, nt, sc, (u32*)nullptr);
        LAUNCH(c, "k_bdr_compact", k_bdr_compact, g, ANSX_DR_NT, 0, s, d_src, d_first, d_cnt, nr, slot, (const u32*)W.dev(w_rmap),
            dR, dG, (const u64*)part, (const u64*)sc, d_offsets, kv[0], kv[1], rng);
        for (u32 sh = 0; sh < kb; sh += 4) {
            LAUNCH(c, "k_dr_digit_count", k_dr_digit_count, g, ANSX_DR_NT, 0, s, kv[cur], (const u64*)sc, sh, hist);
            LAUNCH(c, "k_dr_scan", (k_dr_scan<u32, false>), 1, ANSX_DR_NT, 0, s, hist, 16 * nt, 1u, 0ull, (u64*)nullptr,
                (u32*)nullptr);
            LAUNCH(c, "k_dr_digit_scatter", k_dr_digit_scatter, g, ANSX_DR_NT, 0, s, kv[cur], kv[cur + 1], kv[2 - cur],
                kv[3 - cur], (const u64*)sc, sh, (const u32*)hist);
            cur = 2 - cur;
        }
        LAUNCH(c, "k_dr_tile_max", k_dr_tile_max, g, ANSX_DR_NT, 0, s, kv[cur + 1], (const u64*)sc, partm);
        LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, true>), 1, ANSX_DR_NT, 0, s, partm, nt, 1u, 0ull, sc + ANSX_DR_LASTB1,
            (u32*)nullptr);
        LAUNCH(c, "k_dr_adds", k_dr_adds, g, ANSX_DR_NT, 0, s, kv[cur], kv[cur + 1], (const u64*)sc, (const u64*)partm,
            kv[2 - cur], kv[3 - cur], parta);
        LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, false>), 1, ANSX_DR_NT, 0, s, parta, nt, 1u, 0ull, sc + ANSX_DR_T, (u32*)nullptr);
        const u32* dS = kv[2 - cur];
        const u32* offl = kv[3 - cur];
        LAUNCH(c, "k_bdr_k0", k_bdr_k0, g_nr, ANSX_DR_NT, 0, s, rng, (const u64*)sc, dR, dG, dS, offl, (const u64*)parta);
        LAUNCH(c, "k_bdr_groups", k_bdr_groups, (ng + ANSX_DR_NT) / ANSX_DR_NT, ANSX_DR_NT, 0, s, dG, ng, (const u32*)kv[cur], offl,
            (const u64*)parta, (const u64*)sc, W.dev(w_tg));
        // (the grids over tb follow the ranges or the referenced blocks, whichever is less, in strides: T is not known here)
        const u32 g_tb = (u32)std::min<u64>((std::min<u64>(nbtot, 1 + nr * 16) + ANSX_DR_NT - 1) / ANSX_DR_NT, 4096);
        LAUNCH(c, "k_bdr_blocks", k_bdr_blocks, g_tb, ANSX_DR_NT, 0, s, tb, (const u64*)sc, dS, offl, (const u64*)parta);
        LAUNCH(c, "k_bdr_pass_blocks", k_bdr_pass_blocks, g_tb, ANSX_DR_NT, 0, s, (const u32*)tb, (const u64*)sc, dR, (u32)nref, dG,
            (const u64*)W.dev(w_tg), PB, W.dev(w_ps));
        LAUNCH(c, "k_bdr_pass_pieces", k_bdr_pass_pieces, g, ANSX_DR_NT, 0, s, (const ansx_bdr_range*)rng, (const u64*)sc, dR, dG,
            (const u64*)W.dev(w_tg), PB, W.dev(w_ps));
    }
    HIPCHK(c, hipMemcpyAsync(W.host, W.devp, w_back, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const u64* hsc = W.pin(w_sc);
    if (hsc[ANSX_BDR_BADRANGE] != ~0ull) {
        if (bad_range) *bad_range = (size_t)hsc[ANSX_BDR_BADRANGE];
        return ANSX_ERR_ARG;
    }
    const u64 total = hsc[ANSX_DR_TOTAL], T = hsc[ANSX_DR_T];
    if (total_ints) *total_ints = total;
    if (total > cap) return ANSX_ERR_CAPACITY;
    if (total == 0) return ANSX_OK;
    if (T == 0 || T > nbtot || hsc[ANSX_DR_NNE] == 0) return ANSX_ERR_HIP;  // (cannot happen: a planner fault)
    // (the pinned page is written again by the first pass: what the passes need of it is taken out here, O(passes))
    const std::vector<u64> tg(W.pin(w_tg), W.pin(w_tg) + ng + 1);
    const std::vector<ansx_bdr_pass> ps(W.pin(w_ps), W.pin(w_ps) + nslots);

    // ---- the passes
    const u64 ntn = (hsc[ANSX_DR_NNE] + ANSX_DR_TILE - 1) / ANSX_DR_TILE;  // tiles of non-empty ranges
    for (u32 g = 0; g < ng; g++) {
        const u64 bi = grp[g].bi;
        if (tg[g] > tg[g + 1] || tg[g + 1] > T) return ANSX_ERR_HIP;
        for (u64 ka = tg[g], p = 0; ka < tg[g + 1]; ka += PB, p++) {
            const u64 kb_ = std::min<u64>(ka + PB, tg[g + 1]);
            const u32 Tp = (u32)(kb_ - ka);
            const ansx_bdr_pass& q = ps[grp[g].pslot + p];
            if (q.np > 0xFFFFFFFFull) return ANSX_ERR_ARG;
            if (q.last_n == 0 || q.last_n > bi || q.wl < q.last_n) return ANSX_ERR_HIP;  // (a planner fault)
            Upload D;  // (nothing of it goes up: the pass's plan is built where it is read)
            const auto s_fl = D.add<u32>(4);
            const auto s_B = D.add<ansx_batch_blk>(Tp);
            const auto s_O = D.add<ansx_blk_out>(Tp);
            const auto s_pp = D.add<ansx_piece>(q.np);
            const auto s_wp = D.add<u64>(q.np + 1);
            const auto s_pt = D.add<u64>(2 * ntn);
            u64* agg = nullptr;
            if (sums && (rc = range_sums_workspace(c, bi, Tp, &agg))) return rc;
            if ((rc = ensure(c, c->rng_plan, D.end))) return rc;
            D.devp = (u8*)c->rng_plan.p;
            u32* dflags = D.dev(s_fl);
            LAUNCH(c, "k_bdr_pass_table", k_bdr_pass_table, 1, ANSX_DR_NT, 0, s, (const u32*)(tb + ka), Tp, dR, (u32)nref, (u32)bi,
                dflags, D.dev(s_B), D.dev(s_O));
            if (q.np) {
                LAUNCH(c, "k_bdr_piece_part", k_bdr_piece_part, (u32)ntn, ANSX_DR_NT, 0, s, (const ansx_bdr_range*)rng, (const u64*)sc,
                    dR, dG, (u32)ka, (u32)kb_, D.dev(s_pt));
                LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, false>), 1, ANSX_DR_NT, 0, s, D.dev(s_pt), ntn, 2u, ntn, (u64*)nullptr,
                    (u32*)nullptr);
                LAUNCH(c, "k_bdr_piece_put", k_bdr_piece_put, (u32)ntn, ANSX_DR_NT, 0, s, (const ansx_bdr_range*)rng, (const u64*)sc,
                    dR, dG, (u32)ka, (u32)kb_, (const u64*)D.dev(s_pt), (const ansx_blk_out*)D.dev(s_O), D.dev(s_pp), D.dev(s_wp),
                    q.np, q.ints);
            }
            Sub sub;
            // (the sub-header's maxima are the group's, not the pass's: another decode form at most, the same ints)
            if ((rc = sub_prepare(c, kind, f, Hs[g], (u64)(Tp - 1) * bi + q.last_n, Tp, q.cap_pay, q.wl, D.dev(s_O), &sub))) return rc;
            LAUNCH(c, "k_batch_index", k_batch_index, 1, 1024, 0, s, (const ansx_batch_src*)W.dev(w_S), (const ansx_batch_blk*)D.dev(s_B),
                sub.P.g, Tp, sub.H, sub.cont, q.cap_pay, dflags);
            LAUNCH(c, "k_batch_copy", k_batch_copy, Tp, 256, 0, s, (const ansx_batch_src*)W.dev(w_S), (const ansx_batch_blk*)D.dev(s_B),
                sub.P.g, sub.lay(), sub.cont, q.cap_pay, dflags);
            rc = sub_decode(c, sub, dflags, [&](u32* gflags) -> int {
                int st;
                if (sums && (st = batch_sums_scan(c, sub.list, bi, Tp, D.dev(s_O), D.dev(s_B), W.dev(w_SB), agg, gflags, s))) return st;
                if (!q.np) return ANSX_OK;
                const u32 grid = (u32)std::min<u64>((q.ints + ANSX_PIECE_CHUNK - 1) / ANSX_PIECE_CHUNK, 1u << 20);
                LAUNCH(c, "k_piece_gather", k_piece_gather, grid, 256, 0, s, (const u32*)sub.list, (const ansx_piece*)D.dev(s_pp),
                    (const u64*)D.dev(s_wp), (u32)q.np, q.ints, d_out, (const u32*)gflags);
                return ANSX_OK;
            }, s);
            if (rc == ANSX_ERR_FORMAT && bad_container) *bad_container = count;
            if (rc) return rc;
        }
    }
    return ANSX_OK;
}

// ansx_next_geq_batch_dev (ansx_batchnextgeq.h): the front half above over the lists the targets
// name -> k_ngb_locate, a lane per target -> ONE read-back of the located blocks, checked -> the found targets as ranges
// of one int at the start of their blocks, destination the target's own index -> the passes of the sums call with
// k_ngb_search as the way out.
int next_geq_batch(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, const u32* const* d_bases,
    const size_t* nbases, size_t count, const u32* src, const u32* d_targets, size_t nt, u64* d_pos, u32* d_ids, u64* found,
    size_t* bad_container, hipStream_t s)
{
    int rc;
    BrFront F;
    if ((rc = batch_ranges_front(c, kind, f, d_ins, in_bytes, count, src, nt, nbases, &F, bad_container, s))) return rc;
    const size_t nref = F.ref.size();
    BatchOut out = { OUT_SUMS_SEARCH, nullptr, {}, d_targets, d_pos, d_ids };
    for (const u32 j : F.ref) out.bases.push_back(d_bases[j]);  // (the referenced containers')
    // up: the lists | every target's list; down: every target's block.  24 bytes per referenced container and 8 per
    // target of workspace, the same again pinned on the host.
    Upload U;
    const auto s_l = U.add<ansx_ngb_list>(nref);
    const auto s_rid = U.add<u32>(nt);
    const auto s_blk = U.add<u32>(nt);  // (comes back)
    if ((rc = upload_room(c, U, c->rng_dev))) return rc;
    ansx_ngb_list* hl = U.pin(s_l);
    for (size_t j = 0; j < nref; j++) hl[j] = { (u64)(uintptr_t)out.bases[j], F.rs[j].H.n, F.rs[j].nblocks, 0 };
    U.put(s_rid, F.rid.data());
    HIPCHK(c, hipMemcpyAsync(U.devp, U.host, s_rid.off + s_rid.bytes, hipMemcpyHostToDevice, s));
    LAUNCH(c, "k_ngb_locate", k_ngb_locate, (u32)((nt + ANSX_NGB_NT - 1) / ANSX_NGB_NT), ANSX_NGB_NT, 0, s,
        (const ansx_ngb_list*)U.dev(s_l), (const u32*)U.dev(s_rid), d_targets, (u32)nt, U.dev(s_blk), d_pos, d_ids);
    HIPCHK(c, hipMemcpyAsync(U.pin(s_blk), U.dev(s_blk), 4 * nt, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));

    // every located block against its list; the found targets as ranges, grouped by geometry
    const u32* blk = U.pin(s_blk);
    std::vector<u64> first(nt), off(nt);
    std::vector<u32> cnt(nt);
    GeometryGroups groups;
    u64 nfound = 0;
    for (size_t i = 0; i < nt; i++) {
        const BatchSrc& cs = F.rs[F.rid[i]];
        off[i] = i;
        if (blk[i] == ANSX_NGB_NONE) {
            first[i] = 0, cnt[i] = 0;
            continue;
        }
        if (blk[i] >= cs.nblocks) {  // (cannot happen: k_ngb_locate's b is an index below nblocks)
            if (bad_container) *bad_container = count;
            return ANSX_ERR_FORMAT;
        }
        first[i] = (u64)blk[i] * cs.H.block_ints, cnt[i] = 1;
        groups[br_geometry(cs.H)].push_back((u32)i);
        nfound++;
    }
    const u32 PB = batch_pass_blocks(c);
    rc = for_each_group(groups, count, bad_container, [&](const std::vector<u32>& ids) -> int {
        return batch_ranges_group(c, kind, f, F.rs, F.rid, first.data(), cnt.data(), off, ids, PB, out, s);
    });
    if (rc == ANSX_OK && found) *found = nfound;
    return rc;
}

// --------------------------------------------------------------------------------- batch encode
// ansx_encode_batch_dev: the batch in order, cut at list boundaries into passes of at most P
// blocks -> per pass one plan upload, the ordinary encode phases over its work list (ansx_geo::bin), k_encb_scan +
// k_encb_write assemble every list's container in place, one read-back.  A list of more than P blocks, and every list
// of a form without a batched path, goes through encode_dev into its place.

// For the length of a batch call the context's hint sets are the batch's own, and what ansx_last_encode_stats reports is
// put back: a later ansx_encode_dev finds the context as it left it.
struct EncBatchHints {
    ansx_ctx* c;
    ansx_encode_stats last;
    explicit EncBatchHints(ansx_ctx* c_) : c(c_), last(c_->last) { swap(); }
    ~EncBatchHints()
    {
        swap();
        c->last = last;
    }
    void swap()
    {
        std::swap(c->ns_hint, c->bat.ns_hint);
        std::swap(c->rf_hint, c->bat.rf_hint);
        std::swap(c->t_hint, c->bat.t_hint);
        std::swap(c->wide_hint, c->bat.wide_hint);
        std::swap(c->int_sparse_hint, c->bat.int_sparse_hint);
    }
};

// geometries the batched path takes: the LDS-model codecs, ANSfold and ANSmsb also with compaction (whose blocks are at
// most 16384 ints: make_plan); ANSint has none
bool encode_batch_form(const ansx_geo& g)
{
    if (g.pa) return g.kind == ANSX_MSB || (g.kind == ANSX_FOLD && g.f <= 5);
    // (ANSrfold: the remap of a pass has the LDS forms only, ansx_rfold.h)
    return g.kind == ANSX_MSB || (g.kind == ANSX_FOLD && g.f <= 5) || (g.kind == ANSX_RFOLD && g.f <= 5 && g.block_ints <= 16384u);
}

// One pass: lists [l0, l1) of the batch, NB blocks in all, containers from byte `base` of d_out on.  Writes their
// offsets and sizes and returns the pass's bytes (a multiple of 16) in *pass_bytes.
int encode_batch_pass(ansx_ctx* c, const Plan& P0, const u32* d_in, const u64* offsets, size_t l0, size_t l1, u32 NB,
    u8* d_out, size_t cap, u64 base, u64* out_off, u64* out_bytes, u64* pass_bytes, hipStream_t s)
{
    int rc;
    const u64 bi = P0.g.block_ints;
    const u32 nl = (u32)(l1 - l0);
    // the plan (ansx_plan.h): its upload image in pinned memory, the results read back behind it
    const bool rf = P0.g.kind == ANSX_RFOLD, pa = P0.g.pa != 0;
    const EncPassLayout L = encb_layout(NB, nl, rf || pa);
    const size_t o_l = L.o_l, o_i = L.o_i, o_m = L.o_m, o_r = L.o_r, o_s = L.o_s;
    if ((rc = ensure_pin(c, o_m + sizeof(ansx_encb_res) * ((size_t)nl + 1)))) return rc;
    u8* hb = c->rng_pin;  // (nothing is pending on it: every call that uses it ends in a synchronisation)
    EncPassTables T;
    if (!encb_pass_tables(offsets, l0, l1, bi, NB, pa ? ENCB_REMAP_PA : (rf ? ENCB_REMAP_RFOLD : ENCB_REMAP_NONE), fold_T(P0.g.f), L, hb, &T))
        return ANSX_ERR_ARG;  // (cannot happen: the caller counted the same blocks)
    const u32 longest = T.longest;
    if ((rc = ensure(c, c->enb_plan, L.plan_bytes))) return rc;
    u8* dp = (u8*)c->enb_plan.p;
    HIPCHK(c, hipMemcpyAsync(dp, hb, o_m, hipMemcpyHostToDevice, s));

    // the pass's plan: any n that makes make_plan lay out exactly NB blocks (the table says how long each is); its
    // restart points and hints go to the work area in the wide form, whatever the lists will need
    // g.n is not the pass's ints.  What reads it: the block-range pipeline's size rule (choose_model_form: a pass of 8192 and
    // more blocks forks its model kernels as a list of that many full blocks would -- the ranges are block ranges, so
    // that holds for short blocks too; not measured on a pass); k_encode's wg_sync and buffer view and k_encode_pc,
    // all switched off by g.bin.  choose_model_form sizes by block_ints and the hints, not by g.n.
    Plan P = P0;
    P.g.n = (u64)(NB - 1) * bi + 1;
    P.g.nblocks = NB;
    P.g.bin = (const ansx_blk_in*)dp;
    // (the ints the codec sees are ranks of at most the block's length: 770 MiB of model arrays for 16384 ten-int lists
    // with the codec's own 1024 slots per row)
    if (pa) P.NSP = std::min(P.NSP, min_row_stride(P.g.map, longest));
    set_restart_format(&P, true);
    if ((rc = ensure(c, c->enb_wc, (size_t)P.lay.payload_off + 64))) return rc;
    u8* wc = (u8*)c->enb_wc.p;
    const size_t stream_bound = block_bound(P.g.kind, P.g.f, P.g.block_ints, pa) + 16;
    EncBatchPass B;
    B.hblk = (const ansx_blk_in*)hb;
    B.longest = longest;
    B.in_base = offsets[l0];
    B.in_ints = offsets[l1] - offsets[l0];
    B.remap_ids = rf || pa ? (const u32*)(dp + o_i) : nullptr;
    memcpy(B.remap_ncls, T.ncls, sizeof(T.ncls));
    B.A.bin = P.g.bin;
    B.A.lists = (const ansx_encb_list*)(dp + o_l);
    B.A.mx = (ansx_encb_max*)(dp + o_m);
    B.A.res = (ansx_encb_res*)(dp + o_r);
    B.A.bsum = (u64*)(dp + o_s);
    B.A.nl = nl;
    B.A.ns_cap = 0;
    B.A.forced = 0;
    // (encode_dev's rule: wide where a cursor may pass 24 bits or on request; ANSint never comes here)
    B.A.must_wide = (stream_bound >= ((size_t)1 << ANSX_CK_CURSOR_BITS) || c->dbg.wide_restart) ? 1u : 0u;
    B.A.wide_at = c->dbg.wide_at;
    B.A.base = base;
    B.A.cap = cap;
    B.A.w_ckoff = (const u32*)(wc + P.lay.ckoff_off);
    B.A.w_ckstate = (const u64*)(wc + P.lay.ckstate_off);
    B.A.w_hints = (const u32*)(wc + P.lay.hint_off);
    B.d_out = d_out;
    B.hres = (const ansx_encb_res*)(hb + o_m);
    P.bat = &B;
    size_t work_bytes = 0;
    // (the work area has no payload: its capacity is never the limit, the caller's is checked by k_encb_scan)
    if ((rc = encode_dev_once(c, P, d_in, wc, ~(size_t)0 >> 1, &work_bytes, s))) return rc;
    if (B.hres[nl].off != 1) return ANSX_ERR_HIP;  // (cannot happen: the host accepted an attempt the device refused)
    for (u32 i = 0; i < nl; i++) {
        out_off[l0 + i] = B.hres[i].off;
        out_bytes[l0 + i] = B.hres[i].bytes;
    }
    *pass_bytes = B.hres[nl].bytes;
    return ANSX_OK;
}

int encode_batch(ansx_ctx* c, const Plan& P0, const ansx_opts* opts, const u32* d_in, const u64* offsets, size_t count,
    u8* d_out, size_t cap, u64* out_offsets, u64* out_bytes, size_t* total_bytes, size_t* bad_index, hipStream_t s)
{
    int rc;
    EncBatchHints slot(c);
    const u64 bi = P0.g.block_ints;
    const u32 PB = batch_pass_blocks(c);
    const bool batched = encode_batch_form(P0.g);
    std::vector<u64> oo(count + 1), ob(count);
    u64 cur = 0;
    if (bad_index) *bad_index = count;
    for (size_t i = 0; i < count;) {
        const EncStep st = encb_step(offsets, count, i, bi, PB, batched);
        i = st.l1;
        if (st.NB) {
            u64 pass_bytes = 0;
            if ((rc = encode_batch_pass(c, P0, d_in, offsets, st.l0, st.l1, st.NB, d_out, cap, cur, oo.data(), ob.data(), &pass_bytes, s)))
                return rc;
            cur += pass_bytes;
            continue;
        }
        // the ordinary path, straight into the list's place
        const size_t l = st.l0;
        Plan P;
        if (make_plan((int)P0.g.kind, (int)P0.g.f, (size_t)(offsets[l + 1] - offsets[l]), opts, &P)) return ANSX_ERR_ARG;  // (checked by the entry point)
        size_t bytes = 0;
        if (cur > cap) return ANSX_ERR_CAPACITY;
        if ((rc = encode_dev(c, P, d_in + offsets[l], d_out + cur, cap - cur, &bytes, s))) {
            if (bad_index && rc != ANSX_ERR_HIP) *bad_index = l;
            return rc;
        }
        const u64 r16 = rup(bytes, 16);
        if (cur + r16 > cap) return ANSX_ERR_CAPACITY;
        if (r16 != bytes) HIPCHK(c, hipMemsetAsync(d_out + cur + bytes, 0, r16 - bytes, s));
        oo[l] = cur, ob[l] = bytes;
        cur += r16;
    }
    HIPCHK(c, hipStreamSynchronize(s));  // (the padding behind a list of the ordinary path)
    oo[count] = cur;
    if (out_offsets) memcpy(out_offsets, oo.data(), 8 * (count + 1));
    if (out_bytes) memcpy(out_bytes, ob.data(), 8 * count);
    if (total_bytes) *total_bytes = (size_t)cur;
    return ANSX_OK;
}

// --------------------------------------------------------------------------------- running sums and gaps
// ansx_decode_sums_dev / ansx_decode_batch_sums_dev / ansx_encode_gaps_dev / ansx_encode_batch_gaps_dev (DESIGN.md
// section 3e): the ordinary decode, then k_sums_reduce -> k_sums_carry -> k_sums_apply over the flat output; k_gaps into
// workspace, then the ordinary encode.  A single list is a batch of one.

struct SumsPlan {
    u32* flag;        // ANSX_SS_NONE, or the first list at fault
    const u64* offs;  // the list starts, relative to the first
    u64* agg;         // one aggregate per tile
    u64* carry;       // ... and the carry into it
    u32 head;         // ints between the array and the 16-byte boundary below it
    u32 ntiles;
};

// The device side of a call over the n ints at `addr` in `count` lists, offs[0 .. count] (host, any base): one upload
int sums_prepare(ansx_ctx* c, uintptr_t addr, u64 n, const u64* offs, size_t count, hipStream_t s, SumsPlan* S)
{
    int rc;
    S->head = (u32)(addr >> 2) & 3u;
    const u64 ntiles = (n + S->head + ANSX_SS_TILE - 1) / ANSX_SS_TILE;
    if (ntiles > 0x7FFFFFFFull) return ANSX_ERR_ARG;
    S->ntiles = (u32)ntiles;
    const size_t o_o = 16, o_a = rup(o_o + 8 * (count + 1), 16);
    if ((rc = ensure_pin(c, o_a))) return rc;
    if ((rc = ensure(c, c->sums_plan, o_a + 16 * (size_t)ntiles))) return rc;
    u32* hf = (u32*)c->rng_pin;  // (no copy out of it is pending: every call that uses it ends in a synchronisation)
    hf[0] = ANSX_SS_NONE, hf[1] = 0, hf[2] = 0, hf[3] = 0;
    u64* ho = (u64*)(c->rng_pin + o_o);
    for (size_t i = 0; i <= count; i++) ho[i] = offs[i] - offs[0];
    u8* d = (u8*)c->sums_plan.p;
    HIPCHK(c, hipMemcpyAsync(d, c->rng_pin, o_a, hipMemcpyHostToDevice, s));
    S->flag = (u32*)d;
    S->offs = (const u64*)(d + o_o);
    S->agg = (u64*)(d + o_a);
    S->carry = S->agg + ntiles;
    return ANSX_OK;
}

// the flag word back: ANSX_ERR_DOMAIN and the list when a kernel named one
int sums_finish(ansx_ctx* c, const SumsPlan& S, size_t* bad_index, hipStream_t s)
{
    HIPCHK(c, hipMemcpyAsync(c->pin->flags, S.flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (c->pin->flags[0] == ANSX_SS_NONE) return ANSX_OK;
    if (bad_index) *bad_index = c->pin->flags[0];
    return ANSX_ERR_DOMAIN;
}

// the scan's kernels behind sums_prepare, enqueued
int sums_launch(ansx_ctx* c, u32* d, u64 n, size_t count, SumsPlan& S, hipStream_t s)
{
    u32* base = (u32*)((uintptr_t)d & ~(uintptr_t)15);
    if (S.ntiles > 1) {
        LAUNCH(c, "k_sums_reduce", k_sums_reduce, S.ntiles, ANSX_SS_NT, 0, s, (const u32*)base, S.head, n, S.offs, (u32)count, S.agg);
        LAUNCH(c, "k_sums_carry", k_sums_carry, 1, ANSX_SS_SCAN_NT, 0, s, (const u64*)S.agg, S.carry, (u64)S.ntiles);
    } else {
        // one tile: nothing is carried into it -- the zero behind the flag word; its aggregate is not looked at (a list
        // starts at its first int)
        S.carry = (u64*)(S.flag + 2);
    }
    LAUNCH(c, "k_sums_apply", k_sums_apply, S.ntiles, ANSX_SS_NT, 0, s, base, S.head, n, S.offs, (u32)count, (const u64*)S.agg,
        (const u64*)S.carry, S.flag);
    return ANSX_OK;
}

// d[offs[i] - offs[0] .. offs[i + 1] - offs[0]) -> its inclusive running sums, for every list, in place
int sums_run(ansx_ctx* c, u32* d, u64 n, const u64* offs, size_t count, size_t* bad_index, hipStream_t s)
{
    int rc;
    SumsPlan S;
    if ((rc = sums_prepare(c, (uintptr_t)d, n, offs, count, s, &S))) return rc;
    if ((rc = sums_launch(c, d, n, count, S, s))) return rc;
    return sums_finish(c, S, bad_index, s);
}

// The gaps of the lists of d_in (offs as for sums_run) -> *gaps, workspace with d_in's alignment; d_in is only read
// side: a second array of count + 1 entries (ansx_encode_batch_gaps_bases_dev: where every list's bases start) that
// goes up behind the plan, in front of the call's one synchronisation; d_offs / d_side: where the list starts and that
// array then lie on the device.
struct GapsSide {
    const u64* side;
    const u64* d_offs;
    const u64* d_side;
};
int gaps_run(ansx_ctx* c, const u32* d_in, u64 n, const u64* offs, size_t count, const u32** gaps, size_t* bad_index,
    hipStream_t s, GapsSide* G = nullptr)
{
    int rc;
    SumsPlan S;
    const size_t o_g = rup(16 + 8 * (count + 1), 16), side_bytes = 8 * (count + 1);
    if (G) {  // (both before sums_prepare: it keeps the pinned image it fills, and bat_hdr is no buffer of an encode)
        if ((rc = ensure_pin(c, o_g + side_bytes))) return rc;
        if ((rc = ensure(c, c->bat_hdr, side_bytes))) return rc;
    }
    if ((rc = sums_prepare(c, (uintptr_t)d_in, n, offs, count, s, &S))) return rc;
    if ((rc = ensure(c, c->sums_ints, 4 * ((size_t)n + 4)))) return rc;
    if (G) {
        memcpy(c->rng_pin + o_g, G->side, side_bytes);
        HIPCHK(c, hipMemcpyAsync(c->bat_hdr.p, c->rng_pin + o_g, side_bytes, hipMemcpyHostToDevice, s));
        G->d_offs = S.offs, G->d_side = (const u64*)c->bat_hdr.p;
    }
    const u32* base = (const u32*)((uintptr_t)d_in & ~(uintptr_t)15);
    u32* base_out = (u32*)c->sums_ints.p;
    LAUNCH(c, "k_gaps", k_gaps, S.ntiles, ANSX_SS_NT, 0, s, base, base_out, S.head, n, S.offs, (u32)count, S.flag);
    *gaps = base_out + S.head;
    return sums_finish(c, S, bad_index, s);
}

// ansx_block_bases_dev: the container decoded into rng_list -- no remembered header in or out --
// with k_rs_reduce and k_rs_bases riding on the decode's final read-back, which also carries ANSX_ERR_DOMAIN home.
int block_bases(ansx_ctx* c, int kind, int f, const u8* d_in, size_t in_bytes, u32* d_bases, size_t cap, size_t* nbases,
    hipStream_t s)
{
    int rc;
    ansx_container_header H;
    Plan P;
    if ((rc = range_source(c, kind, f, d_in, in_bytes, s, &H, &P))) return rc;
    const u64 n = H.n, bi = P.g.block_ints;
    const u32 nb = P.g.nblocks;
    *nbases = (size_t)nb + 1;
    if (cap < (size_t)nb + 1) return ANSX_ERR_CAPACITY;
    // a block of at most a chunk is one aggregate, a longer one four per tile
    const u32 tpb = bi <= ANSX_RS_CHUNK ? 0u : (u32)((bi + ANSX_RS_TILE - 1) / ANSX_RS_TILE);
    const u32 per = tpb ? tpb * (ANSX_RS_NT / 64u) : 1u;
    const u64 grid = tpb ? (u64)nb * tpb : ((u64)nb + 3) / 4;
    if (grid > 0x7FFFFFFFull) return ANSX_ERR_ARG;
    if ((rc = ensure(c, c->rng_list, 4 * (size_t)n + 64))) return rc;
    if ((rc = ensure(c, c->sums_plan, 8 * (size_t)nb * per))) return rc;
    u32* list = (u32*)c->rng_list.p;
    u64* agg = (u64*)c->sums_plan.p;
    const std::function<int(const u32*)> epilogue = [&](const u32* gflags) -> int {
        LAUNCH(c, "k_rs_reduce", k_rs_reduce, (u32)grid, ANSX_RS_NT, 0, s, (const u32*)list, n, (u32)bi, nb, tpb, agg, gflags);
        LAUNCH(c, "k_rs_bases", k_rs_bases, 1, ANSX_RS_NT, 0, s, (const u64*)agg, per, nb, d_bases, (u32*)gflags);
        return ANSX_OK;
    };
    DecodeOpts O;
    O.speculate = O.remember = false, O.epilogue = &epilogue;
    return decode_dev(c, P, d_in, in_bytes, list, s, O);
}

// --------------------------------------------------------------------------------- intersection
// ansx_intersect_ids_dev / ansx_intersect_dev (ansx_intersect.h).  A step asks which of nc
// candidates in device memory are ids of one list and writes the members back to back, in one of two forms:
//   selective  ansx_next_geq_dev's path (device_ranges_from) with OUT_SUMS_MATCH as the way out: k_ng_locate, the
//              planner, the decode of the touched blocks, range_sums_scan, k_isect_match.  Workspace: next_geq's plus
//              IsectWork.  Host waits: the planner's read-back and the decode's final one, which brings the total too
//              -- none over ansx_next_geq_dev.
//   full       the whole list decoded into rng_list with no trace in the context (decode_ids), the whole-list scan
//              and k_isect_match_full in the decode's epilogue.  Workspace: 4 bytes per int of the list, the scan's
//              16 bytes per tile of 4096 ints, IsectWork.  Host waits: decode_dev's two (header, final read-back).
// Both end in isect_compact.  The caller has read the header (one more wait per call of ansx_intersect_ids_dev, none per
// step of ansx_intersect_dev, whose headers come in one round trip).  Full when nc >= ANSX_ISECT_FULL_PER_BLOCK * nblocks:
// the measured crossing of the two forms on 4096 blocks of 16384 ints, at 1.2 candidates per block (DESIGN.md section 3i,
// profiles/intersect_bench.json).
#define ANSX_ISECT_FULL_PER_BLOCK 1u

// The two launches every compaction is made of, behind a kernel that has written W's ballots and tile counts over nc
// candidates: the scan of the tile counts -> W.total ...
int isect_tile_scan(ansx_ctx* c, const IsectWork& W, hipStream_t s)
{
    LAUNCH(c, "k_dr_scan", (k_dr_scan<u64, false>), 1, ANSX_DR_NT, 0, s, W.counts, (u64)W.ntiles, 1u, 0ull, W.total, (u32*)nullptr);
    return ANSX_OK;
}
// ... and the values d_cand[i] whose ballot bit is set moved to the front of o (gflags / dflags: the two flag words
// k_isect_compact looks at before it writes).  Any array of nc values may be moved by the same ballots.
int isect_move(ansx_ctx* c, const IsectWork& W, const u32* d_cand, u32 nc, const IsectOut& o, const u32* gflags, const u32* dflags,
    hipStream_t s)
{
    LAUNCH(c, "k_isect_compact", k_isect_compact, W.ntiles, ANSX_ISECT_NT, 0, s, d_cand, nc, (const u64*)W.ballots,
        (const u64*)W.counts, (const u64*)W.total, o.cap, (const u64*)W.wpos, o.ids, o.idx, o.pos, gflags, dflags);
    return ANSX_OK;
}

int isect_compact(ansx_ctx* c, const IsectWork& W, const u32* d_cand, u32 nc, const IsectOut& o, const u32* gflags,
    const u32* dflags, hipStream_t s)
{
    int rc;
    if ((rc = isect_tile_scan(c, W, s)) || (rc = isect_move(c, W, d_cand, nc, o, gflags, dflags, s))) return rc;
    HIPCHK(c, hipMemcpyAsync(&c->pin->isect_total, W.total, 8, hipMemcpyDeviceToHost, s));
    return ANSX_OK;
}

// The container of plan P decoded whole into dst (16-byte aligned, room for 4 n + 64 bytes) as ids -- no remembered
// header in or out -- with the whole-list scan of section 3e and then `extra` (given the decode's flags and the scan's
// flag word, which has a zero word behind it) as the decode's epilogue.  ANSX_ERR_DOMAIN: the sum left 32 bits.
template <class Extra> int decode_ids(ansx_ctx* c, const Plan& P, const u8* d_in, size_t in_bytes, u32* dst, u64 n,
    const Extra& extra, hipStream_t s)
{
    int rc;
    SumsPlan S;
    const u64 offs[2] = { 0, n };
    if ((rc = sums_prepare(c, (uintptr_t)dst, n, offs, 1, s, &S))) return rc;
    u32* hflag = &c->pin->isect_sflag;
    *hflag = ANSX_SS_NONE;
    const std::function<int(const u32*)> epilogue = [&](const u32* gflags) -> int {
        if ((rc = sums_launch(c, dst, n, 1, S, s))) return rc;
        if ((rc = extra((u32*)gflags, (const u32*)S.flag))) return rc;
        HIPCHK(c, hipMemcpyAsync(hflag, S.flag, 4, hipMemcpyDeviceToHost, s));
        return ANSX_OK;
    };
    DecodeOpts O;
    O.speculate = O.remember = false, O.epilogue = &epilogue;
    if ((rc = decode_dev(c, P, d_in, in_bytes, dst, s, O))) return rc;
    return *hflag == ANSX_SS_NONE ? ANSX_OK : ANSX_ERR_DOMAIN;
}

// One step.  src: the list's container, header and plan (range_source, or batch_headers and container_plan).
// *total: the members, on ANSX_OK and on ANSX_ERR_CAPACITY (more than o.cap: nothing is written).
int isect_step(ansx_ctx* c, int kind, int f, const RangeTail& src, size_t in_bytes, const u32* d_bases, size_t nbases,
    const u32* d_cand, u32 nc, const IsectOut& o, u64* total, hipStream_t s)
{
    int rc;
    const u64 n = src.H.n, bi = src.P.g.block_ints;
    const u32 nb = src.P.g.nblocks;
    *total = 0;
    if (nbases != (size_t)nb + 1) return ANSX_ERR_ARG;
    if (n == 0) return ANSX_OK;  // (an empty list has no member)
    c->pin->isect_total = 0;
    const bool full = c->dbg.intersect_form ? c->dbg.intersect_form == 2 : nc >= (u64)ANSX_ISECT_FULL_PER_BLOCK * nb;
    if (!full) {
        RangeOut out = { OUT_SUMS_MATCH, nullptr, d_bases, nbases, d_cand, nc };
        out.isect = o;
        u64 found = 0;  // (the candidates at or below the last id; none: no tail has run)
        if ((rc = device_ranges_from(c, kind, f, src, nullptr, nullptr, nc, nc, nullptr, &found, out, s))) return rc;
        if (found == 0) return ANSX_OK;
    } else {
        if ((rc = ensure(c, c->rng_list, 4 * (size_t)n + 64))) return rc;
        if ((rc = ensure(c, c->rng_dev, IsectWork::bytes(nc, o.pos != nullptr)))) return rc;
        const IsectWork W((u8*)c->rng_dev.p, nc, o.pos != nullptr);
        u32* list = (u32*)c->rng_list.p;
        rc = decode_ids(c, src.P, src.d_in, in_bytes, list, n, [&](u32* gflags, const u32* sflag) -> int {
            LAUNCH(c, "k_isect_match_full", k_isect_match_full, W.ntiles, ANSX_ISECT_NT, 0, s, (const u32*)list, n, bi, d_bases,
                nb, d_cand, nc, W.ballots, W.counts, W.wpos, gflags, sflag);
            return isect_compact(c, W, d_cand, nc, o, gflags, sflag + 1, s);
        }, s);
        if (rc) return rc;
    }
    *total = c->pin->isect_total;
    return *total > o.cap ? ANSX_ERR_CAPACITY : ANSX_OK;
}

// ansx_intersect_dev: every header in one round trip (batch_headers) -> the driver, the list of fewest ints, decoded
// as ids into isect_ids (decode_ids) -> the other lists by ascending n, a step each, the survivors going back and
// forth between the two halves of isect_ids, until a step leaves nothing -> one copy to the caller.  Workspace: the
// step's own and 8 bytes per int of the driver.  Host waits: one for the headers, decode_dev's two for the driver,
// two per step (selective: planner, final; full: header, final), one behind the copy.
int intersect_lists(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, const u32* const* d_bases,
    const size_t* nbases, size_t count, u32* d_out, size_t cap, u64* nfound, size_t* bad, hipStream_t s)
{
    int rc;
    std::vector<BatchSrc> src;
    size_t b = count;
    if ((rc = batch_headers(c, kind, f, d_ins, in_bytes, nullptr, count, &src, &b, s))) {
        if (rc == ANSX_ERR_FORMAT && bad) *bad = b;
        return rc;
    }
    std::vector<u32> ord(count);  // ascending n; ties: the smaller batch index first
    for (size_t i = 0; i < count; i++) ord[i] = (u32)i;
    std::stable_sort(ord.begin(), ord.end(), [&](u32 x, u32 y) { return src[x].H.n < src[y].H.n; });
    const u32 drv = ord[0];
    for (size_t i = 0; i < count; i++)  // (the driver's bases are not read)
        if (i != drv && (!d_bases[i] || nbases[i] != (size_t)src[i].nblocks + 1)) {
            if (bad) *bad = i;
            return ANSX_ERR_ARG;
        }
    auto source = [&](u32 i, RangeTail* t) -> int {
        t->d_in = d_ins[i], t->H = src[i].H;
        if (container_plan(t->H, (u32)kind, (u32)f, in_bytes[i], &t->P)) return ANSX_ERR_FORMAT;  // (cannot happen: batch_headers did)
        t->P.g.payload_bytes = t->H.payload_bytes;
        return ANSX_OK;
    };
    const u64 n0 = src[drv].H.n;
    if (n0 > 0xFFFFFFFFull) return ANSX_ERR_ARG;  // (a step takes at most 2^32 - 1 candidates)
    u64 m = n0;
    u32* buf[2] = { nullptr, nullptr };
    u32 cur = 0;
    if (n0 > 0) {
        const size_t half = rup((size_t)n0, 4) + 16;  // (ints: 16-byte aligned halves with the decoders' slack behind)
        if ((rc = ensure(c, c->isect_ids, 8 * half))) return rc;
        buf[0] = (u32*)c->isect_ids.p, buf[1] = buf[0] + half;
        RangeTail t = {};
        if ((rc = source(drv, &t))) return rc;
        rc = decode_ids(c, t.P, t.d_in, in_bytes[drv], buf[0], n0, [](u32*, const u32*) -> int { return ANSX_OK; }, s);
        if (rc) {
            if ((rc == ANSX_ERR_DOMAIN || rc == ANSX_ERR_FORMAT) && bad) *bad = drv;
            return rc;
        }
    }
    for (size_t k = 1; k < count && m > 0; k++) {
        const u32 i = ord[k];
        RangeTail t = {};
        if ((rc = source(i, &t))) return rc;
        const IsectOut o = { buf[1 - cur], nullptr, nullptr, n0 };
        u64 tot = 0;
        if ((rc = isect_step(c, kind, f, t, in_bytes[i], d_bases[i], nbases[i], buf[cur], (u32)m, o, &tot, s))) {
            if (rc == ANSX_ERR_FORMAT && bad) *bad = count;  // (found on the device)
            if (rc == ANSX_ERR_DOMAIN && bad) *bad = i;
            return rc;
        }
        m = tot, cur = 1 - cur;
    }
    if (nfound) *nfound = m;
    if (m > cap) return ANSX_ERR_CAPACITY;
    if (m == 0) return ANSX_OK;
    HIPCHK(c, hipMemcpyAsync(d_out, buf[cur], 4 * (size_t)m, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ANSX_OK;
}

// --------------------------------------------------------------------------------- queries over a batch of lists
// The host path of ansx_intersect_batch_dev, ansx_union_batch_dev, ansx_bool_batch_dev, ansx_topk_batch_dev and
// ansx_topk_bool_batch_dev: ONE front end (query_front), one budget (query_budget), one loop
// over the groups (run_groups), and the phases below, which the four group functions string together.  A phase enqueues
// only; every host wait stands in a group function.

struct Moved {  // an array the ballots of a step compact: from -> to and, when asked for, every kept value's position -> idx
    const u32* from;
    u32 *to, *idx;
};

// The compact step behind a kernel that has written W's ballots and tile counts over the n candidates of queries
// [seg[j], seg[j + 1]), j < Q: the scan of the tile counts -> W.total, `a` compacted (and `b`, moved by the same ballots,
// when given), and the queries' bounds among what is kept -> nseg.  gf / df: k_isect_compact's two flag words.
int compact_step(ansx_ctx* c, const IsectWork& W, u32 n, const Moved& a, const Moved* b, const u32* seg, size_t Q, u32* nseg,
    const u32* gf, const u32* df, hipStream_t s)
{
    int rc;
    if ((rc = isect_tile_scan(c, W, s))) return rc;
    if ((rc = isect_move(c, W, a.from, n, { a.to, a.idx, nullptr, n }, gf, df, s))) return rc;
    if (b && (rc = isect_move(c, W, b->from, n, { b->to, b->idx, nullptr, n }, gf, df, s))) return rc;
    LAUNCH(c, "k_isectb_bounds", k_isectb_bounds, (u32)((Q + 256) / 256), 256, 0, s, seg, (u32)Q, n, (const u64*)W.ballots,
        (const u64*)W.counts, (const u64*)W.total, nseg);
    return ANSX_OK;
}

// The exclusion step of ansx_bool_batch_dev (ansx_bool.h) behind either positive phase: the n candidates of `cand`
// (d_total: null, or where the device holds how many of them there are), query j's in [seg[j], seg[j + 1]), that are in
// none of their query's lists xt[xo[j] .. xo[j + 1]) -> cand.to, their bounds -> nseg, their count -> W.total.  gf / df:
// k_isect_compact's two flag words.
// (its launch alone: the fused form of the filter step, DESIGN.md section 3s, marks between it and the compact step)
int bool_exclude_launch(ansx_ctx* c, const IsectWork& W, const u32* ids, const u32* cand, u32 n, const u64* d_total, const u32* seg,
    size_t Q, const u32* xo, const ansx_isb_list* xt, const u32* sflag, hipStream_t s)
{
    LAUNCH(c, "k_bool_exclude", k_bool_exclude, W.ntiles, ANSX_ISECT_NT, 0, s, ids, cand, n, d_total, seg, (u32)Q, xo, xt,
        (u32)c->dbg.bool_form, W.ballots, W.counts, sflag);
    return ANSX_OK;
}
int bool_exclude_step(ansx_ctx* c, const IsectWork& W, const u32* ids, const Moved& cand, u32 n, const u64* d_total, const u32* seg,
    size_t Q, const u32* xo, const ansx_isb_list* xt, const u32* sflag, u32* nseg, const u32* gf, const u32* df, hipStream_t s)
{
    int rc;
    if ((rc = bool_exclude_launch(c, W, ids, cand.from, n, d_total, seg, Q, xo, xt, sflag, s))) return rc;
    return compact_step(c, W, n, cand, nullptr, seg, Q, nseg, gf, df, s);
}

// The unique step of ansx_union_batch_dev (ansx_union.h) over a group's last merge buffer: of the n merged ids of
// `heads.from`, query j's in [seg[j], seg[j + 1]), the first of every run of equal ones -> heads.to, its position ->
// heads.idx (when asked for), the queries' bounds among the heads -> hseg, their count -> W.total.  uflag: k_union_heads'
// own flag word, which the compaction looks at as well.
int unique_step(ansx_ctx* c, const IsectWork& W, const Moved& heads, u32 n, const u32* seg, size_t Q, const u32* sflag, u32* uflag,
    u32* hseg, const u32* gf, hipStream_t s)
{
    LAUNCH(c, "k_union_heads", k_union_heads, W.ntiles, ANSX_ISECT_NT, 0, s, heads.from, n, seg, (u32)Q, W.ballots, W.counts, sflag,
        uflag);
    return compact_step(c, W, n, heads, nullptr, seg, Q, hseg, gf, (const u32*)uflag, s);
}

// What the front end leaves for the planners and the groups.  Without payloads the entries of br are the referenced
// lists; with payloads they are the entries of the source list (ansx_plan.h, query_sources): every referenced list's id
// container and, behind each term's, its payload.
struct QueryFront {
    int kind, f;
    size_t count;                   // the containers of the batch
    BrFront br;                     // the entries, their checked headers
    QuerySources src;               // with payloads: the source list
    const u32 *rid, *xrid;          // per term / per excluded term: its list's entry (what the planners read)
    const std::vector<u32>* index;  // per entry: the batch index an error names
    const std::vector<u32>* payof;  // with payloads: per entry, the entry of its payload or ANSX_TOPK_NONE
    std::vector<u32> entry_index;   // (with payloads: what index points to)
    std::vector<u64> n, off;        // per entry: its ints, and where the group at hand decodes it to (every group sets its own lists')
};

// The front end of the five calls: the headers of the containers the terms and the excluded terms name -- with d_pays,
// also of the payloads of the lists that are terms -- in ONE round trip, checked.  ANSX_ERR_FORMAT names in
// *bad_container the smallest batch index whose header fails the checks or whose payload differs from it in n.
// Without excluded terms the caller's array of terms is read where it is.
int query_front(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, const u8* const* d_pays,
    const size_t* pay_bytes, size_t count, const u32* terms, size_t nt, const u32* xterms, size_t nx, QueryFront* Q,
    size_t* bad_container, hipStream_t s)
{
    int rc;
    Q->kind = kind, Q->f = f, Q->count = count;
    std::vector<u32> both;
    const u32* named = terms;
    if (nx) both.assign(terms, terms + nt), both.insert(both.end(), xterms, xterms + nx), named = both.data();
    if (!d_pays) {
        if ((rc = batch_ranges_front(c, kind, f, d_ins, in_bytes, count, named, nt + nx, nullptr, &Q->br, bad_container, s))) return rc;
        Q->rid = Q->br.rid.data(), Q->index = &Q->br.ref, Q->payof = nullptr;
    } else {
        const QuerySources& S = Q->src;
        query_sources(named, nt, nt + nx, count, &Q->src);
        const size_t ne = S.owner.size();
        std::vector<const u8*> ptr(ne);
        std::vector<size_t> len(ne);
        std::vector<u32> all(ne);
        Q->entry_index.resize(ne);
        for (size_t e = 0; e < ne; e++) {
            const size_t i = S.batch_index(e);
            ptr[e] = S.pay[e] ? d_pays[i] : d_ins[i], len[e] = S.pay[e] ? pay_bytes[i] : in_bytes[i];
            all[e] = (u32)e, Q->entry_index[e] = (u32)i;
        }
        size_t failed = ne;
        rc = batch_ranges_front(c, kind, f, ptr.data(), len.data(), ne, all.data(), ne, nullptr, &Q->br, &failed, s);
        if (rc && rc != ANSX_ERR_FORMAT) return rc;
        const size_t bad = query_sources_first_bad(S, Q->br.rs, failed);
        if (bad < ne) {
            if (bad_container) *bad_container = S.batch_index(bad);
            return ANSX_ERR_FORMAT;
        }
        Q->rid = S.rid.data(), Q->index = &Q->entry_index, Q->payof = &S.payof;
    }
    Q->xrid = Q->rid + nt;
    Q->n.resize(Q->br.rs.size());
    for (size_t j = 0; j < Q->n.size(); j++) Q->n[j] = Q->br.rs[j].H.n;
    Q->off.assign(Q->n.size(), 0);
    return ANSX_OK;
}

// The ints a group may take: ANSX_ISECT_BATCH_INTS or the default -- HALF of it for a ranked call, whose groups hold
// twice what an unranked one's do
u64 query_budget(const ansx_ctx* c, bool ranked)
{
    const u64 ints = c->dbg.isect_batch_ints ? c->dbg.isect_batch_ints : ANSX_ISECT_BATCH_INTS_DEFAULT;
    return ranked ? ints / 2 : ints;
}

// The groups of a call, one after the other, and the call's last wait: behind the copies to the caller's arrays
template <class Group, class One> int run_groups(ansx_ctx* c, const std::vector<Group>& groups, const One& one, hipStream_t s)
{
    int rc;
    for (const Group& g : groups)
        if ((rc = one(g))) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    return ANSX_OK;
}

// Where an unranked call's results go: the caller's arrays of cap entries (cnt: ansx_union_batch_dev's counts, or null),
// how many of them the groups so far have taken, and every query's offset
struct IdsOut {
    u32 *ids, *cnt;
    size_t cap;
    u64 run;
    u64* offsets;
};

// Two buffers a step reads one of and writes the other
struct Flip {
    u32* b[2];
    u32 cur = 0;
    u32* from() const { return b[cur]; }
    u32* to() const { return b[1 - cur]; }
    void flip() { cur = 1 - cur; }
};

// ... decode: the group's lists whole, list lists[k] to ids + at[k], back to back, by the passes of ansx_decode_batch_dev;
// with `pay`, the payloads of those that have one to pay + at[k] -- the same layout, any geometry (a list that is only
// excluded has none: its part of pay is never read).  Host waits: those of the passes.
int group_decode(ansx_ctx* c, QueryFront& F, const std::vector<u32>& lists, const std::vector<u64>& at, u32* ids, u32* pay,
    size_t* bad_container, hipStream_t s)
{
    int rc;
    GeometryGroups geo;
    for (size_t k = 0; k < lists.size(); k++) F.off[lists[k]] = at[k], geo[br_geometry(F.br.rs[lists[k]].H)].push_back(lists[k]);
    if ((rc = batch_decode_groups(c, F.kind, F.f, F.br.rs, F.off, geo, F.count, ids, bad_container, s)) || !pay) return rc;
    geo.clear();
    for (size_t k = 0; k < lists.size(); k++) {
        const u32 r = (*F.payof)[lists[k]];
        if (r == ANSX_TOPK_NONE) continue;
        F.off[r] = at[k], geo[br_geometry(F.br.rs[r].H)].push_back(r);
    }
    return batch_decode_groups(c, F.kind, F.f, F.br.rs, F.off, geo, F.count, pay, bad_container, s);
}

// ... group workspace set-up.  The caller has laid out U: what goes up first, then what stays on the device.  Room for
// the first host_bytes of it in the upload page (what the host reads or writes) and for all of it with IsectWork over
// ncand candidates behind it in the device work area; the flag words s_fl zeroed and, when given, the overflow word of
// the ranked calls set (ANSX_TOPK_NONE, three zero words behind it).  No copy out of the page is pending: a group ends
// in a synchronisation.
struct GroupWs {
    u8* work;    // IsectWork's place
    u32* sflag;  // pinned: the scan's flag word, read back
    u64* total;  // pinned: a step's count, read back
};
int group_room(ansx_ctx* c, Upload& U, size_t host_bytes, u64 ncand, Upload::Sec<u32> s_fl, const Upload::Sec<u32>* s_of, GroupWs* ws)
{
    int rc;
    const size_t o_w = rup(U.end, 16);
    if ((rc = ensure_pinned(c, c->isectb_pin, c->isectb_pin_cap, host_bytes))) return rc;
    if ((rc = ensure(c, c->isectb_work, o_w + IsectWork::bytes(ncand, false)))) return rc;
    U.host = c->isectb_pin, U.devp = (u8*)c->isectb_work.p;
    memset(U.pin(s_fl), 0, s_fl.bytes);
    if (s_of) {
        u32* hof = U.pin(*s_of);
        hof[0] = ANSX_TOPK_NONE, hof[1] = hof[2] = hof[3] = 0;
    }
    ws->work = U.devp + o_w, ws->sflag = &c->pin->isect_sflag, ws->total = &c->pin->isect_total;
    return ANSX_OK;
}

// The select state of a ranked group, sections on the device behind what goes up: prefixes | what is left to find |
// cursors | histograms (the cursors are cleared with the histograms behind them)
struct SelectSecs {
    Upload::Sec<u64> pre;
    Upload::Sec<u32> want, cur, hist;
};
SelectSecs select_sections(Upload& U, size_t Q)
{
    SelectSecs t;
    t.pre = U.add<u64>(Q), t.want = U.add<u32>(Q), t.cur = U.add<u32>(rup(Q, 4)), t.hist = U.add<u32>(Q * (size_t)ANSX_TOPK_BINS);
    return t;
}

// ... and, the caller's tables put: the first `up` bytes of U in one copy and, for a ranked group, its select state cleared
int group_upload(ansx_ctx* c, const Upload& U, size_t up, const SelectSecs* sel, hipStream_t s)
{
    HIPCHK(c, hipMemcpyAsync(U.devp, U.host, up, hipMemcpyHostToDevice, s));
    if (sel) HIPCHK(c, hipMemsetAsync(U.dev(sel->cur), 0, sel->hist.off + sel->hist.bytes - sel->cur.off, s));
    return ANSX_OK;
}

// ... scan: the decoded gaps of the group's lists become ids, in place (section 3e's three kernels over all of them)
int group_scan(ansx_ctx* c, u32* ids, const std::vector<u64>& at, hipStream_t s, SumsPlan* S)
{
    int rc;
    const size_t nlists = at.size() - 1;
    if ((rc = sums_prepare(c, (uintptr_t)ids, at.back(), at.data(), nlists, s, S))) return rc;
    return sums_launch(c, ids, at.back(), nlists, *S, s);
}

// ... what its flag word says once it has come home (to ws.sflag) and the host has waited: the first list of the buffer
// whose sum left 32 bits -> ANSX_ERR_DOMAIN and its batch index
int scan_flag_status(const GroupWs& ws, const std::vector<u32>& lists, const std::vector<u32>& index, size_t* bad_container)
{
    const u32 flag = *ws.sflag;
    if (flag == ANSX_SS_NONE) return ANSX_OK;
    if (bad_container && flag < lists.size()) *bad_container = index[lists[flag]];
    return ANSX_ERR_DOMAIN;
}

// ... the drivers' ids gathered into the first candidate buffer, with the queries' first bounds (ansx_intersect_batch.h)
int gather_drivers(ansx_ctx* c, const u32* ids, const ansx_isb_query* G, size_t Q, u64 nc0, u32* cand, u32* seg, const u32* sflag,
    hipStream_t s)
{
    LAUNCH(c, "k_isectb_gather", k_isectb_gather, (u32)((std::max<u64>(nc0, Q + 1) + ANSX_ISECT_TILE - 1) / ANSX_ISECT_TILE),
        ANSX_ISECT_NT, 0, s, ids, G, (u32)Q, cand, (u32)nc0, seg, sflag);
    return ANSX_OK;
}

// a grid; 2^31 non-empty pairs in a round of merges
int merge_tiles_check(const UnbGroup& g, size_t* bad_query)
{
    for (const u64 t : g.tiles)
        if (t > 0x7FFFFFFFull) {
            if (bad_query) *bad_query = g.q0;
            return ANSX_ERR_ARG;
        }
    return ANSX_OK;
}

// ansx_intersect_batch_dev (ansx_intersect_batch.h; the plan: ansx_plan.h, isb_plan): the headers
// of the referenced containers in one round trip (query_front) -> the groups -> per group (isb_group): its lists
// decoded back to back into isectb_ids by the passes of ansx_decode_batch_dev, one segmented scan over all of them,
// k_isectb_gather, then a round per non-driver list of its longest query -- k_isectb_match and the compact step,
// between the two candidate buffers behind the lists -- and one copy of the survivors to the caller.
// Workspace: 4 bytes per int of the group's lists and 8 per int of its drivers (the budget bounds their sum unless one
// query exceeds it alone), a pass's, the scan's 16 bytes per 4096 ints, IsectWork over the candidates, and per query 16
// bytes of tables, 12 of segments and 16 per non-driver term.
// Host waits: one for the headers; per group those of its decode passes (decode_dev's on a sub-container: header and
// final read-back, one more where the form validates the index first), ONE for the scan's flag word and ONE per round,
// which brings the members' count (and, with the last round, the segments); one behind the copies, per call.  None
// grows with the number of queries.
// A group of ansx_bool_batch_dev that excludes something (g.xt) adds its second table to the upload and, where the
// rounds leave candidates, bool_exclude_step and ONE wait behind it; without g.xt nothing here differs.
int isb_group(ansx_ctx* c, QueryFront& F, const IsbGroup& g, IdsOut& out, size_t* bad_container, hipStream_t s)
{
    int rc;
    const size_t Q = g.q1 - g.q0, q1 = rup(Q + 1, 4);
    const u64 L = g.at.back(), nc0 = g.G[Q].dst;
    if (nc0 == 0) {  // (every driver is empty: nothing to look up, nothing is decoded)
        for (size_t j = 0; j <= Q; j++) out.offsets[g.q0 + j] = out.run;
        return ANSX_OK;
    }
    // the lists | two candidate buffers, each with the decoders' slack behind
    const size_t o_c = rup((size_t)L, 4) + 16, half = rup((size_t)nc0, 4) + 16;
    if ((rc = ensure(c, c->isectb_ids, 4 * (o_c + 2 * half)))) return rc;
    u32* ids = (u32*)c->isectb_ids.p;
    Flip buf = { { ids + o_c, ids + o_c + half } };
    if ((rc = group_decode(c, F, g.lists, g.at, ids, nullptr, bad_container, s))) return rc;

    // one upload: zero flag words | queries | round table; behind it on the device: two arrays of segments | IsectWork
    Upload U;
    const auto s_fl = U.add<u32>(4);
    const auto s_g = U.add<ansx_isb_query>(Q + 1);
    const auto s_ro = U.add<u32>(Q + 1);
    const auto s_rt = U.add<ansx_isb_list>(g.rt.size());
    const bool excl = !g.xt.empty();  // (ansx_bool_batch_dev only: the group excludes something)
    const auto s_xo = U.add<u32>(excl ? Q + 1 : 0);
    const auto s_xt = U.add<ansx_isb_list>(g.xt.size());
    const size_t up = U.end;
    const auto s_seg = U.add<u32>(2 * q1);  // (the host's copy: the last round's, read back)
    GroupWs ws;
    if ((rc = group_room(c, U, U.end, nc0, s_fl, nullptr, &ws))) return rc;
    U.put(s_g, g.G.data()), U.put(s_ro, g.rt_off.data());
    if (!g.rt.empty()) U.put(s_rt, g.rt.data());
    if (excl) U.put(s_xo, g.xt_off.data()), U.put(s_xt, g.xt.data());
    if ((rc = group_upload(c, U, up, nullptr, s))) return rc;
    Flip seg = { { U.dev(s_seg), U.dev(s_seg) + q1 } };
    const u32* zero = U.dev(s_fl);

    SumsPlan S;
    if ((rc = group_scan(c, ids, g.at, s, &S))) return rc;
    if ((rc = gather_drivers(c, ids, U.dev(s_g), Q, nc0, buf.from(), seg.from(), S.flag, s))) return rc;
    HIPCHK(c, hipMemcpyAsync(ws.sflag, S.flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = scan_flag_status(ws, g.lists, *F.index, bad_container))) return rc;

    u32 nc = (u32)nc0, r = 0;
    for (; r < g.rounds && nc > 0; r++) {
        const IsectWork W(ws.work, nc, false);
        LAUNCH(c, "k_isectb_match", k_isectb_match, W.ntiles, ANSX_ISECT_NT, 0, s, (const u32*)ids, (const u32*)buf.from(), nc,
            (const u32*)seg.from(), (u32)Q, (const u32*)U.dev(s_ro), (const ansx_isb_list*)U.dev(s_rt), r, W.ballots, W.counts);
        if ((rc = compact_step(c, W, nc, { buf.from(), buf.to(), nullptr }, nullptr, seg.from(), Q, seg.to(), zero, zero, s))) return rc;
        HIPCHK(c, hipMemcpyAsync(ws.total, W.total, 8, hipMemcpyDeviceToHost, s));
        if (r + 1 == g.rounds) HIPCHK(c, hipMemcpyAsync(U.pin(s_seg), seg.to(), 4 * (Q + 1), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        nc = (u32)*ws.total, buf.flip(), seg.flip();
    }
    const bool xran = excl && nc > 0;
    if (xran) {  // ONE exclusion step over what the rounds left (ansx_bool.h), and one more wait
        const IsectWork W(ws.work, nc, false);
        if ((rc = bool_exclude_step(c, W, ids, { buf.from(), buf.to(), nullptr }, nc, nullptr, seg.from(), Q, U.dev(s_xo), U.dev(s_xt),
                 S.flag, seg.to(), zero, zero, s)))
            return rc;
        HIPCHK(c, hipMemcpyAsync(ws.total, W.total, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(U.pin(s_seg), seg.to(), 4 * (Q + 1), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        nc = (u32)*ws.total, buf.flip(), seg.flip();
    }
    // the segments behind the last step: the drivers' (none), what came back, or nothing left
    const u32* hseg = U.pin(s_seg);
    for (size_t j = 0; j <= Q; j++)
        out.offsets[g.q0 + j] = out.run + (xran ? hseg[j] : g.rounds == 0 ? g.G[j].dst : r == g.rounds ? hseg[j] : 0);
    if (nc > 0 && out.run + nc <= out.cap)
        HIPCHK(c, hipMemcpyAsync(out.ids + out.run, buf.from(), 4 * (size_t)nc, hipMemcpyDeviceToDevice, s));
    out.run += nc;
    return ANSX_OK;
}

// ansx_union_batch_dev (ansx_union.h; the plan: ansx_plan.h, unb_plan): the front end of
// ansx_intersect_batch_dev -- the headers of the referenced containers in one round trip, the groups -> per group
// (unb_group): its lists decoded back to back into isectb_ids and scanned into ids, one upload of every round's pair
// table, a launch of k_union_merge per round between the two merge buffers behind the lists, then the unique step over
// the last round's buffer into the other and, with counts, k_union_counts -- and one copy per output to the caller.  The
// context's buffers are those of ansx_intersect_batch_dev (a context runs one call at a time).
// Workspace: 4 bytes per int of the group's lists and 8 per int of its queries' lists as named (16 with counts: the
// heads' positions and the counts), a pass's, the scan's, IsectWork over the merge buffer, and 8 bytes per query and 40
// per pair of tables -- fewer than two pairs per term.
// Host waits: one for the headers; per group those of its decode passes and ONE more, behind the unique step, which
// brings the scan's flag word, the total and the queries' bounds: every size between the scan and the unique step is
// the plan's.  One behind the copies, per call.  None grows with the queries or the rounds.
// A group of ansx_bool_batch_dev that excludes something (g.xt) adds its second table to the upload and
// bool_exclude_step in front of that one wait (the heads' count stays on the device); without g.xt nothing here differs.
int unb_group(ansx_ctx* c, QueryFront& F, const UnbGroup& g, IdsOut& out, size_t* bad_container, size_t* bad_query, hipStream_t s)
{
    int rc;
    const size_t Q = g.q1 - g.q0, q1 = rup(Q + 1, 4);
    const u64 L = g.at.back(), M = g.seg[Q];
    if (M == 0) {  // (every list is empty: nothing is decoded)
        for (size_t j = 0; j <= Q; j++) out.offsets[g.q0 + j] = out.run;
        return ANSX_OK;
    }
    if ((rc = merge_tiles_check(g, bad_query))) return rc;
    // the lists | two merge buffers | with counts: the heads' positions | the counts; each with the decoders' slack behind
    const size_t o_c = rup((size_t)L, 4) + 16, half = rup((size_t)M, 4) + 16;
    if ((rc = ensure(c, c->isectb_ids, 4 * (o_c + (out.cnt ? 4 : 2) * half)))) return rc;
    u32* ids = (u32*)c->isectb_ids.p;
    u32* const mb[2] = { ids + o_c, ids + o_c + half };
    u32* idx = out.cnt ? ids + o_c + 2 * half : nullptr;
    u32* cnt = out.cnt ? ids + o_c + 3 * half : nullptr;
    if ((rc = group_decode(c, F, g.lists, g.at, ids, nullptr, bad_container, s))) return rc;

    // one upload: zero flag words (k_isect_compact's four, k_union_heads' one) | the queries' spans | every round's pairs;
    // behind it on the device: the bounds among the heads | IsectWork
    Upload U;
    const auto s_fl = U.add<u32>(8);
    const auto s_seg = U.add<u32>(Q + 1);
    const auto s_p = U.add<ansx_unb_pair>(g.pairs.size());
    const bool excl = !g.xt.empty();  // (ansx_bool_batch_dev only: the group excludes something)
    const auto s_xo = U.add<u32>(excl ? Q + 1 : 0);
    const auto s_xt = U.add<ansx_isb_list>(g.xt.size());
    const size_t up = U.end;
    const auto s_hs = U.add<u32>(q1);  // (the host's copy: read back)
    const auto s_xs = U.add<u32>(excl ? q1 : 0);  // (the bounds behind the exclusion step)
    GroupWs ws;
    if ((rc = group_room(c, U, U.end, M, s_fl, nullptr, &ws))) return rc;
    U.put(s_seg, g.seg.data()), U.put(s_p, g.pairs.data());
    if (excl) U.put(s_xo, g.xt_off.data()), U.put(s_xt, g.xt.data());
    if ((rc = group_upload(c, U, up, nullptr, s))) return rc;
    const u32* zero = U.dev(s_fl);
    u32* uflag = U.dev(s_fl) + 4;
    const u32* seg = U.dev(s_seg);

    SumsPlan S;
    if ((rc = group_scan(c, ids, g.at, s, &S))) return rc;
    for (u32 r = 0; r < g.rounds; r++) {
        const u32 np = g.roff[r + 1] - g.roff[r];
        if (np == 0) continue;  // (the queries that have this round are empty)
        const u32* from = mb[1 - (r & 1u)];
        LAUNCH(c, "k_union_merge", k_union_merge, (u32)g.tiles[r], ANSX_ISECT_NT, 0, s, (const u32*)ids, from, mb[r & 1u],
            (const ansx_unb_pair*)U.dev(s_p) + g.roff[r], np, (const u32*)S.flag);
    }
    u32 *merged = mb[(g.rounds - 1u) & 1u], *heads = mb[g.rounds & 1u];  // (what the last round wrote, and the other buffer)
    const IsectWork W(ws.work, M, false);
    const u32* hseg = U.dev(s_hs);
    if ((rc = unique_step(c, W, { merged, heads, idx }, (u32)M, seg, Q, S.flag, uflag, U.dev(s_hs), zero, s))) return rc;
    if (out.cnt)
        LAUNCH(c, "k_union_counts", k_union_counts, W.ntiles, ANSX_ISECT_NT, 0, s, (const u32*)idx, hseg, seg, (u32)Q,
            (const u64*)W.total, (u32)M, cnt, (const u32*)S.flag);
    const u32* res = heads;
    if (excl) {  // ONE exclusion step over the heads (ansx_bool.h): their count stays on the device, no wait is added
        if ((rc = bool_exclude_step(c, W, ids, { heads, merged, nullptr }, (u32)M, W.total, hseg, Q, U.dev(s_xo), U.dev(s_xt), S.flag,
                 U.dev(s_xs), zero, uflag, s)))
            return rc;
        hseg = U.dev(s_xs), res = merged;
    }
    HIPCHK(c, hipMemcpyAsync(ws.sflag, S.flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(ws.total, W.total, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(U.pin(s_hs), hseg, 4 * (Q + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = scan_flag_status(ws, g.lists, *F.index, bad_container))) return rc;
    const u64 nu = *ws.total;
    const u32* hs = U.pin(s_hs);
    for (size_t j = 0; j <= Q; j++) out.offsets[g.q0 + j] = out.run + hs[j];
    if (nu > 0 && out.run + nu <= out.cap) {
        HIPCHK(c, hipMemcpyAsync(out.ids + out.run, res, 4 * (size_t)nu, hipMemcpyDeviceToDevice, s));
        if (out.cnt) HIPCHK(c, hipMemcpyAsync(out.cnt + out.run, cnt, 4 * (size_t)nu, hipMemcpyDeviceToDevice, s));
    }
    out.run += nu;
    return ANSX_OK;
}

// ansx_bool_batch_dev (ansx_bool.h) and, as its cases without excluded terms,
// ansx_intersect_batch_dev (op ALL) and ansx_union_batch_dev (op ANY; d_cnt: its counts, null for the other two).  The
// front end over the terms followed by the excluded terms -- still one round trip for the headers -- then the plan of
// the chosen op with the excluded lists (plan_excl_tables) and the op's own groups, which run the exclusion step where
// a group excludes something.
// Workspace: the op's, the excluded lists among the group's lists, and 4 bytes per query and 16 per excluded term
// of tables (ANY: 4 more per query of bounds).  Host waits: ALL one more per group that excludes something and has
// candidates left behind its rounds; ANY none more -- the heads' count stays on the device.
int bool_batch(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, size_t count, int op, const u32* terms,
    const u64* qoff, const u32* xterms, const u64* xqoff, size_t nq, u32* d_out, u32* d_cnt, size_t cap, u64* out_offsets,
    size_t* bad_container, size_t* bad_query, hipStream_t s)
{
    int rc;
    QueryFront F;
    if ((rc = query_front(c, kind, f, d_ins, in_bytes, nullptr, nullptr, count, terms, (size_t)qoff[nq], xterms,
             xqoff ? (size_t)xqoff[nq] : 0, &F, bad_container, s)))
        return rc;
    const u64 budget = query_budget(c, false);
    IdsOut out = { d_out, d_cnt, cap, 0, out_offsets };
    if (op == ANSX_BOOL_ALL) {
        std::vector<IsbGroup> groups;
        if ((rc = isb_plan(F.n.data(), F.n.size(), F.rid, qoff, nq, budget, &groups, bad_query, F.xrid, xqoff))) return rc;
        rc = run_groups(c, groups, [&](const IsbGroup& g) { return isb_group(c, F, g, out, bad_container, s); }, s);
    } else {
        std::vector<UnbGroup> groups;
        if ((rc = unb_plan(F.n.data(), F.n.size(), F.rid, qoff, nq, budget, ANSX_UNION_TILE, &groups, bad_query, F.xrid, xqoff))) return rc;
        rc = run_groups(c, groups, [&](const UnbGroup& g) { return unb_group(c, F, g, out, bad_container, bad_query, s); }, s);
    }
    return rc ? rc : out.run > cap ? ANSX_ERR_CAPACITY : ANSX_OK;
}

// ansx_topk_batch_dev (ansx_topk.h; the plan: unb_plan with the terms behind its pairs).  The front
// end of the calls above over the id containers AND the payloads of the referenced lists, interleaved (list u of the
// referenced ones at 2u, its payload at 2u + 1), still one round trip for the headers; the groups of unb_plan under HALF
// the budget -- a group holds twice what a union's does; per group (topk_group): ids and payloads decoded with the same
// offsets into two buffers of one layout, the scan over the ids, one upload of the pair and weight tables, a launch of
// k_topk_merge per round, the unique step as in unb_group (with positions), k_topk_scores and the ranked tail: the eight
// rounds of k_topk_hist / k_topk_pick, k_topk_gather and k_topk_sort, which writes the caller's arrays.
// Workspace: 4 (8 with payloads) bytes per int of the group's lists, 20 per int of its queries' lists as named (two key and
// two value merge buffers, the scores), a pass's, the scan's, IsectWork over the merge buffer, and per query 8 k bytes of
// slots, 1 KiB of histogram, 24 bytes of state and bounds and 48 per pair of tables.
// Host waits: one for the headers; per group those of its decode passes (ids, then payloads) and ONE behind the sort,
// which brings the scan's flag word, the overflow word and the bounds among the heads; one per call at the end.  None
// between merge rounds or select rounds; no grid depends on data the host has not seen.
struct TopkOut {
    const u32* weights;
    u32 k, pow2;
    u32 *ids, *scores, *counts;
    bool pays;
    // ansx_topk_bool_batch_dev: the overflow word is lowered by k_topkb_check, behind the exclusion
    // step; form: ANSX_TOPKB_FORM_*
    bool check;
    u32 form;
    // ansx_topk_query_batch_dev: null, or every query's threshold as it applies (query_split's m,
    // by the call's query number) and, for a group with required terms, the weight of every optional term as named in
    // isb_plan's orid; qform: ANSX_TOPKQ_FORM_*
    const u32 *msm = nullptr, *oweights = nullptr;
    u32 qform = 0;
    // ansx_topk_scored_batch_dev: null, or the scorer that turns the payloads into impacts
    const ansx_scorer* scorer = nullptr;
    // ansx_topk_facets_batch_dev: null, or the column the results are counted over; null, or where
    // every query's |R(q)| goes (host)
    const ansx_facets* facets = nullptr;
    u32* totals = nullptr;
    // ansx_topk_filter_batch_dev: null, or the columns and the clauses that cut R(q) down to R'(q)
    const ansx_filters* filters = nullptr;
};

// ... the impact step of ansx_topk_scored_batch_dev (ansx_topk_scored.h) behind the scan: the payload of every posting of
// every list of the group that has one -> its impact, in place (k_topk_impacts: ONE launch).  impact_tables, before
// anything of the group is launched: the host's table over the group's lists (impact_plan), which goes up with the
// group's other tables; more than 2^31 - 1 tiles: ANSX_ERR_ARG with the group's first query.  An id the norms have no
// entry for lowers the scan's flag word: the wait that brings it home is the group's own.
struct ImpactTables {
    std::vector<ansx_impact_list> P;
    u64 tiles = 0;
    u32 rounds = ANSX_IMPACT_ROUNDS_DEFAULT;
};
int impact_tables(const ansx_ctx* c, const std::vector<u32>& lists, const std::vector<u64>& at, const std::vector<u32>* payof, size_t q0,
    ImpactTables* T, size_t* bad_query)
{
    T->rounds = c->dbg.topk_impact_rounds ? c->dbg.topk_impact_rounds : ANSX_IMPACT_ROUNDS_DEFAULT;
    const int rc = impact_plan(lists, at, payof, T->rounds * ANSX_IMPACT_NT * 4u, &T->P, &T->tiles);
    if (rc && bad_query) *bad_query = q0;
    return rc;
}
// the workgroups of the staged form that the chip holds at the kernel's occupancy with srows rows of stage
template <u32 ROUNDS> int impact_staged_wgs(ansx_ctx* c, u32 srows, u32* wgs)
{
    const u32 key = ROUNDS << 16 | srows;
    const auto it = c->impact_wgs.find(key);
    if (it != c->impact_wgs.end()) {
        *wgs = it->second;
        return ANSX_OK;
    }
    int per_cu = 0;
    HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_topk_impacts<ROUNDS, true>, (int)ANSX_IMPACT_NT,
                  (size_t)srows * ANSX_IMPACT_COLS * 4u));
    *wgs = c->impact_wgs[key] = (u32)std::max(per_cu, 1) * c->num_cus;
    return ANSX_OK;
}
template <u32 ROUNDS> int impact_launch(ansx_ctx* c, const ansx_scorer& sc, const ImpactTables& T, const ansx_impact_list* d_P,
    const u32* ids, u32* pay, u32* sflag, hipStream_t s)
{
    const u32 np = (u32)T.P.size(), ntiles = (u32)T.tiles, rows = sc.tf_rows;
    // (the default is the staged form: DESIGN.md section 3q, "the form")
    if (c->dbg.topk_impact_form == (int)ANSX_IMPACT_FORM_GLOBAL) {
        LAUNCH(c, "k_topk_impacts", (k_topk_impacts<ROUNDS, false>), ntiles, ANSX_IMPACT_NT, 0, s, ids, pay, d_P, np, ntiles, sc.d_norms,
            (u64)sc.ndocs, sc.d_table, rows, 0u, sflag);
        return ANSX_OK;
    }
    const u32 srows = std::min(rows, c->dbg.topk_impact_stage ? c->dbg.topk_impact_stage : ANSX_IMPACT_STAGE_ROWS);
    u32 wgs = 0;
    int rc;
    if ((rc = impact_staged_wgs<ROUNDS>(c, srows, &wgs))) return rc;
    if (c->dbg.topk_impact_grid) wgs = c->dbg.topk_impact_grid;
    LAUNCH(c, "k_topk_impacts", (k_topk_impacts<ROUNDS, true>), std::min(wgs, ntiles), ANSX_IMPACT_NT, (size_t)srows * ANSX_IMPACT_COLS * 4u,
        s, ids, pay, d_P, np, ntiles, sc.d_norms, (u64)sc.ndocs, sc.d_table, rows, srows, sflag);
    return ANSX_OK;
}
int impact_step(ansx_ctx* c, const ansx_scorer& sc, const ImpactTables& T, const ansx_impact_list* d_P, const u32* ids, u32* pay,
    u32* sflag, hipStream_t s)
{
    if (T.P.empty()) return ANSX_OK;  // (no list of the group has a payload: nothing is scored)
    return T.rounds == 1 ? impact_launch<1>(c, sc, T, d_P, ids, pay, sflag, s)
        : T.rounds == 2  ? impact_launch<2>(c, sc, T, d_P, ids, pay, sflag, s)
                         : impact_launch<4>(c, sc, T, d_P, ids, pay, sflag, s);
}

// ... the optional step of ansx_topk_query_batch_dev (ansx_topk_query.h) behind the required rounds: the n candidates of
// `cand` with `score` beside them (d_total: null, or where the device holds their count), query j's in [seg[j], seg[j + 1]),
// take the postings of their query's optional lists ot[oo[j] .. oo[j + 1]) -- the scores in place -- and those with at
// least msm[j] of them -> cand.to, their scores -> score.to, their bounds -> nseg, their count -> W.total.
struct ShouldTables {
    const u32* oo;
    const ansx_isb_list* ot;
    const u32 *ow, *msm;
    u32 form;
};
int should_step(ansx_ctx* c, const IsectWork& W, const u32* ids, const u32* pay, const Moved& cand, const Moved& score, u32 n,
    const u64* d_total, const u32* seg, size_t Q, const ShouldTables& T, const u32* sflag, u32* nseg, const u32* gf, const u32* df,
    hipStream_t s)
{
    LAUNCH(c, "k_topkq_should", k_topkq_should, W.ntiles, ANSX_ISECT_NT, 0, s, ids, pay, cand.from, (u32*)score.from, n, d_total, seg, (u32)Q,
        T.oo, T.ot, T.ow, T.msm, T.form, W.ballots, W.counts, sflag);
    return compact_step(c, W, n, cand, &score, seg, Q, nseg, gf, df, s);
}

// ... its threshold step behind k_topk_scores, for a group without required terms in which some query asks for two
// entries or more (k_topkq_atleast): the heads with at least msm[j] entries -> heads.to, their scores -> score.to, their
// bounds -> nseg, their count -> W.total, which held the heads'
int atleast_step(ansx_ctx* c, const IsectWork& W, const u32* idx, const Moved& heads, const Moved& score, u32 n, const u32* hseg,
    const u32* seg, size_t Q, const u32* msm, const u32* sflag, u32* nseg, const u32* gf, const u32* df, hipStream_t s)
{
    LAUNCH(c, "k_topkq_atleast", k_topkq_atleast, W.ntiles, ANSX_ISECT_NT, 0, s, idx, hseg, seg, (u32)Q, (const u64*)W.total, n, msm,
        W.ballots, W.counts, sflag);
    return compact_step(c, W, n, heads, &score, hseg, Q, nseg, gf, df, s);
}

// The select of a ranked call over the candidates (ids[h], score[h]), h < min(*total, n), query j's in [hseg[j], hseg[j + 1]),
// all on the device: the eight rounds of k_topk_hist / k_topk_pick, k_topk_gather and k_topk_sort, which writes the
// caller's arrays.  ntiles: the tiles of n.  T: the select state in U (select_sections), cleared; slots: 8 k bytes per query.
struct Ranked {
    const u32 *ids, *score, *hseg;
    const u64* total;
    u32 n, ntiles;
};
int topk_select(ansx_ctx* c, const Ranked& R, size_t Q, const Upload& U, const SelectSecs& T, u64* slots, size_t q0, const TopkOut& o,
    const u32* sflag, hipStream_t s)
{
    for (u32 r = 0; r < ANSX_TOPK_ROUNDS; r++) {
        LAUNCH(c, "k_topk_hist", k_topk_hist, R.ntiles, ANSX_ISECT_NT, 0, s, R.ids, R.score, R.hseg, (u32)Q, R.total, R.n, r,
            (const u64*)U.dev(T.pre), U.dev(T.hist), sflag);
        LAUNCH(c, "k_topk_pick", k_topk_pick, (u32)((Q + 3) / 4), 256, 0, s, R.hseg, (u32)Q, o.k, r, U.dev(T.pre), U.dev(T.want),
            U.dev(T.hist), sflag);
    }
    LAUNCH(c, "k_topk_gather", k_topk_gather, R.ntiles, ANSX_ISECT_NT, 0, s, R.ids, R.score, R.hseg, (u32)Q, R.total, R.n, o.k,
        (const u64*)U.dev(T.pre), U.dev(T.cur), slots, sflag);
    LAUNCH(c, "k_topk_sort", k_topk_sort, (u32)Q, ANSX_ISECT_NT, 0, s, (const u64*)slots, R.hseg, (u64)q0, o.k, o.pow2, o.ids, o.scores, sflag);
    return ANSX_OK;
}

// ... the facet step of ansx_topk_facets_batch_dev (ansx_facet.h) in front of the ranked tail, behind every step that
// filters: the ids of R fall into the rows of counts of queries q0 .. q0 + Q (k_facet_count: ONE launch, no wait, no
// upload).  An id the column has no entry for lowers the bad-id word, the third of s_of, which facet_word raises before
// the group's upload and ranked_tail sends home with the overflow word.
void facet_word(const TopkOut& o, const Upload& U, Upload::Sec<u32> s_of)
{
    if (o.facets) U.pin(s_of)[2] = ANSX_TOPK_NONE;
}
// the workgroups of the lds form that the chip holds at the kernel's occupancy with nvalues words of LDS
template <bool COMBINE> int facet_lds_wgs(ansx_ctx* c, u32 nvalues, u32* wgs)
{
    const u32 key = nvalues << 1 | (COMBINE ? 1u : 0u);  // (nvalues <= ANSX_FACET_LDS_VALUES)
    const auto it = c->facet_wgs.find(key);
    if (it != c->facet_wgs.end()) {
        *wgs = it->second;
        return ANSX_OK;
    }
    int per_cu = 0;
    HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_facet_count<true, COMBINE>, (int)ANSX_ISECT_NT, (size_t)nvalues * 4u));
    *wgs = c->facet_wgs[key] = (u32)std::max(per_cu, 1) * c->num_cus;
    return ANSX_OK;
}
template <bool COMBINE> int facet_launch_lds(ansx_ctx* c, const Ranked& R, size_t Q, const ansx_facets& f, u32* rows, u32* d_bad,
    const u32* sflag, hipStream_t s)
{
    u32 wgs = 0;
    int rc;
    if ((rc = facet_lds_wgs<COMBINE>(c, f.nvalues, &wgs))) return rc;
    if (c->dbg.facet_grid) wgs = c->dbg.facet_grid;
    LAUNCH(c, "k_facet_count", (k_facet_count<true, COMBINE>), std::min(wgs, R.ntiles), ANSX_ISECT_NT, (size_t)f.nvalues * 4u, s, R.ids, R.hseg,
        (u32)Q, R.total, R.n, f.d_values, (u64)f.ndocs, f.nvalues, rows, d_bad, sflag);
    return ANSX_OK;
}
int facet_step(ansx_ctx* c, const Ranked& R, size_t Q, size_t q0, const TopkOut& o, u32* d_bad, const u32* sflag, hipStream_t s)
{
    const ansx_facets& f = *o.facets;
    u32* rows = f.d_counts + q0 * (size_t)f.nvalues;
    // (the default is the lds form where the values fit: DESIGN.md section 3r, "the form")
    if (f.nvalues > ANSX_FACET_LDS_VALUES || c->dbg.facet_form == (int)ANSX_FACET_FORM_ATOMIC) {
        LAUNCH(c, "k_facet_count", (k_facet_count<false, false>), R.ntiles, ANSX_ISECT_NT, 0, s, R.ids, R.hseg, (u32)Q, R.total, R.n, f.d_values,
            (u64)f.ndocs, f.nvalues, rows, d_bad, sflag);
        return ANSX_OK;
    }
    return c->dbg.facet_no_combine ? facet_launch_lds<false>(c, R, Q, f, rows, d_bad, sflag, s)
                                   : facet_launch_lds<true>(c, R, Q, f, rows, d_bad, sflag, s);
}

// ... the filter step of ansx_topk_filter_batch_dev (ansx_filter.h) behind every other step that filters and in front of
// facet_step: the ids of R that pass their query's clauses.  A group's clause table (filter_tables): Q + 1 offsets and its
// queries' clauses with the column's address in them; both ride in the group's one upload.  Empty where no query of the
// group has a clause: such a group launches and uploads nothing more.  An id the columns have no entry for lowers the
// bad-id word, the fourth of s_of, which filter_word raises (in the page: a group without clauses never copies it back).
struct FilterTables {
    std::vector<u32> off;
    std::vector<ansx_filter_dev> cl;
    bool active() const { return !cl.empty(); }
};
void filter_tables(const TopkOut& o, size_t q0, size_t Q, FilterTables* T)
{
    if (!o.filters) return;
    const ansx_filters& f = *o.filters;
    const u64 a = f.fqoff[q0], b = f.fqoff[q0 + Q];
    if (a == b) return;
    T->off.resize(Q + 1);
    for (size_t j = 0; j <= Q; j++) T->off[j] = (u32)(f.fqoff[q0 + j] - a);  // (at most ANSX_FILTER_MAX_CLAUSES per query)
    T->cl.resize((size_t)(b - a));
    for (u64 e = a; e < b; e++) {
        const ansx_filter_clause& k = f.clauses[e];
        T->cl[(size_t)(e - a)] = { f.d_columns[k.column], k.lo, k.hi, k.flags, 0u };
    }
}
void filter_word(const TopkOut& o, const Upload& U, Upload::Sec<u32> s_of)
{
    if (o.filters) U.pin(s_of)[3] = ANSX_TOPK_NONE;
}
// does the step ride on the exclusion step of a group that has one (the fused form), or run on its own
bool filter_fused(const ansx_ctx* c, bool excl) { return excl && c->dbg.filter_form != (int)ANSX_FILTER_FORM_OWN; }
template <bool PRIOR> int filter_mark(ansx_ctx* c, const IsectWork& W, const u32* cand, u32 n, const u64* d_total, const u32* seg, size_t Q,
    const u32* foff, const ansx_filter_dev* fc, const TopkOut& o, u32* d_bad, const u32* sflag, hipStream_t s)
{
    LAUNCH(c, "k_filter_mark", k_filter_mark<PRIOR>, W.ntiles, ANSX_ISECT_NT, 0, s, cand, seg, (u32)Q, d_total, n, foff, fc,
        (u64)o.filters->ndocs, W.ballots, W.counts, d_bad, sflag);
    return ANSX_OK;
}
// the own form, atleast_step's shape: the mark, then ids and scores moved by its ballots, the new bounds -> nseg, the
// count -> W.total
int filter_step(ansx_ctx* c, const IsectWork& W, const Moved& cand, const Moved& score, u32 n, const u64* d_total, const u32* seg, size_t Q,
    const u32* foff, const ansx_filter_dev* fc, const TopkOut& o, u32* d_bad, const u32* sflag, u32* nseg, const u32* gf, const u32* df,
    hipStream_t s)
{
    int rc;
    if ((rc = filter_mark<false>(c, W, cand.from, n, d_total, seg, Q, foff, fc, o, d_bad, sflag, s))) return rc;
    return compact_step(c, W, n, cand, &score, seg, Q, nseg, gf, df, s);
}

// ... the ranked tail over the candidates R of queries q0 .. q0 + Q: k_topkb_check when the call asks for it (it lowers
// the overflow word s_of over the scores that are left), the select, and the overflow word and the bounds on their way
// home to the upload page (the bounds to s_back) -- in front of them the scan's flag word, to h_sflag, where the host
// has not seen it yet (null: it has); with facets the bad-id word rides in the overflow word's copy, and so does the
// filter's where the group has a clause (`filtered`).  The caller waits; ranked_counts reads what came.
int ranked_tail(ansx_ctx* c, const Ranked& R, size_t Q, size_t q0, const TopkOut& o, const Upload& U, const SelectSecs& T, u64* slots,
    Upload::Sec<u32> s_of, Upload::Sec<u32> s_back, const u32* sflag, u32* h_sflag, hipStream_t s, bool filtered = false)
{
    int rc;
    if (o.check)
        LAUNCH(c, "k_topkb_check", k_topkb_check, R.ntiles, ANSX_ISECT_NT, 0, s, R.score, R.hseg, (u32)Q, R.total, R.n, U.dev(s_of), sflag);
    if ((rc = topk_select(c, R, Q, U, T, slots, q0, o, sflag, s))) return rc;
    if (h_sflag) HIPCHK(c, hipMemcpyAsync(h_sflag, sflag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(U.pin(s_of), U.dev(s_of), filtered ? 16 : o.facets ? 12 : 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(U.pin(s_back), R.hseg, 4 * (Q + 1), hipMemcpyDeviceToHost, s));
    return ANSX_OK;
}
// the first query of the group with a score of 2^32 - 1 or more among its results -> ANSX_ERR_DOMAIN; then, with filters,
// the first with an id the columns have no entry for; then, with facets, the first with an id the column has no entry
// for -> ANSX_ERR_DOMAIN; else the counts and the totals, from the same bounds
int ranked_counts(const u32* h_of, const u32* h_seg, size_t Q, size_t q0, const TopkOut& o, size_t* bad_query)
{
    const u32 fbad = o.filters ? h_of[3] : ANSX_TOPK_NONE;  // (a group without clauses: filter_word's, never copied over)
    const u32 bad = h_of[0] != ANSX_TOPK_NONE ? h_of[0] : fbad != ANSX_TOPK_NONE ? fbad : o.facets ? h_of[2] : ANSX_TOPK_NONE;
    if (bad != ANSX_TOPK_NONE) {
        if (bad_query) *bad_query = q0 + bad;
        return ANSX_ERR_DOMAIN;
    }
    if (o.counts)
        for (size_t j = 0; j < Q; j++) o.counts[q0 + j] = std::min<u32>(o.k, h_seg[j + 1] - h_seg[j]);
    if (o.totals)
        for (size_t j = 0; j < Q; j++) o.totals[q0 + j] = h_seg[j + 1] - h_seg[j];
    return ANSX_OK;
}
// no query of the group has a result: every slot is ANSX_NO_ID / 0
int ranked_nothing(ansx_ctx* c, size_t Q, size_t q0, const TopkOut& o, hipStream_t s)
{
    LAUNCH(c, "k_topk_sort", k_topk_sort, (u32)Q, ANSX_ISECT_NT, 0, s, (const u64*)nullptr, (const u32*)nullptr, (u64)q0, o.k, o.pow2,
        o.ids, o.scores, (const u32*)nullptr);
    if (o.counts) memset(o.counts + q0, 0, 4 * Q);
    if (o.totals) memset(o.totals + q0, 0, 4 * Q);
    return ANSX_OK;
}

int topk_group(ansx_ctx* c, QueryFront& F, const UnbGroup& g, const TopkOut& o, size_t* bad_container, size_t* bad_query, hipStream_t s)
{
    int rc;
    const size_t Q = g.q1 - g.q0, q1 = rup(Q + 1, 4);
    const u64 L = g.at.back(), M = g.seg[Q];
    if (M == 0) return ranked_nothing(c, Q, g.q0, o, s);  // (every list is empty: nothing is decoded)
    if ((rc = merge_tiles_check(g, bad_query))) return rc;
    ImpactTables IT;  // (ansx_topk_scored_batch_dev only: the lists whose payloads become impacts)
    if (o.scorer && (rc = impact_tables(c, g.lists, g.at, F.payof, g.q0, &IT, bad_query))) return rc;
    // the lists | their payloads | two key and two value merge buffers | the scores | the slots (u64: at an even int); each
    // with the decoders' slack behind
    const size_t o_c = rup((size_t)L, 4) + 16, half = rup((size_t)M, 4) + 16;
    const size_t o_m = (o.pays ? 2 : 1) * o_c, o_s = o_m + 5 * half;
    if ((rc = ensure(c, c->isectb_ids, 4 * o_s + 8 * Q * (size_t)o.k))) return rc;
    u32* ids = (u32*)c->isectb_ids.p;
    u32* pay = o.pays ? ids + o_c : nullptr;
    u32* const kb[2] = { ids + o_m, ids + o_m + half };
    u32* const vb[2] = { ids + o_m + 2 * half, ids + o_m + 3 * half };
    u32* score = ids + o_m + 4 * half;
    u64* slots = (u64*)(ids + o_s);
    if ((rc = group_decode(c, F, g.lists, g.at, ids, pay, bad_container, s))) return rc;

    // one upload: zero flag words (k_isect_compact's four, k_union_heads' one) | the overflow word | the queries' spans |
    // every round's pairs | their weights | with exclusions (ansx_topk_bool_batch_dev) the second table; behind it on the
    // device: the bounds among the heads | those behind the exclusion step | the select state | IsectWork
    Upload U;
    const auto s_fl = U.add<u32>(8);
    const auto s_of = U.add<u32>(4);
    const auto s_seg = U.add<u32>(Q + 1);
    const auto s_p = U.add<ansx_unb_pair>(g.pairs.size());
    const auto s_w = U.add<u32>(2 * g.pairs.size());
    const bool excl = !g.xt.empty();  // (ansx_topk_bool_batch_dev only: the group excludes something)
    const auto s_xo = U.add<u32>(excl ? Q + 1 : 0);
    const auto s_xt = U.add<ansx_isb_list>(g.xt.size());
    // (ansx_topk_query_batch_dev only: some query of the group asks for two entries or more -- the thresholds go up too)
    const bool least = o.msm && std::any_of(o.msm + g.q0, o.msm + g.q1, [](u32 m) { return m >= 2; });
    const auto s_m = U.add<u32>(least ? Q : 0);
    const auto s_ip = U.add<ansx_impact_list>(IT.P.size());
    // (ansx_topk_filter_batch_dev only: some query of the group has a clause -- the clause table goes up too)
    FilterTables FT;
    filter_tables(o, g.q0, Q, &FT);
    const bool filt = FT.active(), fused = filt && filter_fused(c, excl);
    const auto s_fo = U.add<u32>(FT.off.size());
    const auto s_fc = U.add<ansx_filter_dev>(FT.cl.size());
    const size_t up = U.end;
    const auto s_hs = U.add<u32>(q1);  // (the host's copy: read back)
    const auto s_xs = U.add<u32>(excl ? q1 : 0);
    const auto s_as = U.add<u32>(least ? q1 : 0);
    const auto s_fs = U.add<u32>(filt && !fused ? q1 : 0);
    const SelectSecs s_sel = select_sections(U, Q);
    GroupWs ws;
    if ((rc = group_room(c, U, s_hs.off + s_hs.bytes, M, s_fl, &s_of, &ws))) return rc;
    facet_word(o, U, s_of), filter_word(o, U, s_of);
    if (filt) U.put(s_fo, FT.off.data()), U.put(s_fc, FT.cl.data());
    U.put(s_seg, g.seg.data()), U.put(s_p, g.pairs.data());
    if (excl) U.put(s_xo, g.xt_off.data()), U.put(s_xt, g.xt.data());
    if (least) U.put(s_m, o.msm + g.q0);
    if (!IT.P.empty()) U.put(s_ip, IT.P.data());
    u32* hw = U.pin(s_w);
    for (size_t i = 0; i < g.pterm.size(); i++) hw[i] = g.pterm[i] == ANSX_TOPK_NONE ? 0u : o.weights[g.pterm[i]];
    if ((rc = group_upload(c, U, up, &s_sel, s))) return rc;
    const u32* zero = U.dev(s_fl);
    u32* uflag = U.dev(s_fl) + 4;
    const u32* seg = U.dev(s_seg);

    SumsPlan S;
    if ((rc = group_scan(c, ids, g.at, s, &S))) return rc;
    if (o.scorer && (rc = impact_step(c, *o.scorer, IT, U.dev(s_ip), ids, pay, S.flag, s))) return rc;
    for (u32 r = 0; r < g.rounds; r++) {
        const u32 np = g.roff[r + 1] - g.roff[r];
        if (np == 0) continue;  // (the queries that have this round are empty)
        const u32 to = r & 1u, from = 1 - to;
        LAUNCH(c, "k_topk_merge", k_topk_merge, (u32)g.tiles[r], ANSX_ISECT_NT, 0, s, (const u32*)ids, (const u32*)pay, (const u32*)kb[from],
            (const u32*)vb[from], kb[to], vb[to], (const ansx_unb_pair*)U.dev(s_p) + g.roff[r],
            (const u32*)U.dev(s_w) + 2 * (size_t)g.roff[r], np, (const u32*)S.flag);
    }
    // what the last round wrote, and the other pair of buffers: the heads' ids and positions go where it read
    const u32 fin = (g.rounds - 1u) & 1u;
    u32 *merged = kb[fin], *values = vb[fin], *heads = kb[1 - fin], *idx = vb[1 - fin];
    const IsectWork W(ws.work, M, false);
    if ((rc = unique_step(c, W, { merged, heads, idx }, (u32)M, seg, Q, S.flag, uflag, U.dev(s_hs), zero, s))) return rc;
    // (ansx_topk_bool_batch_dev: a score that leaves 32 bits may belong to an excluded id -- the scores' word is one that
    // nobody reads, and k_topkb_check lowers the real one over what the exclusion step leaves)
    LAUNCH(c, "k_topk_scores", k_topk_scores, W.ntiles, ANSX_ISECT_NT, 0, s, (const u32*)idx, (const u32*)values, (const u32*)U.dev(s_hs),
        seg, (u32)Q, (const u64*)W.total, (u32)M, score, U.dev(s_of) + (o.check ? 1 : 0), (const u32*)S.flag);
    Ranked R = { heads, score, U.dev(s_hs), W.total, (u32)M, W.ntiles };
    // (what a step compacts into: the merged ids and their values are through, and a second step writes where the first read)
    Flip hb = { { heads, merged } }, vs = { { score, values } };
    if (least) {  // ansx_topk_query_batch_dev: the threshold over the heads, the scores moved by the same ballots: no wait
        if ((rc = atleast_step(c, W, idx, { hb.from(), hb.to(), nullptr }, { vs.from(), vs.to(), nullptr }, (u32)M, R.hseg, seg, Q,
                 U.dev(s_m), S.flag, U.dev(s_as), zero, uflag, s)))
            return rc;
        hb.flip(), vs.flip();
        R.ids = hb.from(), R.score = vs.from(), R.hseg = U.dev(s_as);
    }
    if (fused) {  // ansx_topk_filter_batch_dev: the exclusion's launch, the filter's mark over its ballots, ONE compact step
        if ((rc = bool_exclude_launch(c, W, ids, hb.from(), (u32)M, W.total, R.hseg, Q, U.dev(s_xo), U.dev(s_xt), S.flag, s))) return rc;
        if ((rc = filter_mark<true>(c, W, hb.from(), (u32)M, W.total, R.hseg, Q, U.dev(s_fo), U.dev(s_fc), o, U.dev(s_of) + 3, S.flag, s)))
            return rc;
        if ((rc = compact_step(c, W, (u32)M, { hb.from(), hb.to(), nullptr }, nullptr, R.hseg, Q, U.dev(s_xs), zero, uflag, s))) return rc;
    } else if (excl) {  // ONE exclusion step over the heads, as in unb_group, and the scores moved by the same ballots: no wait
        if ((rc = bool_exclude_step(c, W, ids, { hb.from(), hb.to(), nullptr }, (u32)M, W.total, R.hseg, Q, U.dev(s_xo), U.dev(s_xt), S.flag,
                 U.dev(s_xs), zero, uflag, s)))
            return rc;
    }
    if (excl) {
        if ((rc = isect_move(c, W, vs.from(), (u32)M, { vs.to(), nullptr, nullptr, M }, zero, uflag, s))) return rc;
        hb.flip(), vs.flip();
        R.ids = hb.from(), R.score = vs.from(), R.hseg = U.dev(s_xs);
    }
    if (filt && !fused) {  // ansx_topk_filter_batch_dev, the own form: the mark and a compact step of its own: no wait
        if ((rc = filter_step(c, W, { hb.from(), hb.to(), nullptr }, { vs.from(), vs.to(), nullptr }, (u32)M, W.total, R.hseg, Q, U.dev(s_fo),
                 U.dev(s_fc), o, U.dev(s_of) + 3, S.flag, U.dev(s_fs), zero, uflag, s)))
            return rc;
        hb.flip(), vs.flip();
        R.ids = hb.from(), R.score = vs.from(), R.hseg = U.dev(s_fs);
    }
    if (o.facets && (rc = facet_step(c, R, Q, g.q0, o, U.dev(s_of) + 2, S.flag, s))) return rc;
    if ((rc = ranked_tail(c, R, Q, g.q0, o, U, s_sel, slots, s_of, s_hs, S.flag, ws.sflag, s, filt))) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = scan_flag_status(ws, g.lists, *F.index, bad_container))) return rc;
    return ranked_counts(U.pin(s_of), U.pin(s_hs), Q, g.q0, o, bad_query);
}

// ansx_topk_bool_batch_dev (ansx_topk_bool.h).  The front end of ansx_topk_batch_dev over the terms
// followed by the excluded terms: the id containers of every referenced list and, behind each list some query names as
// a term, its payload -- a list that is only excluded has none -- still one round trip for the headers.  Then the plan
// of the chosen op with the excluded lists under HALF the budget: ANY runs topk_group, which adds the exclusion step and
// k_topkb_check between k_topk_scores and the select; ALL runs topkb_group: ids and payloads decoded with the same
// offsets, the scan, one upload of the tables with the weights beside them, k_isectb_gather, then per round
// k_topkb_match and the compact step over the ids and the scores -- at least one round, which seeds the scores and drops
// a driver's repeats -- the exclusion step where the group excludes something, and the ranked tail.
// Workspace (ALL): 4 (8 with payloads) bytes per int of the group's lists, 16 per int of its drivers (two candidate and
// two score buffers), a pass's, the scan's, IsectWork over the candidates, and per query 8 k bytes of slots, 1 KiB of
// histogram, 60 bytes of tables, state and bounds, 20 per non-driver term and 16 per excluded term.
// Host waits (ALL): one for the headers; per group those of its decode passes (ids, then payloads), ONE for the scan's
// flag word, ONE per round, which brings the members' count, and ONE behind the sort, which brings the overflow word and
// the bounds; one per call at the end.  The exclusion step adds none: its count stays on the device, and the select's
// grids cover the last count the host has seen.
int topkb_group(ansx_ctx* c, QueryFront& F, const IsbGroup& g, const TopkOut& o, size_t* bad_container, size_t* bad_query, hipStream_t s)
{
    int rc;
    const size_t Q = g.q1 - g.q0, q1 = rup(Q + 1, 4);
    const u64 L = g.at.back(), nc0 = g.G[Q].dst;
    if (nc0 == 0) return ranked_nothing(c, Q, g.q0, o, s);  // (every driver is empty: nothing is decoded)
    ImpactTables IT;  // (ansx_topk_scored_batch_dev only: the lists whose payloads become impacts)
    if (o.scorer && (rc = impact_tables(c, g.lists, g.at, F.payof, g.q0, &IT, bad_query))) return rc;
    // the lists | their payloads | two candidate and two score buffers | the slots (u64: at an even int); each with the
    // decoders' slack behind
    const size_t o_c = rup((size_t)L, 4) + 16, half = rup((size_t)nc0, 4) + 16;
    const size_t o_m = (o.pays ? 2 : 1) * o_c, o_s = o_m + 4 * half;
    if ((rc = ensure(c, c->isectb_ids, 4 * o_s + 8 * Q * (size_t)o.k))) return rc;
    u32* ids = (u32*)c->isectb_ids.p;
    u32* pay = o.pays ? ids + o_c : nullptr;
    Flip buf = { { ids + o_m, ids + o_m + half } };
    Flip sb = { { ids + o_m + 2 * half, ids + o_m + 3 * half } };
    u64* slots = (u64*)(ids + o_s);
    if ((rc = group_decode(c, F, g.lists, g.at, ids, pay, bad_container, s))) return rc;

    // one upload: zero flag words | the overflow word | queries | their drivers' weights | round table | its weights | with
    // exclusions the second table; behind it on the device: two arrays of segments | the select state | IsectWork
    Upload U;
    const auto s_fl = U.add<u32>(4);
    const auto s_of = U.add<u32>(4);
    const auto s_g = U.add<ansx_isb_query>(Q + 1);
    const auto s_wd = U.add<u32>(Q);
    const auto s_ro = U.add<u32>(Q + 1);
    const auto s_rt = U.add<ansx_isb_list>(g.rt.size());
    const auto s_rw = U.add<u32>(g.rt.size());
    const bool excl = !g.xt.empty();
    const auto s_xo = U.add<u32>(excl ? Q + 1 : 0);
    const auto s_xt = U.add<ansx_isb_list>(g.xt.size());
    // (ansx_topk_query_batch_dev only: the group has an optional term or a threshold -- a third table, its weights and the
    // thresholds go up too)
    const bool should = o.msm && (!g.ot.empty() || std::any_of(o.msm + g.q0, o.msm + g.q1, [](u32 m) { return m != 0; }));
    const auto s_oo = U.add<u32>(should ? Q + 1 : 0);
    const auto s_ot = U.add<ansx_isb_list>(should ? g.ot.size() : 0);
    const auto s_ow = U.add<u32>(should ? g.ot.size() : 0);
    const auto s_m = U.add<u32>(should ? Q : 0);
    const auto s_ip = U.add<ansx_impact_list>(IT.P.size());
    // (ansx_topk_filter_batch_dev only: some query of the group has a clause -- the clause table goes up too)
    FilterTables FT;
    filter_tables(o, g.q0, Q, &FT);
    const bool filt = FT.active(), fused = filt && filter_fused(c, excl);
    const auto s_fo = U.add<u32>(FT.off.size());
    const auto s_fc = U.add<ansx_filter_dev>(FT.cl.size());
    const size_t up = U.end;
    const auto s_seg = U.add<u32>(2 * q1);  // (the host's copy: the last step's, read back)
    const SelectSecs s_sel = select_sections(U, Q);
    GroupWs ws;
    if ((rc = group_room(c, U, s_seg.off + s_seg.bytes, nc0, s_fl, &s_of, &ws))) return rc;
    facet_word(o, U, s_of), filter_word(o, U, s_of);
    if (filt) U.put(s_fo, FT.off.data()), U.put(s_fc, FT.cl.data());
    U.put(s_g, g.G.data()), U.put(s_ro, g.rt_off.data());
    if (!g.rt.empty()) U.put(s_rt, g.rt.data());
    for (size_t j = 0; j < Q; j++) U.pin(s_wd)[j] = o.weights[g.dterm[j]];
    for (size_t e = 0; e < g.rterm.size(); e++) U.pin(s_rw)[e] = o.weights[g.rterm[e]];
    if (excl) U.put(s_xo, g.xt_off.data()), U.put(s_xt, g.xt.data());
    if (should) {
        U.put(s_oo, g.ot_off.data()), U.put(s_m, o.msm + g.q0);
        if (!g.ot.empty()) U.put(s_ot, g.ot.data());
        for (size_t e = 0; e < g.oterm.size(); e++) U.pin(s_ow)[e] = o.oweights[g.oterm[e]];
    }
    if (!IT.P.empty()) U.put(s_ip, IT.P.data());
    if ((rc = group_upload(c, U, up, &s_sel, s))) return rc;
    Flip seg = { { U.dev(s_seg), U.dev(s_seg) + q1 } };
    const u32* zero = U.dev(s_fl);

    SumsPlan S;
    if ((rc = group_scan(c, ids, g.at, s, &S))) return rc;
    if (o.scorer && (rc = impact_step(c, *o.scorer, IT, U.dev(s_ip), ids, pay, S.flag, s))) return rc;
    if ((rc = gather_drivers(c, ids, U.dev(s_g), Q, nc0, buf.from(), seg.from(), S.flag, s))) return rc;
    HIPCHK(c, hipMemcpyAsync(ws.sflag, S.flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = scan_flag_status(ws, g.lists, *F.index, bad_container))) return rc;

    // (at least one round: the first seeds the scores and drops the repeats of a driver, whatever the queries' terms)
    const u32 rounds = std::max<u32>(g.rounds, 1u);
    u32 nc = (u32)nc0;
    for (u32 r = 0; r < rounds && nc > 0; r++) {
        const IsectWork W(ws.work, nc, false);
        const Moved scores = { sb.from(), sb.to(), nullptr };
        LAUNCH(c, "k_topkb_match", k_topkb_match, W.ntiles, ANSX_ISECT_NT, 0, s, (const u32*)ids, (const u32*)pay, (const u32*)buf.from(),
            sb.from(), nc, (const u32*)seg.from(), (u32)Q, (const ansx_isb_query*)U.dev(s_g), (const u32*)U.dev(s_wd),
            (const u32*)U.dev(s_ro), (const ansx_isb_list*)U.dev(s_rt), (const u32*)U.dev(s_rw), r, o.form, W.ballots, W.counts);
        if ((rc = compact_step(c, W, nc, { buf.from(), buf.to(), nullptr }, &scores, seg.from(), Q, seg.to(), zero, zero, s))) return rc;
        HIPCHK(c, hipMemcpyAsync(ws.total, W.total, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        nc = (u32)*ws.total, buf.flip(), sb.flip(), seg.flip();
    }
    if (nc == 0) return ranked_nothing(c, Q, g.q0, o, s);  // (a round left nothing: no id is in all lists of any query)
    const IsectWork W(ws.work, nc, false);  // (total: the last round's, nc, at the same place)
    if (should) {  // ansx_topk_query_batch_dev: ONE optional step over what the rounds left, whatever the optional lists: no wait
        const ShouldTables T = { U.dev(s_oo), U.dev(s_ot), U.dev(s_ow), U.dev(s_m), o.qform };
        if ((rc = should_step(c, W, ids, pay, { buf.from(), buf.to(), nullptr }, { sb.from(), sb.to(), nullptr }, nc, nullptr, seg.from(), Q,
                 T, S.flag, seg.to(), zero, zero, s)))
            return rc;
        buf.flip(), sb.flip(), seg.flip();
    }
    if (fused) {  // ansx_topk_filter_batch_dev: the exclusion's launch, the filter's mark over its ballots, ONE compact step
        const u64* tot = should ? W.total : nullptr;
        if ((rc = bool_exclude_launch(c, W, ids, buf.from(), nc, tot, seg.from(), Q, U.dev(s_xo), U.dev(s_xt), S.flag, s))) return rc;
        if ((rc = filter_mark<true>(c, W, buf.from(), nc, tot, seg.from(), Q, U.dev(s_fo), U.dev(s_fc), o, U.dev(s_of) + 3, S.flag, s)))
            return rc;
        if ((rc = compact_step(c, W, nc, { buf.from(), buf.to(), nullptr }, nullptr, seg.from(), Q, seg.to(), zero, zero, s))) return rc;
    } else if (excl) {  // ONE exclusion step over what the rounds left (behind an optional step, their count is the device's), the
                        // scores moved by the same ballots: no wait
        if ((rc = bool_exclude_step(c, W, ids, { buf.from(), buf.to(), nullptr }, nc, should ? W.total : nullptr, seg.from(), Q, U.dev(s_xo), U.dev(s_xt),
                 S.flag, seg.to(), zero, zero, s)))
            return rc;
    }
    if (excl) {
        if ((rc = isect_move(c, W, sb.from(), nc, { sb.to(), nullptr, nullptr, nc }, zero, zero, s))) return rc;
        buf.flip(), sb.flip(), seg.flip();
    }
    if (filt && !fused) {  // ansx_topk_filter_batch_dev, the own form: the mark and a compact step of its own: no wait
        if ((rc = filter_step(c, W, { buf.from(), buf.to(), nullptr }, { sb.from(), sb.to(), nullptr }, nc, W.total, seg.from(), Q,
                 U.dev(s_fo), U.dev(s_fc), o, U.dev(s_of) + 3, S.flag, seg.to(), zero, zero, s)))
            return rc;
        buf.flip(), sb.flip(), seg.flip();
    }
    const Ranked R = { buf.from(), sb.from(), seg.from(), W.total, nc, W.ntiles };
    if (o.facets && (rc = facet_step(c, R, Q, g.q0, o, U.dev(s_of) + 2, S.flag, s))) return rc;
    if ((rc = ranked_tail(c, R, Q, g.q0, o, U, s_sel, slots, s_of, s_seg, S.flag, nullptr, s, filt))) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    return ranked_counts(U.pin(s_of), U.pin(s_seg), Q, g.q0, o, bad_query);
}

// The two ranked calls: ansx_topk_bool_batch_dev and, as its case ANY with nothing excluded and no check,
// ansx_topk_batch_dev (`check`: the overflow word is k_topkb_check's, not k_topk_scores').
int topk_bool_batch(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, const u8* const* d_pays,
    const size_t* pay_bytes, size_t count, int op, bool check, const u32* terms, const u32* weights, const u64* qoff, const u32* xterms,
    const u64* xqoff, size_t nq, u32 k, u32* d_out_ids, u32* d_out_scores, u32* out_counts, size_t* bad_container, size_t* bad_query,
    hipStream_t s)
{
    int rc;
    QueryFront F;
    if ((rc = query_front(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, terms, (size_t)qoff[nq], xterms,
             xqoff ? (size_t)xqoff[nq] : 0, &F, bad_container, s)))
        return rc;
    const u64 budget = query_budget(c, true);
    u32 pow2 = 1;
    while (pow2 < k) pow2 <<= 1;
    const TopkOut o = { weights, k, pow2, d_out_ids, d_out_scores, out_counts, d_pays != nullptr, check,
        c->dbg.topk_bool_form == 1 ? ANSX_TOPKB_FORM_SEARCH : ANSX_TOPKB_FORM_DEFAULT };
    if (op == ANSX_BOOL_ALL) {
        std::vector<IsbGroup> groups;
        if ((rc = isb_plan(F.n.data(), F.n.size(), F.rid, qoff, nq, budget, &groups, bad_query, F.xrid, xqoff, true))) return rc;
        return run_groups(c, groups, [&](const IsbGroup& g) { return topkb_group(c, F, g, o, bad_container, bad_query, s); }, s);
    }
    std::vector<UnbGroup> groups;
    if ((rc = unb_plan(F.n.data(), F.n.size(), F.rid, qoff, nq, budget, ANSX_UNION_TILE, &groups, bad_query, F.xrid, xqoff, true)))
        return rc;
    return run_groups(c, groups, [&](const UnbGroup& g) { return topk_group(c, F, g, o, bad_container, bad_query, s); }, s);
}

// ansx_topk_query_batch_dev (ansx_topk_query.h).  The front end of ansx_topk_bool_batch_dev over
// ALL terms, required and optional, followed by the excluded terms; query_plan (ansx_plan.h, host-only): the terms split
// by occur, the batch cut into runs of one kind, every run planned by its kind's planner under HALF the budget with its
// query numbers offset -- ALL runs are planned before anything is launched -- and the runs' groups in batch order:
//   kind R  topkb_group over the REQUIRED terms (isb_plan with the optional terms as orid / oqoff: their lists are
//           decoded with the group's): the rounds as they are, then should_step where the group has an optional term or
//           a threshold, then the exclusion step, which takes the device's count behind it, and the ranked tail;
//   kind O  topk_group over the terms: up to k_topk_scores as it is, then atleast_step where some query asks for two
//           entries or more, the exclusion step and the ranked tail.
// Neither step adds a host wait: the waits per group are topkb_group's and topk_group's.  Workspace: topkb_group's with
// the optional lists among the group's, plus per query 4 bytes of threshold and 4 of table offset and per optional term
// 16 of table and 4 of weight; topk_group's, plus 8 bytes per query (threshold and bounds) where the threshold step runs.
// ansx_topk_scored_batch_dev (ansx_topk_scored.h) is the same call with a scorer: the same front,
// plan, runs and groups, and in every group that decodes something impact_step behind the scan -- one launch, no wait, 24
// bytes of table per list with a payload.  scorer null: ansx_topk_query_batch_dev, launch for launch.
// ansx_topk_facets_batch_dev (ansx_facet.h) is that call with facets and / or totals: the counts
// zeroed once behind the plan, and in every group that reaches its ranked tail facet_step in front of it -- one launch, no
// wait, no upload; the totals come from the bounds the tail's wait brings home.  Both null: the scored call, launch for launch.
// ansx_topk_filter_batch_dev (ansx_filter.h) is that call with filters: in every group in which some
// query has a clause the filter step in front of facet_step -- fused into the exclusion step (one launch) or on its own
// (five), no wait, the clause table in the group's upload.  filters null: the facets call, launch for launch.
int topk_scored_batch(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, const u8* const* d_pays,
    const size_t* pay_bytes, size_t count, const u32* terms, const u32* weights, const u8* occur, const u64* qoff, const u32* msm,
    const u32* xterms, const u64* xqoff, const ansx_scorer* scorer, const ansx_facets* facets, size_t nq, u32 k, u32* d_out_ids,
    u32* d_out_scores, u32* out_counts, u32* out_totals, size_t* bad_container, size_t* bad_query, hipStream_t s,
    const ansx_filters* filters = nullptr)
{
    int rc;
    QueryFront F;
    if ((rc = query_front(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, terms, (size_t)qoff[nq], xterms,
             xqoff ? (size_t)xqoff[nq] : 0, &F, bad_container, s)))
        return rc;
    const u64 budget = query_budget(c, true);
    u32 pow2 = 1;
    while (pow2 < k) pow2 <<= 1;
    // the whole plan before anything is launched: a limit names the first query in batch order, whatever its kind
    QueryPlan Q;
    if ((rc = query_plan(F.n.data(), F.n.size(), F.rid, occur, qoff, msm, F.xrid, xqoff, nq, budget, ANSX_UNION_TILE, &Q, bad_query)))
        return rc;
    const QuerySplit& P = Q.split;
    std::vector<u32> rw(P.rpos.size()), ow(P.opos.size());  // the weights beside the split terms
    for (size_t i = 0; i < rw.size(); i++) rw[i] = weights[P.rpos[i]];
    for (size_t i = 0; i < ow.size(); i++) ow[i] = weights[P.opos[i]];
    TopkOut o = { weights, k, pow2, d_out_ids, d_out_scores, out_counts, d_pays != nullptr, true,
        c->dbg.topk_bool_form == 1 ? ANSX_TOPKB_FORM_SEARCH : ANSX_TOPKB_FORM_DEFAULT };
    o.msm = P.m.data(), o.oweights = ow.data(), o.qform = (u32)c->dbg.topk_query_form;
    o.scorer = scorer, o.facets = facets, o.totals = out_totals, o.filters = filters;
    if (facets) HIPCHK(c, hipMemsetAsync(facets->d_counts, 0, 4 * nq * (size_t)facets->nvalues, s));
    TopkOut oreq = o;  // (a group of kind R reads its drivers' and rounds' weights at the required terms' places)
    oreq.weights = rw.data();
    for (const QueryPlan::Run& run : Q.plans) {
        for (const IsbGroup& g : run.req)
            if ((rc = topkb_group(c, F, g, oreq, bad_container, bad_query, s))) return rc;
        for (const UnbGroup& g : run.opt)
            if ((rc = topk_group(c, F, g, o, bad_container, bad_query, s))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(s));
    return ANSX_OK;
}
int topk_query_batch(ansx_ctx* c, int kind, int f, const u8* const* d_ins, const size_t* in_bytes, const u8* const* d_pays,
    const size_t* pay_bytes, size_t count, const u32* terms, const u32* weights, const u8* occur, const u64* qoff, const u32* msm,
    const u32* xterms, const u64* xqoff, size_t nq, u32 k, u32* d_out_ids, u32* d_out_scores, u32* out_counts, size_t* bad_container,
    size_t* bad_query, hipStream_t s)
{
    return topk_scored_batch(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, qoff, msm, xterms, xqoff, nullptr,
        nullptr, nq, k, d_out_ids, d_out_scores, out_counts, nullptr, bad_container, bad_query, s);
}

// The argument checks of the random-access entry points, one per argument shape: everything a call decides before the
// context is touched.  The plain and the sums entry of a shape share them; what a sums or search entry adds (bases,
// targets, outputs) it checks itself.
// ... a container and ranges in host arrays
int ranges_args(const ansx_ctx* c, const uint8_t* d_in, const uint32_t* d_out, const uint64_t* first, const uint32_t* count,
    size_t nranges)
{
    if (!c || !d_in || !d_out) return ANSX_ERR_ARG;
    if (nranges > 0 && (!first || !count)) return ANSX_ERR_ARG;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 3u)) return ANSX_ERR_ARG;
    return ANSX_OK;
}

// ... a batch and queries over it (ansx_intersect_batch_dev; ansx_union_batch_dev, which has the optional d_out_cnt)
int queries_args(const ansx_ctx* c, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count, const uint32_t* terms,
    const uint64_t* qoff, size_t nqueries, const uint32_t* d_out_ids, const uint32_t* d_out_cnt, size_t out_capacity,
    const uint64_t* out_offsets, size_t* bad_container, size_t* bad_query)
{
    if (!c) return ANSX_ERR_ARG;
    if (nqueries > 0 && (!d_ins || !in_bytes || !terms || !qoff || !out_offsets)) return ANSX_ERR_ARG;
    if ((!d_out_ids && out_capacity > 0) || ((uintptr_t)d_out_ids & 3u)) return ANSX_ERR_ARG;
    if ((d_out_cnt && !d_out_ids) || ((uintptr_t)d_out_cnt & 3u)) return ANSX_ERR_ARG;
    if (count > 0xFFFFFFFFull || nqueries > 0xFFFFFFFFull || (nqueries > 0 && qoff[nqueries] > 0xFFFFFFFFull)) return ANSX_ERR_ARG;
    for (size_t q = 0; q < nqueries; q++)
        if ((q == 0 && qoff[0] != 0) || qoff[q + 1] <= qoff[q]) {  // (an empty query has no list)
            if (bad_query) *bad_query = q;
            return ANSX_ERR_ARG;
        }
    for (size_t q = 0; q < nqueries; q++)
        for (u64 j = qoff[q]; j < qoff[q + 1]; j++)
            if (terms[j] >= count) {
                if (bad_query) *bad_query = q;
                return ANSX_ERR_ARG;
            }
    for (size_t q = 0; q < nqueries; q++)  // (only the containers some query names are looked at)
        for (u64 j = qoff[q]; j < qoff[q + 1]; j++)
            if (!d_ins[terms[j]] || ((uintptr_t)d_ins[terms[j]] & 15u)) {
                if (bad_query) *bad_query = q;
                if (bad_container) *bad_container = terms[j];
                return ANSX_ERR_ARG;
            }
    return ANSX_OK;
}

// ... a container and ranges in device arrays
int device_ranges_args(const ansx_ctx* c, const uint8_t* d_in, const uint32_t* d_out, const uint64_t* d_first,
    const uint32_t* d_count, size_t nranges, const uint64_t* d_offsets)
{
    if (ranges_args(c, d_in, d_out, d_first, d_count, nranges)) return ANSX_ERR_ARG;
    if (((uintptr_t)d_first & 7u) || ((uintptr_t)d_count & 3u) || ((uintptr_t)d_offsets & 7u)) return ANSX_ERR_ARG;
    return nranges > 0xFFFFFFFFull ? ANSX_ERR_ARG : ANSX_OK;
}

// ... a batch and src[0..n), the container every range or target names; with_bases: every named container's bases too.
// *bad: the first range or target that names no container of the batch, else the first whose container (or bases) is
// null or misaligned -- only the containers some range names are looked at.
int batch_src_args(const ansx_ctx* c, const uint8_t* const* d_ins, const size_t* in_bytes, bool with_bases,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* src, size_t n, size_t* bad)
{
    if (!c || count > 0xFFFFFFFFull || n > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (n > 0 && (!src || !d_ins || !in_bytes || (with_bases && (!d_bases || !nbases)))) return ANSX_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (src[i] >= count) {
            if (bad) *bad = i;
            return ANSX_ERR_ARG;
        }
    for (size_t i = 0; i < n; i++)
        if (!d_ins[src[i]] || ((uintptr_t)d_ins[src[i]] & 15u)
            || (with_bases && (!d_bases[src[i]] || ((uintptr_t)d_bases[src[i]] & 3u)))) {
            if (bad) *bad = i;
            return ANSX_ERR_ARG;
        }
    return ANSX_OK;
}

// What every entry point of the family does behind its checks: the device, the stream, and the body run where the
// host's arrays of a huge query or batch may not fit
template <class F> int run_call(ansx_ctx* c, void* stream, const F& body)
{
    HIPCHK(c, hipSetDevice(c->device));
    try {
        return body(stream ? (hipStream_t)stream : c->stream);
    } catch (const std::bad_alloc&) {
        c->last_hip = (int)hipErrorOutOfMemory;
        return ANSX_ERR_HIP;
    }
}

// the call of a batch entry with nothing to do (T: the entry's type of a total)
template <class T> int empty_batch(uint64_t* offsets, T* total)
{
    if (offsets) offsets[0] = 0;
    if (total) *total = 0;
    return ANSX_OK;
}

// ... a batch (ansx_decode_batch_dev, ansx_decode_batch_sums_dev)
int decode_batch_args(const ansx_ctx* c, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count, const uint32_t* d_out,
    size_t out_capacity_ints)
{
    if (!c || count > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (count > 0 && (!d_ins || !in_bytes)) return ANSX_ERR_ARG;
    if ((!d_out && out_capacity_ints > 0) || ((uintptr_t)d_out & 3u)) return ANSX_ERR_ARG;
    for (size_t i = 0; i < count; i++)
        if (!d_ins[i] || ((uintptr_t)d_ins[i] & 15u)) return ANSX_ERR_ARG;
    return ANSX_OK;
}

// ... those of the single-list encode entries (ansx_encode_dev and the two gaps variants), with the list's plan
int encode_args(const ansx_ctx* c, int kind, int f, const uint32_t* d_in, size_t n, const uint8_t* d_out, const size_t* out_bytes,
    const ansx_opts* opts, Plan* P)
{
    if (!c || !d_in || !d_out || !out_bytes) return ANSX_ERR_ARG;
    if (((uintptr_t)d_out & 15u) || ((uintptr_t)d_in & 3u)) return ANSX_ERR_ARG;
    return make_plan(kind, f, n, opts, P);
}

// ... and those of the batch encode entries (ansx_encode_batch_dev and the two gaps variants)
int encode_batch_args(const ansx_ctx* c, int kind, int f, const uint32_t* d_in, const uint64_t* offsets, size_t count,
    const uint8_t* d_out, size_t* bad_index, const ansx_opts* opts, Plan* P0)
{
    if (!c || count > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (count > 0 && (!d_in || !offsets || !d_out)) return ANSX_ERR_ARG;
    if (((uintptr_t)d_out & 15u) || ((uintptr_t)d_in & 3u)) return ANSX_ERR_ARG;
    if (opts && opts->block_ints == ANSX_SINGLE_STREAM) return ANSX_ERR_ARG;  // (a batch yields containers)
    int rc = make_plan(kind, f, 1, opts, P0);  // kind, fidelity and options, as for any list
    if (rc) return rc;
    for (size_t i = 0; i < count; i++) {
        Plan P;
        if (offsets[i + 1] < offsets[i]) return ANSX_ERR_ARG;
        if (offsets[i + 1] == offsets[i] || make_plan(kind, f, (size_t)(offsets[i + 1] - offsets[i]), opts, &P)) {
            if (bad_index) *bad_index = i;  // an empty list (or one no container can hold), as ansx_encode_dev refuses n == 0
            return ANSX_ERR_ARG;
        }
    }
    return ANSX_OK;
}

}  // namespace

namespace {
struct RcclApi {
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;  // optional: only reported (ansx_last_gather_ranks)
    bool ok = false;
};
const RcclApi& rccl_api()
{
    static RcclApi api = [] {
        RcclApi a;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return a;
        a.AllGather = (decltype(a.AllGather))dlsym(h, "ncclAllGather");
        a.GroupStart = (decltype(a.GroupStart))dlsym(h, "ncclGroupStart");
        a.GroupEnd = (decltype(a.GroupEnd))dlsym(h, "ncclGroupEnd");
        a.Send = (decltype(a.Send))dlsym(h, "ncclSend");
        a.Recv = (decltype(a.Recv))dlsym(h, "ncclRecv");
        a.CommCount = (decltype(a.CommCount))dlsym(h, "ncclCommCount");
        a.ok = a.AllGather && a.GroupStart && a.GroupEnd && a.Send && a.Recv;
        return a;
    }();
    return api;
}
}  // namespace

// ================================================================================= C ABI
extern "C" {

int ansx_init(int device, ansx_ctx** out)
{
    if (!out) return ANSX_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return ANSX_ERR_NO_DEVICE;
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) return ANSX_ERR_NO_DEVICE;
    }
    if (device >= ndev) return ANSX_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return ANSX_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ANSX_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ANSX_ERR_NO_DEVICE;  // gfx950-only code object
    ansx_ctx* c = new ansx_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount > 0 ? (u32)prop.multiProcessorCount : 256u;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess) {
        delete c;
        return ANSX_ERR_HIP;
    }
    if (hipHostMalloc((void**)&c->pin, sizeof(PinPage), hipHostMallocDefault) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return ANSX_ERR_HIP;
    }
    static const char* const names[] = { "ANSX_TEST_TABLE16_FIXUP", "ANSX_ENCODE_GTAB16", "ANSX_PARSE_GENERIC", "ANSX_PARSE_WIN", "ANSX_PARSE_FAST",
        "ANSX_DECODE_TABLE", "ANSX_NO_STREAM_LDS", "ANSX_DECODE_MODE", "ANSX_PARSE_STAGE_WORDS", "ANSX_MODEL_FUSED", "ANSX_MODEL_SYNC", "ANSX_NS_HINT", "ANSX_T_HINT", "ANSX_NO_FAST_MODEL", "ANSX_FAST_GUARD", "ANSX_CAND_CHAINS", "ANSX_NEAR_BAND", "ANSX_TEST_NEAR_FLIP", "ANSX_WIDE_RESTART", "ANSX_TEST_WIDE_AT",
        "ANSX_BATCH_PASS_BLOCKS", "ANSX_MODEL_PIPELINE", "ANSX_DECODE_SETUP", "ANSX_MODEL_CHAIN", "ANSX_INTERSECT_FORM", "ANSX_ISECT_BATCH_INTS", "ANSX_BOOL_FORM" };
    for (const char* nm : names)
        if (const char* v = getenv(nm))
            if (ansx_debug_set(c, nm, v) != ANSX_OK)  // (a value the key does not take selects nothing: said, not passed over)
                fprintf(stderr, "ansx_init: %s=\"%s\" is not a value of that key, ignored\n", nm, v);
    *out = c;
    return ANSX_OK;
}

int ansx_last_encode_stats(const ansx_ctx* c, ansx_encode_stats* out)
{
    if (!c || !out) return ANSX_ERR_ARG;
    *out = c->last;
#ifdef ANSX_STAMPS
    {
        static unsigned long long h[16 * 256 + 16];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_stamps), sizeof(h)) == hipSuccess) {
            double acc[16] = {};
            int nn = 0;
#ifdef ANSX_STAMPS_RF
            const int last = 8;
#else
            const int last = 10;
#endif
            for (int w = 0; w < 256; w++) {
                if (!h[w * 16] || !h[w * 16 + last]) continue;
                nn++;
                for (int i = 1; i <= last; i++) acc[i] += (double)(h[w * 16 + i] - h[w * 16 + i - 1]);
            }
            fprintf(stderr, "[stamps] %d workgroups, 100 MHz ticks per phase:", nn);
            for (int i = 1; i <= 10; i++) fprintf(stderr, " %d:%.0f", i, nn ? acc[i] / nn : 0.0);
#ifdef ANSX_STAMPS_RF
            { double a9 = 0, a10 = 0, a2 = 0; int m = 0; for (int w = 0; w < 256; w++) if (h[w*16+9] && h[w*16+10] && h[w*16+1]) { a9 += (double)(h[w*16+9]-h[w*16+1]); a10 += (double)(h[w*16+10]-h[w*16+9]); a2 += (double)(h[w*16+2]-h[w*16+10]); m++; }
              if (m) fprintf(stderr, "  [insert split: clear %.0f count %.0f merge %.0f]", a9/m, a10/m, a2/m); }
#endif
            fprintf(stderr, "\n");
#ifdef ANSX_STAMPS_RF
            {
                unsigned long long t0 = ~0ull, t1 = 0;
                for (int w = 0; w < 256; w++) if (h[w * 16] && h[w * 16 + 8]) { t0 = std::min(t0, h[w * 16]); t1 = std::max(t1, h[w * 16 + 8]); }
                fprintf(stderr, "[stamps] rfold: first start .. last end = %llu ticks\n", t1 - t0);
                for (int w = 0; w < 256; w += 8)
                    fprintf(stderr, "[stamps]  wg %5d start %7llu dur %5llu xcc %llx\n", w * 61 + 7, h[w * 16] - t0, h[w * 16 + 8] - h[w * 16], h[w * 16 + 9]);
            }
#endif
            double cc = 0, cl = 0, ct = 0;
            int n2 = 0;
            for (int w = 0; w < 256; w++)
                if (h[w * 16 + 14]) cc += (double)h[w * 16 + 12], cl += (double)h[w * 16 + 13], ct += (double)h[w * 16 + 14], n2++;
            if (n2) fprintf(stderr, "[stamps] k_candidates (%d waves): commit %.0f loop %.0f total %.0f ticks\n", n2, cc / n2, cl / n2, ct / n2);
        }
    }
#endif
    return ANSX_OK;
}

int ansx_last_encode_form(const ansx_ctx* c, ansx_encode_form_report* out)
{
    if (!c || !out) return ANSX_ERR_ARG;
    *out = c->last_form;
    return ANSX_OK;
}

int ansx_last_decode_stats(const ansx_ctx* c, ansx_decode_stats* out)
{
    if (!c || !out) return ANSX_ERR_ARG;
    *out = c->last_dec;
    return ANSX_OK;
}

// a key that takes one of two words: 0 for ""/"0"/NULL, 1 / 2 for the words, -1 for anything else
static int debug_word(const char* value, const char* one, const char* two)
{
    if (!value || !value[0] || !strcmp(value, "0")) return 0;
    return !strcmp(value, one) ? 1 : !strcmp(value, two) ? 2 : -1;
}

int ansx_debug_set(ansx_ctx* c, const char* name, const char* value)
{
    if (!c || !name) return ANSX_ERR_ARG;
    const bool on = value != nullptr && value[0] != 0 && strcmp(value, "0") != 0;
    if (!strcmp(name, "ANSX_TEST_TABLE16_FIXUP")) c->dbg.table16_fixup = on;
    else if (!strcmp(name, "ANSX_ENCODE_GTAB16")) c->dbg.encode_gtab16 = on;
    else if (!strcmp(name, "ANSX_PARSE_GENERIC")) c->dbg.parse_generic = on;
    else if (!strcmp(name, "ANSX_PARSE_WIN")) c->dbg.parse_win = on;
    else if (!strcmp(name, "ANSX_PARSE_FAST")) c->dbg.parse_fast = on;
    else if (!strcmp(name, "ANSX_DECODE_TABLE")) c->dbg.decode_table = on;
    else if (!strcmp(name, "ANSX_NO_STREAM_LDS")) c->dbg.no_stream_lds = on;
    else if (!strcmp(name, "ANSX_MODEL_FUSED")) c->dbg.model_fused = on;
    else if (!strcmp(name, "ANSX_MODEL_SYNC")) c->dbg.model_sync = on;
    else if (!strcmp(name, "ANSX_DECODE_MODE")) {
        const int w = debug_word(value, "ring", "staged");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.decode_mode = w;
    }
    else if (!strcmp(name, "ANSX_PARSE_STAGE_WORDS")) c->dbg.parse_stage_words = value ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_NS_HINT")) c->dbg.ns_hint = value ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_T_HINT")) c->dbg.t_hint = value ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_NO_FAST_MODEL")) c->dbg.no_fast_model = on;
    else if (!strcmp(name, "ANSX_WIDE_RESTART")) c->dbg.wide_restart = on;
    else if (!strcmp(name, "ANSX_NO_PC")) c->dbg.no_pc = on;
    else if (!strcmp(name, "ANSX_FORCE_PC")) c->dbg.force_pc = on;
    else if (!strcmp(name, "ANSX_USE_PC")) c->dbg.use_pc = on;
    else if (!strcmp(name, "ANSX_NO_PC_AUTO")) c->dbg.no_pc_auto = on;
    else if (!strcmp(name, "ANSX_NO_BIG_GEO")) c->dbg.no_big_geo = on;
    else if (!strcmp(name, "ANSX_FIN_ONE_WAVE")) c->dbg.fin_one_wave = on;
    else if (!strcmp(name, "ANSX_TEST_SP_BITS")) c->dbg.test_sp_bits = value ? (u32)atoi(value) : 0u;
    else if (!strcmp(name, "ANSX_PC_B_PAIRS")) c->dbg.pc_b_pairs = (value && value[0] == '1') ? 1u : 2u;
    else if (!strcmp(name, "ANSX_ENCODE_MODE2")) c->dbg.encode_mode2 = on;
    else if (!strcmp(name, "ANSX_DECODE_SMALL_RING")) {
        const int w = debug_word(value, "never", "always");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.decode_small_ring = w;
    }
    else if (!strcmp(name, "ANSX_DECODE_PAIR")) {
        const int w = debug_word(value, "never", "always");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.decode_pair = w;
    }
    else if (!strcmp(name, "ANSX_DECODE_SETUP")) {
        if (!value || !value[0] || !strcmp(value, "0")) c->dbg.setup_old = false;
        else if (!strcmp(value, "old")) c->dbg.setup_old = true;
        else return ANSX_ERR_ARG;
    }
    else if (!strcmp(name, "ANSX_MODEL_CHAIN")) {
        if (!value || !value[0] || !strcmp(value, "0")) c->dbg.chain_old = false;
        else if (!strcmp(value, "old")) c->dbg.chain_old = true;
        else return ANSX_ERR_ARG;
    }
    else if (!strcmp(name, "ANSX_INTERSECT_FORM")) {
        const int w = debug_word(value, "selective", "full");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.intersect_form = w;
    }
    else if (!strcmp(name, "ANSX_BOOL_FORM")) {
        const int w = debug_word(value, "search", "staged");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.bool_form = w;
    }
    else if (!strcmp(name, "ANSX_TOPK_QUERY_FORM")) {
        const int w = debug_word(value, "search", "staged");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.topk_query_form = w;
    }
    else if (!strcmp(name, "ANSX_TOPK_IMPACT_FORM")) {
        const int w = debug_word(value, "global", "staged");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.topk_impact_form = w;
    }
    else if (!strcmp(name, "ANSX_TOPK_IMPACT_TILE")) {
        const u32 v = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 0u;
        if (v != 0 && v != 1024 && v != 2048 && v != 4096) return ANSX_ERR_ARG;
        c->dbg.topk_impact_rounds = v / 1024u;
    }
    else if (!strcmp(name, "ANSX_TOPK_IMPACT_STAGE")) {
        const u32 v = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 0u;
        if (v > ANSX_IMPACT_STAGE_MAX) return ANSX_ERR_ARG;
        c->dbg.topk_impact_stage = v;
    }
    else if (!strcmp(name, "ANSX_TOPK_IMPACT_GRID")) c->dbg.topk_impact_grid = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_FACET_FORM")) {
        const int w = debug_word(value, "atomic", "lds");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.facet_form = w;
    }
    else if (!strcmp(name, "ANSX_FILTER_FORM")) {
        const int w = debug_word(value, "own", "fused");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.filter_form = w;
    }
    else if (!strcmp(name, "ANSX_FACET_GRID")) c->dbg.facet_grid = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_FACET_NO_COMBINE")) c->dbg.facet_no_combine = on;
    else if (!strcmp(name, "ANSX_TOPK_BOOL_FORM")) {
        const int w = debug_word(value, "search", "bounded");
        if (w < 0) return ANSX_ERR_ARG;
        c->dbg.topk_bool_form = w;
    }
    else if (!strcmp(name, "ANSX_DECODE_PAIR_LDS")) c->dbg.pair_lds_limit = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_FORGET_HINTS")) {  // the next call of every geometry is a first call again (bench.py: first_call_ms)
        c->ns_hint.clear();
        c->rf_hint.clear();
        c->t_hint.clear();
        c->wide_hint.clear();
        c->bat.ns_hint.clear(), c->bat.rf_hint.clear(), c->bat.t_hint.clear(), c->bat.wide_hint.clear(), c->bat.int_sparse_hint.clear();
        c->hdrs.clear();
    }
    else if (!strcmp(name, "ANSX_TEST_WIDE_AT")) {
        const u32 v = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 16u;
        if (v > 16) return ANSX_ERR_ARG;
        c->dbg.wide_at = v;
    }
    else if (!strcmp(name, "ANSX_NEAR_BAND")) c->dbg.near_band = (value && value[0]) ? strtod(value, nullptr) : ANSX_NEAR_BAND;
    else if (!strcmp(name, "ANSX_TEST_NEAR_FLIP")) c->dbg.near_flip = on;
    else if (!strcmp(name, "ANSX_BATCH_PASS_BLOCKS")) c->dbg.batch_pass_blocks = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_ISECT_BATCH_INTS")) c->dbg.isect_batch_ints = (value && value[0]) ? (u64)strtoull(value, nullptr, 10) : 0ull;
    else if (!strcmp(name, "ANSX_RANGE_SUMS_WG_MAX")) c->dbg.range_sums_wg_max = (value && value[0]) ? (u32)strtoul(value, nullptr, 10) : 0u;
    else if (!strcmp(name, "ANSX_MODEL_PIPELINE")) {
        if (!value || !value[0] || !strcmp(value, "0")) c->dbg.model_pipeline = 0;
        else if (!strcmp(value, "never")) c->dbg.model_pipeline = ANSX_PIPE_NEVER;
        else if (!strcmp(value, "always")) c->dbg.model_pipeline = ANSX_PIPE_ALWAYS;
        else {
            char* end = nullptr;
            const unsigned long v = strtoul(value, &end, 10);
            if (value[0] < '0' || value[0] > '9' || *end != 0 || v < 1 || v > ANSX_PIPE_MAX_RANGES) return ANSX_ERR_ARG;
            c->dbg.model_pipeline = (int)v;
        }
    }
    else if (!strcmp(name, "ANSX_CAND_CHAINS")) {
        const u32 v = value ? (u32)strtoul(value, nullptr, 10) : 0u;
        if (v > 2) return ANSX_ERR_ARG;
        c->dbg.cand_chains = v;
    } else if (!strcmp(name, "ANSX_FAST_GUARD")) c->dbg.fast_guard = (value && value[0]) ? strtod(value, nullptr) : ANSX_FAST_GUARD;
    else return ANSX_ERR_ARG;
    return ANSX_OK;
}

void ansx_destroy(ansx_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (hipStream_t st : c->pipe_stream)  // (idle unless a call failed in the middle: drained before anything is freed)
        if (st) (void)hipStreamSynchronize(st);
    for (hipEvent_t e : c->pipe_ev) (void)hipEventDestroy(e);
    for (hipStream_t st : c->pipe_stream)
        if (st) (void)hipStreamDestroy(st);
    DevBuf* bufs[] = { &c->pre_work, &c->hist, &c->hterm, &c->sortF, &c->sortSym, &c->attS, &c->prevS, &c->attMeta, &c->blk,
        &c->table, &c->tab32, &c->scratch, &c->misc, &c->mapped, &c->mostfreq, &c->stage_in, &c->stage_out,
        &c->dec_s2s, &c->dec_cum, &c->dec_info, &c->plain, &c->rf_tmp, &c->log2lut, &c->pa_alpha, &c->pa_info, &c->pairs, &c->lg2i, &c->sizes, &c->nearlist, &c->force, &c->geo_big,
        &c->rng_plan, &c->rng_cont, &c->rng_list, &c->rng_dev, &c->bat_hdr, &c->enb_plan, &c->enb_wc, &c->sums_plan, &c->sums_ints, &c->isect_ids, &c->isectb_ids, &c->isectb_work };
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (auto& kv : c->geo)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& r : c->recs) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->rng_pin) (void)hipHostFree(c->rng_pin);
    if (c->isectb_pin) (void)hipHostFree(c->isectb_pin);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* ansx_strerror(int st)
{
    switch (st) {
    case ANSX_OK: return "ok";
    case ANSX_ERR_ARG: return "invalid argument";
    case ANSX_ERR_CAPACITY: return "output buffer too small";
    case ANSX_ERR_FORMAT: return "malformed container or stream";
    case ANSX_ERR_HIP: return "HIP runtime error";
    case ANSX_ERR_NO_DEVICE: return "no usable gfx950 device";
    case ANSX_ERR_DOMAIN: return "input value outside [0, 2^30)";
    case ANSX_ERR_MODEL: return "frequency normalisation hit the reference's degenerate exit";
    default: return "unknown status";
    }
}

int ansx_last_hip_error(const ansx_ctx* c) { return c ? c->last_hip : 0; }

int ansx_codec_name(int kind, int f, char* buf, size_t buflen)
{
    if (kind == ANSX_MSB) return snprintf(buf, buflen, "ANSmsb");
    if (kind == ANSX_INT) return snprintf(buf, buflen, "ANS");  // methods.hpp:485
    return snprintf(buf, buflen, "%s-%d", kind == ANSX_RFOLD ? "ANSrfold" : "ANSfold", f);
}

size_t ansx_bound(int kind, int f, size_t n, const ansx_opts* opts)
{
    Plan P;
    if (make_plan(kind, f, n, opts, &P)) return 0;
    if (!P.plain) set_restart_format(&P, true);  // (the larger of the two index forms)
    size_t per = block_bound(kind, (u32)f, 0, false);
    return (size_t)P.lay.payload_off + (size_t)P.g.nblocks * per + (P.g.pa ? 11 : 7) * n + 64;
}

int ansx_encode_dev(ansx_ctx* c, int kind, int f, const uint32_t* d_in, size_t n, uint8_t* d_out,
    size_t cap, size_t* out_bytes, const ansx_opts* opts, void* stream)
{
    Plan P;
    int rc = encode_args(c, kind, f, d_in, n, d_out, out_bytes, opts, &P);
    if (rc) return rc;
    return run_call(c, stream, [&](hipStream_t s) { return encode_dev(c, P, d_in, d_out, cap, out_bytes, s); });
}

int ansx_decode_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes,
    uint32_t* d_out, size_t n, const ansx_opts* opts, void* stream)
{
    if (!c || !d_in || !d_out) return ANSX_ERR_ARG;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return ANSX_ERR_ARG;
    Plan P;
    int rc = make_plan(kind, f, n, opts, &P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return decode_dev(c, P, d_in, in_bytes, d_out, s);
}

int ansx_decode_ranges_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes, const uint64_t* first,
    const uint32_t* count, size_t nranges, uint32_t* d_out, size_t out_capacity_ints, void* stream)
{
    // (every argument check comes before the context is touched)
    if (ranges_args(c, d_in, d_out, first, count, nranges)) return ANSX_ERR_ARG;
    if (nranges == 0) return ANSX_OK;
    const RangeOut out = { OUT_GATHER, d_out };
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_ranges(c, kind, f, d_in, in_bytes, (const u64*)first, count, nranges, out_capacity_ints, out, s);
    });
}

int ansx_decode_device_ranges_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes,
    const uint64_t* d_first, const uint32_t* d_count, size_t nranges, uint32_t* d_out, size_t out_capacity_ints,
    uint64_t* d_offsets, uint64_t* total_ints, void* stream)
{
    // (every argument check comes before the context is touched)
    if (device_ranges_args(c, d_in, d_out, d_first, d_count, nranges, d_offsets)) return ANSX_ERR_ARG;
    if (nranges == 0) return empty_batch(nullptr, total_ints);
    const RangeOut out = { OUT_GATHER, d_out };
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_device_ranges(c, kind, f, d_in, in_bytes, (const u64*)d_first, d_count, nranges, out_capacity_ints,
            (u64*)d_offsets, (u64*)total_ints, out, s);
    });
}

int ansx_decode_ranges_sums_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes, const uint32_t* d_bases,
    size_t nbases, const uint64_t* first, const uint32_t* count, size_t nranges, uint32_t* d_out, size_t out_capacity_ints,
    void* stream)
{
    // (every argument check comes before the context is touched)
    if (ranges_args(c, d_in, d_out, first, count, nranges)) return ANSX_ERR_ARG;
    if (nranges > 0 && (!d_bases || ((uintptr_t)d_bases & 3u))) return ANSX_ERR_ARG;
    if (nranges == 0) return ANSX_OK;
    const RangeOut out = { OUT_SUMS_GATHER, d_out, d_bases, nbases };
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_ranges(c, kind, f, d_in, in_bytes, (const u64*)first, count, nranges, out_capacity_ints, out, s);
    });
}

int ansx_decode_device_ranges_sums_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes,
    const uint32_t* d_bases, size_t nbases, const uint64_t* d_first, const uint32_t* d_count, size_t nranges, uint32_t* d_out,
    size_t out_capacity_ints, uint64_t* d_offsets, uint64_t* total_ints, void* stream)
{
    // (every argument check comes before the context is touched)
    if (device_ranges_args(c, d_in, d_out, d_first, d_count, nranges, d_offsets)) return ANSX_ERR_ARG;
    if (nranges > 0 && (!d_bases || ((uintptr_t)d_bases & 3u))) return ANSX_ERR_ARG;
    if (nranges == 0) return empty_batch(nullptr, total_ints);
    const RangeOut out = { OUT_SUMS_GATHER, d_out, d_bases, nbases };
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_device_ranges(c, kind, f, d_in, in_bytes, (const u64*)d_first, d_count, nranges, out_capacity_ints,
            (u64*)d_offsets, (u64*)total_ints, out, s);
    });
}

int ansx_next_geq_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes, const uint32_t* d_bases,
    size_t nbases, const uint32_t* d_targets, size_t ntargets, uint64_t* d_pos, uint32_t* d_ids, uint64_t* found, void* stream)
{
    // (every argument check comes before the context is touched)
    if (!c || !d_in) return ANSX_ERR_ARG;
    if (ntargets > 0 && (!d_bases || !d_targets || (!d_pos && !d_ids))) return ANSX_ERR_ARG;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_bases & 3u) || ((uintptr_t)d_targets & 3u) || ((uintptr_t)d_pos & 7u)
        || ((uintptr_t)d_ids & 3u))
        return ANSX_ERR_ARG;
    if (ntargets > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (ntargets == 0) return empty_batch(nullptr, found);
    const RangeOut out = { OUT_SUMS_SEARCH, nullptr, d_bases, nbases, d_targets, (u32)ntargets, (u64*)d_pos, d_ids };
    u64 total = 0;  // (the targets found; the ranges are the front's own: no first, count or offsets from here)
    const int rc = run_call(c, stream, [&](hipStream_t s) {
        return decode_device_ranges(c, kind, f, d_in, in_bytes, nullptr, nullptr, ntargets, ntargets, nullptr, &total, out, s);
    });
    if (rc == ANSX_OK && found) *found = total;
    return rc;
}

int ansx_intersect_ids_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes, const uint32_t* d_bases,
    size_t nbases, const uint32_t* d_cand, size_t ncand, uint32_t* d_out_ids, uint32_t* d_out_idx, uint64_t* d_out_pos,
    size_t out_capacity, uint64_t* nfound, void* stream)
{
    // (every argument check comes before the context is touched)
    if (!c || !d_in) return ANSX_ERR_ARG;
    if (ncand > 0 && (!d_bases || !d_cand || (!d_out_ids && !d_out_idx && !d_out_pos))) return ANSX_ERR_ARG;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_bases & 3u) || ((uintptr_t)d_cand & 3u) || ((uintptr_t)d_out_ids & 3u)
        || ((uintptr_t)d_out_idx & 3u) || ((uintptr_t)d_out_pos & 7u))
        return ANSX_ERR_ARG;
    if (ncand > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (ncand == 0) return empty_batch(nullptr, nfound);
    const IsectOut o = { d_out_ids, d_out_idx, (u64*)d_out_pos, (u64)out_capacity };
    u64 total = 0;
    const int rc = run_call(c, stream, [&](hipStream_t s) -> int {
        int r;
        RangeTail t = { d_in };
        if ((r = range_source(c, kind, f, d_in, in_bytes, s, &t.H, &t.P))) return r;
        return isect_step(c, kind, f, t, in_bytes, d_bases, nbases, d_cand, (u32)ncand, o, &total, s);
    });
    if ((rc == ANSX_OK || rc == ANSX_ERR_CAPACITY) && nfound) *nfound = total;
    return rc;
}

int ansx_intersect_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, uint32_t* d_out_ids, size_t out_capacity,
    uint64_t* nfound, size_t* bad_container, void* stream)
{
    // (every argument check comes before the context is touched)
    if (!c || count == 0 || count > 0xFFFFFFFFull || !d_ins || !in_bytes) return ANSX_ERR_ARG;
    if (count > 1 && (!d_bases || !nbases)) return ANSX_ERR_ARG;
    if ((!d_out_ids && out_capacity > 0) || ((uintptr_t)d_out_ids & 3u)) return ANSX_ERR_ARG;
    for (size_t i = 0; i < count; i++)
        if (!d_ins[i] || ((uintptr_t)d_ins[i] & 15u) || (d_bases && ((uintptr_t)d_bases[i] & 3u))) {
            if (bad_container) *bad_container = i;
            return ANSX_ERR_ARG;
        }
    return run_call(c, stream, [&](hipStream_t s) {
        return intersect_lists(c, kind, f, d_ins, in_bytes, d_bases, nbases, count, d_out_ids, out_capacity, (u64*)nfound,
            bad_container, s);
    });
}

int ansx_intersect_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count,
    const uint32_t* terms, const uint64_t* qoff, size_t nqueries, uint32_t* d_out_ids, size_t out_capacity,
    uint64_t* out_offsets, size_t* bad_container, size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched)
    if (queries_args(c, d_ins, in_bytes, count, terms, qoff, nqueries, d_out_ids, nullptr, out_capacity, out_offsets, bad_container,
            bad_query))
        return ANSX_ERR_ARG;
    if (nqueries == 0) return empty_batch(out_offsets, (u64*)nullptr);
    return run_call(c, stream, [&](hipStream_t s) {
        return bool_batch(c, kind, f, d_ins, in_bytes, count, ANSX_BOOL_ALL, terms, (const u64*)qoff, nullptr, nullptr, nqueries, d_out_ids,
            nullptr, out_capacity, (u64*)out_offsets, bad_container, bad_query, s);
    });
}

int ansx_union_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count,
    const uint32_t* terms, const uint64_t* qoff, size_t nqueries, uint32_t* d_out_ids, uint32_t* d_out_cnt, size_t out_capacity,
    uint64_t* out_offsets, size_t* bad_container, size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched)
    if (queries_args(c, d_ins, in_bytes, count, terms, qoff, nqueries, d_out_ids, d_out_cnt, out_capacity, out_offsets, bad_container,
            bad_query))
        return ANSX_ERR_ARG;
    if (nqueries == 0) return empty_batch(out_offsets, (u64*)nullptr);
    return run_call(c, stream, [&](hipStream_t s) {
        return bool_batch(c, kind, f, d_ins, in_bytes, count, ANSX_BOOL_ANY, terms, (const u64*)qoff, nullptr, nullptr, nqueries, d_out_ids,
            d_out_cnt, out_capacity, (u64*)out_offsets, bad_container, bad_query, s);
    });
}

// ... what ansx_bool_batch_dev adds to queries_args: op and the excluded terms
static int bool_args(const uint8_t* const* d_ins, size_t count, int op, const uint32_t* xterms, const uint64_t* xqoff, size_t nqueries,
    size_t* bad_container, size_t* bad_query)
{
    if (op != ANSX_BOOL_ALL && op != ANSX_BOOL_ANY) return ANSX_ERR_ARG;
    if (!xqoff || nqueries == 0) return ANSX_OK;
    for (size_t q = 0; q < nqueries; q++)
        if ((q == 0 && xqoff[0] != 0) || xqoff[q + 1] < xqoff[q]) {
            if (bad_query) *bad_query = q;
            return ANSX_ERR_ARG;
        }
    if (xqoff[nqueries] > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (!xterms && xqoff[nqueries] > 0) return ANSX_ERR_ARG;
    for (size_t q = 0; q < nqueries; q++)
        for (u64 j = xqoff[q]; j < xqoff[q + 1]; j++)
            if (xterms[j] >= count) {
                if (bad_query) *bad_query = q;
                return ANSX_ERR_ARG;
            }
    for (size_t q = 0; q < nqueries; q++)
        for (u64 j = xqoff[q]; j < xqoff[q + 1]; j++)
            if (!d_ins[xterms[j]] || ((uintptr_t)d_ins[xterms[j]] & 15u)) {
                if (bad_query) *bad_query = q;
                if (bad_container) *bad_container = xterms[j];
                return ANSX_ERR_ARG;
            }
    return ANSX_OK;
}

int ansx_bool_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count, int op,
    const uint32_t* terms, const uint64_t* qoff, const uint32_t* xterms, const uint64_t* xqoff, size_t nqueries, uint32_t* d_out_ids,
    size_t out_capacity, uint64_t* out_offsets, size_t* bad_container, size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched)
    if (queries_args(c, d_ins, in_bytes, count, terms, qoff, nqueries, d_out_ids, nullptr, out_capacity, out_offsets, bad_container,
            bad_query))
        return ANSX_ERR_ARG;
    if (bool_args(d_ins, count, op, xterms, xqoff, nqueries, bad_container, bad_query)) return ANSX_ERR_ARG;
    if (nqueries == 0) return empty_batch(out_offsets, (u64*)nullptr);
    return run_call(c, stream, [&](hipStream_t s) {
        return bool_batch(c, kind, f, d_ins, in_bytes, count, op, terms, (const u64*)qoff, xterms, (const u64*)xqoff, nqueries, d_out_ids,
            nullptr, out_capacity, (u64*)out_offsets, bad_container, bad_query, s);
    });
}

// ... what the ranked calls check: queries_args and the weights, k, the outputs and the payloads of the named lists
static int topk_args(const ansx_ctx* c, const uint8_t* const* d_ins, const size_t* in_bytes, const uint8_t* const* d_pays,
    const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights, const uint64_t* qoff, size_t nqueries,
    uint32_t k, const uint32_t* d_out_ids, const uint32_t* d_out_scores, size_t* bad_container, size_t* bad_query)
{
    uint64_t offs_stand_in = 0;  // (the parents' out_offsets: these calls have none)
    if (queries_args(c, d_ins, in_bytes, count, terms, qoff, nqueries, d_out_ids, nullptr, 0, &offs_stand_in, bad_container, bad_query))
        return ANSX_ERR_ARG;
    if (nqueries > 0 && !weights) return ANSX_ERR_ARG;
    if (k == 0 || k > ANSX_TOPK_MAX_K || (u64)nqueries * k > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (!d_out_ids || ((uintptr_t)d_out_scores & 3u)) return ANSX_ERR_ARG;
    if (d_pays && nqueries > 0) {
        if (!pay_bytes) return ANSX_ERR_ARG;
        for (size_t q = 0; q < nqueries; q++)  // (only the payloads of the lists some query names are looked at)
            for (u64 j = qoff[q]; j < qoff[q + 1]; j++)
                if (!d_pays[terms[j]] || ((uintptr_t)d_pays[terms[j]] & 15u)) {
                    if (bad_query) *bad_query = q;
                    if (bad_container) *bad_container = terms[j];
                    return ANSX_ERR_ARG;
                }
    }
    return ANSX_OK;
}

int ansx_topk_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint64_t* qoff, size_t nqueries, uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts,
    size_t* bad_container, size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched)
    if (topk_args(c, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, qoff, nqueries, k, d_out_ids, d_out_scores, bad_container,
            bad_query))
        return ANSX_ERR_ARG;
    if (nqueries == 0) return ANSX_OK;
    return run_call(c, stream, [&](hipStream_t s) {
        return topk_bool_batch(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, ANSX_BOOL_ANY, false, terms, weights, (const u64*)qoff,
            nullptr, nullptr, nqueries, k, d_out_ids, d_out_scores, out_counts, bad_container, bad_query, s);
    });
}

int ansx_topk_bool_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, int op, const uint32_t* terms, const uint32_t* weights,
    const uint64_t* qoff, const uint32_t* xterms, const uint64_t* xqoff, size_t nqueries, uint32_t k, uint32_t* d_out_ids,
    uint32_t* d_out_scores, uint32_t* out_counts, size_t* bad_container, size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched)
    if (topk_args(c, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, qoff, nqueries, k, d_out_ids, d_out_scores, bad_container,
            bad_query))
        return ANSX_ERR_ARG;
    if (bool_args(d_ins, count, op, xterms, xqoff, nqueries, bad_container, bad_query)) return ANSX_ERR_ARG;
    if (nqueries == 0) return ANSX_OK;
    return run_call(c, stream, [&](hipStream_t s) {
        return topk_bool_batch(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, op, true, terms, weights, (const u64*)qoff, xterms,
            (const u64*)xqoff, nqueries, k, d_out_ids, d_out_scores, out_counts, bad_container, bad_query, s);
    });
}

// ... what ansx_topk_query_batch_dev and ansx_topk_scored_batch_dev check: topk_args, the excluded terms, the occur values
static int topk_query_args(const ansx_ctx* c, const uint8_t* const* d_ins, const size_t* in_bytes, const uint8_t* const* d_pays,
    const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights, const uint8_t* occur, const uint64_t* qoff,
    const uint32_t* xterms, const uint64_t* xqoff, size_t nqueries, uint32_t k, const uint32_t* d_out_ids, const uint32_t* d_out_scores,
    size_t* bad_container, size_t* bad_query)
{
    if (topk_args(c, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, qoff, nqueries, k, d_out_ids, d_out_scores, bad_container,
            bad_query))
        return ANSX_ERR_ARG;
    if (bool_args(d_ins, count, ANSX_BOOL_ALL, xterms, xqoff, nqueries, bad_container, bad_query)) return ANSX_ERR_ARG;
    if (occur)
        for (size_t q = 0; q < nqueries; q++)
            for (u64 j = qoff[q]; j < qoff[q + 1]; j++)
                if (occur[j] != ANSX_OCCUR_SHOULD && occur[j] != ANSX_OCCUR_MUST) {
                    if (bad_query) *bad_query = q;
                    return ANSX_ERR_ARG;
                }
    return ANSX_OK;
}

int ansx_topk_query_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff, size_t nqueries,
    uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts, size_t* bad_container, size_t* bad_query,
    void* stream)
{
    // (every argument check comes before the context is touched)
    if (topk_query_args(c, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, qoff, xterms, xqoff, nqueries, k, d_out_ids,
            d_out_scores, bad_container, bad_query))
        return ANSX_ERR_ARG;
    if (nqueries == 0) return ANSX_OK;
    return run_call(c, stream, [&](hipStream_t s) {
        return topk_query_batch(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, (const u64*)qoff, msm, xterms,
            (const u64*)xqoff, nqueries, k, d_out_ids, d_out_scores, out_counts, bad_container, bad_query, s);
    });
}

// ... what a scorer adds, behind them
static int scorer_args(const ansx_scorer* scorer, const uint8_t* const* d_pays)
{
    if (!scorer) return ANSX_OK;
    if (!d_pays) return ANSX_ERR_ARG;  // (a term frequency is needed)
    if (!scorer->d_norms || !scorer->d_table || ((uintptr_t)scorer->d_table & 3u)) return ANSX_ERR_ARG;
    if (scorer->ndocs == 0 || (u64)scorer->ndocs > ((u64)1 << 32)) return ANSX_ERR_ARG;
    if (scorer->tf_rows == 0 || scorer->tf_rows > ANSX_IMPACT_MAX_ROWS) return ANSX_ERR_ARG;
    return ANSX_OK;
}

// ... what facets add, behind them
static int facets_args(const ansx_facets* facets)
{
    if (!facets) return ANSX_OK;
    if (!facets->d_values || !facets->d_counts || ((uintptr_t)facets->d_values & 3u) || ((uintptr_t)facets->d_counts & 3u)) return ANSX_ERR_ARG;
    if (facets->ndocs == 0 || (u64)facets->ndocs > ((u64)1 << 32)) return ANSX_ERR_ARG;
    if (facets->nvalues == 0 || facets->nvalues > ANSX_FACET_MAX_VALUES) return ANSX_ERR_ARG;
    return ANSX_OK;
}

int ansx_topk_scored_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff,
    const ansx_scorer* scorer, size_t nqueries, uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts,
    size_t* bad_container, size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched: the parent's, then the scorer's)
    if (topk_query_args(c, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, qoff, xterms, xqoff, nqueries, k, d_out_ids,
            d_out_scores, bad_container, bad_query))
        return ANSX_ERR_ARG;
    if (scorer_args(scorer, d_pays)) return ANSX_ERR_ARG;
    if (nqueries == 0) return ANSX_OK;
    return run_call(c, stream, [&](hipStream_t s) {
        return topk_scored_batch(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, (const u64*)qoff, msm, xterms,
            (const u64*)xqoff, scorer, nullptr, nqueries, k, d_out_ids, d_out_scores, out_counts, nullptr, bad_container, bad_query, s);
    });
}

int ansx_topk_facets_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff,
    const ansx_scorer* scorer, const ansx_facets* facets, size_t nqueries, uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores,
    uint32_t* out_counts, uint32_t* out_totals, size_t* bad_container, size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched: the parent's, the scorer's, then the facets')
    if (topk_query_args(c, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, qoff, xterms, xqoff, nqueries, k, d_out_ids,
            d_out_scores, bad_container, bad_query))
        return ANSX_ERR_ARG;
    if (scorer_args(scorer, d_pays)) return ANSX_ERR_ARG;
    if (facets_args(facets)) return ANSX_ERR_ARG;
    if (nqueries == 0) return ANSX_OK;
    return run_call(c, stream, [&](hipStream_t s) {
        return topk_scored_batch(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, (const u64*)qoff, msm, xterms,
            (const u64*)xqoff, scorer, facets, nqueries, k, d_out_ids, d_out_scores, out_counts, out_totals, bad_container, bad_query, s);
    });
}

// ... what filters add, behind them: the pointers, the columns' number, the columns the clauses name, ndocs, the offsets,
// then per query -- *bad_query the first that offends -- the number of its clauses, their columns and flags
static int filters_args(const ansx_filters* fl, size_t nqueries, size_t* bad_query)
{
    if (!fl) return ANSX_OK;
    if (!fl->d_columns || !fl->fqoff) return ANSX_ERR_ARG;
    const u64 ncl = fl->fqoff[nqueries];
    if (!fl->clauses && ncl > 0) return ANSX_ERR_ARG;
    if (fl->ncolumns == 0 || fl->ncolumns > ANSX_FILTER_MAX_COLUMNS) return ANSX_ERR_ARG;
    for (u64 e = 0; e < ncl; e++) {
        const u32 col = fl->clauses[e].column;
        if (col < fl->ncolumns && (!fl->d_columns[col] || ((uintptr_t)fl->d_columns[col] & 3u))) return ANSX_ERR_ARG;
    }
    if (fl->ndocs == 0 || (u64)fl->ndocs > ((u64)1 << 32)) return ANSX_ERR_ARG;
    if (fl->fqoff[0] != 0) return ANSX_ERR_ARG;
    for (size_t q = 0; q < nqueries; q++)
        if (fl->fqoff[q] > fl->fqoff[q + 1]) return ANSX_ERR_ARG;
    for (size_t q = 0; q < nqueries; q++) {
        bool bad = fl->fqoff[q + 1] - fl->fqoff[q] > ANSX_FILTER_MAX_CLAUSES;
        for (u64 e = fl->fqoff[q]; !bad && e < fl->fqoff[q + 1]; e++)
            bad = fl->clauses[e].column >= fl->ncolumns || (fl->clauses[e].flags & ~ANSX_FILTER_NOT) != 0;
        if (bad) {
            if (bad_query) *bad_query = q;
            return ANSX_ERR_ARG;
        }
    }
    return ANSX_OK;
}

int ansx_topk_filter_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff,
    const ansx_scorer* scorer, const ansx_facets* facets, const ansx_filters* filters, size_t nqueries, uint32_t k,
    uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts, uint32_t* out_totals, size_t* bad_container,
    size_t* bad_query, void* stream)
{
    // (every argument check comes before the context is touched: the parent's, the scorer's, the facets', then the filters')
    if (topk_query_args(c, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, qoff, xterms, xqoff, nqueries, k, d_out_ids,
            d_out_scores, bad_container, bad_query))
        return ANSX_ERR_ARG;
    if (scorer_args(scorer, d_pays)) return ANSX_ERR_ARG;
    if (facets_args(facets)) return ANSX_ERR_ARG;
    if (filters_args(filters, nqueries, bad_query)) return ANSX_ERR_ARG;
    if (nqueries == 0) return ANSX_OK;
    return run_call(c, stream, [&](hipStream_t s) {
        return topk_scored_batch(c, kind, f, d_ins, in_bytes, d_pays, pay_bytes, count, terms, weights, occur, (const u64*)qoff, msm, xterms,
            (const u64*)xqoff, scorer, facets, nqueries, k, d_out_ids, d_out_scores, out_counts, out_totals, bad_container, bad_query, s,
            filters);
    });
}

int ansx_union_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count,
    uint32_t* d_out_ids, uint32_t* d_out_cnt, size_t out_capacity, uint64_t* nfound, size_t* bad_container, void* stream)
{
    // the batch call with the one query 0, 1, ..., count - 1
    if (!c || count == 0 || count > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    std::vector<u32> terms;
    try {
        terms.resize(count);
    } catch (const std::bad_alloc&) {
        c->last_hip = (int)hipErrorOutOfMemory;
        return ANSX_ERR_HIP;
    }
    for (size_t i = 0; i < count; i++) terms[i] = (u32)i;
    const uint64_t qoff[2] = { 0, (uint64_t)count };
    uint64_t offs[2] = { 0, 0 };
    size_t bad_query = 0;
    const int rc = ansx_union_batch_dev(c, kind, f, d_ins, in_bytes, count, terms.data(), qoff, 1, d_out_ids, d_out_cnt, out_capacity,
        offs, bad_container, &bad_query, stream);
    if ((rc == ANSX_OK || rc == ANSX_ERR_CAPACITY) && nfound) *nfound = offs[1];
    return rc;
}

int ansx_block_bases_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes, uint32_t* d_bases,
    size_t bases_capacity, size_t* nbases, void* stream)
{
    // (every argument check comes before the context is touched)
    if (!c || !d_in || !nbases) return ANSX_ERR_ARG;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_bases & 3u)) return ANSX_ERR_ARG;
    if (!d_bases && bases_capacity > 0) return ANSX_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return block_bases(c, kind, f, d_in, in_bytes, d_bases, bases_capacity, nbases, s);
}

int ansx_decode_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count,
    uint32_t* d_out, size_t out_capacity_ints, uint64_t* offsets, uint64_t* total_ints, size_t* bad_index, void* stream)
{
    // (every argument check comes before the context is touched)
    if (decode_batch_args(c, d_ins, in_bytes, count, d_out, out_capacity_ints)) return ANSX_ERR_ARG;
    if (count == 0) return empty_batch(offsets, total_ints);
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_batch(c, kind, f, d_ins, in_bytes, count, d_out, out_capacity_ints, (u64*)offsets, (u64*)total_ints,
            bad_index, s);
    });
}

int ansx_decode_batch_ranges_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, const uint32_t* src, const uint64_t* first, const uint32_t* cnt, size_t nranges, uint32_t* d_out,
    size_t out_capacity_ints, uint64_t* offsets, uint64_t* total_ints, size_t* bad_container, size_t* bad_range, void* stream)
{
    // (every argument check comes before the context is touched)
    if (nranges > 0 && (!first || !cnt)) return ANSX_ERR_ARG;
    if ((!d_out && out_capacity_ints > 0) || ((uintptr_t)d_out & 3u)) return ANSX_ERR_ARG;
    if (batch_src_args(c, d_ins, in_bytes, false, nullptr, nullptr, count, src, nranges, bad_range)) return ANSX_ERR_ARG;
    if (nranges == 0) return empty_batch(offsets, total_ints);
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_batch_ranges(c, kind, f, d_ins, in_bytes, count, src, (const u64*)first, cnt, nranges, d_out,
            out_capacity_ints, (u64*)offsets, (u64*)total_ints, bad_container, bad_range, nullptr, nullptr, s);
    });
}

int ansx_decode_batch_ranges_sums_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* src, const uint64_t* first,
    const uint32_t* cnt, size_t nranges, uint32_t* d_out, size_t out_capacity_ints, uint64_t* offsets, uint64_t* total_ints,
    size_t* bad_container, size_t* bad_range, void* stream)
{
    // (every argument check comes before the context is touched)
    if (nranges > 0 && (!first || !cnt)) return ANSX_ERR_ARG;
    if ((!d_out && out_capacity_ints > 0) || ((uintptr_t)d_out & 3u)) return ANSX_ERR_ARG;
    if (batch_src_args(c, d_ins, in_bytes, true, d_bases, nbases, count, src, nranges, bad_range)) return ANSX_ERR_ARG;
    if (nranges == 0) return empty_batch(offsets, total_ints);
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_batch_ranges(c, kind, f, d_ins, in_bytes, count, src, (const u64*)first, cnt, nranges, d_out,
            out_capacity_ints, (u64*)offsets, (u64*)total_ints, bad_container, bad_range, d_bases, nbases, s);
    });
}

// (every argument check of the two entries below: before the context is touched)
static int batch_device_ranges_args(const ansx_ctx* c, const uint8_t* const* d_ins, const size_t* in_bytes, bool with_bases,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* d_src, const uint64_t* d_first,
    const uint32_t* d_cnt, size_t nranges, const uint32_t* d_out, size_t out_capacity_ints, const uint64_t* d_offsets)
{
    if (!c || count > 0xFFFFFFFFull || nranges > 0xFFFFFFFFull) return ANSX_ERR_ARG;
    if (nranges > 0 && (!d_src || !d_first || !d_cnt || !d_ins || !in_bytes)) return ANSX_ERR_ARG;
    if (with_bases && (!d_bases || !nbases)) return ANSX_ERR_ARG;
    if (((uintptr_t)d_src & 3u) || ((uintptr_t)d_first & 7u) || ((uintptr_t)d_cnt & 3u) || ((uintptr_t)d_out & 3u)
        || ((uintptr_t)d_offsets & 7u))
        return ANSX_ERR_ARG;
    if (!d_out && out_capacity_ints > 0) return ANSX_ERR_ARG;
    return ANSX_OK;
}

// no ranges: total 0 and, the one thing such a call enqueues, d_offsets[0] = 0
static int batch_device_ranges_none(ansx_ctx* c, uint64_t* d_offsets, uint64_t* total_ints, void* stream)
{
    if (total_ints) *total_ints = 0;
    if (!d_offsets) return ANSX_OK;
    return run_call(c, stream, [&](hipStream_t s) -> int {
        HIPCHK(c, hipMemsetAsync(d_offsets, 0, 8, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return ANSX_OK;
    });
}

int ansx_decode_batch_device_ranges_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, const uint32_t* d_src, const uint64_t* d_first, const uint32_t* d_cnt, size_t nranges, uint32_t* d_out,
    size_t out_capacity_ints, uint64_t* d_offsets, uint64_t* total_ints, size_t* bad_container, size_t* bad_range, void* stream)
{
    if (batch_device_ranges_args(c, d_ins, in_bytes, false, nullptr, nullptr, count, d_src, d_first, d_cnt, nranges, d_out,
            out_capacity_ints, d_offsets))
        return ANSX_ERR_ARG;
    if (nranges == 0) return batch_device_ranges_none(c, d_offsets, total_ints, stream);
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_batch_device_ranges(c, kind, f, d_ins, in_bytes, count, d_src, (const u64*)d_first, d_cnt, nranges, d_out,
            out_capacity_ints, (u64*)d_offsets, (u64*)total_ints, bad_container, bad_range, nullptr, nullptr, s);
    });
}

int ansx_decode_batch_device_ranges_sums_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* d_src, const uint64_t* d_first,
    const uint32_t* d_cnt, size_t nranges, uint32_t* d_out, size_t out_capacity_ints, uint64_t* d_offsets, uint64_t* total_ints,
    size_t* bad_container, size_t* bad_range, void* stream)
{
    if (batch_device_ranges_args(c, d_ins, in_bytes, true, d_bases, nbases, count, d_src, d_first, d_cnt, nranges, d_out,
            out_capacity_ints, d_offsets))
        return ANSX_ERR_ARG;
    if (nranges == 0) return batch_device_ranges_none(c, d_offsets, total_ints, stream);
    return run_call(c, stream, [&](hipStream_t s) {
        return decode_batch_device_ranges(c, kind, f, d_ins, in_bytes, count, d_src, (const u64*)d_first, d_cnt, nranges, d_out,
            out_capacity_ints, (u64*)d_offsets, (u64*)total_ints, bad_container, bad_range, d_bases, nbases, s);
    });
}

int ansx_next_geq_batch_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* src, const uint32_t* d_targets,
    size_t ntargets, uint64_t* d_pos, uint32_t* d_ids, uint64_t* found, size_t* bad_container, size_t* bad_target, void* stream)
{
    // (every argument check comes before the context is touched)
    if (ntargets > 0 && (!d_targets || (!d_pos && !d_ids))) return ANSX_ERR_ARG;
    if (((uintptr_t)d_targets & 3u) || ((uintptr_t)d_pos & 7u) || ((uintptr_t)d_ids & 3u)) return ANSX_ERR_ARG;
    if (batch_src_args(c, d_ins, in_bytes, true, d_bases, nbases, count, src, ntargets, bad_target)) return ANSX_ERR_ARG;
    if (ntargets == 0) return empty_batch(nullptr, found);
    return run_call(c, stream, [&](hipStream_t s) {
        return next_geq_batch(c, kind, f, d_ins, in_bytes, d_bases, nbases, count, src, d_targets, ntargets, (u64*)d_pos, d_ids,
            (u64*)found, bad_container, s);
    });
}

int ansx_encode_batch_dev(ansx_ctx* c, int kind, int f, const uint32_t* d_in, const uint64_t* offsets, size_t count,
    uint8_t* d_out, size_t out_capacity, uint64_t* out_offsets, uint64_t* out_bytes, size_t* total_bytes, size_t* bad_index,
    const ansx_opts* opts, void* stream)
{
    // (every argument check comes before the context is touched)
    Plan P0;
    int rc = encode_batch_args(c, kind, f, d_in, offsets, count, d_out, bad_index, opts, &P0);
    if (rc) return rc;
    if (count == 0) return empty_batch(out_offsets, total_bytes);
    return run_call(c, stream, [&](hipStream_t s) {
        return encode_batch(c, P0, opts, d_in, (const u64*)offsets, count, d_out, out_capacity, (u64*)out_offsets, (u64*)out_bytes,
            total_bytes, bad_index, s);
    });
}

int ansx_decode_sums_dev(ansx_ctx* c, int kind, int f, const uint8_t* d_in, size_t in_bytes, uint32_t* d_out, size_t n,
    const ansx_opts* opts, void* stream)
{
    if (!c || !d_in || !d_out) return ANSX_ERR_ARG;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 3u)) return ANSX_ERR_ARG;
    Plan P;
    int rc = make_plan(kind, f, n, opts, &P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // the decoders store 16 bytes at a time: an output that is not aligned for them is decoded in workspace and copied
    u32* dec = d_out;
    if ((uintptr_t)d_out & 15u) {
        if ((rc = ensure(c, c->sums_ints, 4 * (n + 4)))) return rc;
        dec = (u32*)c->sums_ints.p;
    }
    if ((rc = decode_dev(c, P, d_in, in_bytes, dec, s))) return rc;
    if (dec != d_out) HIPCHK(c, hipMemcpyAsync(d_out, dec, 4 * n, hipMemcpyDeviceToDevice, s));
    const u64 offs[2] = { 0, (u64)n };
    return sums_run(c, d_out, (u64)n, offs, 1, nullptr, s);
}

int ansx_decode_batch_sums_dev(ansx_ctx* c, int kind, int f, const uint8_t* const* d_ins, const size_t* in_bytes, size_t count,
    uint32_t* d_out, size_t out_capacity_ints, uint64_t* offsets, uint64_t* total_ints, size_t* bad_index, void* stream)
{
    // (every argument check comes before the context is touched)
    int rc;
    if ((rc = decode_batch_args(c, d_ins, in_bytes, count, d_out, out_capacity_ints))) return rc;
    if (count == 0) return empty_batch(offsets, total_ints);
    return run_call(c, stream, [&](hipStream_t s) -> int {
        std::vector<u64> off(count + 1);  // (the scan needs the offsets whether the caller asked for them or not)
        u64 total = 0;
        rc = decode_batch(c, kind, f, d_ins, in_bytes, count, d_out, out_capacity_ints, off.data(), &total, bad_index, s);
        if (rc == ANSX_OK || rc == ANSX_ERR_CAPACITY) {
            if (offsets) memcpy(offsets, off.data(), 8 * (count + 1));
            if (total_ints) *total_ints = total;
        }
        if (rc || total == 0) return rc;
        // every pass of every geometry group is through: one scan over the whole output
        return sums_run(c, d_out, total, off.data(), count, bad_index, s);
    });
}

int ansx_encode_gaps_dev(ansx_ctx* c, int kind, int f, const uint32_t* d_in, size_t n, uint8_t* d_out, size_t cap,
    size_t* out_bytes, const ansx_opts* opts, void* stream)
{
    Plan P;
    int rc = encode_args(c, kind, f, d_in, n, d_out, out_bytes, opts, &P);
    if (rc) return rc;
    return run_call(c, stream, [&](hipStream_t s) -> int {
        const u64 offs[2] = { 0, (u64)n };
        const u32* gaps = nullptr;
        if ((rc = gaps_run(c, d_in, (u64)n, offs, 1, &gaps, nullptr, s))) return rc;
        return encode_dev(c, P, gaps, d_out, cap, out_bytes, s);
    });
}

int ansx_encode_gaps_bases_dev(ansx_ctx* c, int kind, int f, const uint32_t* d_in, size_t n, uint8_t* d_out, size_t cap,
    size_t* out_bytes, const ansx_opts* opts, uint32_t* d_bases, size_t bases_capacity, size_t* nbases, void* stream)
{
    if (!nbases || ((uintptr_t)d_bases & 3u) || (!d_bases && bases_capacity > 0)) return ANSX_ERR_ARG;
    if (opts && opts->block_ints == ANSX_SINGLE_STREAM) return ANSX_ERR_ARG;  // (a stream has no blocks)
    Plan P;
    int rc = encode_args(c, kind, f, d_in, n, d_out, out_bytes, opts, &P);
    if (rc) return rc;
    *nbases = (size_t)P.g.nblocks + 1;
    if (bases_capacity < (size_t)P.g.nblocks + 1) return ANSX_ERR_CAPACITY;
    return run_call(c, stream, [&](hipStream_t s) -> int {
        const u64 offs[2] = { 0, (u64)n };
        const u32* gaps = nullptr;
        if ((rc = gaps_run(c, d_in, (u64)n, offs, 1, &gaps, nullptr, s))) return rc;
        // the ids do not decrease: the id in front of a block is the sum of every gap in front of it
        LAUNCH(c, "k_rs_ids_bases", k_rs_ids_bases, P.g.nblocks / ANSX_RS_NT + 1, ANSX_RS_NT, 0, s, d_in, (u64)n, P.g.block_ints,
            P.g.nblocks, d_bases);
        return encode_dev(c, P, gaps, d_out, cap, out_bytes, s);
    });
}

int ansx_encode_batch_gaps_dev(ansx_ctx* c, int kind, int f, const uint32_t* d_in, const uint64_t* offsets, size_t count,
    uint8_t* d_out, size_t out_capacity, uint64_t* out_offsets, uint64_t* out_bytes, size_t* total_bytes, size_t* bad_index,
    const ansx_opts* opts, void* stream)
{
    // (every argument check comes before the context is touched)
    Plan P0;
    int rc = encode_batch_args(c, kind, f, d_in, offsets, count, d_out, bad_index, opts, &P0);
    if (rc) return rc;
    if (count == 0) return empty_batch(out_offsets, total_bytes);
    return run_call(c, stream, [&](hipStream_t s) -> int {
        const u32* gaps = nullptr;
        if ((rc = gaps_run(c, d_in + offsets[0], offsets[count] - offsets[0], (const u64*)offsets, count, &gaps, bad_index, s)))
            return rc;
        std::vector<u64> off(count + 1);  // the lists' places in the workspace
        for (size_t i = 0; i <= count; i++) off[i] = offsets[i] - offsets[0];
        return encode_batch(c, P0, opts, gaps, off.data(), count, d_out, out_capacity, (u64*)out_offsets, (u64*)out_bytes,
            total_bytes, bad_index, s);
    });
}

int ansx_encode_batch_gaps_bases_dev(ansx_ctx* c, int kind, int f, const uint32_t* d_in, const uint64_t* offsets, size_t count,
    uint8_t* d_out, size_t out_capacity, uint64_t* out_offsets, uint64_t* out_bytes, size_t* total_bytes, size_t* bad_index,
    const ansx_opts* opts, uint32_t* d_bases, size_t bases_capacity, uint64_t* base_offsets, size_t* total_bases, void* stream)
{
    // (every argument check comes before the context is touched)
    Plan P0;
    int rc = encode_batch_args(c, kind, f, d_in, offsets, count, d_out, bad_index, opts, &P0);
    if (rc) return rc;
    if (((uintptr_t)d_bases & 3u) || (!d_bases && bases_capacity > 0)) return ANSX_ERR_ARG;
    // where every list's bases start: a pure function of the offsets and the options
    // (a size query allocates nothing: the caller's array, if any, takes them)
    const u64 bi = P0.g.block_ints;
    auto bases_offsets = [&](u64* boff) {
        u64 nb = 0;
        for (size_t i = 0; i < count; i++) {
            if (boff) boff[i] = nb;
            nb += (offsets[i + 1] - offsets[i] + bi - 1) / bi + 1;
        }
        if (boff) boff[count] = nb;
        return nb;
    };
    const u64 nbases = bases_offsets((u64*)base_offsets);
    if (total_bases) *total_bases = (size_t)nbases;
    if (bases_capacity < nbases) return ANSX_ERR_CAPACITY;
    if (count == 0) return empty_batch(out_offsets, total_bytes);
    return run_call(c, stream, [&](hipStream_t s) -> int {
        std::vector<u64> boff(count + 1);
        bases_offsets(boff.data());
        const u32* gaps = nullptr;
        GapsSide G = { boff.data(), nullptr, nullptr };
        if ((rc = gaps_run(c, d_in + offsets[0], offsets[count] - offsets[0], (const u64*)offsets, count, &gaps, bad_index, s, &G)))
            return rc;
        // the ids do not decrease: the id in front of a block is the sum of every gap of its list in front of it
        LAUNCH(c, "k_rs_batch_ids_bases", k_rs_batch_ids_bases, (u32)((nbases + ANSX_RS_NT - 1) / ANSX_RS_NT), ANSX_RS_NT, 0, s,
            d_in + offsets[0], G.d_offs, G.d_side, (u32)count, (u32)bi, nbases, d_bases);
        std::vector<u64> off(count + 1);  // the lists' places in the workspace
        for (size_t i = 0; i <= count; i++) off[i] = offsets[i] - offsets[0];
        return encode_batch(c, P0, opts, gaps, off.data(), count, d_out, out_capacity, (u64*)out_offsets, (u64*)out_bytes,
            total_bytes, bad_index, s);
    });
}

int ansx_encode(ansx_ctx* c, int kind, int f, const uint32_t* in, size_t n, uint8_t* out, size_t cap,
    size_t* out_bytes, const ansx_opts* opts)
{
    if (!c || !in || !out || !out_bytes) return ANSX_ERR_ARG;
    Plan P;
    int rc = make_plan(kind, f, n, opts, &P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    size_t bound = ansx_bound(kind, f, n, opts);
    size_t dcap = cap < bound ? cap : bound;
    if ((rc = ensure(c, c->stage_in, n * 4 + 16))) return rc;
    if ((rc = ensure(c, c->stage_out, dcap + 64))) return rc;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->stage_in.p, in, n * 4, hipMemcpyHostToDevice, s));
    size_t nb = 0;
    rc = encode_dev(c, P, (const u32*)c->stage_in.p, (u8*)c->stage_out.p, dcap, &nb, s);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->stage_out.p, nb, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *out_bytes = nb;
    return ANSX_OK;
}

int ansx_decode(ansx_ctx* c, int kind, int f, const uint8_t* in, size_t in_bytes, uint32_t* out,
    size_t n, const ansx_opts* opts)
{
    if (!c || !in || !out) return ANSX_ERR_ARG;
    Plan P;
    int rc = make_plan(kind, f, n, opts, &P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->stage_out, in_bytes + 64))) return rc;
    if ((rc = ensure(c, c->stage_in, n * 4 + 16))) return rc;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->stage_out.p, in, in_bytes, hipMemcpyHostToDevice, s));
    rc = decode_dev(c, P, (const u8*)c->stage_out.p, in_bytes, (u32*)c->stage_in.p, s);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->stage_in.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ANSX_OK;
}

int ansx_merge_containers_dev(ansx_ctx* c, const uint8_t* const* d_parts, const size_t* part_bytes, int nparts,
    uint8_t* d_out, size_t cap, size_t* out_bytes, void* stream)
{
    if (!c || !d_parts || !part_bytes || !d_out || !out_bytes || nparts < 1 || nparts > ANSX_MERGE_MAX_PARTS) return ANSX_ERR_ARG;
    if ((uintptr_t)d_out & 15u) return ANSX_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // the part headers decide the layout: one small read-back
    u8* hp = c->pin->part_hdr[0];
    std::vector<ansx_container_header> H((size_t)nparts);
    for (int i = 0; i < nparts; i += 63) {
        const int m = std::min(63, nparts - i);
        for (int j = 0; j < m; j++) {
            if (!d_parts[i + j] || ((uintptr_t)d_parts[i + j] & 7u) || part_bytes[i + j] < sizeof(ansx_container_header)) return ANSX_ERR_ARG;
            HIPCHK(c, hipMemcpyAsync(hp + 64 * j, d_parts[i + j], 64, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(c, hipStreamSynchronize(s));
        for (int j = 0; j < m; j++) {
            int rc = parse_header(hp + 64 * j, part_bytes[i + j], &H[(size_t)(i + j)]);
            if (rc) return rc;
        }
    }
    ansx_merge_desc D;
    memset(&D, 0, sizeof(D));
    u64 nblocks = 0, n = 0, pay = 0;
    u32 maxlg = 0, maxns = 0;
    for (int i = 0; i < nparts; i++) {
        const ansx_container_header& h = H[(size_t)i];
        if (h.kind != H[0].kind || h.fidelity != H[0].fidelity || h.block_ints != H[0].block_ints
            || h.ckpt_interval != H[0].ckpt_interval || h.ckpts_per_block != H[0].ckpts_per_block)
            return ANSX_ERR_FORMAT;
        if (i + 1 < nparts && h.n % h.block_ints != 0) return ANSX_ERR_FORMAT;  // only the last part may end in a partial block
        if (h.payload_offset > part_bytes[i] || h.payload_bytes > part_bytes[i] - h.payload_offset) return ANSX_ERR_FORMAT;
        if (h.payload_offset > 0xFFFFFFFFull) return ANSX_ERR_FORMAT;
        // the kernel derives every section of a part from its header's nblocks: the header must describe exactly the
        // layout its own geometry implies (as decode_dev checks), or a crafted part could send the copy past its buffer
        {
            if (h.n == 0 || h.block_ints == 0 || h.block_ints == ANSX_SINGLE_STREAM) return ANSX_ERR_FORMAT;
            ansx_opts po = { h.block_ints, h.ckpt_interval ? h.ckpt_interval : ANSX_NO_CHECKPOINTS,
                (h.kind & 0x100u) ? (u32)ANSX_FLAG_COMPACT_ALPHABET : 0u, 0 };
            Plan PP;
            if (make_plan((int)(h.kind & 0xFFu), (int)h.fidelity, (size_t)h.n, &po, &PP)) return ANSX_ERR_FORMAT;
            set_restart_format(&PP, (h.kind & ANSX_KIND_WIDE_RESTART) != 0);
            if (PP.g.nblocks != h.nblocks || PP.g.nckf != h.ckpts_per_block || PP.lay.payload_off != h.payload_offset) return ANSX_ERR_FORMAT;
        }
        D.part[i].src = d_parts[i];
        D.part[i].first_block = nblocks;
        D.part[i].pay_base = pay;
        D.part[i].payload_bytes = h.payload_bytes;
        D.part[i].nblocks = h.nblocks;
        D.part[i].payload_off = (u32)h.payload_offset;
        nblocks += h.nblocks;
        n += h.n;
        pay += h.payload_bytes;
        maxlg = std::max(maxlg, h.max_log2_frame);
        maxns = std::max(maxns, h.max_nsyms);
    }
    if (nblocks > 0x7FFFFFFFull) return ANSX_ERR_ARG;
    // (bit 8 of the kind word: per-block alphabet compaction -- a flag of the plan, kept in the merged header)
    ansx_opts o = { H[0].block_ints, H[0].ckpt_interval ? H[0].ckpt_interval : ANSX_NO_CHECKPOINTS,
        (H[0].kind & 0x100u) ? (u32)ANSX_FLAG_COMPACT_ALPHABET : 0u, 0 };
    Plan P;
    if (make_plan((int)(H[0].kind & 0xFFu), (int)H[0].fidelity, (size_t)n, &o, &P)) return ANSX_ERR_FORMAT;
    // (bit 9: the restart-point format.  The parts agree on it -- their kind words are equal -- and the result keeps it;
    // a part that needed wide restart points next to parts that did not is refused: re-encode those with ANSX_WIDE_RESTART)
    set_restart_format(&P, (H[0].kind & ANSX_KIND_WIDE_RESTART) != 0);
    if (P.g.nblocks != nblocks || P.g.nckf != H[0].ckpts_per_block) return ANSX_ERR_FORMAT;
    const u64 total = P.lay.payload_off + pay;
    if (total > cap) return ANSX_ERR_CAPACITY;
    D.nparts = (u32)nparts;
    D.nckf = P.g.nckf;
    D.ckw = P.g.ckw;
    D.ckoff_off = P.lay.ckoff_off;
    D.ckstate_off = P.lay.ckstate_off;
    D.hint_off = P.lay.hint_off;
    D.payload_off = P.lay.payload_off;
    // header, final index entry, alignment padding: written from the host image
    HIPCHK(c, hipMemsetAsync(d_out, 0, (size_t)P.lay.payload_off, s));
    ansx_container_header M = H[0];
    M.n = n;
    M.nblocks = (u32)nblocks;
    M.max_log2_frame = maxlg;
    M.max_nsyms = maxns;
    {
        u32 mp = 0;
        for (int i = 0; i < nparts; i++) mp = std::max<u32>(mp, H[(size_t)i].max_present_m1);
        M.max_present_m1 = (u16)mp;
    }
    M.payload_bytes = pay;
    M.payload_offset = P.lay.payload_off;
    memcpy(hp, &M, 64);
    memcpy(hp + 64, &pay, 8);
    HIPCHK(c, hipMemcpyAsync(d_out, hp, 64, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_out + 64 + 8 * nblocks, hp + 64, 8, hipMemcpyHostToDevice, s));
    u64 max_pieces = 1;
    for (int i = 0; i < nparts; i++) {
        const u64 nb_ = D.part[i].nblocks;
        const u64 cko_unit = D.ckw ? 4 : ANSX_CK_RECORD, cks_unit = D.ckw ? 32 : 0;  // (as k_merge_containers walks them)
        const u64 pieces = (8 * nb_ + 65535) / 65536 + (cko_unit * nb_ * D.nckf + 65535) / 65536 + (cks_unit * nb_ * D.nckf + 65535) / 65536
            + (32 * nb_ + 65535) / 65536 + (D.part[i].payload_bytes + 65535) / 65536;
        max_pieces = std::max(max_pieces, pieces);
    }
    prof_begin(c, "k_merge_containers", s);
    hipLaunchKernelGGL(k_merge_containers, dim3((u32)max_pieces, (u32)nparts), dim3(256), 0, s, D, d_out);
    prof_end(c, s);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));  // hp is reused by the next call
    *out_bytes = (size_t)total;
    return ANSX_OK;
}

// ---------------------------------------------------------------------------------------------
// Multi-GPU gather over RCCL: ncclAllGather of the container sizes, then one grouped
// ncclSend / ncclRecv round -- every rank straight to the root, each over its own xGMI link -- and the merge
// kernel on the root.  librccl is not a link-time dependency of this library: the five entry points are
// resolved with dlopen at first use (a caller that holds an ncclComm_t has the library loaded already).
int ansx_gather_containers(ansx_ctx* c, void* nccl_comm, int rank, int nranks, int root, const uint8_t* d_container,
    size_t bytes, uint8_t* d_recv, size_t slot_bytes, uint8_t* d_merged, size_t merged_cap, size_t* merged_bytes,
    void* stream)
{
    if (!c || !nccl_comm || !d_container || !merged_bytes || nranks < 1 || nranks > ANSX_MERGE_MAX_PARTS || rank < 0
        || rank >= nranks || root < 0 || root >= nranks || bytes < sizeof(ansx_container_header))
        return ANSX_ERR_ARG;
    if (rank == root && (!d_recv || !d_merged || (slot_bytes & 15u) || ((uintptr_t)d_recv & 15u))) return ANSX_ERR_ARG;
    const RcclApi& R = rccl_api();
    if (!R.ok) return ANSX_ERR_NO_DEVICE;  // no RCCL library on this system
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    ncclComm_t comm = (ncclComm_t)nccl_comm;
    *merged_bytes = 0;
    // 1. sizes of all rank containers AND every rank's idea of slot_bytes, everywhere: the capacity check below uses the
    //    ROOT's slot_bytes on every rank, so that all ranks take the same branch (a rank that returned early on its own
    //    value would leave the root waiting in its ncclRecv)
    int rc;
    if ((rc = ensure(c, c->misc, 64 + 8 * (3 * (size_t)ANSX_MERGE_MAX_PARTS + 2)))) return rc;
    u64* d_sizes = (u64*)((u8*)c->misc.p + 64);
    u64* h_sizes = c->pin->rank_sizes;
    const u64 mine[2] = { (u64)bytes, (u64)slot_bytes };
    HIPCHK(c, hipMemcpyAsync(d_sizes + 2 * ANSX_MERGE_MAX_PARTS, mine, 16, hipMemcpyHostToDevice, s));
    if (R.AllGather(d_sizes + 2 * ANSX_MERGE_MAX_PARTS, d_sizes, 2, ncclUint64, comm, s) != ncclSuccess) return ANSX_ERR_HIP;
    HIPCHK(c, hipMemcpyAsync(h_sizes, d_sizes, 16 * (size_t)nranks, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    int comm_ranks = 0;
    if (R.CommCount && R.CommCount(comm, &comm_ranks) == ncclSuccess) c->last_gather_ranks = comm_ranks;
    const u64 root_slot = h_sizes[2 * root + 1];
    std::vector<size_t> sizes((size_t)nranks);
    for (int r = 0; r < nranks; r++) {
        sizes[(size_t)r] = (size_t)h_sizes[2 * r];
        if (h_sizes[2 * r] > root_slot || h_sizes[2 * r] < sizeof(ansx_container_header)) return ANSX_ERR_CAPACITY;
    }
    // 2. every rank's container into its slot on the root
    if (R.GroupStart() != ncclSuccess) return ANSX_ERR_HIP;
    bool bad = false;
    if (rank == root) {
        for (int r = 0; r < nranks; r++)
            if (r != root) bad |= R.Recv(d_recv + (size_t)r * slot_bytes, sizes[(size_t)r], ncclUint8, r, comm, s) != ncclSuccess;
    } else {
        bad |= R.Send(d_container, bytes, ncclUint8, root, comm, s) != ncclSuccess;
    }
    if (R.GroupEnd() != ncclSuccess || bad) return ANSX_ERR_HIP;
    if (rank != root) return ANSX_OK;
    HIPCHK(c, hipMemcpyAsync(d_recv + (size_t)root * slot_bytes, d_container, bytes, hipMemcpyDeviceToDevice, s));
    // 3. one container
    std::vector<const uint8_t*> parts((size_t)nranks);
    for (int r = 0; r < nranks; r++) parts[(size_t)r] = d_recv + (size_t)r * slot_bytes;
    return ansx_merge_containers_dev(c, parts.data(), sizes.data(), nranks, d_merged, merged_cap, merged_bytes, s);
}

int ansx_last_gather_ranks(const ansx_ctx* c) { return c ? c->last_gather_ranks : 0; }

int ansx_container_info(const uint8_t* container, size_t bytes, ansx_container_header* out)
{
    if (!container || !out) return ANSX_ERR_ARG;
    return parse_header(container, bytes, out);
}

int ansx_profile_enable(ansx_ctx* c, int on)
{
    if (!c) return ANSX_ERR_ARG;
    c->profile = on != 0;
    return ANSX_OK;
}

static void prof_collect(ansx_ctx* c)
{
    for (auto& r : c->recs) {
        float ms = 0.f;
        (void)hipEventSynchronize(r.e1);
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        auto it = c->acc.find(r.name);
        if (it == c->acc.end()) {
            c->order.push_back(r.name);
            c->acc[r.name] = std::make_pair((double)ms, (u64)1);
        } else {
            it->second.first += ms;
            it->second.second += 1;
        }
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    c->recs.clear();
}

int ansx_profile_reset(ansx_ctx* c)
{
    if (!c) return ANSX_ERR_ARG;
    prof_collect(c);
    c->acc.clear();
    c->order.clear();
    return ANSX_OK;
}

int ansx_profile_get(ansx_ctx* c, ansx_kernel_time* out, int max_entries, int* count)
{
    if (!c || !count) return ANSX_ERR_ARG;
    prof_collect(c);
    int k = 0;
    for (auto& name : c->order) {
        if (out && k < max_entries) {
            memset(&out[k], 0, sizeof(out[k]));
            strncpy(out[k].name, name.c_str(), sizeof(out[k].name) - 1);
            out[k].total_ms = c->acc[name].first;
            out[k].launches = c->acc[name].second;
        }
        k++;
    }
    *count = k;
    return ANSX_OK;
}

size_t ansx_workspace_bytes(const ansx_ctx* c)
{
    if (!c) return 0;
    const DevBuf* bufs[] = { &c->pre_work, &c->hist, &c->hterm, &c->sortF, &c->sortSym, &c->attS, &c->prevS, &c->attMeta, &c->blk,
        &c->table, &c->tab32, &c->scratch, &c->misc, &c->mapped, &c->mostfreq, &c->stage_in, &c->stage_out,
        &c->dec_s2s, &c->dec_cum, &c->dec_info, &c->plain, &c->rf_tmp, &c->pa_alpha, &c->pa_info, &c->pairs, &c->sizes,
        &c->rng_plan, &c->rng_cont, &c->rng_list, &c->rng_dev, &c->bat_hdr, &c->enb_plan, &c->enb_wc, &c->sums_plan, &c->sums_ints, &c->isect_ids, &c->isectb_ids, &c->isectb_work };
    size_t t = 0;
    for (const DevBuf* b : bufs) t += b->cap;
    return t;
}

double ansx_host_log2(double x) { return ansx_log2_portable(x); }

static int gen_setup(int dist, double a, double b, uint64_t seed, ansx_gen_params* P)
{
    if (dist == ANSX_GEN_UNIFORM) {
        if (!(a >= 0.0 && a <= b && b <= 4294967295.0) || a != __builtin_floor(a) || b != __builtin_floor(b)) return ANSX_ERR_ARG;
    } else if (dist == ANSX_GEN_GEOMETRIC) {
        if (!(a > 0.0 && a < 1.0)) return ANSX_ERR_ARG;
    } else if (dist == ANSX_GEN_ZIPF) {
        if (!(a >= 1.0 && a <= 1073741823.0 && b > 0.0 && b < 64.0) || a != __builtin_floor(a)) return ANSX_ERR_ARG;
    } else return ANSX_ERR_ARG;
    P->dist = (u32)dist;
    P->seed = seed;
    P->a = a;
    P->b = b;
    gen_prepare(P);
    return ANSX_OK;
}

int ansx_generate_dev(ansx_ctx* c, int dist, double a, double b, uint64_t seed, uint64_t first_index,
    uint32_t* d_out, size_t n, void* stream)
{
    if (!c || !d_out || n == 0) return ANSX_ERR_ARG;
    ansx_gen_params P;
    int rc = gen_setup(dist, a, b, seed, &P);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    LAUNCH(c, "k_generate", k_generate, (n + 255) / 256, 256, 0, s, P, d_out, (u64)n, (u64)first_index);
    return ANSX_OK;
}

int ansx_generate_host(int dist, double a, double b, uint64_t seed, uint64_t first_index, uint32_t* out, size_t n)
{
    if (!out || n == 0) return ANSX_ERR_ARG;
    ansx_gen_params P;
    int rc = gen_setup(dist, a, b, seed, &P);
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) out[i] = gen_value(P, first_index + i);
    return ANSX_OK;
}

int ansx_zipf_from_uniform(double n, double q, double u01, uint32_t* k, int* accepted)
{
    if (!k || !accepted || !(u01 >= 0.0 && u01 <= 1.0)) return ANSX_ERR_ARG;
    ansx_gen_params P;
    int rc = gen_setup(ANSX_GEN_ZIPF, n, q, 0, &P);
    if (rc) return rc;
    *accepted = gen_zipf_try(P, u01, k) ? 1 : 0;
    return ANSX_OK;
}

int ansx_selftest_log2(ansx_ctx* c, const double* in, double* out, size_t n)
{
    if (!c || !in || !out || n == 0) return ANSX_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->stage_in, n * 8))) return rc;
    if ((rc = ensure(c, c->stage_out, n * 8))) return rc;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->stage_in.p, in, n * 8, hipMemcpyHostToDevice, s));
    LAUNCH(c, "k_selftest_log2", k_selftest_log2, (n + 255) / 256, 256, 0, s, (const double*)c->stage_in.p,
        (double*)c->stage_out.p, (u64)n);
    HIPCHK(c, hipMemcpyAsync(out, c->stage_out.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ANSX_OK;
}

int ansx_selftest_div(ansx_ctx* c, const double* a, const double* b, double* out, size_t n)
{
    if (!c || !a || !b || !out || n == 0) return ANSX_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->stage_in, 2 * n * 8))) return rc;
    if ((rc = ensure(c, c->stage_out, n * 8))) return rc;
    hipStream_t s = c->stream;
    double* da = (double*)c->stage_in.p;
    HIPCHK(c, hipMemcpyAsync(da, a, n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(da + n, b, n * 8, hipMemcpyHostToDevice, s));
    LAUNCH(c, "k_selftest_div", k_selftest_div, (n + 255) / 256, 256, 0, s, (const double*)da,
        (const double*)(da + n), (double*)c->stage_out.p, (u64)n);
    HIPCHK(c, hipMemcpyAsync(out, c->stage_out.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ANSX_OK;
}

}  // extern "C"
