/*
 * ansx — MI355X-native ANSfold / ANSrfold codec: C-ABI boundary.
 *
 * This is the drop-in boundary for ONE hot path of mpetri/ans-large-alphabet: the
 * ANSfold<f> / ANSrfold<f> encode()/decode() pair.  Plain pointers and sizes only, so any host
 * language can bind it (the reference is header-only C++17 and has no FFI; the C++ mirror with
 * the reference's exact static signatures is ans_large_alphabet_amd/include/ansx_methods.hpp).
 *
 * What each entry point replaces in the reference (paths relative to /root/reference):
 *
 *   ansx_encode / ansx_encode_dev   ANSfold<f>::encode   include/methods.hpp:535-540
 *                                   -> ans_fold_compress<f>           include/ans_fold.hpp:238-281
 *                                   ANSrfold<f>::encode  include/methods.hpp:555-560
 *                                   -> ans_reorder_fold_compress<f>   include/ans_reorder_fold.hpp:312-355
 *   ansx_decode / ansx_decode_dev   ANSfold<f>::decode   include/methods.hpp:541-546
 *                                   -> ans_fold_decompress<f>         include/ans_fold.hpp:283-311
 *                                   ANSrfold<f>::decode  include/methods.hpp:561-566
 *                                   -> ans_reorder_fold_decompress<f> include/ans_reorder_fold.hpp:357-385
 *   ansx_bound                      the harness's "n*8 bytes" output sizing, src/table_efficiency.cpp:73-74
 *                                   (the reference never checks dstCapacity, ans_fold.hpp:239-240)
 *   ansx_codec_name                 ANSfold<f>::name / ANSrfold<f>::name  include/methods.hpp:530-533,550-553
 *
 * Output format.  A reference encode() call is 4 serial rANS chains, so device
 * parallelism comes from independent blocks.  With opts.block_ints != ANSX_SINGLE_STREAM the
 * output is a *container*: a 64-byte header, a block index, decoder restart points, then the
 * concatenation of one UNMODIFIED reference stream per block — each block's bytes are
 * identical to what ANSfold<f>::encode(block) / ANSrfold<f>::encode(block) writes (modulo the
 * reference's own indeterminate padding bits, SURVEY F2, which are written as zero).
 * With opts.block_ints == ANSX_SINGLE_STREAM the output is exactly one reference stream for the
 * whole list (no header); ansx_decode with the same option accepts streams produced by the
 * reference CPU encoder.  Container layout: see DESIGN.md section 3 and ansx_container_header.
 *
 * Errors: the reference has none on this path (malformed input is UB, capacity is unchecked);
 * every function here returns an ansx_status instead.  n == 0 is an error (the reference never
 * terminates on it); values must be < 2^30 (rfold: value + 2^(f+7) < 2^30), the
 * reference's own decode limit (ans_fold.hpp:198-200).
 *
 * Threading: a context is bound to one device and must not be used from two host threads at
 * once; distinct contexts are independent (the reference codec is stateless and re-entrant).
 */
#ifndef ANSX_H
#define ANSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ansx_ctx ansx_ctx;

typedef enum {
    ANSX_FOLD = 0,  /* ANSfold<f>  */
    ANSX_RFOLD = 1, /* ANSrfold<f> */
    ANSX_MSB = 2,   /* ANSmsb (include/methods.hpp:499-515 -> include/ans_msb.hpp); fidelity must be 0 */
    ANSX_INT = 3    /* ANSint, name() == "ANS" (include/methods.hpp:484-497 -> include/ans_int.hpp); fidelity must be 0.
                       Its model spans every value up to the largest (ans_int.hpp:41-51).  Plain: any values below 2^30,
                       block container or ANSX_SINGLE_STREAM (= the bytes of ans_int_compress).  Lists whose values
                       stay below 16384 use a dense model; beyond that every block is modelled over its distinct
                       values (ranks) and only its prelude ranges over the values -- the same bytes -- which takes
                       blocks (single-stream: lists) of any length with at most 16384 DISTINCT values each:
                       ANSX_ERR_DOMAIN otherwise, and for a block
                       whose prelude would exceed 64 KiB (about 32 bits per distinct value).  A plain-ANSint
                       container carries no parse hints and its max_nsyms bounds a block's DISTINCT values, so its bytes
                       do not tell which of the two models wrote it.  With ANSX_FLAG_COMPACT_ALPHABET: the
                       harness's own layout, a block's dense ranks behind an alphabet header.  32-bit frequencies:
                       frames up to 2^27 (beyond, the reference's own 64-bit bound overflows) */
} ansx_kind;

typedef enum {
    ANSX_OK = 0,
    ANSX_ERR_ARG = 1,       /* bad kind / fidelity / n == 0 / null pointer / bad options      */
    ANSX_ERR_CAPACITY = 2,  /* output buffer too small (see ansx_bound)                        */
    ANSX_ERR_FORMAT = 3,    /* container/stream failed validation                              */
    ANSX_ERR_HIP = 4,       /* a HIP runtime call failed (ansx_last_hip_error has the code)    */
    ANSX_ERR_NO_DEVICE = 5, /* no usable gfx950 device                                         */
    ANSX_ERR_DOMAIN = 6,    /* an input value is outside the reference's decodable domain      */
    ANSX_ERR_MODEL = 7      /* normalisation hit the reference's degenerate exit   */
} ansx_status;

#define ANSX_SINGLE_STREAM 0xFFFFFFFFu /* opts.block_ints: one plain reference stream          */
#define ANSX_NO_CHECKPOINTS 0xFFFFFFFFu /* opts.ckpt_interval: no decoder restart points        */
/* Largest fidelity accepted.  The reference instantiates ANSfold<1..8> (methods.hpp:529-567) but is only
 * sound up to 7 (rfold<8> truncates symbols to u16, fold<8> can hit the u16 bail-out).  f <= 5
 * (up to 16384 symbol slots) keeps a block's model in a CU's LDS; f = 6, 7 (32 Ki / 64 Ki slots) run the same
 * stages with their per-block arrays in HBM -- correct and bit-identical, not tuned.  f = 8: ANSX_ERR_ARG. */
#define ANSX_MAX_FIDELITY 7
#define ANSX_DEFAULT_BLOCK_INTS 16384u
#define ANSX_DEFAULT_CKPT_INTERVAL 1024u

/* opts.flags.  ANSX_FLAG_COMPACT_ALPHABET: per-block alphabet compaction, the scheme of the reference's
 * src/pseudo_adaptive.cpp:85-130 -- every block is stored as u32 sigma | u32 universe | interpolative code of
 * the running sums of its sigma distinct values | the codec's stream of the block with each value replaced
 * by its 1-based rank among them (nothing when sigma == 1): byte for byte what that harness writes for the
 * block (it only measures sizes; decoding is this library's own).  For ANSX_FOLD, ANSX_MSB, ANSX_INT; blocks
 * of at most 16384 ints (ANSX_INT: 16380, default 8192); the sum of a block's distinct values must stay
 * below 2^32 - 1, as in the harness (ANSX_ERR_DOMAIN). */
#define ANSX_FLAG_COMPACT_ALPHABET 1u

typedef struct {
    uint32_t block_ints;    /* ints per independent reference stream (a multiple of 4); 0 = default.  A block's
                               worst-case stream, hdr + 8 + 4 NSP + 7 block_ints + 32 bytes (DESIGN.md section 3;
                               + 16), must stay below 2^31: block indices, stream sizes and restart cursors are
                               32-bit and the decoders refuse a longer block stream.  That is block_ints below
                               about 306.7 million for the fold codecs (ANSX_SINGLE_STREAM: n); beyond it ANSX_ERR_ARG
                               and ansx_bound() == 0 */
    uint32_t ckpt_interval; /* ints between decoder restart points (multiple of 4); 0 = default */
    uint32_t flags;         /* ANSX_FLAG_* bits                                                */
    uint32_t reserved;
} ansx_opts;

/* 64-byte container header (little endian), see DESIGN.md section 3. */
typedef struct {
    uint8_t magic[6];       /* "ANSXv3"                                                         */
    uint16_t max_present_m1; /* (max over blocks of the symbols PRESENT in the block) - 1: sizes the
                               decoder's per-present-symbol table (<= max_nsyms - 1; untrusted
                               like every other field: a block with more is a format error)     */
    uint32_t kind;          /* ansx_kind | 0x100 if ANSX_FLAG_COMPACT_ALPHABET | 0x200 if the restart
                               points are in the wide form (u32 cursor + 4 x u64 states: ANSint, frames
                               above 2^16, block_ints whose worst-case block stream + 16 reaches 2^24
                               bytes) instead of packed 29-byte records (4 x 52-bit states + 24-bit cursor) */
    uint32_t fidelity;
    uint64_t n;             /* total ints                                                       */
    uint32_t block_ints;
    uint32_t ckpt_interval; /* 0 = none                                                         */
    uint32_t nblocks;
    uint32_t max_log2_frame; /* max over blocks of log2(M)                                      */
    uint32_t max_nsyms;      /* max over blocks of max_sym + 1                                  */
    uint32_t ckpts_per_block; /* restart points stored per block (fixed stride)                 */
    uint64_t payload_bytes;  /* sum of block stream sizes                                       */
    uint64_t payload_offset; /* byte offset of the first block stream                           */
} ansx_container_header;

typedef struct {
    char name[48];
    double total_ms;
    uint64_t launches;
} ansx_kernel_time;

/* Context: one per (process, device).  device < 0 -> current device. */
int ansx_init(int device, ansx_ctx** ctx);
void ansx_destroy(ansx_ctx* ctx);

const char* ansx_strerror(int status);
int ansx_last_hip_error(const ansx_ctx* ctx);
/* "ANSfold-<f>" / "ANSrfold-<f>" (methods.hpp:530-533,550-553); returns chars written. */
int ansx_codec_name(int kind, int fidelity, char* buf, size_t buflen);

/* Worst-case output bytes for n ints with these options (>= any actual output). */
size_t ansx_bound(int kind, int fidelity, size_t n, const ansx_opts* opts);

/* Host-buffer entry points (H2D + device path + D2H). */
int ansx_encode(ansx_ctx* ctx, int kind, int fidelity, const uint32_t* in, size_t n, uint8_t* out,
    size_t out_capacity, size_t* out_bytes, const ansx_opts* opts);
int ansx_decode(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* in, size_t in_bytes,
    uint32_t* out, size_t n, const ansx_opts* opts);

/* Device-pointer entry points: in/out are HBM resident; `stream` is a hipStream_t (NULL = the
 * context's own stream, an ordinary blocking stream: it orders implicitly against work on the legacy
 * default stream -- e.g. PyTorch's default stream, whose handle is 0 -- but NOT against other
 * non-blocking streams; pass the stream the input was produced on if there is one).  They return
 * after the result size / status has been read back. */
int ansx_encode_dev(ansx_ctx* ctx, int kind, int fidelity, const uint32_t* d_in, size_t n,
    uint8_t* d_out, size_t out_capacity, size_t* out_bytes, const ansx_opts* opts, void* stream);
int ansx_decode_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes,
    uint32_t* d_out, size_t n, const ansx_opts* opts, void* stream);

/* Random access: decode `nranges` ranges [first[i], first[i] + count[i]) of the list held in a CONTAINER (not a
 * single-stream reference stream) without decoding the blocks no range touches.  first / count are HOST arrays;
 * d_in (16-byte aligned) and d_out (4-byte aligned) are device memory.  Range i is written to
 * d_out[sum_{j<i} count[j] ...]; ranges may overlap, repeat, be unsorted, or have count 0.  The output is
 * bit-identical to concatenating full[first[i] : first[i] + count[i]], where full is what ansx_decode_dev returns for
 * the same container.  Every container form the library writes is accepted (any codec, compaction, either
 * restart-point format, no restart points, any block_ints, merged containers); the container's header defines n.
 * Errors: ANSX_ERR_ARG for a null ctx / d_in / d_out, a null first or count with nranges > 0, a misaligned pointer,
 * or any first[i] + count[i] > n (checked on the host against the header, before anything is launched);
 * ANSX_ERR_CAPACITY when sum(count) > out_capacity_ints; ANSX_ERR_FORMAT when kind / fidelity differ from the header,
 * the input is not a container, or an index entry of a touched block is invalid.  nranges == 0 or all counts 0:
 * ANSX_OK with nothing launched.
 * Selectivity: of an untouched block nothing is read -- stream, restart points, parse hints, index entries -- and no
 * kernel's grid grows with the container's block count: the touched blocks are copied into a workspace container
 * (header + their index entries, rebased), which the ordinary decode path decodes, and the ranges are gathered from
 * it.  The call leaves no trace in the context that later ansx_decode_dev / ansx_encode_dev calls would see (no
 * remembered header, no per-geometry hint).  Returns after the status has been read back, like ansx_decode_dev. */
int ansx_decode_ranges_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes,
    const uint64_t* first, const uint32_t* count, size_t nranges, uint32_t* d_out, size_t out_capacity_ints,
    void* stream);

/* Random access with the ranges in DEVICE memory: as ansx_decode_ranges_dev, except that d_first (8-byte aligned) and
 * d_count (4-byte aligned) are device arrays, read on `stream` (a kernel that wrote them earlier on that stream is
 * ordered before), and the plan -- touched blocks, range positions -- is built on the device: no copy of O(nranges)
 * bytes in either direction.  Output, selectivity, the accepted forms and the promise to leave no trace in the context
 * are those of ansx_decode_ranges_dev; no kernel's grid grows with the container's block count (grids scale with
 * nranges or with the number of touched blocks).
 * d_offsets (optional, 8-byte aligned device array of nranges + 1 u64): the exclusive prefix sum of count -- where
 * range i starts in d_out -- and the total; written on ANSX_OK and ANSX_ERR_CAPACITY, unspecified after other errors.
 * *total_ints (optional, host): sum(count), set on ANSX_OK and ANSX_ERR_CAPACITY (the size of a retry).
 * Errors decided on the host, before anything is launched: ANSX_ERR_ARG for a null ctx / d_in / d_out, a null d_first
 * or d_count with nranges > 0, a misaligned pointer (d_in 16, d_out 4, d_first 8, d_count 4, d_offsets 8 bytes), or
 * nranges > UINT32_MAX; ANSX_ERR_FORMAT as for ansx_decode_ranges_dev (kind / fidelity differ from the header, not a
 * container).  nranges == 0: ANSX_OK, *total_ints = 0, nothing launched.
 * Errors decided on the device, read back before any byte of d_out is written: ANSX_ERR_ARG if any
 * first[i] + count[i] > n, ANSX_ERR_CAPACITY if sum(count) > out_capacity_ints (ANSX_ERR_ARG wins when both hold);
 * ANSX_ERR_FORMAT for an invalid index entry of a touched block.  Returns after the status has been read back. */
int ansx_decode_device_ranges_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes,
    const uint64_t* d_first, const uint32_t* d_count, size_t nranges, uint32_t* d_out, size_t out_capacity_ints,
    uint64_t* d_offsets, uint64_t* total_ints, void* stream);

/* A batch of containers in one call (posting lists, column chunks: one container per term or chunk).  d_ins[i]
 * (16-byte aligned DEVICE pointers, HOST array) are `count` containers of the codec (kind, fidelity), in_bytes[i]
 * bounding each; container i decodes to d_out[offsets[i] .. offsets[i] + n_i), n_i from its own header, in batch order
 * and back to back -- bit-identical to ansx_decode_dev on each in turn, outputs concatenated.  Every container form
 * ansx_decode_dev reads is accepted, and the containers may differ in geometry (block_ints, ckpt_interval, compaction,
 * restart-point format); the same pointer may appear more than once, in any order.  d_out: 4-byte aligned.
 * offsets (optional, HOST array of count + 1): the exclusive prefix sums of the n_i, and the total; *total_ints
 * (optional): sum(n_i).  Both are written on ANSX_OK and ANSX_ERR_CAPACITY, so d_out = NULL, out_capacity_ints = 0
 * is a size query.
 * Errors decided before the context is touched: ANSX_ERR_ARG for a null ctx, a null d_ins or in_bytes with count > 0,
 * a null d_ins[i], a misaligned pointer, d_out == NULL with out_capacity_ints > 0, or count > UINT32_MAX.
 * count == 0: ANSX_OK, total 0, nothing launched.
 * Errors decided on the host, before any byte of d_out is written (all headers come back in one round trip):
 * ANSX_ERR_FORMAT if in_bytes[i] < 64, input i is a single-stream stream (no header), its kind or fidelity is not the
 * call's, or any other check of ansx_decode_dev on its header fails -- *bad_index (optional) is then i, the first such
 * container; ANSX_ERR_CAPACITY if sum(n_i) > out_capacity_ints.
 * Errors decided on the device (an invalid index entry or block stream): ANSX_ERR_FORMAT with *bad_index = count --
 * unlike the range entries, d_out is then unspecified (earlier passes may have written their containers) and the
 * failing container is not known.
 * The context stays usable after any error, and the call leaves no trace in it (nothing enters the cached headers of
 * ansx_decode_dev, no per-geometry hint changes).  Synchronous, like ansx_decode_dev; the inputs are read on
 * `stream`.  Work is done in passes of at most 16384 blocks per geometry (ANSX_BATCH_PASS_BLOCKS), and the
 * workspace is bounded by one pass, not by the batch. */
int ansx_decode_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, uint32_t* d_out, size_t out_capacity_ints, uint64_t* offsets, uint64_t* total_ints, size_t* bad_index,
    void* stream);

/* Ranges of a batch of containers in one call: the product of ansx_decode_ranges_dev and ansx_decode_batch_dev (a few
 * ranges out of each of many posting lists or column chunks).  d_ins / in_bytes / count: the batch, as for
 * ansx_decode_batch_dev.  src, first, cnt: HOST arrays of nranges; range i is ints [first[i], first[i] + cnt[i]) of
 * container src[i], written to d_out[offsets[i] ..): the ranges in order and back to back.  offsets (optional, HOST
 * array of nranges + 1): the exclusive prefix sums of cnt, and the total; *total_ints (optional): sum(cnt).  The output
 * is bit-identical to slicing what ansx_decode_dev returns for each container.  Ranges may overlap, repeat, be unsorted,
 * have count 0 and name containers in any order; the same pointer may stand at several batch positions (they are then
 * distinct sources); every container form ansx_decode_dev reads is accepted, and the containers of one call may differ
 * in geometry.  d_out: 4-byte aligned.
 * Selectivity: a container is REFERENCED when some range names it (count 0 included).  Of an unreferenced container
 * nothing is read, not even its header, and d_ins[i] / in_bytes[i] are not examined (null is allowed).  Of a referenced
 * container only the header, the index entries of touched blocks and the bytes of touched blocks are read.  No kernel's
 * grid grows with count or with any container's block count: grids grow with the referenced containers, the touched
 * blocks and the ints asked for.
 * Errors decided before the context is touched (ANSX_ERR_ARG): a null ctx; a null src, first, cnt, d_ins or in_bytes
 * with nranges > 0; count or nranges > UINT32_MAX; d_out misaligned, or NULL with out_capacity_ints > 0;
 * src[i] >= count -- *bad_range (optional) is then i, the first such range; a null or not 16-byte aligned pointer of a
 * referenced container -- *bad_range is then the first range naming it.  nranges == 0: ANSX_OK, total 0,
 * offsets[0] = 0, nothing launched, whatever count is.
 * Errors decided on the host, before any byte of d_out is written (the headers of the referenced containers come back in
 * one round trip), in this order: ANSX_ERR_FORMAT under exactly ansx_decode_batch_dev's header checks --
 * *bad_container (optional) is then the first failing container in batch order; ANSX_ERR_ARG if first[i] > n or
 * cnt[i] > n - first[i] against the named container's own n -- *bad_range is then the first such range;
 * ANSX_ERR_CAPACITY if sum(cnt) > out_capacity_ints.  offsets and *total_ints are written on ANSX_OK and
 * ANSX_ERR_CAPACITY, so d_out = NULL, out_capacity_ints = 0 is a size query.
 * Errors found on the device (an invalid index entry or stream of a touched block): ANSX_ERR_FORMAT with
 * *bad_container = count; d_out is then unspecified, as for ansx_decode_batch_dev, but nothing is ever written at or
 * beyond d_out + out_capacity_ints.
 * The context stays usable after any error, and the call leaves no trace in it (no cached header, no per-geometry
 * hint).  Synchronous; the inputs are read on `stream`.  Work is done per geometry in passes of at most 16384 touched
 * blocks (ANSX_BATCH_PASS_BLOCKS); device workspace is bounded by one pass and the plan of its pieces, plus 72 bytes per
 * referenced container. */
int ansx_decode_batch_ranges_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, const uint32_t* src, const uint64_t* first, const uint32_t* cnt, size_t nranges, uint32_t* d_out,
    size_t out_capacity_ints, uint64_t* offsets, uint64_t* total_ints, size_t* bad_container, size_t* bad_range,
    void* stream);

/* A batch of lists in one call: the writer's side of ansx_decode_batch_dev (posting lists, column chunks).  List i is
 * d_in[offsets[i] .. offsets[i + 1]); offsets is a HOST array of count + 1 non-decreasing int offsets -- the layout
 * ansx_decode_batch_dev returns -- and d_in is 4-byte aligned device memory: a list may start at any int.  Container i
 * is written to d_out + out_offsets[i] (d_out: 16-byte aligned): out_offsets[i] is a multiple of 16, the containers
 * stand in batch order, back to back, out_bytes[i] is container i's exact size, and the padding bytes in between are
 * zero; out_offsets[count] and *total_bytes are the end of the last container rounded up to 16.  out_offsets (count + 1)
 * and out_bytes (count) are optional HOST arrays; d_out + out_offsets[i] with out_bytes[i] feed ansx_decode_batch_dev
 * directly.  Container i is byte for byte what ansx_encode_dev(kind, fidelity, list i, opts) writes from a fresh
 * context: header (max_nsyms, max_present_m1 and max_log2_frame are maxima over that list's own blocks), index,
 * restart points, parse hints and payload; its restart points are wide exactly when that list alone would have had
 * wide ones, so two lists of one batch may differ in form.
 * Capacity: sum_i rup16(ansx_bound(kind, fidelity, n_i, opts)), rup16 = rounded up to a multiple of 16, is always
 * enough.
 * Errors decided before the context is touched (ANSX_ERR_ARG): a null ctx; a null d_in, offsets or d_out with
 * count > 0; a misaligned pointer; count > UINT32_MAX; decreasing offsets; an empty list -- *bad_index (optional) is
 * then the first empty list, as ansx_encode_dev refuses n == 0; a bad kind, fidelity or options, as for
 * ansx_encode_dev; opts->block_ints == ANSX_SINGLE_STREAM (a batch yields containers).  count == 0: ANSX_OK, total 0,
 * nothing launched.
 * Errors found on the device: ANSX_ERR_DOMAIN, ANSX_ERR_MODEL, ANSX_ERR_CAPACITY, with *bad_index = count unless the
 * list is known (one that was encoded on its own, see below; lists of ANSX_RFOLD with fidelity 1..5 and compacted lists
 * of ANSX_FOLD with fidelity 1..5 and of ANSX_MSB run in passes and are among those not named).  d_out is then
 * unspecified, but nothing is ever written
 * at or beyond d_out + out_capacity.  The context stays usable after any error.
 * How the work is done.  ANSX_FOLD and ANSX_RFOLD (block_ints <= 16384) with fidelity 1..5 and ANSX_MSB take the batched
 * path, ANSX_FOLD and ANSX_MSB also with ANSX_FLAG_COMPACT_ALPHABET: the
 * lists are grouped, in batch order and cut at list boundaries only, into passes of at most 16384 blocks
 * (ANSX_BATCH_PASS_BLOCKS, the key ansx_decode_batch_dev uses); the model, prelude and encoder kernels run once per
 * pass over all its blocks, one kernel pair assembles every container of the pass in place, and one read-back per pass
 * returns its status, offsets and sizes.  A list of 16 or more full blocks (or of more than one pass's blocks) is
 * encoded by the ordinary path into its place: it amortises its own overheads, at the cost of a call of ansx_encode_dev.
 * ANSX_RFOLD's remap of a pass runs one kernel per class of blocks: blocks of fewer than T = 2^(fidelity + 7) ints are
 * copied (they cannot have T distinct values), blocks of T..1024 ints take a kernel with one wave per block, longer
 * blocks the hash-table kernel of ansx_encode_dev; a table that the batch's own hint sized too small repeats the pass,
 * not the batch.  With compaction the remap of a pass has two classes: blocks of up to 1024 ints take a kernel with
 * one wave per block that sorts the block (no table, nothing to size or repeat), longer blocks the hash-set kernel of
 * ansx_encode_dev, sized from the batch's own hint; a set that is too small repeats the pass.  ANSX_INT (with and
 * without compaction) and fidelity 6, 7 have NO batched
 * path yet: they are accepted and bit-identical, but every list is encoded on its own inside the call, at the cost
 * of a loop of ansx_encode_dev.  Workspace: bounded by one pass (or the largest single list), not by the batch; for
 * ANSX_RFOLD it includes the pass's remapped ints and T * 4 bytes per block of the pass for the selected values
 * (256 MiB for a full pass of 16384 blocks at fidelity 5), with compaction 8 bytes per int of the pass (ranks and
 * alphabets), and the model arrays' rows of a compacted pass are as long as the ranks of its longest block need, not
 * as the codec's alphabet.
 * No trace: the call keeps the alphabet and frame hints it learns in a slot of its own and puts
 * ansx_last_encode_stats back, so a later ansx_encode_dev behaves -- path and bytes -- as if the batch call had not
 * happened; a batch of short lists does not teach the context a small alphabet.  Synchronous, like ansx_encode_dev;
 * the input is read on `stream`. */
int ansx_encode_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint32_t* d_in, const uint64_t* offsets, size_t count,
    uint8_t* d_out, size_t out_capacity, uint64_t* out_offsets, uint64_t* out_bytes, size_t* total_bytes, size_t* bad_index,
    const ansx_opts* opts, void* stream);

/* Docids: running sums and gaps.  A posting list is stored as the gaps between its sorted
 * document ids and read as the ids; these four calls are the two ends.  For a list x the sums are
 * s[i] = x[0] + ... + x[i] (inclusive); for a list d the gaps are g[0] = d[0], g[i] = d[i] - d[i - 1]; every list of a
 * batch starts afresh; decode_sums(encode_gaps(d)) == d for every non-decreasing d whose gaps the codec accepts.  Whole
 * containers and whole batches only (running sums of RANGES: the calls with block bases further down), 32-bit
 * outputs, no change of the container format: the bytes are those of the ordinary calls on the gaps.
 *
 * ansx_decode_sums_dev: the arguments and the behaviour of ansx_decode_dev -- the accepted forms, ANSX_SINGLE_STREAM
 * included, the remembered headers, the hints, the errors -- then d_out[0 .. n) is replaced in place by its running
 * sums (three kernels over tiles of the output: per-tile aggregates, one workgroup that scans them, per-tile scan and
 * store; partial sums are carried in 64 bits).  ANSX_ERR_DOMAIN if any running sum exceeds 2^32 - 1, found on the device
 * and read back before the call returns; d_out is then unspecified.  Nothing is written outside d_out[0 .. n).  Unlike
 * ansx_decode_dev, d_out needs only 4-byte alignment (an output that is not 16-byte aligned is decoded in workspace, 4
 * bytes per int, and copied). */
int ansx_decode_sums_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes,
    uint32_t* d_out, size_t n, const ansx_opts* opts, void* stream);

/* ansx_decode_batch_sums_dev: the arguments and the behaviour of ansx_decode_batch_dev -- the same checks in the same
 * order, the same offsets, the same size query, no trace in the context -- then every list
 * d_out[offsets[i] .. offsets[i + 1]) is replaced by its own running sums: one segmented scan over the whole output,
 * after the last pass of the last geometry group, that restarts at every list.  ANSX_ERR_DOMAIN when the sum of some list
 * exceeds 2^32 - 1; *bad_index (optional) is then the first such list in batch order and d_out is unspecified.  A format
 * error found on the device is reported as by ansx_decode_batch_dev, and nothing is scanned. */
int ansx_decode_batch_sums_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, uint32_t* d_out, size_t out_capacity_ints, uint64_t* offsets, uint64_t* total_ints, size_t* bad_index,
    void* stream);

/* ansx_encode_gaps_dev: the arguments of ansx_encode_dev, d_in holding n non-decreasing ids.  The gaps are written to
 * workspace of the context (4 bytes per int, grow-only, counted by ansx_workspace_bytes) and encoded by the ordinary
 * path: the output bytes, *out_bytes, ansx_last_encode_stats and what the context learns are exactly those of
 * ansx_encode_dev on the gaps; d_in is not modified.  ANSX_ERR_DOMAIN if an id is smaller than the one before it -- decided
 * by comparing the neighbours, not by the wrapped difference, which can come out below 2^30 -- and nothing is encoded
 * then; the gaps themselves pass the encoder's own domain checks like any input (a gap of 2^30 or more:
 * ANSX_ERR_DOMAIN). */
int ansx_encode_gaps_dev(ansx_ctx* ctx, int kind, int fidelity, const uint32_t* d_in, size_t n, uint8_t* d_out,
    size_t out_capacity, size_t* out_bytes, const ansx_opts* opts, void* stream);

/* ansx_encode_batch_gaps_dev: the arguments of ansx_encode_batch_dev, list i holding non-decreasing ids; its first gap
 * is its own first id, so a list may start below the end of the list before it.  The argument errors decided before the
 * context is touched are those of ansx_encode_batch_dev, *bad_index included.  ANSX_ERR_DOMAIN with *bad_index = the
 * first list that holds a decrease, nothing encoded; otherwise the call is byte for byte ansx_encode_batch_dev on the
 * gaps, its errors, *bad_index and its promise to leave no trace included.  Workspace: 4 bytes per int of the BATCH
 * for the gaps -- the one place where this call is not bounded by a pass. */
int ansx_encode_batch_gaps_dev(ansx_ctx* ctx, int kind, int fidelity, const uint32_t* d_in, const uint64_t* offsets,
    size_t count, uint8_t* d_out, size_t out_capacity, uint64_t* out_offsets, uint64_t* out_bytes, size_t* total_bytes,
    size_t* bad_index, const ansx_opts* opts, void* stream);

/* Docids of ranges: block bases beside the container.  For a container of n gaps in nblocks
 * blocks of block_ints ints the bases are nblocks + 1 values of uint32_t in 4-byte aligned DEVICE memory of the caller:
 * bases[b] is the sum of ints [0, b * block_ints), so bases[0] = 0 and bases[nblocks] is the sum of the whole list, its
 * last id -- the skip table an inverted index keeps anyway.  Nothing in the container refers to them; the container
 * format and every other call are as they were.  Two calls produce them, two read them.
 *
 * ansx_block_bases_dev: the bases of an existing container.  Every form ansx_decode_dev reads is accepted except a
 * single-stream stream, which has no blocks (ANSX_ERR_FORMAT, as in the range calls).  The container is decoded into
 * workspace of the context (4 bytes per int, grow-only, counted by ansx_workspace_bytes), per-block 64-bit sums are
 * taken, and one workgroup scans them into d_bases.  *nbases = nblocks + 1 is set on ANSX_OK and on ANSX_ERR_CAPACITY
 * (bases_capacity < nblocks + 1), which is decided from the header before anything is launched: d_bases = NULL,
 * bases_capacity = 0 is a size query.  ANSX_ERR_DOMAIN if the sum of the list exceeds 2^32 - 1; d_bases is then
 * unspecified.  The errors of the decode are those of ansx_decode_dev.  Errors decided before the context is touched:
 * ANSX_ERR_ARG for a null ctx / d_in / nbases, d_in not 16-byte aligned, d_bases not 4-byte aligned, or d_bases == NULL
 * with bases_capacity > 0.  The call leaves no trace in the context (no remembered header, no per-geometry hint), like
 * the range calls.  Returns after the status has been read back. */
int ansx_block_bases_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes, uint32_t* d_bases,
    size_t bases_capacity, size_t* nbases, void* stream);

/* ansx_encode_gaps_bases_dev: ansx_encode_gaps_dev for the writer who wants the bases as well -- its arguments, then
 * d_bases, bases_capacity and nbases as above.  The container bytes, *out_bytes, ansx_last_encode_stats and what the
 * context learns are exactly those of ansx_encode_gaps_dev.  Once the ids have passed the check for decreases, one
 * kernel reads the bases off them: bases[0] = 0, bases[b] = d_in[b * block_ints - 1], bases[nblocks] = d_in[n - 1],
 * block_ints being the value opts resolves to.  Decided on the host before anything is launched: ANSX_ERR_ARG as for
 * ansx_encode_gaps_dev, for a null nbases, a misaligned d_bases, d_bases == NULL with bases_capacity > 0 and for
 * opts->block_ints == ANSX_SINGLE_STREAM (a stream has no blocks); ANSX_ERR_CAPACITY, with *nbases set, when
 * bases_capacity < nblocks + 1.  After an error of the encode d_bases is unspecified. */
int ansx_encode_gaps_bases_dev(ansx_ctx* ctx, int kind, int fidelity, const uint32_t* d_in, size_t n, uint8_t* d_out,
    size_t out_capacity, size_t* out_bytes, const ansx_opts* opts, uint32_t* d_bases, size_t bases_capacity,
    size_t* nbases, void* stream);

/* ansx_decode_ranges_sums_dev: ansx_decode_ranges_dev returning ids.  Range i is s[first[i]] .. s[first[i] + count[i] - 1],
 * s being what ansx_decode_sums_dev returns for the container; the ranges lie in d_out exactly as ansx_decode_ranges_dev
 * lays out the gaps.  Everything else is that call's: the accepted forms, what ranges may look like, the errors and
 * their order, selectivity, no kernel's grid growing with the container's block count, no trace in the context, the
 * number of host round trips -- the sums add no synchronisation and no read-back of their own.  Between the decode of
 * the touched blocks and the gather, the work list is scanned in place, restarting at every touched block b from
 * d_bases[b] (ansx_rangesums.h).  In addition:
 *   ANSX_ERR_ARG before the context is touched for a null or misaligned (4 bytes) d_bases with nranges > 0;
 *   ANSX_ERR_ARG on the host, once the header is known and before any launch, if nbases != nblocks + 1;
 *   of d_bases only entries b and b + 1 of touched blocks b are read;
 *   every touched block is scanned whole, and d_bases[b] + (the sum of block b, in 64 bits) must equal d_bases[b + 1].
 *   If it does not, the bases are not this container's: ANSX_ERR_FORMAT, found on the device and reported through the
 *   flag and the read-back of the decode's own format errors, and like those it leaves d_out unwritten.  Consistent
 *   bases also prove that no running sum inside a touched block leaves 32 bits, so there is no ANSX_ERR_DOMAIN here. */
int ansx_decode_ranges_sums_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes,
    const uint32_t* d_bases, size_t nbases, const uint64_t* first, const uint32_t* count, size_t nranges, uint32_t* d_out,
    size_t out_capacity_ints, void* stream);

/* ansx_decode_device_ranges_sums_dev: the same over ansx_decode_device_ranges_dev -- its arguments with d_bases, nbases
 * behind in_bytes, its errors in its order, d_offsets and *total_ints unchanged -- with the additional rules of
 * ansx_decode_ranges_sums_dev. */
int ansx_decode_device_ranges_sums_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes,
    const uint32_t* d_bases, size_t nbases, const uint64_t* d_first, const uint32_t* d_count, size_t nranges,
    uint32_t* d_out, size_t out_capacity_ints, uint64_t* d_offsets, uint64_t* total_ints, void* stream);

/* ansx_next_geq_dev: search by value over the bases.  Let s be what ansx_decode_sums_dev returns
 * for the container, n ids, non-decreasing.  For every target t = d_targets[i]: d_pos[i] = min{ j : s[j] >= t } -- the
 * lower bound: of equal ids (zero gaps) the first, which may lie in an earlier block than the last -- and
 * d_ids[i] = s[d_pos[i]].  t = 0 gives position 0.  If t > s[n - 1]: d_pos[i] = n and d_ids[i] = ANSX_NO_ID.  2^32 - 1 can
 * be a real id, so d_pos[i] == n is the authoritative "not found"; a caller who asks for ids only must keep the last id
 * below 2^32 - 1 or compare t with bases[nblocks] themselves.  Targets may be unsorted and may repeat.
 * d_targets: ntargets uint32_t in 4-byte aligned DEVICE memory, read on `stream` (a kernel that wrote them earlier on that
 * stream is ordered before).  d_pos (8-byte aligned) and d_ids (4-byte aligned): DEVICE arrays of ntargets; either may
 * be NULL, not both.  *found (optional, host): the number of targets with d_pos[i] < n, set on ANSX_OK.
 * Accepted forms, header checks, no trace in the context and "returns after the status has been read back" are exactly
 * those of ansx_decode_device_ranges_sums_dev (every container form the range calls accept; a single-stream stream is
 * ANSX_ERR_FORMAT), and so are the two host round trips: the header, then the planner's scalars with the status.
 * One exception: when NO target is found the range path ends at the planner's scalars; the outputs are then filled by
 * a kernel of their own and the call waits for it, a third host wait, so that it returns with its outputs written as on
 * every other path.
 * Errors, in this order:
 *   before the context is touched, ANSX_ERR_ARG for a null ctx or d_in; a null d_bases or d_targets, or both outputs
 *   null, with ntargets > 0; a misaligned pointer (d_in 16 bytes, d_bases 4, d_targets 4, d_pos 8, d_ids 4);
 *   ntargets > UINT32_MAX.  ntargets == 0: ANSX_OK, *found = 0, nothing launched, the context untouched;
 *   on the host once the header is known, before any launch: ANSX_ERR_FORMAT as in the range calls, then ANSX_ERR_ARG
 *   if nbases != nblocks + 1;
 *   on the device: ANSX_ERR_FORMAT for an invalid index entry or stream of a touched block, and for bases that fail
 *   the check of the sums range calls at a touched block b (d_bases[b] + the block's sum in 64 bits != d_bases[b + 1]),
 *   through the decode's flag word and its one read-back.  NEITHER output array is written then.
 * What the bases promise.  The search trusts d_bases to be this container's (non-decreasing, bases[0] = 0, as
 * ansx_block_bases_dev or ansx_encode_gaps_bases_dev made them) and must not be changed while the call runs.  It verifies
 * what the sums range calls verify and only at TOUCHED blocks -- the blocks some target was sent to.  A wrong entry
 * elsewhere can send a target to a block that is not its own WITHOUT DETECTION: the answer is then the lower bound inside
 * that block, clamped to it.  What holds for any content of d_bases is memory safety: nothing is read outside
 * d_bases[0 .. nbases), the container and d_targets[0 .. ntargets), nothing is written outside d_pos[0 .. ntargets) and
 * d_ids[0 .. ntargets), and every search loop ends.
 * Selectivity: of a block no target lands in, nothing is read -- no stream, restart point, hint or index entry; targets
 * beyond the last id touch no block; no kernel's grid grows with the container's block count.  Of d_bases the locate
 * step may read any entry (O(log nblocks) per target, most of them from a copy in LDS) -- the one difference from the
 * sums range calls, which read entries b and b + 1 only.  Workspace: that of the range calls for the touched blocks plus
 * 28 bytes per target. */
#define ANSX_NO_ID 0xFFFFFFFFu
int ansx_next_geq_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes, const uint32_t* d_bases,
    size_t nbases, const uint32_t* d_targets, size_t ntargets, uint64_t* d_pos, uint32_t* d_ids, uint64_t* found,
    void* stream);

/* Batches of gap-coded lists: written with their bases, sliced as ids and searched, one call each (DESIGN.md
 * section 3h).
 *
 * ansx_encode_batch_gaps_bases_dev is ansx_encode_batch_gaps_dev for the writer who also wants the block bases of every
 * list: that call's arguments, then d_bases (DEVICE, 4-byte aligned, bases_capacity entries), base_offsets (HOST,
 * count + 1 entries, optional) and total_bases (optional).  List i has nb_i = ceil(n_i / block_ints) blocks, block_ints
 * the value opts resolves to, and its nb_i + 1 bases stand at d_bases[base_offsets[i] .. base_offsets[i + 1]), back to
 * back in batch order: bases_i[0] = 0, bases_i[b] = ids_i[b * block_ints - 1], bases_i[nb_i] = ids_i[n_i - 1], what
 * ansx_block_bases_dev returns for container i.  base_offsets is the exclusive prefix sum of nb_i + 1, a pure function
 * of offsets and the options, computed on the host before any launch.  The bases are read off the ids by one kernel,
 * a thread per entry, behind the check for decreases; no host round trip is added.  The containers, out_offsets,
 * out_bytes, *total_bytes, *bad_index, the errors and the no-trace promise are exactly those of
 * ansx_encode_batch_gaps_dev.  Additional errors: ANSX_ERR_ARG, before the context is touched, for a misaligned d_bases
 * or d_bases == NULL with bases_capacity > 0; ANSX_ERR_CAPACITY, on the host before any launch, when bases_capacity <
 * sum(nb_i + 1) -- base_offsets and *total_bases are written then, so d_bases = NULL, bases_capacity = 0 is a size query.
 * After an error of the encode d_bases is unspecified. */
int ansx_encode_batch_gaps_bases_dev(ansx_ctx* ctx, int kind, int fidelity, const uint32_t* d_in, const uint64_t* offsets,
    size_t count, uint8_t* d_out, size_t out_capacity, uint64_t* out_offsets, uint64_t* out_bytes, size_t* total_bytes,
    size_t* bad_index, const ansx_opts* opts, uint32_t* d_bases, size_t bases_capacity, uint64_t* base_offsets,
    size_t* total_bases, void* stream);

/* ansx_decode_batch_ranges_sums_dev: ansx_decode_batch_ranges_dev returning ids.  Range i is s[first[i]] ..
 * s[first[i] + cnt[i] - 1] of container src[i], s what ansx_decode_sums_dev returns for that container.  d_bases[i]
 * (HOST array of `count` DEVICE pointers, 4-byte aligned) are the block bases of container i and nbases[i] (HOST) their
 * number; d_bases + base_offsets[i] of the writer above feeds it directly.  The layout of d_out, offsets, the size
 * query, what ranges may look like, mixed geometries, one pointer at several batch positions, the errors and their
 * order, no trace in the context, the passes and the number of host round trips are ansx_decode_batch_ranges_dev's: the
 * sums add no synchronisation and no read-back.  Between a pass's decode and its gather the pass's work list is scanned
 * in place, restarting at every touched block from that block's own container's base.
 * Selectivity: of an unreferenced container neither d_bases[i] nor nbases[i] is examined (null is allowed); of a
 * referenced one only entries b and b + 1 of touched blocks b are read.
 * Additional errors: ANSX_ERR_ARG before the context is touched for a null d_bases or nbases array with nranges > 0, or
 * a null or misaligned d_bases[i] of a referenced container (*bad_range: the first range naming it); ANSX_ERR_ARG on
 * the host, after the header checks and before the range checks, if nbases[i] != nblocks_i + 1 for a referenced
 * container (*bad_container: the first such); ANSX_ERR_FORMAT, found on the device, *bad_container = count, if the
 * bases of a touched block are not the container's: every touched block is scanned whole and bases[b] + (its sum in 64
 * bits) must be bases[b + 1].  It travels through the pass's flag word and its read-back and that pass's gather writes
 * nothing; d_out is unspecified, nothing is written at or beyond d_out + out_capacity_ints. */
int ansx_decode_batch_ranges_sums_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins,
    const size_t* in_bytes, const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* src,
    const uint64_t* first, const uint32_t* cnt, size_t nranges, uint32_t* d_out, size_t out_capacity_ints, uint64_t* offsets,
    uint64_t* total_ints, size_t* bad_container, size_t* bad_range, void* stream);

/* ansx_decode_batch_device_ranges_dev / ansx_decode_batch_device_ranges_sums_dev: ansx_decode_batch_ranges_dev /
 * ansx_decode_batch_ranges_sums_dev with (src, first, cnt) in DEVICE memory and the plan built on the device
 * ("device plan").  d_ins / in_bytes (and d_bases / nbases) are HOST arrays of `count` entries as
 * there.  d_src (4-byte aligned), d_first (8) and d_cnt (4) are DEVICE arrays of nranges entries, read on `stream`: a
 * kernel that wrote them earlier on that stream is ordered before the read.  d_out receives, byte for byte, what the
 * host-array call writes for the same ranges: range i at d_out[offsets[i] ..), in range order, back to back; ranges
 * may overlap, repeat, be unsorted, have count 0 and name the containers in any order; one pointer may stand at
 * several batch positions; geometries may be mixed.  d_offsets (optional, DEVICE, 8-byte aligned, nranges + 1 entries)
 * receives the exclusive prefix sum of cnt and the total; *total_ints (optional, HOST) the total.  Both are written on
 * ANSX_OK and ANSX_ERR_CAPACITY.
 * Nothing on the host grows with nranges: host work and copies are O(count) + O(referenced containers) + O(passes), and
 * the call waits for the device three times before the passes -- the number of referenced containers, their headers,
 * the plan's scalars -- and then as the host-array call does for every pass's decode.
 * Errors, in this order; nothing of d_out is written before the last of them is decided:
 *   before the context is touched, ANSX_ERR_ARG for a null ctx; a null d_src / d_first / d_cnt / d_ins / in_bytes with
 *   nranges > 0; a misaligned d_src, d_first, d_cnt, d_out or d_offsets; d_out == NULL with out_capacity_ints > 0; count
 *   or nranges > UINT32_MAX; for the sums a null d_bases or nbases array.  nranges == 0: ANSX_OK, *total_ints = 0 and,
 *   the one thing such a call enqueues, d_offsets[0] = 0 if d_offsets is given; the context is otherwise untouched;
 *   found on the device, before any header is judged: ANSX_ERR_ARG with *bad_range = the smallest i with
 *   d_src[i] >= count; then ANSX_ERR_ARG with *bad_range = the first range that names a container whose d_ins entry (for
 *   the sums: or d_bases entry) is null or not 16-byte (4-byte) aligned;
 *   on the host, once the referenced headers are back: ANSX_ERR_FORMAT with *bad_container = the first referenced
 *   container in batch order that fails the checks of ansx_decode_batch_ranges_dev; for the sums then ANSX_ERR_ARG with
 *   *bad_container where nbases[i] != nblocks_i + 1; ANSX_ERR_ARG if the referenced containers have 2^32 - 1 blocks or
 *   more together;
 *   on the device, read back with the plan's scalars: ANSX_ERR_ARG with *bad_range = the smallest i with first[i] > n or
 *   cnt[i] > n - first[i], n that of container src[i]; then ANSX_ERR_CAPACITY if sum(cnt) > out_capacity_ints
 *   (d_out = NULL with capacity 0 is the size query);
 *   from a pass: ANSX_ERR_FORMAT with *bad_container = count (a bad stream or index entry; for the sums also foreign
 *   bases at a touched block).  d_out is then unspecified; nothing is written at or beyond d_out + out_capacity_ints.
 * The context stays usable after any error and keeps no trace of the call.
 * Selectivity is that of the host-array call with two differences: d_ins[i] / in_bytes[i] / d_bases[i] of ALL count
 * containers are copied to the device unjudged (null is allowed for an unreferenced one), and one workgroup scans 4
 * bytes of marks per container of the batch.  No container but a referenced one is read, and of those the header, the
 * index entries and bytes of touched blocks and, for the sums, bases b and b + 1 of touched blocks b.
 * Workspace beyond the host-array call's: 24 bytes per container of the batch (32 for the sums) and 12 per
 * min(count, nranges); 160 per referenced container (176); 48 per range and 112 per 4096 ranges; 4 per block of a
 * referenced container; 48 per pass the referenced blocks could make.  A pass's 24 bytes per block and 24 per piece
 * are those of the host-array call, built on the device where that call uploads them. */
int ansx_decode_batch_device_ranges_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins,
    const size_t* in_bytes, size_t count, const uint32_t* d_src, const uint64_t* d_first, const uint32_t* d_cnt,
    size_t nranges, uint32_t* d_out, size_t out_capacity_ints, uint64_t* d_offsets, uint64_t* total_ints,
    size_t* bad_container, size_t* bad_range, void* stream);
int ansx_decode_batch_device_ranges_sums_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins,
    const size_t* in_bytes, const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* d_src,
    const uint64_t* d_first, const uint32_t* d_cnt, size_t nranges, uint32_t* d_out, size_t out_capacity_ints,
    uint64_t* d_offsets, uint64_t* total_ints, size_t* bad_container, size_t* bad_range, void* stream);

/* ansx_next_geq_batch_dev: ansx_next_geq_dev over a batch.  With s the ids of container src[i], n of them:
 * d_pos[i] = min{ j : s[j] >= d_targets[i] } (the lower bound: of equal ids the first), d_ids[i] = s[d_pos[i]]; beyond
 * the last id d_pos[i] = n of that container and d_ids[i] = ANSX_NO_ID.  src is a HOST array of ntargets entries,
 * d_targets DEVICE (4-byte aligned, read on `stream`), d_pos / d_ids DEVICE (8 / 4-byte aligned; either may be NULL,
 * not both).  *found (optional): the number of targets found, set on ANSX_OK.  Targets may be unsorted, may repeat and
 * may name the lists in any order.
 * How it runs: the headers of the referenced containers in one round trip (the front half of
 * ansx_decode_batch_ranges_dev); k_ngb_locate, a lane per target, finds the smallest block b of its list with
 * bases[b + 1] >= t and writes n / ANSX_NO_ID where there is none; ONE read-back of the located blocks, 4 bytes per
 * target -- one host round trip MORE than ansx_decode_batch_ranges_dev; the host checks every value and runs the plan
 * of the ranges call over the found targets, one int at the start of each one's block; per pass the decode, the scan of
 * the sums call and a lower bound over the block's scanned ids, clamped to the block's own length.  When no target is
 * found no pass runs; the outputs are written on return all the same.
 * Errors, in this order: before the context is touched, ANSX_ERR_ARG for a null ctx, null arrays or both outputs null
 * with ntargets > 0, a misaligned d_targets / d_pos / d_ids, count or ntargets > UINT32_MAX, src[i] >= count
 * (*bad_target = i), then a null or misaligned d_ins[src[i]] (16 bytes) or d_bases[src[i]] (4 bytes) (*bad_target: the
 * first target naming it).  ntargets == 0: ANSX_OK, *found = 0, nothing launched, the context untouched.  Once the
 * headers are known: ANSX_ERR_FORMAT with *bad_container for a header that fails the checks, then ANSX_ERR_ARG with
 * *bad_container if nbases[i] != nblocks_i + 1.  On the device: ANSX_ERR_FORMAT with *bad_container = count for a stream
 * or index entry of a touched block, or bases that are not the container's at a touched block; the outputs are
 * unspecified then.  Nothing is ever written outside d_pos[0 .. ntargets) and d_ids[0 .. ntargets).
 * What the bases promise is word for word ansx_next_geq_dev's: verified at touched blocks only, a wrong entry elsewhere
 * can misdirect a target undetected, memory safety and termination hold for any content.
 * Selectivity: an unreferenced container is not examined (null d_ins[i] / d_bases[i] allowed); of a block no target
 * lands in nothing is read; no kernel's grid grows with count or with a container's block count; the locate step may
 * read any entry of a REFERENCED container's bases.
 * Workspace: that of one pass (ANSX_BATCH_PASS_BLOCKS blocks) plus 28 bytes per target (its list, its block, its piece
 * of the plan) and 96 bytes per referenced container (address, header, and the list's entry for the locate step), and
 * the same again in pinned host memory. */
int ansx_next_geq_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, const uint32_t* src, const uint32_t* d_targets,
    size_t ntargets, uint64_t* d_pos, uint32_t* d_ids, uint64_t* found, size_t* bad_container, size_t* bad_target,
    void* stream);

/* Intersection of gap-coded lists.
 *
 * ansx_intersect_ids_dev: the members of a candidate array in one list.  Let s be what ansx_decode_sums_dev returns for
 * the container, n ids.  Candidate i is a member when some s[j] == d_cand[i].  The members are written in candidate
 * order, back to back -- a stable filter: a candidate that repeats is kept every time it is a member; candidates may be
 * unsorted.  For the k-th member, i_k its index in d_cand: d_out_ids[k] its value, d_out_idx[k] = i_k, d_out_pos[k] =
 * min{ j : s[j] == value }, the lower bound as in ansx_next_geq_dev.  Membership is decided from "found and equal", never
 * from a comparison with ANSX_NO_ID: a candidate 2^32 - 1 is a member exactly when the list's last id is 2^32 - 1.
 * d_cand: ncand uint32_t in 4-byte aligned DEVICE memory, read on `stream`.  d_out_ids, d_out_idx (4-byte aligned),
 * d_out_pos (8-byte aligned): DEVICE arrays of out_capacity entries; any may be NULL, not all three; none may overlap
 * d_cand.  *nfound (optional, host): the number of members, set on ANSX_OK and on ANSX_ERR_CAPACITY.
 * Accepted forms, header checks, what the bases promise, no trace in the context and "returns after the status has been
 * read back" are ansx_next_geq_dev's (a single-stream stream is ANSX_ERR_FORMAT).
 * Errors, in this order:
 *   before the context is touched, ANSX_ERR_ARG for a null ctx or d_in; a null d_bases or d_cand, or all three outputs
 *   null, with ncand > 0; a misaligned pointer (d_in 16 bytes, d_bases 4, d_cand 4, d_out_ids 4, d_out_idx 4,
 *   d_out_pos 8); ncand > UINT32_MAX.  ncand == 0: ANSX_OK, *nfound = 0, nothing launched, the context untouched;
 *   on the host once the header is known, before any launch: ANSX_ERR_FORMAT as in the range calls, then ANSX_ERR_ARG
 *   if nbases != nblocks + 1;
 *   on the device: ANSX_ERR_FORMAT for an invalid index entry or stream, and for bases that are not the list's at a
 *   touched block -- a block some candidate was sent to; ANSX_ERR_DOMAIN or ANSX_ERR_FORMAT for a list whose sum leaves
 *   32 bits (it has no valid bases).  NO output array is written then;
 *   ANSX_ERR_CAPACITY when there are more members than out_capacity: *nfound is the size of a retry and no output
 *   entry is written.
 * A wrong entry of d_bases at an untouched block can misdirect a candidate undetected, which here means that a member
 * may be missed.  Memory safety and termination hold for any content of d_bases and d_cand.
 * Two forms of one step, with identical outputs for valid inputs.  Selective (ncand < nblocks): ansx_next_geq_dev's
 * path -- of a block no candidate lands in nothing is read, no grid grows with the block count -- with the match and
 * the compaction in the search's place.  Workspace: ansx_next_geq_dev's plus 8 bytes per 64 candidates and, with
 * d_out_pos, 8 per candidate.  Host waits: ansx_next_geq_dev's three and none more (the total rides on the last).
 * Full (ncand >= nblocks, where the candidates reach most blocks anyway): the whole list decoded to ids in workspace,
 * 4 bytes per int, the bases checked against it at touched blocks.  Host waits: three (the header twice, the status). */
int ansx_intersect_ids_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* d_in, size_t in_bytes,
    const uint32_t* d_bases, size_t nbases, const uint32_t* d_cand, size_t ncand, uint32_t* d_out_ids, uint32_t* d_out_idx,
    uint64_t* d_out_pos, size_t out_capacity, uint64_t* nfound, void* stream);

/* ansx_intersect_dev: the ids common to `count` lists.  The batch arrays are ansx_next_geq_batch_dev's: HOST arrays of
 * DEVICE pointers, mixed geometries allowed, the same pointer at several positions allowed.  The result: the ids of
 * the DRIVER -- the list of fewest ints, of equal ones the smallest batch index -- that occur in every other list,
 * ascending, with the driver's own multiplicities; count == 1 gives that list's ids.  d_out_ids: DEVICE, 4-byte aligned,
 * out_capacity entries.  *nfound (optional, host): the size of the result, set on ANSX_OK and ANSX_ERR_CAPACITY, where
 * nothing is written: d_out_ids = NULL, out_capacity = 0 is a size query.
 * How it runs: every header in one round trip; the driver decoded as ids into workspace; the other lists in ascending
 * order of n, each one step of ansx_intersect_ids_dev (ids only, the form chosen per step) over the survivors so far;
 * the loop stops as soon as a step leaves nothing, and the lists behind are not read beyond their headers; one copy.
 * Errors, in this order: before the context is touched, ANSX_ERR_ARG for a null ctx, count == 0, null arrays (d_bases
 * and nbases may be NULL for count == 1), a null d_out_ids with out_capacity > 0 or a misaligned one, and with
 * *bad_container = i for a null or misaligned d_ins[i] (16 bytes) or a misaligned d_bases[i] (4);
 *   ANSX_ERR_FORMAT with *bad_container = i for the first header that fails decode_dev's checks;
 *   ANSX_ERR_ARG with *bad_container = i for the first list but the driver, whose bases are not read, with a null
 *   d_bases[i] or nbases[i] != nblocks_i + 1;
 *   ANSX_ERR_DOMAIN with *bad_container = the driver if its sum leaves 32 bits;
 *   from a step: ANSX_ERR_FORMAT found on the device with *bad_container = count, as in the batch calls;
 *   ANSX_ERR_CAPACITY.
 * No trace is left in the context, which stays usable after any error.  Workspace: the step's own, 8 bytes per int of
 * the driver, and the whole list (4 bytes per int) of a full-form step.  Host waits: one for the headers, two for the
 * driver, two per step (selective: the planner's scalars, the status; full: the header, the status), one for the copy. */
int ansx_intersect_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint32_t* const* d_bases, const size_t* nbases, size_t count, uint32_t* d_out_ids, size_t out_capacity,
    uint64_t* nfound, size_t* bad_container, void* stream);

/* ansx_intersect_batch_dev: many conjunctive queries over one batch of gap-coded lists in one call (DESIGN.md section
 * 3j).  The batch is d_ins / in_bytes / count as above (HOST arrays of DEVICE pointers, 16-byte aligned; mixed
 * geometries allowed).  Query q names the lists terms[qoff[q] .. qoff[q + 1]) (HOST arrays; qoff has nqueries + 1
 * entries from 0, ascending, no query empty).  d_out_ids[out_offsets[q] .. out_offsets[q + 1]) is exactly what
 * ansx_intersect_dev returns for those lists in that order: the ids of the query's driver -- its list of fewest ints, of
 * equal ones the earliest position in the query -- that occur in every other list, ascending, with the driver's
 * multiplicities; a one-term query gives that list's ids.  A list may appear in many queries and more than once in
 * one.  d_out_ids: DEVICE, 4-byte aligned, out_capacity entries; out_offsets: HOST, nqueries + 1 entries,
 * out_offsets[0] = 0 and out_offsets[nqueries] the total.  No block bases are needed.
 * How it runs: the headers of the referenced containers in one round trip; the queries are cut, in order, into groups
 * whose referenced lists plus twice their drivers' ints stay within 2^28 ints (ANSX_ISECT_BATCH_INTS; a query above it
 * is a group of its own; a list two groups name is decoded in both) and whose drivers' ints stay below 2^32.  Per
 * group: its lists are decoded whole, back to back, by the passes of ansx_decode_batch_dev; one segmented scan makes
 * them ids; every query's driver ids become the candidates; then one round per non-driver list of the group's longest
 * query, lists in ascending n, over the survivors of ALL queries at once (a query with no list left passes its
 * candidates through), until nothing is left; one copy of the survivors to d_out_ids.
 * Errors, in this order: before the context is touched, ANSX_ERR_ARG for a null ctx; a null d_ins, in_bytes, terms, qoff
 * or out_offsets with nqueries > 0; a null d_out_ids with out_capacity > 0 or a misaligned one; count, nqueries or
 * qoff[nqueries] above UINT32_MAX; with *bad_query = q for qoff[0] != 0, a decrease or an empty query; with *bad_query
 * for a terms[j] >= count; with *bad_query the first query that names it and *bad_container = its batch index for a
 * null or misaligned d_ins[t] of a REFERENCED list.  nqueries == 0: ANSX_OK, nothing is launched, the context is
 * untouched.  Then ANSX_ERR_FORMAT with *bad_container = the smallest batch index of a referenced container whose
 * header fails decode_dev's checks (a single-stream stream is one such);
 *   ANSX_ERR_ARG with *bad_query for a driver of 2^32 ints or more;
 *   found on the device: ANSX_ERR_FORMAT with *bad_container = count for a bad stream or index entry; ANSX_ERR_DOMAIN
 *   with *bad_container = a referenced list whose sum leaves 32 bits -- of the first group at fault, the first in the
 *   order of its buffer (ascending batch index);
 *   ANSX_ERR_CAPACITY when the total exceeds out_capacity: out_offsets is complete, so d_out_ids = NULL, out_capacity = 0
 *   is a size query; nothing is written at or beyond d_out_ids + out_capacity, what lies below is unspecified.
 * Containers no query names are not examined and may be NULL.  No trace is left in the context, which stays usable
 * after any error.  Workspace: per group 4 bytes per int of its lists and 8 per int of its drivers (1 GiB at the
 * default budget unless one query needs more), a decode pass's, 16 bytes per 4096 ints for the scan, and per query 28
 * bytes plus 16 per non-driver term.  Host waits: one for the headers; per group those of its decode passes (header
 * and status of every pass, one more where a pass validates its index first), one for the scan's flag word and one
 * per round; one per call behind the copies, after which the call returns.  None grows with the number of queries. */
int ansx_intersect_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, const uint32_t* terms, const uint64_t* qoff, size_t nqueries, uint32_t* d_out_ids, size_t out_capacity,
    uint64_t* out_offsets, size_t* bad_container, size_t* bad_query, void* stream);

/* ansx_union_batch_dev: many disjunctive queries over one batch of gap-coded lists in one call.
 * The batch, terms, qoff, out_offsets, bad_container and bad_query are ansx_intersect_batch_dev's: HOST arrays of
 * 16-byte aligned DEVICE pointers, mixed geometries allowed; a list may appear in many queries and more than once in
 * one; containers no query names are not examined and may be NULL.  No block bases are needed.
 * d_out_ids[out_offsets[q] .. out_offsets[q + 1]) are the distinct ids that occur in at least one of the lists of
 * query q, ascending, each once: with s_t what ansx_decode_sums_dev returns for list t, the sorted distinct values of
 * the concatenation of s_t over the query's terms.  d_out_cnt (optional; DEVICE, 4-byte aligned, shares out_capacity and
 * out_offsets) holds for every id written the number of entries equal to it in that concatenation: for lists without
 * repeated ids the number of matching terms; a list named twice counts twice, a list's own repeats count.  A one-term
 * query gives that list's distinct ids.  0xFFFFFFFF is an id like any other; nothing compares with ANSX_NO_ID.
 * d_out_ids: DEVICE, 4-byte aligned, out_capacity entries; NULL only with out_capacity == 0.
 * How it runs: the headers of the referenced containers in one round trip; the queries are cut, in order, into groups
 * whose referenced lists plus twice the ints of their queries' lists as named stay within 2^28 ints
 * (ANSX_ISECT_BATCH_INTS; a query above it is a group of its own; a list two groups name is decoded in both) and whose
 * queries' lists stay below 2^32 ints together.  Per group: its lists are decoded whole, back to back, by the passes of
 * ansx_decode_batch_dev; one segmented scan makes them ids, so every list is a sorted run; ceil(log2(most terms of a
 * query)) rounds, at least one, of pairwise merges over ALL queries at once, one launch each, from host-made tables (a
 * query of fewer terms joins in the last rounds, its first round reading the decoded lists where they lie); the first
 * of every run of equal ids inside a query is kept and compacted, its count the distance to the next; one copy per
 * output to the caller.
 * Errors, in this order: before the context is touched, ansx_intersect_batch_dev's argument checks with the same
 * *bad_query / *bad_container, and ANSX_ERR_ARG for a misaligned d_out_cnt or one given with a NULL d_out_ids.
 * nqueries == 0: ANSX_OK, nothing is launched, the context is untouched.  Then ANSX_ERR_FORMAT with *bad_container = the
 * smallest batch index of a referenced container whose header fails decode_dev's checks;
 *   ANSX_ERR_ARG with *bad_query = the first query whose lists together have 2^32 ints or more (a run offset has 32
 *   bits), or the first query of a group one of whose rounds would take 2^31 workgroups or more;
 *   found on the device: ANSX_ERR_FORMAT with *bad_container = count for a bad stream or index entry; ANSX_ERR_DOMAIN
 *   with *bad_container = a referenced list whose sum leaves 32 bits -- of the first group at fault, the first in the
 *   order of its buffer (ascending batch index);
 *   ANSX_ERR_CAPACITY when the total exceeds out_capacity: out_offsets is complete, so d_out_ids = NULL, out_capacity = 0
 *   is a size query; nothing is written at or beyond out_capacity in either output, what lies below is unspecified.
 * No trace is left in the context, which stays usable after any error.  Workspace: per group 4 bytes per int of its
 * lists and 8 per int of its queries' lists as named (16 with d_out_cnt), a decode pass's, 16 bytes per 4096 ints for
 * the scan, 8 bytes per 64 merged ints, 8 bytes per query and 40 per pair, fewer than two pairs per term.  Host waits:
 * one for the headers; per group those of its decode passes and one behind the unique step (the scan's flag word, the
 * total and the queries' bounds; no size in between depends on the data); one per call behind the copies.  None grows
 * with the number of queries or of rounds. */
int ansx_union_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, const uint32_t* terms, const uint64_t* qoff, size_t nqueries, uint32_t* d_out_ids, uint32_t* d_out_cnt,
    size_t out_capacity, uint64_t* out_offsets, size_t* bad_container, size_t* bad_query, void* stream);

/* ansx_union_dev: the batch call above with the single query 0, 1, ..., count - 1 -- a thin wrapper, not a second
 * path.  *nfound (optional, host): the number of distinct ids, set on ANSX_OK and ANSX_ERR_CAPACITY, so d_out_ids = NULL,
 * out_capacity = 0 is a size query.  count == 0: ANSX_ERR_ARG, as in ansx_intersect_dev.  Every other error as above. */
int ansx_union_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, uint32_t* d_out_ids, uint32_t* d_out_cnt, size_t out_capacity, uint64_t* nfound,
    size_t* bad_container, void* stream);

/* ansx_bool_batch_dev: Boolean queries with exclusion over one batch of gap-coded lists in one call (DESIGN.md section
 * 3l).  The batch, terms, qoff, d_out_ids, out_capacity, out_offsets, bad_container, bad_query and stream are exactly
 * ansx_intersect_batch_dev's.  op says how a query's terms combine: */
#define ANSX_BOOL_ALL 0 /* a query's terms are intersected (ansx_intersect_batch_dev's result) */
#define ANSX_BOOL_ANY 1 /* a query's terms are united      (ansx_union_batch_dev's ids)        */
/* Query q EXCLUDES the lists xterms[xqoff[q] .. xqoff[q + 1]) -- HOST arrays; xqoff has nqueries + 1 entries, starts at
 * 0 and is non-decreasing: a query may exclude nothing.  xqoff == NULL: no query excludes anything, and xterms may be
 * NULL as well.  A list may be excluded by many queries and named more than once.
 * Result of query q: with P what ansx_intersect_batch_dev (ANSX_BOOL_ALL) or ansx_union_batch_dev without counts
 * (ANSX_BOOL_ANY) returns for its terms, and X the set of ids that occur in at least one of its excluded lists, P with
 * every entry whose id is in X removed; the order and, under ALL, the driver's multiplicities are kept.  0xFFFFFFFF is
 * an id like any other: membership is "found and equal", nothing compares with ANSX_NO_ID.  With no excluded list
 * anywhere the output and out_offsets are the parent call's exactly.  A list may be both a term and excluded: under ANY
 * its ids vanish, under ALL the result is empty.
 * How it runs: the headers of all REFERENCED containers -- those a term or an excluded term names; the others are not
 * examined and may be NULL -- in one round trip; the parent's groups under the same budget (ANSX_ISECT_BATCH_INTS), an
 * excluded list counting once among the group's lists; per group the parent's positive phase unchanged, then, when the
 * group excludes something and candidates are left, ONE exclusion step over the candidates of all its queries however
 * many lists they exclude (k_bool_exclude, csrc/ansx_bool.h), then the copy to the caller.  A group that excludes nothing runs
 * exactly the parent's sequence.
 * Errors, in this order: before the context is touched, the parents' argument checks on terms / qoff and the outputs with
 * the same *bad_query / *bad_container; ANSX_ERR_ARG for an op other than the two values; for a non-NULL xqoff with
 * xqoff[0] != 0 or a decrease (*bad_query = the query); for xqoff[nqueries] > UINT32_MAX; for a NULL xterms with
 * xqoff[nqueries] > 0; for an xterms[j] >= count (*bad_query); for a null or misaligned d_ins[t] of an excluded list
 * (*bad_query, *bad_container).  nqueries == 0: ANSX_OK, nothing is launched, the context is untouched.  Then
 * ANSX_ERR_FORMAT with *bad_container = the smallest referenced batch index whose header fails decode_dev's checks;
 *   ANSX_ERR_ARG with *bad_query for the parent plan's limits: ALL, the first query whose driver has 2^32 ints or more;
 *   ANY, the first query whose terms together have 2^32 ints or more, or the first query of a group one of whose rounds
 *   would take 2^31 workgroups or more.  An excluded list may have any length;
 *   found on the device: ANSX_ERR_FORMAT with *bad_container = count; ANSX_ERR_DOMAIN with *bad_container = a referenced
 *   list, an excluded one included, whose sum leaves 32 bits, as in the parents;
 *   ANSX_ERR_CAPACITY when the total exceeds out_capacity: out_offsets is complete, so d_out_ids = NULL, out_capacity = 0
 *   is a size query; nothing is written at or beyond out_capacity.
 * No trace is left in the context, which stays usable after any error.  Workspace: the parent's, with the excluded lists
 * among the group's, and 4 bytes per query and 16 per excluded term of tables.  Host waits: ALL, one more than the
 * parent per group in which the step runs; ANY, the parent's -- the number of heads stays on the device.
 * Out of scope: union counts behind an exclusion (there is no d_out_cnt), a minimum-should-match threshold, nested
 * expressions, and fusing the unique step into the last merge round. */
int ansx_bool_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    size_t count, int op, const uint32_t* terms, const uint64_t* qoff, const uint32_t* xterms, const uint64_t* xqoff,
    size_t nqueries, uint32_t* d_out_ids, size_t out_capacity, uint64_t* out_offsets, size_t* bad_container,
    size_t* bad_query, void* stream);

/* ansx_topk_batch_dev: ranked disjunctive queries over one batch of gap-coded lists in one call (DESIGN.md section 3m,
 * csrc/ansx_topk.h).  The batch, terms, qoff, bad_container, bad_query and stream are ansx_union_batch_dev's.  weights is
 * a HOST array beside terms: weights[j] belongs to the term named at terms[j].  d_pays[t] (HOST array of 16-byte aligned
 * DEVICE pointers, pay_bytes[t] its size) is a container of the same codec holding a value per posting of list t (a term
 * frequency); its header's n must equal the list's, its geometry may differ.  d_pays == NULL: every payload is 1 and
 * pay_bytes is ignored.
 * With s_t the ids ansx_decode_sums_dev gives for list t and p_t what ansx_decode_dev gives for its payload, query q scores
 *   score(d) = sum over j in [qoff[q], qoff[q + 1]), t = terms[j], of the sum over i with s_t[i] == d of weights[j] * p_t[i]
 * for every id d of its union: a list named twice contributes twice, a list's own repeated ids each contribute, a score
 * of 0 is still a result.  Its result is the union's ids ordered by (score descending, id ascending) and cut to the first
 * k, at a fixed stride: d_out_ids[q * k + r] and d_out_scores[q * k + r] (optional) for r < out_counts[q] =
 * min(k, distinct ids) -- out_counts an optional HOST array of nqueries -- and ANSX_NO_ID / 0 in the entries behind, so
 * the whole image of nqueries * k entries is defined; there is no size query.  0xFFFFFFFF is an id like any other.
 * A product weight * payload is taken in 64 bits and saturates at 2^32 - 1; the sum per id is taken in 64 bits and a sum
 * of 2^32 - 1 or more is ANSX_ERR_DOMAIN with *bad_query = the first such query in batch order (an atomic minimum on the
 * device, read back with the group's one wait); the outputs are unspecified then.
 * Errors, in this order: before the context is touched, ANSX_ERR_ARG for the parents' checks on ctx / batch / terms /
 * qoff with the same *bad_query / *bad_container; a null weights with nqueries > 0; k == 0 or k > ANSX_TOPK_MAX_K;
 * nqueries * k > UINT32_MAX; a null or misaligned d_out_ids or a misaligned d_out_scores; with d_pays, a null pay_bytes or
 * a null or misaligned d_pays[t] of a referenced list (*bad_query, *bad_container).  nqueries == 0: ANSX_OK, nothing is
 * launched, the context is untouched.  Then ANSX_ERR_FORMAT with *bad_container = the smallest referenced batch index
 * whose id header or payload header fails decode_dev's checks or whose payload's n differs from the list's;
 *   ANSX_ERR_ARG with *bad_query for the union plan's limits;
 *   found on the device: ANSX_ERR_FORMAT with *bad_container = count; ANSX_ERR_DOMAIN with *bad_container = a list whose
 *   id sum leaves 32 bits, or with *bad_query for a score (above).
 * Unreferenced containers and payloads are not examined and may be NULL.  No trace is left in the context, which stays
 * usable after any error.  Groups, workspace and host waits: DESIGN.md section 3m -- the union's groups under half of
 * ANSX_ISECT_BATCH_INTS; one wait for the headers, per group its decode passes' and ONE behind the sort, one per call.
 * Out of scope: floating-point scores (length-normalised integer impacts, BM25 among them: ansx_topk_scored_batch_dev,
 * below), k above 1024, dynamic pruning (WAND / MaxScore).  Exclusion behind a ranked query and a ranked AND:
 * ansx_topk_bool_batch_dev, below. */
#define ANSX_TOPK_MAX_K 1024u
int ansx_topk_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint64_t* qoff, size_t nqueries, uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts,
    size_t* bad_container, size_t* bad_query, void* stream);

/* ansx_topk_bool_batch_dev: ranked Boolean queries -- `+a +b` by score, anything ranked with NOT deleted behind it -- in
 * one call (csrc/ansx_topk_bool.h).  op is ANSX_BOOL_ALL or ANSX_BOOL_ANY; xterms / xqoff are
 * ansx_bool_batch_dev's (xqoff == NULL: nothing is excluded; non-decreasing; a query may exclude nothing); every other
 * argument is ansx_topk_batch_dev's.
 * The result set R(q) of query q is a set of DISTINCT ids: under ANY the ids that occur in at least one list named in its
 * terms, under ALL the ids that occur in every one of them; in both cases less every id that occurs in at least one of
 * its excluded lists.  score(d) is ansx_topk_batch_dev's formula unchanged -- the sum over the query's terms j, t =
 * terms[j], and over all i with s_t[i] == d of sat32(weights[j] * p_t[i]): a list named twice contributes twice, and a
 * list's own repeated ids each contribute, under ALL the driver's too, while the id appears once.  The output is
 * ansx_topk_batch_dev's image: R(q) ordered by (score descending, id ascending), cut to k, at stride k, ANSX_NO_ID / 0
 * behind the results, out_counts[q] = min(k, |R(q)|); 0xFFFFFFFF is an id like any other.  With op == ANSX_BOOL_ANY and
 * no exclusions every output equals ansx_topk_batch_dev's.
 * A score of 2^32 - 1 or more OF AN ID OF R(q) is ANSX_ERR_DOMAIN with *bad_query = the first such query in batch order.
 * An excluded id, and under ALL an id that a later list lacks, is no error whatever its partial sum.
 * A list that is only excluded needs no payload: its d_pays[t] is not examined and may be NULL.  Unreferenced containers
 * and payloads are not examined either.  A list may be both a term and excluded (ALL: an empty result; ANY: its ids
 * vanish).
 * Errors, in this order: before the context is touched, ANSX_ERR_ARG for ansx_topk_batch_dev's checks, for an op outside
 * the two values, and for ansx_bool_batch_dev's checks on xterms / xqoff with the same *bad_query / *bad_container.
 * nqueries == 0: ANSX_OK, nothing is launched.  Then ANSX_ERR_FORMAT with *bad_container = the smallest referenced batch
 * index whose id header fails decode_dev's checks or -- for a term's list -- whose payload header fails them or whose
 * payload's n differs, the id header before the payload;
 *   ANSX_ERR_ARG with *bad_query for the chosen plan's limits (ALL: ansx_intersect_batch_dev's; ANY: the union's);
 *   found on the device, as in the parents: ANSX_ERR_FORMAT with *bad_container = count; ANSX_ERR_DOMAIN with
 *   *bad_container = a referenced list, an excluded one included, whose id sum leaves 32 bits, or with *bad_query for a
 *   score (above).
 * No trace is left in the context, which stays usable after any error.  Groups: the chosen parent's, with the excluded
 * lists, under half of ANSX_ISECT_BATCH_INTS.  Host waits: one for the headers; per group its decode passes'; ALL: one
 * for the scan's flag word, one per round of its longest query (at least one round) and ONE behind the sort; ANY: ONE
 * behind the sort; one per call.  The exclusion step adds none.
 * Out of scope: floating-point scores (BM25-style integer impacts: ansx_topk_scored_batch_dev, below), k above 1024,
 * dynamic pruning (WAND / MaxScore), a minimum-should-match threshold, nested expressions.  (Required, optional and excluded terms with a threshold in one query:
 * ansx_topk_query_batch_dev, below.) */
int ansx_topk_bool_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, int op, const uint32_t* terms,
    const uint32_t* weights, const uint64_t* qoff, const uint32_t* xterms, const uint64_t* xqoff, size_t nqueries,
    uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts, size_t* bad_container,
    size_t* bad_query, void* stream);

/* ansx_topk_query_batch_dev: ranked flat Boolean queries -- `+a b c -d`, or `a b c d` with "at least two must match" -- in
 * one call (csrc/ansx_topk_query.h).  There is no op.  occur is a HOST array beside terms: occur[j]
 * says whether the term named at terms[j] is required (ANSX_OCCUR_MUST) or optional (ANSX_OCCUR_SHOULD); NULL: every term
 * is optional.  msm is a HOST array of nqueries thresholds; NULL: all zero.  Every other argument is
 * ansx_topk_bool_batch_dev's.
 * With s_t the ids of list t, M(q) the required and S(q) the optional terms of query q, matches(d) is the number of
 * ENTRIES equal to d in the concatenation of s_t over S(q) as named -- the count ansx_union_batch_dev writes to d_out_cnt:
 * a list named twice counts twice, and a list's own repeats count; for lists without repeats it is the number of
 * matching optional terms.  The threshold is m = msm[q] where M(q) is not empty and max(msm[q], 1) where it is: a query
 * of optional terms only must match one of them.  The result set R(q) is the set of DISTINCT ids d that occur in every
 * list of M(q), have matches(d) >= m and occur in no excluded list of q.  The host takes no shortcut from m and the
 * number of terms: the counts decide (a threshold no id reaches is an empty result).
 * score(d) is ansx_topk_batch_dev's formula unchanged over ALL of the query's terms, required and optional: the sum over
 * the postings of d of sat32(weights[j] * payload).  A list may be required and optional in one query: it scores twice
 * and counts once in matches.  A list may be both a term and excluded.  The output image, out_counts, the order (score
 * descending, id ascending) and ANSX_NO_ID / 0 behind the results are ansx_topk_bool_batch_dev's; 0xFFFFFFFF is an id
 * like any other.
 * Two identities, every output array equal byte for byte: every term MUST with msm NULL or all 0 is
 * ansx_topk_bool_batch_dev under ANSX_BOOL_ALL; every term SHOULD (or occur NULL) with every msm[q] <= 1 (or NULL) is
 * ansx_topk_bool_batch_dev under ANSX_BOOL_ANY -- and the same kernels are launched.
 * A score of 2^32 - 1 or more OF AN ID OF R(q) is ANSX_ERR_DOMAIN with *bad_query = the first such query in batch order.
 * An id that misses a required list, fails the threshold or is excluded is no error, whatever its partial sum.
 * Errors, in this order: before the context is touched, ANSX_ERR_ARG for ansx_topk_bool_batch_dev's checks less the op,
 * then for an occur[j] outside the two values (*bad_query).  nqueries == 0: ANSX_OK, nothing is launched.  Then
 * ANSX_ERR_FORMAT with *bad_container = the smallest referenced batch index, the id header before the payload; a list
 * that is only excluded needs no payload.  Then ANSX_ERR_ARG with *bad_query = the first query in batch order that
 * exceeds its plan's limits -- with a required term: its shortest REQUIRED list has 2^32 ints or more; without one: the
 * union plan's limits -- every query is planned before anything is launched.  Then the parents' device errors.
 * No trace is left in the context, which stays usable after any error.
 * Groups: the batch is cut into maximal runs of consecutive queries of one kind -- "has a required term" or "has none" --
 * and every run is planned as the parent of its kind plans it, under half of ANSX_ISECT_BATCH_INTS; the runs' groups
 * execute in batch order and every result lands at q * k.  A batch that alternates kinds gets a group per run: a caller
 * with many queries sorts them by kind.  With a required term the driver is the shortest REQUIRED list and the rounds
 * are the other required lists; ONE further launch (k_topkq_should) serves all optional lists of all queries of the
 * group, where it has an optional term or a threshold.  Without one the ANY path runs, with one filter
 * (k_topkq_atleast) where some threshold is 2 or more.
 * Host waits: exactly ansx_topk_bool_batch_dev's per group (ALL's with a required term, ANY's without); neither new step
 * adds one.  Workspace: the parent's, the optional lists among the group's decoded lists, plus per query 4 bytes of
 * threshold and 4 of table offset and per optional term 16 of table and 4 of weight (the match count lives in
 * registers); without a required term the parent's, plus 8 bytes per query (threshold and bounds) where the filter runs.
 * Out of scope: floating-point scores (BM25-style integer impacts: ansx_topk_scored_batch_dev, below), k above 1024,
 * dynamic pruning, nested expressions beyond the flat form, a threshold counted in distinct terms instead of postings, one group across query kinds, an unranked variant
 * (ansx_union_batch_dev's counts serve it). */
#define ANSX_OCCUR_SHOULD 0
#define ANSX_OCCUR_MUST 1
int ansx_topk_query_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff,
    size_t nqueries, uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts, size_t* bad_container,
    size_t* bad_query, void* stream);

/* ansx_topk_scored_batch_dev: ansx_topk_query_batch_dev with length-normalised scores -- BM25 and its kin as quantised
 * integer impacts -- in one call (csrc/ansx_topk_scored.h).  scorer stands in front of nqueries;
 * every other argument is ansx_topk_query_batch_dev's, in its order.
 * A scorer names two DEVICE arrays: d_norms, a byte per document id d < ndocs (its length class), and d_table, tf_rows
 * rows of 256 uint32_t, row-major (4-byte aligned): the impact of a payload (a term frequency) at a norm.  A payload of
 * tf_rows or more reads row tf_rows - 1; a payload of 0 reads row 0.  With a scorer the contribution of posting i of list
 * t, named at terms[j], is
 *   sat32(weights[j] * d_table[min(p_t[i], tf_rows - 1) * 256 + d_norms[s_t[i]]])
 * where the parent has sat32(weights[j] * p_t[i]).  Everything else is ansx_topk_query_batch_dev's contract word for
 * word: the result sets and matches, the thresholds, exclusion and order, the output image and out_counts, the overflow
 * rule (a score of 2^32 - 1 or more of an id of R(q)), the groups, the budget and the host waits.  The IDF is the
 * caller's weights; bm25_norms / bm25_table of the Python package make the two arrays for BM25.
 * scorer == NULL is ansx_topk_query_batch_dev: the same bytes come out and the same kernels are launched.
 * Errors, in this order: before the context is touched, ANSX_ERR_ARG for every check of ansx_topk_query_batch_dev with
 * the same *bad_query / *bad_container; then, with neither touched, for a scorer with d_pays == NULL (a term frequency is
 * needed); a null d_norms or d_table, or a d_table that is not 4-byte aligned; ndocs == 0 or ndocs > 2^32; tf_rows == 0
 * or tf_rows > 256.  nqueries == 0: ANSX_OK, nothing is launched.  Then the parent's errors, and one more found on the
 * device: an id of ndocs or more in a list that has a payload in the group -- a list some query names as a required or
 * optional term -- is ANSX_ERR_DOMAIN with *bad_container = that list's batch index; nothing is read at that id.  Where
 * several lists of a group offend, or one of them and a list whose id sum leaves 32 bits, the one first in the group's
 * buffer is named.  A list that is only excluded is never looked up: its ids may be anything.  The comparison is made in
 * 64 bits: ndocs == 2^32 admits the id 0xFFFFFFFF.  A plan's limit more: the tiles of the rewriting kernel over a
 * group, 2^31 - 1 at most (ANSX_ERR_ARG with *bad_query = the group's first query).
 * No trace is left in the context, which stays usable after any error.
 * Per group that decodes something ONE launch is added (k_topk_impacts, behind the scan, in front of the first kernel
 * that reads a payload), no host wait, no upload of its own, and 24 bytes of table per list with a payload.
 * Out of scope: floating-point scores, per-field norms or several scorers in one call, norms wider than a byte, k above
 * 1024, dynamic pruning, a scorer for the unranked calls. */
typedef struct ansx_scorer {
    const uint8_t* d_norms;  /* DEVICE, ndocs bytes: the length class of document id d */
    size_t ndocs;            /* 1 .. 2^32 */
    const uint32_t* d_table; /* DEVICE, tf_rows * 256 uint32_t, row-major: the impact of (tf, norm) */
    uint32_t tf_rows;        /* 1 .. 256; a payload of tf_rows or more reads row tf_rows - 1 */
} ansx_scorer;
int ansx_topk_scored_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff,
    const ansx_scorer* scorer, size_t nqueries, uint32_t k, uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts,
    size_t* bad_container, size_t* bad_query, void* stream);

/* ansx_topk_facets_batch_dev: ansx_topk_scored_batch_dev that also says how many documents matched and how they fall
 * over one category column -- the rest of a results page -- in one call (csrc/ansx_facet.h).
 * facets stands behind scorer and out_totals behind out_counts; every other argument is ansx_topk_scored_batch_dev's, in
 * its order.  The result set R(q), the scores, the order, the output image and out_counts are that call's, word for
 * word, with and without a scorer.  facets == NULL && out_totals == NULL is that call: the same bytes come out and the
 * same kernels are launched.
 * out_totals (optional, HOST, nqueries entries): out_totals[q] = |R(q)|, not cut to k.  It comes from the bounds the
 * group's last wait already brings home: no launch, no copy and no wait is added.  A group that ends early -- every list
 * or every driver empty, or a round that leaves nothing -- writes zeros.
 * facets (optional): d_values is a DEVICE column, the value of document id d < ndocs (4-byte aligned), and d_counts
 * DEVICE room for nqueries * nvalues counts (4-byte aligned), row q at q * nvalues:
 *   d_counts[q * nvalues + v] = the number of ids d of R(q) with d_values[d] == v, for v < nvalues.
 * A value of nvalues or more is "no value" and is counted nowhere (a caller marks documents without the field so,
 * 0xFFFFFFFF for instance); hence the sum of row q is at most out_totals[q].  An id counts once, however many postings
 * it has, and the counts run over all of R(q), not only over the k results.  The call zeroes all nqueries * nvalues
 * counts itself, on `stream`, before the first group.  After any error d_counts is unspecified.
 * A bad id: an id of ndocs or more that is an id of R(q) is ANSX_ERR_DOMAIN with *bad_query = the first such query of its
 * group; nothing is read at that id.  The comparison is made in 64 bits: ndocs == 2^32 admits the id 0xFFFFFFFF.  An id
 * that misses a required list, fails the threshold or is excluded is never looked up, whatever its value -- the rule of
 * an overflowing score.  Where a group has both a score overflow and a bad id, the overflow is reported.
 * Errors, in this order: before the context is touched, every ANSX_ERR_ARG of ansx_topk_scored_batch_dev, the scorer's
 * included, with the same *bad_query / *bad_container; then, with neither touched, ANSX_ERR_ARG for a null or misaligned
 * d_values or d_counts; ndocs == 0 or ndocs > 2^32; nvalues == 0 or nvalues > ANSX_FACET_MAX_VALUES.  nqueries == 0:
 * ANSX_OK, nothing is launched and nothing is zeroed.  Then the parent's errors and the bad id above.
 * Per group that reaches its ranked tail ONE launch is added (k_facet_count, between the last step that filters and the
 * select), no host wait and no upload of its own; the bad-id word rides home with the overflow word.  No trace is left in
 * the context, which stays usable after any error.
 * Out of scope: multi-valued fields, numeric ranges / buckets, the top values of a facet, several facet columns in one
 * call, columns narrower than 32 bits, facets for the unranked calls, a call without a ranking (k == 0). */
#define ANSX_FACET_MAX_VALUES (1u << 24)
typedef struct ansx_facets {
    const uint32_t* d_values; /* DEVICE, ndocs uint32_t, 4-byte aligned: the facet value of document id d */
    size_t ndocs;             /* 1 .. 2^32 */
    uint32_t nvalues;         /* 1 .. ANSX_FACET_MAX_VALUES: values 0 .. nvalues - 1 are counted */
    uint32_t* d_counts;       /* DEVICE, nqueries * nvalues uint32_t, 4-byte aligned, row q at q * nvalues */
} ansx_facets;
int ansx_topk_facets_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff,
    const ansx_scorer* scorer, const ansx_facets* facets, size_t nqueries, uint32_t k, uint32_t* d_out_ids,
    uint32_t* d_out_scores, uint32_t* out_counts, uint32_t* out_totals, size_t* bad_container, size_t* bad_query, void* stream);

/* ansx_topk_filter_batch_dev: ansx_topk_facets_batch_dev with range filters over document columns -- `year in [2019,
 * 2024]`, `price <= 5000`, `language != 7`, the click on a facet value (`brand == 17`) -- applied BEFORE the ranking, the
 * totals and the facet counts (csrc/ansx_filter.h).  filters stands behind facets; every other
 * argument is ansx_topk_facets_batch_dev's, in its order.  filters == NULL is that call: the same bytes come out and the
 * same kernels are launched.
 * A column is a DEVICE array of ndocs uint32_t, the value of document id d < ndocs (4-byte aligned); d_columns is a HOST
 * array of their ncolumns addresses.  Query q's clauses are clauses[fqoff[q] .. fqoff[q + 1]) (HOST).
 * A clause passes for document d iff (lo <= v && v <= hi) != ((flags & ANSX_FILTER_NOT) != 0), v = d_columns[column][d].
 * lo > hi is legal: the empty range, which with ANSX_FILTER_NOT admits every document.  No value has a special meaning: a
 * caller's "no field" marker such as 0xFFFFFFFF passes or fails like any value.  (Signed integers and floats compare as
 * uint32 after an order-preserving map: the sign bit flipped, and for floats the usual sign-dependent flip.)
 * A query's clauses are conjunctive.  A query with no clauses is not filtered and looks nothing up.
 * The result set: with R(q) the scored call's, R'(q) = { d in R(q) : every clause of q passes }.  Everything
 * ansx_topk_facets_batch_dev defines over R(q) is defined over R'(q), word for word: the scores and the order (score
 * descending, id ascending), the output image with ANSX_NO_ID / 0 behind it, out_counts[q] = min(k, |R'(q)|),
 * out_totals[q] = |R'(q)|, the facet counts, and the overflow rule: a score of 2^32 - 1 or more is an error only for an
 * id of R'(q).
 * A bad id: an id of ndocs or more that is in R(q) of a query with at least one clause is ANSX_ERR_DOMAIN with
 * *bad_query = the first such query of its group; nothing is read at that id.  The comparison is made in 64 bits:
 * ndocs == 2^32 admits the id 0xFFFFFFFF.  An id that misses a required list, fails the threshold or is excluded is never
 * looked up, whatever its value.  Where one group has several errors the order is: the score overflow, then the filter's
 * bad id, then the facets' bad id.
 * Errors, in this order: before the context is touched, every ANSX_ERR_ARG of ansx_topk_facets_batch_dev (the scorer's
 * and the facets' included), with the same *bad_query / *bad_container; then, with neither touched, ANSX_ERR_ARG for a
 * null d_columns or fqoff, or null clauses with fqoff[nqueries] > 0; ncolumns == 0 or above ANSX_FILTER_MAX_COLUMNS;
 * a null or misaligned column that some clause of clauses[0 .. fqoff[nqueries]) names (a column no clause names is never
 * touched and may be null); ndocs == 0 or ndocs > 2^32; fqoff[0] != 0 or a descending fqoff; then, with *bad_query = the first offending query, more than
 * ANSX_FILTER_MAX_CLAUSES clauses, a column >= ncolumns, a flags with a bit other than ANSX_FILTER_NOT.  nqueries == 0:
 * ANSX_OK, nothing is launched.  Then the parent's errors and the bad id above.
 * Per group in which some query has a clause: where the group excludes something ONE launch is added (k_filter_mark
 * between k_bool_exclude and its compaction), else five (k_filter_mark and a compact step); Q + 1 offsets and 24 bytes
 * per clause ride in the group's one upload, the bad-id word rides home with the overflow word, and no host wait is
 * added.  A group none of whose queries has a clause launches and uploads nothing more.  No trace is left in the
 * context, which stays usable after any error.
 * Out of scope: OR between clauses, multi-valued fields, columns narrower or wider than 32 bits, drill-sideways facet
 * counts (a facet's counts without its own filter), filters for the unranked calls, a bitmap of live documents. */
#define ANSX_FILTER_MAX_COLUMNS 64u
#define ANSX_FILTER_MAX_CLAUSES 16u /* per query */
#define ANSX_FILTER_NOT 1u
typedef struct ansx_filter_clause { uint32_t column, lo, hi, flags; } ansx_filter_clause; /* HOST */
typedef struct ansx_filters {
    const uint32_t* const* d_columns;  /* HOST array of ncolumns DEVICE pointers, each ndocs uint32_t, 4-byte aligned */
    uint32_t ncolumns;                 /* 1 .. ANSX_FILTER_MAX_COLUMNS */
    size_t ndocs;                      /* 1 .. 2^32, one for all columns */
    const ansx_filter_clause* clauses; /* HOST, fqoff[nqueries] entries */
    const uint64_t* fqoff;             /* HOST, nqueries + 1: query q's clauses are [fqoff[q], fqoff[q + 1]) */
} ansx_filters;
int ansx_topk_filter_batch_dev(ansx_ctx* ctx, int kind, int fidelity, const uint8_t* const* d_ins, const size_t* in_bytes,
    const uint8_t* const* d_pays, const size_t* pay_bytes, size_t count, const uint32_t* terms, const uint32_t* weights,
    const uint8_t* occur, const uint64_t* qoff, const uint32_t* msm, const uint32_t* xterms, const uint64_t* xqoff,
    const ansx_scorer* scorer, const ansx_facets* facets, const ansx_filters* filters, size_t nqueries, uint32_t k,
    uint32_t* d_out_ids, uint32_t* d_out_scores, uint32_t* out_counts, uint32_t* out_totals, size_t* bad_container,
    size_t* bad_query, void* stream);

/* Multi-GPU concatenation (the path shards by contiguous ranges of whole blocks, one container per
 * GPU; the reference is single-threaded and has no counterpart -- its per-block calls in
 * src/pseudo_adaptive.cpp:77-130 are the unit that is sharded).  d_parts[i] (8-byte aligned DEVICE
 * pointers, HOST array) are `nparts` <= 64 containers of the same codec / block_ints / ckpt_interval, in
 * list order, every one but the last holding whole blocks only; part_bytes[i] bounds each.  Writes ONE
 * container over all their blocks to d_out (16-byte aligned device memory, which must not overlap the
 * parts): index entries rebased, restart points and payload copied by one HIP kernel.  ansx_decode_dev
 * on the result returns the concatenated list.  The parts must agree on the restart-point format too (their
 * kind words are compared whole); a part that needed the wide form next to parts that did not is refused
 * (ANSX_ERR_FORMAT) -- encode such inputs with ANSX_WIDE_RESTART set on every rank. */
int ansx_merge_containers_dev(ansx_ctx* ctx, const uint8_t* const* d_parts, const size_t* part_bytes, int nparts,
    uint8_t* d_out, size_t out_capacity, size_t* out_bytes, void* stream);

/* The same over RCCL, for a C / C++ host with one process (or thread) per GPU: every rank calls this
 * with its own container; sizes are exchanged with ncclAllGather, every rank sends its container straight to the root
 * (grouped ncclSend / ncclRecv: one hop, each sender on its own xGMI link), and the root merges the slots with
 * ansx_merge_containers_dev.  nccl_comm: an ncclComm_t of the system's RCCL (librccl.so.1 is resolved at first use,
 * this library does not link it).  d_recv (root only): nranks * slot_bytes bytes, 16-byte aligned slots; a rank
 * container larger than slot_bytes fails the call on every rank (ANSX_ERR_CAPACITY).  *merged_bytes: size of the
 * merged container on the root, 0 elsewhere.  Blocks until the sizes are known; the transfers and the merge run on
 * `stream`.  slot_bytes is the ROOT's: it travels with the sizes, every rank checks every container against it and all
 * ranks return the same ANSX_ERR_CAPACITY together (a non-root rank's own argument is ignored).  A non-root rank returns
 * with its ncclSend queued on `stream`: d_container must stay untouched until that stream has been synchronised. */
int ansx_gather_containers(ansx_ctx* ctx, void* nccl_comm, int rank, int nranks, int root, const uint8_t* d_container,
    size_t bytes, uint8_t* d_recv, size_t slot_bytes, uint8_t* d_merged, size_t merged_cap, size_t* merged_bytes,
    void* stream);

/* Ranks of the communicator the context's most recent ansx_gather_containers call ran on, as RCCL itself reports them
 * (ncclCommCount); 0 before the first call.  For bench lines / logs that must show N GPUs really took part. */
int ansx_last_gather_ranks(const ansx_ctx* ctx);

/* Parse + validate a container header held in HOST memory. */
int ansx_container_info(const uint8_t* container, size_t bytes, ansx_container_header* out);

/* Per-kernel device timing (hipEvent pairs around every launch) for bench.py's roofline leg. */
int ansx_profile_enable(ansx_ctx* ctx, int on);
int ansx_profile_reset(ansx_ctx* ctx);
int ansx_profile_get(ansx_ctx* ctx, ansx_kernel_time* out, int max_entries, int* count);

/* Facts about the context's most recent ansx_encode / ansx_encode_dev call.
 *   near_threshold_decisions  frame-size stop-rule comparisons XH < 1.001 H (ans_util.hpp:149) whose two sides
 *                             agreed to 1e-12 relative.  The reference evaluates log2 with libm, this library
 *                             with its own portable log2 (<= 1 ulp apart): such a comparison is the only place
 *                             where the two could decide differently.  Expected to be 0, always.  Blocks with
 *                             such a comparison are decided again on the host with libm's log2 (the reference's
 *                             own arithmetic, ans_util.hpp:100-157), and if the host disagrees the call is
 *                             repeated with its decision forced: parity does not rest on this being 0.
 *   host_redecided            blocks whose frame size the host's re-decision changed (expected 0)
 *   path                      0 discovery (alphabet size read back mid-call), 1 launched back to back on the
 *                             context's hints for this geometry (largest alphabet; for ANSrfold and the
 *                             compaction layer also the most distinct values a block had, which sizes their
 *                             per-block hash tables), 2 the same with the fused model kernel; + 16: a hint
 *                             did not hold and the call was repeated on the discovery path; + 32: a frame above
 *                             2^16 turned up in a call laid out for packed restart points and the call was
 *                             repeated with wide ones (remembered per geometry, but only as the attempt to run
 *                             FIRST); + 64: the remembered wide form was not needed by this input and the call was
 *                             repeated with packed restart points; + 128: the producer / consumer encoder kernel
 *                             (k_encode_pc) ran in the attempt whose container was returned (never a leftover of an
 *                             earlier attempt or call: an attempt that ends in the integer-state encoder clears it); + 256: plain ANSint modelled in rank space (values of 16384 and more; remembered per geometry
 *                             as the attempt to run first, and given up again by a call whose values are small); + 512: that call was repeated with
 *                             the full-size arrays of the value-range prelude writer.  Either way the output bytes -- the restart-point
 *                             format included -- are a function of the input and the options only. */
typedef struct {
    uint32_t max_nsyms;
    uint32_t max_log2_frame;
    uint32_t near_threshold_decisions;
    uint32_t path;
    uint32_t host_redecided;
} ansx_encode_stats;
int ansx_last_encode_stats(const ansx_ctx* ctx, ansx_encode_stats* out);

/* The forms of the context's most recent encode, as they were launched: which instantiation of every templated kernel
 * of the model phase, the remap front, the prelude writers and the encoder ran, and in what shape (DESIGN.md section 5,
 * "Host side of an encode call").  The fields are copies of the values the launches were made with, for the attempt
 * whose container was returned (a repeated call reports its last attempt).  ansx_encode_batch_dev reports its last
 * pass -- or the last list that went alone -- and, unlike ansx_last_encode_stats, does not put the earlier report
 * back.  A call that fails leaves the previous values.  For tests and logs: no encode path looks at it.
 *   attempt           ANSX_FORM_OPTIMISTIC   launched back to back on the geometry's hints (ns_cap != 0), else discovery
 *                     ANSX_FORM_FAST_MODEL   k_candidates / k_model_finish instead of the exact model kernels
 *                     ANSX_FORM_FUSED        k_model_fused (hist, sort, fin and prelude are then "NONE")
 *                     ANSX_FORM_RANK_SPACE   plain ANSint modelled in rank space
 *                     ANSX_FORM_SP_FULL_LDS  ... and its prelude writer repeated with the full-size LDS arrays
 *                     ANSX_FORM_BATCH_PASS   a pass of ansx_encode_batch_dev (blocks through the per-block table)
 *   ns_cap, nt        the alphabet hint of the attempt (0: discovery) and the candidates per block of the fast model
 *                     path (0: the exact model kernels)
 *   hist .. big_geo   the model phase: k_fold_hist's variant, its workgroups per block (cpb), whether the entropy sum is
 *                     deferred to k_sort_entropy / taken in k_fold_hist itself; k_sort_entropy's variant;
 *                     k_model_finish's variant (ANSX_FIN_NONE where it did not run) and alphabet capacity (fcap, 0
 *                     likewise); chains per lane of the last k_candidates launch (0: none); the block-range pipeline's
 *                     range count (0: one launch of each kernel over all blocks) and blocks per range; whether
 *                     k_model_finish<0> took its tree nodes from the table built for alphabets above 4096 slots
 *   rf .. pa_uqcap    the remap front: ANSrfold's form (ANSX_RF_NONE: no ANSrfold) and its table slots; the compaction
 *                     layer's (and rank-space ANSint's) hash-set and value-list sizes, pa_small: the hint-sized kernel
 *                     (all three 0 where neither ran; a batch pass: of its large class)
 *   prelude ..        the exact form's prelude writer (ANSX_PRE_NONE: k_model_finish or k_model_fused wrote the
 *   pre_cap           preludes), whether k_table16_from32 ran first, and the writer's array length (0 under NONE)
 *   enc .. first      the encoder: the kernel that took the blocks the pair kernel left (ANSX_ENC_NONE: it left none)
 *                     with its grid, threads and bytes of dynamic LDS; the criterion that chose the pair kernel
 *                     (ANSX_PC_NONE: none) with its pairs per workgroup and S -- pc_grid == 0 with a criterion: the
 *                     restart rule then refused it --, the pair launch's workgroups and the blocks it took (first)
 *   nblocks           blocks of the call (a batch pass: of the pass) */
typedef enum { ANSX_HIST_WORDS = 0, ANSX_HIST_PACKED = 1, ANSX_HIST_NONE = 2 } ansx_form_hist;
typedef enum { ANSX_SORT_U16 = 0, ANSX_SORT_U32 = 1, ANSX_SORT_U32_UNSTAGED = 2, ANSX_SORT_NONE = 3 } ansx_form_sort;
typedef enum { ANSX_FIN_WAVES = 0, ANSX_FIN_16_5 = 1, ANSX_FIN_16_8 = 2, ANSX_FIN_ONE_WAVE_5 = 3, ANSX_FIN_ONE_WAVE_8 = 4,
    ANSX_FIN_GENERIC_5 = 5, ANSX_FIN_GENERIC_8 = 6, ANSX_FIN_NONE = 7 } ansx_form_fin;
/* (ANSX_RF_SORT: no geometry reaches it while ANSX_RF_HBM_HASH takes every ANSrfold-6 and -7 list) */
typedef enum { ANSX_RF_NONE = 0, ANSX_RF_HBM_HASH = 1, ANSX_RF_LDS_OPT = 2, ANSX_RF_LDS_FULL = 3, ANSX_RF_SORT = 4 } ansx_form_rf;
typedef enum { ANSX_PRE_W4 = 0, ANSX_PRE_W16 = 1, ANSX_PRE_RANK_SPACE = 2, ANSX_PRE_GENERIC = 3, ANSX_PRE_GENERIC_HBM = 4,
    ANSX_PRE_NONE = 5 } ansx_form_prelude;
typedef enum { ANSX_ENC_INT_STATE = 0, ANSX_ENC_MODE1 = 1, ANSX_ENC_MODE2 = 2, ANSX_ENC_NONE = 3 } ansx_form_enc;
typedef enum { ANSX_PC_NONE = 0, ANSX_PC_A = 1, ANSX_PC_B = 2, ANSX_PC_C = 3 } ansx_form_pc;
#define ANSX_FORM_OPTIMISTIC 1u
#define ANSX_FORM_FAST_MODEL 2u
#define ANSX_FORM_FUSED 4u
#define ANSX_FORM_RANK_SPACE 8u
#define ANSX_FORM_SP_FULL_LDS 16u
#define ANSX_FORM_BATCH_PASS 32u
typedef struct {
    uint32_t attempt, ns_cap, nt;
    uint32_t hist, cpb, h_deferred, h_in_hist, sort, fin, fcap, cand_chains, nranges, range_blocks, big_geo;
    uint32_t rf, rf_slots, pa_small, pa_slots, pa_uqcap;
    uint32_t prelude, table16_first, pre_cap;
    uint32_t enc, enc_grid, enc_threads, enc_lds, criterion, pairs, S, pc_grid, first;
    uint32_t nblocks;
} ansx_encode_form_report;
int ansx_last_encode_form(const ansx_ctx* ctx, ansx_encode_form_report* out);

/* The form of the context's most recent decode, as it ran: which prelude parser and which block decoder, in what
 * launch shape.  Every read call ends in one decode of a container or of a sub-container built for the call (the range
 * calls, the batch calls pass by pass, the sums / ids variants, next_geq); the fields describe that decode, for the
 * attempt whose result was returned, and the last pass of a call wins.  A call that fails before a form is chosen
 * leaves the previous values.  For tests and logs: no decode path looks at it.
 *   parser            ANSX_PARSER_DONE     plain ANSint: k_int_sparse_parse has filled the tables, no parser launch
 *                     ANSX_PARSER_GENERIC  the generic kernel, one lane per block
 *                     ANSX_PARSER_PAR      eight lanes per block on the container's parse hints (the default);
 *                                          p_variant 0 windowed subtrees, 1 u16 value arrays, 2 u32 value arrays
 *                     ANSX_PARSER_FAST     one lane per block, the E-array fast loop; p_variant = staged words
 *                     ANSX_PARSER_WIN      one lane per block, windowed; p_variant = staged words (128 | 256)
 *   decoder           ANSX_DECODER_STAGED      rank / select tables, one block per workgroup; stream_cap != 0: the
 *                                              block's stream staged in LDS, 0: read from HBM
 *                     ANSX_DECODER_RING        the same with per-quad 512-byte stream rings
 *                     ANSX_DECODER_SMALL_RING  the same with per-quad 256-byte speculative rings
 *                     ANSX_DECODER_PAIR        two blocks per workgroup, 512-byte rings
 *                     ANSX_DECODER_TABLE       slot -> symbol tables in LDS (stream_cap as for STAGED)
 *                     ANSX_DECODER_GTAB        slot -> symbol tables in HBM (frames above 2^16 that LDS cannot hold)
 *   p_grid .. d_lds   workgroups, threads per workgroup and bytes of dynamic LDS of the parser's and of the decoder's
 *                     launch (p_lds 0 and the parser's shape unused under ANSX_PARSER_DONE)
 *   stream_cap        bytes of LDS a block's stream is staged in (STAGED and the table forms), else 0
 *   maxM, max_ns, max_ep, max_block_bytes
 *                     the bounds the form was chosen from: largest frame, bound on a block's symbol indices, bound on
 *                     the symbols present in a block, largest block stream (0: never looked up -- the ring forms do
 *                     not need it)
 *   nblocks           blocks of the container that was decoded (a range call: the touched blocks; a batch call: the
 *                     blocks of its last pass)
 *   flags             ANSX_DECODE_INDEX_VALIDATED  k_validate_index ran and its result was read back before the form
 *                                                  was chosen
 *                     ANSX_DECODE_ON_REMEMBERED    the attempt ran on the header remembered for the container's shape
 *                     ANSX_DECODE_REPEATED         an attempt on a remembered header was given up and the call repeated
 *                                                  on the container's own */
typedef enum { ANSX_PARSER_DONE = 0, ANSX_PARSER_GENERIC = 1, ANSX_PARSER_PAR = 2, ANSX_PARSER_FAST = 3, ANSX_PARSER_WIN = 4 } ansx_parser;
typedef enum { ANSX_DECODER_STAGED = 0, ANSX_DECODER_RING = 1, ANSX_DECODER_SMALL_RING = 2, ANSX_DECODER_PAIR = 3,
    ANSX_DECODER_TABLE = 4, ANSX_DECODER_GTAB = 5 } ansx_decoder;
#define ANSX_DECODE_INDEX_VALIDATED 1u
#define ANSX_DECODE_ON_REMEMBERED 2u
#define ANSX_DECODE_REPEATED 4u
typedef struct {
    uint32_t parser, p_variant, decoder;
    uint32_t p_grid, p_threads, p_lds;
    uint32_t d_grid, d_threads, d_lds;
    uint32_t stream_cap;
    uint32_t maxM, max_ns, max_ep, max_block_bytes;
    uint32_t nblocks;
    uint32_t flags;
} ansx_decode_stats;
int ansx_last_decode_stats(const ansx_ctx* ctx, ansx_decode_stats* out);

/* Synthetic inputs of the reference's benchmark harness (src/generate_inputs.cpp:94-122, include/
 * zipf_dist.hpp:49-59) as counter-based generators: element i is a pure function of (seed, first_index + i),
 * so a list can be produced in pieces, on any number of GPUs, or on the host, with identical values.
 *   ANSX_GEN_UNIFORM    a = lo, b = hi (inclusive)            std::uniform_int_distribution
 *   ANSX_GEN_GEOMETRIC  a = p                                 std::geometric_distribution (failures before a success)
 *   ANSX_GEN_ZIPF       a = n (values 1..n), b = exponent q   zipf_distribution (rejection-inversion)
 * The distributions are the reference's; the random stream is not (std::mt19937 + libstdc++ + libm cannot be
 * reproduced bit for bit on a GPU).  ansx_generate_dev writes to device memory on `stream` (NULL = the
 * context's stream) and returns without synchronising; ansx_generate_host is the same function on the CPU. */
typedef enum { ANSX_GEN_UNIFORM = 0, ANSX_GEN_GEOMETRIC = 1, ANSX_GEN_ZIPF = 2 } ansx_gen_dist;
int ansx_generate_dev(ansx_ctx* ctx, int dist, double a, double b, uint64_t seed, uint64_t first_index,
    uint32_t* d_out, size_t n, void* stream);
int ansx_generate_host(int dist, double a, double b, uint64_t seed, uint64_t first_index, uint32_t* out, size_t n);

/* Test / experiment hook: select one of the equivalent internal code paths (all must produce identical
 * bytes).  Names are those of the environment variables read once by ansx_init: ANSX_DECODE_MODE
 * ("ring" | "staged"; ""/"0"/NULL: the default; anything else: ANSX_ERR_ARG), ANSX_DECODE_TABLE,
 * ANSX_NO_STREAM_LDS, ANSX_PARSE_GENERIC, ANSX_PARSE_WIN, ANSX_PARSE_FAST,
 * ANSX_PARSE_STAGE_WORDS (number), ANSX_ENCODE_GTAB16, ANSX_TEST_TABLE16_FIXUP, ANSX_MODEL_FUSED, ANSX_MODEL_SYNC,
 * ANSX_NS_HINT (number: alphabet-size hint for every call instead of the per-geometry one the context
 * learns; too small a value only costs a repeat on the general path), ANSX_T_HINT (number: candidate frame sizes per
 * block of the fast model path), ANSX_NO_FAST_MODEL, ANSX_FAST_GUARD / ANSX_NEAR_BAND (numbers: relative bands around
 * the stop-rule threshold inside which the fast path repeats on the exact one / the host re-decides),
 * ANSX_TEST_NEAR_FLIP (the device decides close calls the wrong way), ANSX_CAND_CHAINS (1 | 2), ANSX_MODEL_PIPELINE
 * ("never" | "always" | a range count 1 .. 64; ""/"0"/NULL: by the call's size; anything else: ANSX_ERR_ARG -- the
 * block-range pipeline of the fast model path: the call's blocks in contiguous ranges, their histograms one after the
 * other on the caller's stream, the model kernels of every range but the last on two side streams of the context, all
 * joined on the caller's stream in front of the encoder; "always" / a number pipeline any list that takes the fast model
 * path, however short, except in per-kernel profile mode and on a stream that is being captured), ANSX_WIDE_RESTART
 * (wide restart points in every container -- the one switch here that changes the output: the index, not the block
 * streams), ANSX_TEST_WIDE_AT (number <= 16: frames above 2^this count as too large for packed restart points),
 * ANSX_DECODE_SETUP ("old"; ""/"0"/NULL: the default; anything else: ANSX_ERR_ARG -- the per-block setup of a decode
 * call as it was before the value-array subtree parser and the scan-free table build: windowed subtrees in
 * k_parse_prelude_par whatever the alphabet, one prefix scan per round of symbols in the decoder's table build; for the
 * cross-check test and the paired timing of tests/tools/bench_decode_setup.py), ANSX_MODEL_CHAIN ("old"; ""/"0"/NULL:
 * the default; anything else: ANSX_ERR_ARG -- the fast model path as it was before k_model_maxima: every block of
 * k_model_finish reads and raises the call's running maxima itself; for the cross-check test and the paired timing of
 * tests/tools/bench_model_chain.py), ANSX_INTERSECT_FORM ("selective" | "full"; ""/"0"/NULL: by the candidates per block;
 * anything else: ANSX_ERR_ARG -- the form of every step of ansx_intersect_ids_dev and ansx_intersect_dev; for the tests,
 * which compare the two, and the timing of tests/tools/bench_intersect.py), ANSX_ISECT_BATCH_INTS (number: the ints a
 * group of ansx_intersect_batch_dev may take, its lists once and its drivers' twice, and a group of ansx_union_batch_dev,
 * its lists once and its queries' lists as named twice; ""/"0"/NULL: 2^28 -- the results do not depend on it; the tests
 * force several groups and a group per query), ANSX_BOOL_FORM ("search" | "staged"; ""/"0"/NULL: the default rule;
 * anything else: ANSX_ERR_ARG -- how a tile of k_bool_exclude that lies inside one query meets an excluded list: "search"
 * never stages the list's range in LDS, "staged" stages it whenever it fits ANSX_BOOL_STAGE ints; the outputs are the
 * same; for the tests, which compare them, and the timing of tests/tools/bench_bool_batch.py);
 * through this call only (round 4): ANSX_NO_PC / ANSX_FORCE_PC / ANSX_NO_PC_AUTO / ANSX_PC_B_PAIRS (the producer /
 * consumer encoder never / whatever the list length / only on request; pairs per workgroup of its two-round shape),
 * ANSX_ENCODE_MODE2, ANSX_DECODE_PAIR, ANSX_DECODE_SMALL_RING ("never" | "always"; ""/"0"/NULL: the default; anything
 * else: ANSX_ERR_ARG, as for ANSX_DECODE_MODE), ANSX_FORGET_HINTS, ANSX_NO_BIG_GEO,
 * ANSX_FIN_ONE_WAVE, ANSX_TEST_SP_BITS (number: words of the rank-space ANSint prelude writer's bit buffer on its first
 * attempt), ANSX_RANGE_SUMS_WG_MAX (number: the largest block_ints whose touched blocks the sums variants of the range
 * calls scan in one kernel, a workgroup per block; larger blocks take the three-phase scan; ""/"0"/NULL: 65536 -- for the
 * paired timing of tests/tools/bench_range_sums.py, the results do not depend on it)  (flags: "1" on, "0"/""/NULL off).
 * Unknown name: ANSX_ERR_ARG.  ansx_init, which has no way to return such an error, leaves a key whose environment value
 * is refused at its default and says so in one line on stderr. */
int ansx_debug_set(ansx_ctx* ctx, const char* name, const char* value);

/* Bytes of device workspace currently held by the context. */
size_t ansx_workspace_bytes(const ansx_ctx* ctx);

/* One pass of the Zipf generator's rejection loop for a given canonical uniform u01 in [0, 1] (unit tests: the map
 * uniform -> value is compared with include/zipf_dist.hpp:49-59 driven by the same uniforms): candidate value *k and
 * whether it is accepted.  Host only, no device needed. */
int ansx_zipf_from_uniform(double n, double q, double u01, uint32_t* k, int* accepted);

/* Host evaluation of the portable log2 used by the device normaliser (unit tests only). */
double ansx_host_log2(double x);
/* The same function evaluated on the DEVICE for n inputs (host arrays): the normaliser relies on
 * host and device results being bit-identical. */
int ansx_selftest_log2(ansx_ctx* ctx, const double* in, double* out, size_t n);
/* The normaliser's division helper (exact for integer-valued operands below 2^31, see
 * csrc/ansx_dev.h) evaluated on the device: out[i] = a[i] / b[i], to be compared with IEEE division. */
int ansx_selftest_div(ansx_ctx* ctx, const double* a, const double* b, double* out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* ANSX_H */
