// ansx -- the integer names and the plain structs and constants the host's plans (ansx_plan.h) fill and the kernels read
// them through.  No code: it builds with a plain host compiler, and the kernel headers take it through ansx_dev.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;

// One block of a batch pass: its ints and where they start in the pass's output.  Blocks of many containers share one
// sub-container there, so any of them may be short and the output of block b does not start at b * block_ints.
struct ansx_blk_out {
    u64 off;  // first int in the output (a multiple of 4: the decoders' 16-byte stores)
    u32 n;    // ints
    u32 pad_;
};

struct ansx_range_piece {  // one range with count > 0: where its ints sit in the sub-list and in the output
    u64 src, dst, count;
};

#define ANSX_RANGE_CHUNK 4096u  // ints per workgroup of k_range_gather

struct ansx_batch_src {  // a source container of a pass
    u64 base;            // its device address
    u64 ckoff_off, ckstate_off, hint_off, payload_off;  // its layout (make_plan's for its own n)
    u64 payload_bytes;   // its header's: index_entry_ok on its own entries
    u32 nblocks;
    u32 pad_;
};

struct ansx_batch_blk {  // block k of a pass is block b of source src
    u32 src, b;
};

struct ansx_piece {  // ints [src, src + count) of the pass's work list go to [dst, dst + count) of the caller's buffer;
    u64 src, dst;    // count = wpos[i + 1] - wpos[i], wpos the exclusive prefix of the counts over the pass (count > 0)
};

#define ANSX_PIECE_CHUNK 4096u  // ints per workgroup of k_piece_gather (k_range_gather's chunk)

// LDS geometry of the decode kernels, shared with the host's choice of the decode form (ansx_decode_form.h), which
// sizes the dynamic LDS the kernels carve.
#define ANSX_PF_SW 128u            // k_parse_prelude_fast: staged words per lane
#define ANSX_PAR_SW 32u            // k_parse_prelude_par: staged words per lane
#define ANSX_PAR_STK 11u           // stack rows of its value-array form: depth <= 10 (subtrees of <= 1023 items) + dump
#define ANSX_PAR_SLICE_WORDS ((ANSX_PAR_SW + 48u) * 64u)  // a wave's LDS slice: stage + the windowed form's 3 x 16 stack rows
// per-quad stream ring of the block decoder: ANSX_RING_CHK steps per refill check, 32 bytes per lane and step of check
// interval per refill (>= the 28 bytes a quad can consume per step)
#ifndef ANSX_RING_CHK
#define ANSX_RING_CHK 4
#endif
#define ANSX_DEC_SCRATCH 96u  // k_decode_rank: scan scratch + error flag between the tables and the stream area
#define ANSX_RING_BYTES (128 * ANSX_RING_CHK)
#define ANSX_RING_STRIDE (ANSX_RING_BYTES + 16)  // + 8 mirror bytes (ring bytes 0..7 once more) and padding to 16
#define ANSX_SRING_BYTES 256                       // the speculative small ring, see dec_segments_ring_small
#define ANSX_SRING_STRIDE (ANSX_SRING_BYTES + 16)

struct ansx_brs_src {  // a source of a pass, beside its ansx_batch_src: the caller's bases of that container
    u64 bases;         // device address of its nblocks + 1 entries (4-byte aligned)
    u32 nblocks;
    u32 pad_;
};
