"""Size regimes, the part that needs no device: the Python builder's restart-point form on both sides of the cursor
rule, ansx_bound against the builder's containers at the rungs of the block-size ladder, and the option limits
("Size regimes"; the GPU side is test_gpu_size_regimes.py)."""
import ctypes as C

import numpy as np
import pytest

import container_py as cp
import oracle_lib as ol

CURSOR_LIMIT = 1 << 24
PAIR_MAX_BLOCK_INTS = 1 << 22
STREAM_LIMIT = 1 << 31  # a block's worst-case stream (+ 16) stays below this


@pytest.fixture(scope="module")
def A(oracle_built):
    import ans_large_alphabet_amd as A_

    return A_


def bound(A, kind, f, n, block_ints=0, ckpt_interval=0, flags=0):
    o = A.make_opts(block_ints, ckpt_interval, flags)
    return A.lib().ansx_bound(kind, f, n, C.byref(o))


CODECS = [(ol.FOLD, 1), (ol.FOLD, 5), (ol.FOLD, 7), (ol.RFOLD, 1), (ol.RFOLD, 3), (ol.MSB, 0), (ol.INT, 0)]


@pytest.mark.parametrize("kind,f", CODECS)
def test_bound_formula_and_thresholds(kind, f):
    """block_bound as documented, and the geometries the GPU tests sit on: multiples of 4 on both sides of each rule."""
    nsp = {ol.MSB: 2048, ol.INT: 16384}.get(kind, 1 << (f + 9))
    hdr = 4 + 4 * (1 << (f + 7)) if kind == ol.RFOLD else 0
    assert cp.block_bound(kind, f, 16384) == hdr + 8 + 4 * nsp + 7 * 16384 + 32
    assert cp.block_bound(kind, f, 16384, compact=True) == cp.block_bound(kind, f, 16384) + 8 + 4 * 16384 + 8
    assert cp.scratch_stride(kind, f, 16384) % 256 == 0 and 0 <= cp.scratch_stride(kind, f, 16384) - cp.block_bound(kind, f, 16384) - 16 < 256
    at = cp.first_block_ints(lambda b: cp.block_bound(kind, f, b) + 16 >= CURSOR_LIMIT)
    assert at % 4 == 0 and not cp.wide_by_geometry(kind, f, at - 4) and cp.wide_by_geometry(kind, f, at)
    assert cp.block_bound(kind, f, at - 4) + 16 < CURSOR_LIMIT <= cp.block_bound(kind, f, at) + 16
    assert 2_300_000 < at < 2_400_000  # "about 2.4 M ints"


def test_builder_decides_the_form_from_the_geometry():
    """The same 41 ints: packed in blocks below the cursor rule, wide at it -- although no cursor comes near 2^24 (the
    form follows from block_ints, not from the streams) -- and pack_restart_points still refuses a cursor it cannot hold."""
    data = ol.gen_inputs("zipf20s1.2", 41, seed=1)
    at = cp.first_block_ints(lambda b: cp.block_bound(ol.FOLD, 1, b) + 16 >= CURSOR_LIMIT)
    below, wide = (cp.build_container(ol.FOLD, 1, data, b, 16) for b in (at - 4, at))
    hb, hw = (np.frombuffer(c[:64].tobytes(), dtype=np.uint32) for c in (below, wide))
    assert hb[2] == ol.FOLD and hw[2] == ol.FOLD | 0x200
    assert hb[6] == at - 4 and hw[6] == at
    cpb = [cp.nseg(b, 16) - 1 for b in (at - 4, at)]
    # the two forms hold the same restart points: two (41 ints, one every 16) in thousands of slots
    s, info, st, off = ol.oracle_encode(ol.FOLD, 1, data, ckpt_interval=16)
    assert st.shape[0] == 2
    lay = cp.layout(1, cpb[1], True)
    assert np.array_equal(wide[lay[1]:lay[1] + 8].view(np.uint32), off)
    assert np.array_equal(wide[lay[2]:lay[2] + 64].view(np.uint64).reshape(2, 4), st)
    assert np.array_equal(below[80:80 + 58], cp.pack_restart_points(st, off))
    assert np.array_equal(below[-s.size:], s) and np.array_equal(wide[-s.size:], s)
    # header, two index entries, the restart points (29 bytes each | u32 cursors, pad to 8, 4 x u64 states), pad to 16, hints
    assert below.size == (80 + 29 * cpb[0] + 15) // 16 * 16 + 32 + s.size
    assert wide.size == ((80 + 4 * cpb[1] + 7) // 8 * 8 + 32 * cpb[1] + 15) // 16 * 16 + 32 + s.size
    # an explicit form overrides the rule
    assert np.array_equal(cp.build_container(ol.FOLD, 1, data, at - 4, 16, wide=True)[8:12].view(np.uint32), [ol.FOLD | 0x200])
    with pytest.raises(AssertionError):
        cp.pack_restart_points(np.zeros((1, 4), dtype=np.uint64), np.array([CURSOR_LIMIT], dtype=np.uint32))
    cp.pack_restart_points(np.zeros((1, 4), dtype=np.uint64), np.array([CURSOR_LIMIT - 1], dtype=np.uint32))


def rungs():
    at = cp.first_block_ints(lambda b: cp.block_bound(ol.FOLD, 1, b) + 16 >= CURSOR_LIMIT)
    return [at - 4, at, PAIR_MAX_BLOCK_INTS, PAIR_MAX_BLOCK_INTS + 128]


@pytest.mark.parametrize("block", rungs())
def test_bound_covers_the_builder_at_every_rung(A, block):
    """ansx_bound (sized for the wide index) is at least the builder's container of one full block and a tail, for data
    near the worst case: three exception bytes per int.  (The 19 M-int rung is left to the GPU file.)"""
    rng = np.random.default_rng(block)
    data = rng.integers(1 << 24, 1 << 30, block + 1001, dtype=np.uint32)
    cont = cp.build_container(ol.FOLD, 1, data, block, 1024)
    room = bound(A, ol.FOLD, 1, data.size, block, 1024)
    assert room >= cont.size, (room, cont.size)
    assert bool(cont[8:12].view(np.uint32)[0] & 0x200) == (cp.block_bound(ol.FOLD, 1, block) + 16 >= CURSOR_LIMIT)
    assert cont.size > 3.7 * data.size  # (the data is heavy: 30 bits per int)


def test_option_limits(A):
    ok = bound(A, ol.FOLD, 1, 1000, 64)
    assert ok > 0
    for bi in (2, 63, 65, 66):
        assert bound(A, ol.FOLD, 1, 1000, bi) == 0                  # block_ints not a multiple of 4
    assert bound(A, ol.FOLD, 1, 1000, 1 << 31) == 0                  # block_ints >= 2^31
    assert bound(A, ol.FOLD, 1, 1000, (1 << 31) + 4) == 0
    assert bound(A, ol.FOLD, 1, 4 * ((1 << 31) - 1), 4) > 0          # 2^31 - 1 blocks
    assert bound(A, ol.FOLD, 1, 4 * ((1 << 31) - 1) + 1, 4) == 0     # one more
    assert bound(A, ol.FOLD, 1, (1 << 31), A.SINGLE_STREAM) == 0     # single stream: n >= 2^31
    assert bound(A, ol.FOLD, 1, 1 << 20, A.SINGLE_STREAM) > 0
    assert bound(A, ol.FOLD, 1, 1000, 64, 6) == 0                    # restart interval not a multiple of 4


@pytest.mark.parametrize("kind,f", CODECS)
def test_block_stream_limit(A, kind, f):
    """A block whose worst-case stream (+ 16) reaches 2^31 bytes is refused: the decoders' index checks refuse a block
    stream of 2^31 bytes, and stream sizes and wide restart cursors are 32-bit.  Single-stream mode: the list is the block."""
    at = cp.first_block_ints(lambda b: cp.block_bound(kind, f, b) + 16 >= STREAM_LIMIT)
    assert cp.block_bound(kind, f, at - 4) + 16 < STREAM_LIMIT <= cp.block_bound(kind, f, at) + 16
    assert 300_000_000 < at < 307_000_000
    assert bound(A, kind, f, 1000, at - 4) > 0 and bound(A, kind, f, 1000, at) == 0
    assert bound(A, kind, f, 1000, (1 << 31) - 4) == 0
    assert bound(A, kind, f, at - 4, A.SINGLE_STREAM) > 0 and bound(A, kind, f, at, A.SINGLE_STREAM) == 0
    # the bound of the longest accepted block holds its worst-case stream
    assert bound(A, kind, f, at - 4, at - 4) >= cp.block_bound(kind, f, at - 4)


@pytest.mark.parametrize("kind,f,compact", [(ol.FOLD, 1, False), (ol.MSB, 0, False), (ol.INT, 0, False), (ol.FOLD, 1, True), (ol.INT, 0, True)])
def test_oracle_pass_over_all_blocks_equals_block_by_block(oracle_built, kind, f, compact):
    """oracle_blocks_full (what the GPU tests of 65538-block containers compare with) against one oracle call per block."""
    block, ckpt = 64, 16
    data = (ol.gen_inputs("zipf20s1.2", 40 * block + 37, seed=9) % np.uint32(3000)).astype(np.uint32)
    data[5 * block:6 * block] = 7 if compact else data[5 * block:6 * block]  # (compaction: a block of one distinct value)
    got = ol.oracle_blocks_full(kind, f, data, block, ckpt, compact=compact)
    for b in range(41):
        blk = data[b * block:(b + 1) * block]
        if compact:
            s, pinfo, info, st, off = ol.oracle_pa_encode(kind, f, blk, ckpt_interval=ckpt)
            hints = ol.prelude_hints(s, pinfo.header_bytes + info.header_bytes) if pinfo.sigma != 1 else np.zeros(8, np.uint32)
        else:
            s, info, st, off = ol.oracle_encode(kind, f, blk, ckpt_interval=ckpt)
            hints = ol.prelude_hints(s, info.header_bytes)
        assert got["sizes"][b] == s.size and got["hash"][b] == ol.hash_spans(s, [0, s.size])[0], b
        assert got["ckpt"][b] == ol.ckpt_digest(st[None], off[None])[0], b
        assert got["present"][b] == info.present_syms and np.array_equal(got["hints"][b], hints), b
    if not compact:
        plain = ol.oracle_blocks_digest(kind, f, data, block, ckpt)
        assert np.array_equal(plain[0], got["sizes"]) and np.array_equal(plain[1], got["hash"]) and np.array_equal(plain[2], got["ckpt"])
        assert plain[3:] == (got["max_lg"], got["max_ns"])
