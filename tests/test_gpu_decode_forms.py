"""Every prelude parser and every block decoder of a decode call on the GPU (-m gpu), each named by the call itself.

choose_decode_form (csrc/ansx_decode_form.h) picks one of eight parser variants and one of six decoders from the
container's header bounds, the geometry and the debug keys; ansx_last_decode_stats reports the pick.  Every case here
encodes on the module's context, pins every block of the container to the oracle (check_container of test_gpu_parity;
compacted containers: the oracle's compacted stream of every block, as test_compacted_blocks_match_oracle does), decodes
under a named set of keys and asserts the exact ints AND the reported form.  The expected form is a literal of the case
table, never recomputed from the chooser: a case whose data or keys do not reach the form it names fails and says so.

Parsers (section b).  The class of a container's bounds decides what each parser key ends in, so every case names its
class and asserts it on the header.  Compacted containers code ranks: ANSfold-1 puts a block of 1024 ranks into at most
260 symbols, so the compacted 766-value mixture is of the "array" class, and the compacted "window" class (584 .. 899
symbols) runs on ANSfold-3 over blocks of 800 distinct values.  The u32 value arrays of the subtree parser (variant 2)
need a frame of 2^16 on at most 287 symbols; test_subtree_parser_with_u32_arrays says which alphabets get there.

Boundaries (section c).  With ANSfold-7 the normaliser picks a frame of 2^16 for blocks of 17 000 .. 22 000 all-distinct
values; there the rank tables pass 150 KiB behind 17 140 present symbols and the slot table of a 2^16 frame (128 KiB)
leaves no room for 17 141 cumulative counts, so that boundary goes from the rank decoder straight to DEC_GTAB -- it is
pinned here as such.  DEC_TABLE is reached at a frame of 2^15 (a block of 32768 ints, every value once or twice): 18 164
present symbols are the rank decoder's last (153 600 bytes exactly), 18 165 .. 22 014 take DEC_TABLE (22 014: 153 600
bytes again), 22 015 and a block of 32768 distinct symbols DEC_GTAB.  Plain ANSint: with the ansint.json recipe (zeros
and a few other values) the smallest block, in steps of 4 ints, whose frame exceeds 2^16 has 25 272 ints (2^17).
"""
import contextlib

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_parity import check_container

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def torch():
    torch_ = pytest.importorskip("torch")
    torch_.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return torch_


@pytest.fixture(scope="module")
def ctx(A, torch, oracle_built):
    return A.Context(0)


@contextlib.contextmanager
def keys(ctx, env):
    try:
        for k, v in env.items():
            ctx.debug_set(k, v)
        yield
    finally:
        for k in env:
            ctx.debug_set(k, None)


# name -> (kind, fidelity, codec options, keys of the ENCODE)
CODECS = {
    "fold1": (ol.FOLD, 1, {}, {}),
    "fold3": (ol.FOLD, 3, {}, {}),
    "fold5": (ol.FOLD, 5, {}, {}),
    "rfold1": (ol.RFOLD, 1, {}, {}),
    "rfold3": (ol.RFOLD, 3, {}, {}),
    "msb": (ol.MSB, 0, {}, {}),
    "fold1-compact": (ol.FOLD, 1, {"compact": True}, {}),
    "fold3-compact": (ol.FOLD, 3, {"compact": True}, {}),
    "int": (ol.INT, 0, {"compact": False}, {}),
    "fold1-wide": (ol.FOLD, 1, {}, {"ANSX_WIDE_RESTART": "1"}),
    "fold7": (ol.FOLD, 7, {}, {}),
}


def make_codec(A, ctx, name, block, ckpt):
    kind, f, kw, _ = CODECS[name]
    ck = ckpt if ckpt else A.NO_CHECKPOINTS
    if kind == ol.MSB:
        return A.ANSmsb(ctx=ctx, block_ints=block, ckpt_interval=ck, **kw)
    if kind == ol.INT:
        return A.ANSint(ctx=ctx, block_ints=block, ckpt_interval=ck, **kw)
    return (A.ANSfold if kind == ol.FOLD else A.ANSrfold)(f, ctx=ctx, block_ints=block, ckpt_interval=ck, **kw)


def fit(name, data):
    """The list as the codec takes it: ANSrfold's value limit, plain ANSint's dense model, and with compaction a block's
    distinct values summing to less than 2^32."""
    kind, f, kw, _ = CODECS[name]
    if kw.get("compact"):
        return (data % np.uint32(1 << 21)).astype(np.uint32)
    if kind == ol.RFOLD:
        return np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
    if kind == ol.INT:
        return (data % np.uint32(16384)).astype(np.uint32)
    return data


def encode_pinned(A, ctx, name, data, block, ckpt):
    """-> (codec, container, header): encoded here, every block the oracle's"""
    kind, f, kw, enc_keys = CODECS[name]
    codec = make_codec(A, ctx, name, block, ckpt)
    with keys(ctx, enc_keys):
        cont = codec.encode(data)
    if kw.get("compact"):
        parts = A.parse_container(cont)
        H = parts["header"]
        assert H.n == data.size and H.block_ints == block and (H.kind & 0xFF) == kind and H.kind & 0x100
        for b in range(H.nblocks):
            exp, pinfo, info, st, off = ol.oracle_pa_encode(kind, f, data[b * block:(b + 1) * block], ckpt_interval=ckpt)
            got = parts["streams"][b]
            assert got.size == exp.size and np.array_equal(got, exp), (name, b)
            k = st.shape[0]
            assert np.array_equal(parts["ckpt_off"][b][:k], off) and np.array_equal(parts["ckpt_state"][b][:k], st), (name, b)
    else:
        H = check_container(A, cont, data, kind, f, block, ckpt)["header"]
    if enc_keys:
        assert H.kind & 0x200, "wide restart points were asked for"
    return codec, cont, H


def decode_as(ctx, codec, cont, data, env, want, tag):
    """Decode under `env`; the ints, then the form: want = dict of ansx_decode_stats fields (stream_cap: True = staged)"""
    with keys(ctx, env):
        back = codec.decode(cont, data.size)
        st = ctx.last_decode_stats()
    assert np.array_equal(back, data), (tag, env)
    for k, v in want.items():
        got = (st[k] != 0) if isinstance(v, bool) else st[k]
        assert got == v, "%s under %s did not reach %s = %r: the call reports %r" % (tag, env, k, v, st)
    return st


# ------------------------------------------------------------------------------------------------ a. decoders
BLOCK, CKPT = 1024, 256
RING = {"ANSX_DECODE_MODE": "ring"}
# name -> (keys, the form with two and more blocks, the form with one block)
DECODERS = {
    "staged": ({"ANSX_DECODE_MODE": "staged"}, {"decoder": "STAGED", "stream_cap": True}, None),
    "staged-hbm": ({"ANSX_DECODE_MODE": "staged", "ANSX_NO_STREAM_LDS": "1"}, {"decoder": "STAGED", "stream_cap": False}, None),
    "ring": (dict(RING, ANSX_DECODE_SMALL_RING="never"), {"decoder": "RING", "stream_cap": False, "max_block_bytes": 0}, None),
    "small-ring": (dict(RING, ANSX_DECODE_SMALL_RING="always"), {"decoder": "SMALL_RING", "stream_cap": False}, None),
    # a single block: the pair key is refused and says so -- the 512-byte rings, one block per workgroup
    "pair": (dict(RING, ANSX_DECODE_PAIR="always", ANSX_DECODE_SMALL_RING="never"), {"decoder": "PAIR"}, {"decoder": "RING"}),
    # (staged while tables + stream stay within 52 KiB: asserted per case below)
    "table": ({"ANSX_DECODE_TABLE": "1"}, {"decoder": "TABLE"}, None),
}


def lean_list(n):
    return ol.gen_inputs("zipf20s1.2", n, seed=91)


def heavy_list(n):
    """2^24 .. 2^30 values (up to 28 stream bytes per step), then a lean stream with bursts of them"""
    rng = np.random.default_rng(8)
    d = ol.gen_inputs("zipf20s1.2", n, seed=3).copy()
    d[:n // 2] = rng.integers(1 << 24, 1 << 30, size=n // 2, dtype=np.uint32)
    for a in range(n // 2, n - 200, 700):
        d[a:a + 160] = rng.integers(1 << 29, 1 << 30, size=160, dtype=np.uint32)
    return d


DEC_CODECS = ["fold1", "fold3", "fold5", "rfold1", "rfold3", "msb", "fold1-compact", "int", "fold1-wide"]
# blocks: 1, 2, 3, 4 with a partial last one, 5 (and 2, 3, 5: exact multiples of block_ints -- the last ring window
# ends at the container's last byte)
LENGTHS = [BLOCK, 2 * BLOCK, 3 * BLOCK, 3 * BLOCK + 300, 5 * BLOCK]


@pytest.mark.parametrize("kind_of_data", ["lean", "heavy"])
@pytest.mark.parametrize("name", DEC_CODECS)
def test_every_decoder_runs_and_says_so(A, ctx, name, kind_of_data):
    whole = fit(name, (lean_list if kind_of_data == "lean" else heavy_list)(LENGTHS[-1]))
    for n in LENGTHS:
        data = whole[:n] if kind_of_data == "lean" else whole[LENGTHS[-1] // 2 - n // 2:][:n]  # (heavy: both halves in reach)
        codec, cont, H = encode_pinned(A, ctx, name, data, BLOCK, CKPT)
        if name == "int":  # a rank decoder applies only while the frame allows it
            assert H.max_log2_frame <= 16, "plain ANSint case left the rank decoders' frames: %d" % H.max_log2_frame
        nblocks = (n + BLOCK - 1) // BLOCK
        for dec, (env, many, one) in DECODERS.items():
            want = dict(one if (nblocks == 1 and one) else many, nblocks=nblocks)
            if CODECS[name][2].get("compact"):
                want.pop("max_block_bytes", None)  # (a compacted container is never decoded without its index)
            st = decode_as(ctx, codec, cont, data, env, want, (name, kind_of_data, n, dec))
            assert st["parser"] == ("DONE" if name == "int" else "PAR")
            if dec == "pair" and nblocks > 1:
                assert st["d_grid"] == (nblocks + 1) // 2
            if dec == "table":  # ANSfold-5 on the heavy list: 12 304 symbols, 4 (max_ns + 2) + 2 * 2^10 + the stream pass 52 KiB
                assert (st["stream_cap"] != 0) == ((name, kind_of_data) != ("fold5", "heavy")), st


def test_table_decoder_reads_an_unstaged_stream(A, ctx):
    """DEC_TABLE with the stream read from HBM: the table forms stage by their own rule (tables + stream <= 52 KiB), so
    this takes blocks whose streams are longer than that: 16384 heavy ints."""
    block, ckpt = 16384, 1024
    data = heavy_list(2 * block + 500)
    data[block:] = heavy_list(2 * block)[:block + 500]
    for name in ("fold1", "rfold1"):
        d = fit(name, data)
        codec, cont, H = encode_pinned(A, ctx, name, d, block, ckpt)
        decode_as(ctx, codec, cont, d, {"ANSX_DECODE_TABLE": "1"}, {"decoder": "TABLE", "stream_cap": False, "nblocks": 3}, name)


# ------------------------------------------------------------------------------------------------ b. parsers
def alphabet_list(kind, n):
    rng = np.random.default_rng(5)
    if kind == "one":
        return np.full(n, 7, dtype=np.uint32)
    if kind == "two":
        return rng.integers(3, 5, size=n).astype(np.uint32)
    if kind == "256":
        return rng.integers(0, 256, size=n).astype(np.uint32)
    if kind == "mix766":  # the three-class mixture of test_prelude_parser_paths
        third = n // 3
        d = np.concatenate([rng.integers(0, 256, third), rng.integers(256, 1 << 16, third), rng.integers(1 << 16, 1 << 24, n - 2 * third)])
        d = d.astype(np.uint32)
        rng.shuffle(d)
        return d
    if kind == "set800":  # every full block holds the same 800 distinct values (224 of them twice): compacted, 801 symbols
        vals = (np.arange(800, dtype=np.uint64) * 2741 % (1 << 21)).astype(np.uint32)
        assert np.unique(vals).size == 800
        return vals[(np.arange(n) % BLOCK) % 800]
    if kind == "uniform21":  # (a compacted block's distinct values must sum to less than 2^32)
        return ol.gen_inputs("uniform24", n, seed=6) >> np.uint32(3)
    assert kind == "uniform24"
    return ol.gen_inputs("uniform24", n, seed=6)


# the keys of every parser, and what runs by the class of the container's bounds (max_nsyms, frame):
#   "array"  frame + alphabet + 3 <= 65535 and at most 583 symbols: u16 value arrays in the subtree parser
#   "window" up to 899 symbols: windowed subtrees, the fast loop still applies
#   "large"  more than 1024 symbols: windowed subtrees, the fast loop is refused (windowed lane parser, 256 words)
PARSERS = {
    "par": ({}, {"array": ("PAR", 1), "window": ("PAR", 0), "large": ("PAR", 0)}),
    "par-old": ({"ANSX_DECODE_SETUP": "old"}, {"array": ("PAR", 0), "window": ("PAR", 0), "large": ("PAR", 0)}),
    "fast": ({"ANSX_PARSE_FAST": "1"}, {"array": ("FAST", 128), "window": ("FAST", 128), "large": ("WIN", 256)}),
    "fast-64": ({"ANSX_PARSE_FAST": "1", "ANSX_PARSE_STAGE_WORDS": "64"}, {"array": ("FAST", 64), "window": ("FAST", 64), "large": ("WIN", 256)}),
    "fast-32": ({"ANSX_PARSE_FAST": "1", "ANSX_PARSE_STAGE_WORDS": "32"}, {"array": ("FAST", 32), "window": ("FAST", 32), "large": ("WIN", 256)}),
    "fast-2": ({"ANSX_PARSE_FAST": "1", "ANSX_PARSE_STAGE_WORDS": "2"}, {"array": ("FAST", 2), "window": ("FAST", 2), "large": ("WIN", 256)}),
    "win": ({"ANSX_PARSE_WIN": "1"}, {"array": ("WIN", 128), "window": ("WIN", 128), "large": ("WIN", 256)}),
    "generic": ({"ANSX_PARSE_GENERIC": "1"}, {"array": ("GENERIC", 0), "window": ("GENERIC", 0), "large": ("GENERIC", 0)}),
}

# (codec, alphabet, class of its bounds)
PARSE_CASES = [
    ("fold1", "one", "array"), ("fold1", "two", "array"), ("fold1", "256", "array"), ("fold1", "mix766", "window"),
    ("rfold1", "one", "array"), ("rfold1", "two", "array"), ("rfold1", "256", "array"), ("rfold1", "mix766", "window"),
    ("fold1-compact", "one", "array"), ("fold1-compact", "two", "array"), ("fold1-compact", "256", "array"), ("fold1-compact", "mix766", "array"),
    ("fold3", "uniform24", "large"), ("fold5", "uniform24", "large"), ("rfold3", "uniform24", "large"), ("fold3-compact", "uniform21", "large"),
    # (ANSfold-1 codes a compacted block of 1024 ints in at most 260 symbols: the window class takes ANSfold-3, ranks below 1024)
    ("fold3-compact", "set800", "window"),
]


@pytest.mark.parametrize("nblocks", [9, 65])  # eight lanes per block: a full wave and a ragged one; more than one workgroup of lane parsers
@pytest.mark.parametrize("name,alphabet,cls", PARSE_CASES)
def test_every_parser_runs_and_says_so(A, ctx, name, alphabet, cls, nblocks):
    n = (nblocks - 1) * BLOCK + 333
    data = fit(name, alphabet_list(alphabet, n))
    codec, cont, H = encode_pinned(A, ctx, name, data, BLOCK, CKPT)
    ns, frame = int(H.max_nsyms), 1 << int(H.max_log2_frame)
    got_cls = "array" if (frame + ns + 3 <= 65535 and ns <= 583) else "window" if (frame + ns + 3 <= 65535 and ns <= 899) else "large" if ns > 1024 else None
    assert got_cls == cls, "the data of (%s, %s) has %d symbols at a frame of %d: not the class %s its case names" % (name, alphabet, ns, frame, cls)
    for pname, (env, by_cls) in PARSERS.items():
        parser, variant = by_cls[cls]
        st = decode_as(ctx, codec, cont, data, env, {"parser": parser, "p_variant": variant, "nblocks": nblocks}, (name, alphabet, nblocks, pname))
        if parser == "PAR":
            assert st["p_grid"] * (st["p_threads"] // 64) * 8 >= nblocks
        else:
            assert st["p_grid"] == (nblocks + 63) // 64 and st["p_threads"] == 64


# PARSE_PAR variant 2 (u32 value arrays) needs at most 287 symbols AND frame + alphabet + 3 > 65535, that is a frame of
# 2^16: the normaliser goes there for a small alphabet only when a value is rare enough, so these blocks are almost
# constant.  Blocks of 9416 ints (compaction takes blocks of up to 16384; 9416 is the shortest at which the oracle gives
# all nine cases below that frame) with restarts every 1024.  The alphabets that reach it: two symbols (one other value
# per block), up to 160 and up to 257 symbols (other values sprinkled through the constant; compacted they are 16 and 100
# ranks).  Those that cannot: a one-symbol block (its frame is 2^15 at most, compacted 2^0), and
# everything above 287 symbols -- the 766-symbol mixture and the alphabets of thousands -- whose depth-3 subtree
# (max_ns >> 3 items + 2 sentinels, 64 lanes, 4 bytes) no longer fits the 37 rows of a wave's slice.
U32_BLOCK, U32_CKPT = 9416, 1024


def sparse_list(alphabet, n):
    d = np.full(n, 9, dtype=np.uint32)
    if alphabet == "two":
        d[U32_BLOCK // 2::U32_BLOCK] = 12
    else:
        pos = np.arange(37, n, 701 if alphabet == "160" else 97)
        d[pos] = (np.arange(pos.size) % (150 if alphabet == "160" else 255) + 10).astype(np.uint32)
    return d


@pytest.mark.parametrize("nblocks", [9, 65])
@pytest.mark.parametrize("alphabet,ns_max", [("two", 13), ("160", 160), ("257", 257)])
@pytest.mark.parametrize("name", ["fold1", "rfold1", "fold1-compact"])
def test_subtree_parser_with_u32_arrays(A, ctx, name, alphabet, ns_max, nblocks):
    n = (nblocks - 1) * U32_BLOCK + 7000
    data = fit(name, sparse_list(alphabet, n))
    codec, cont, H = encode_pinned(A, ctx, name, data, U32_BLOCK, U32_CKPT)
    assert H.max_log2_frame == 16 and H.max_nsyms <= ns_max <= 287, (H.max_log2_frame, H.max_nsyms)
    st = decode_as(ctx, codec, cont, data, {}, {"parser": "PAR", "p_variant": 2, "nblocks": nblocks}, (name, alphabet, nblocks))
    assert st["p_grid"] * (st["p_threads"] // 64) * 8 >= nblocks
    decode_as(ctx, codec, cont, data, {"ANSX_DECODE_SETUP": "old"}, {"parser": "PAR", "p_variant": 0}, (name, alphabet, nblocks))
    # (the fast loop is refused: its values are 16 bits)
    decode_as(ctx, codec, cont, data, {"ANSX_PARSE_FAST": "1"}, {"parser": "WIN", "p_variant": 128}, (name, alphabet, nblocks))


# ------------------------------------------------------------------------------------------------ c. boundaries
def fold_value(f, sym):
    """the smallest value ANSfold-f maps to symbol `sym`"""
    T, D = 1 << (f + 7), 255 << (f - 1)
    sym = np.asarray(sym, dtype=np.uint64)
    k = (sym >= T).astype(np.uint64) + (sym >= T + D) + (sym >= T + 2 * D)
    return ((sym - k * D) << (8 * k)).astype(np.uint32)


# (present symbols, ints of the block, the frame the normaliser picks, the form, bytes of its LDS or None)
BOUNDARY = [
    (17140, 17140, 16, {"decoder": "STAGED", "stream_cap": False, "d_lds": 16384 + 8 * 17140 + 96}),  # 153 600: the limit
    (17141, 17144, 16, {"decoder": "GTAB"}),     # (17 141 distinct and three of them again: blocks are multiples of 4)
    (18164, 32768, 15, {"decoder": "STAGED", "stream_cap": False, "d_lds": 8192 + 8 * 18164 + 96}),  # 153 600 again
    (18165, 32768, 15, {"decoder": "TABLE", "stream_cap": False}),
    (22014, 32768, 15, {"decoder": "TABLE", "stream_cap": False, "d_lds": 4 * 22016 + 65536}),       # 153 600
    (22015, 32768, 15, {"decoder": "GTAB"}),
    (32768, 32768, 15, {"decoder": "GTAB"}),
]


@pytest.mark.parametrize("present,ints,lg,want", BOUNDARY)
def test_natural_boundaries_between_decoders(A, ctx, present, ints, lg, want):
    """No key set: ANSfold-7 on blocks in which `present` symbols occur once (and the first ints - present of them twice)."""
    syms = np.arange(present)
    blk = fold_value(7, np.concatenate([syms, syms[:ints - present]]))
    data = np.concatenate([blk, blk[:100]])  # two blocks
    codec, cont, H = encode_pinned(A, ctx, "fold7", data, ints, 1024)
    assert H.max_log2_frame == lg and H.max_nsyms == present and H.max_present_m1 + 1 == present, (H.max_log2_frame, H.max_nsyms, H.max_present_m1)
    st = decode_as(ctx, codec, cont, data, {}, dict(want, parser="PAR", nblocks=2, maxM=1 << lg, max_ep=present), present)
    assert st["index_validated"]  # (none of these is a ring form)


@pytest.mark.parametrize("twin", [0, 20000])
def test_plain_ansint_above_the_rank_decoders_frames(A, ctx, twin):
    """Frames above 2^16 have one natural form, DEC_GTAB behind k_int_sparse_parse: the smallest such block of the
    ansint.json recipe, and its rank-space twin (values of 16384 and more)."""
    n = 25272
    data = np.full(n + 100, twin, dtype=np.uint32)
    data[n // 2] += 5
    data[n + 50] += 5
    codec, cont, H = encode_pinned(A, ctx, "int", data, n, 256)
    assert H.max_log2_frame == 17, H.max_log2_frame
    assert bool(ctx.last_encode_stats()["path"] & 256) == bool(twin)
    decode_as(ctx, codec, cont, data, {}, {"decoder": "GTAB", "parser": "DONE", "nblocks": 2, "maxM": 1 << 17}, twin)


# ------------------------------------------------------------------------------------------------ d. other entries
def to_dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32 if arr.dtype == np.uint32 else arr.dtype)).cuda()


PAIR = DECODERS["pair"][0]
SMALL = DECODERS["small-ring"][0]


@pytest.fixture(scope="module")
def eight_blocks(A, torch, ctx):
    """(shared, never changed) eight blocks of small gaps in device memory, and their block bases"""
    data = (lean_list(7 * BLOCK + 500) % np.uint32(4096)).astype(np.uint32)
    codec, cont, H = encode_pinned(A, ctx, "fold1", data, BLOCK, CKPT)
    dev = to_dev(torch, cont)
    bases = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nbases = codec.block_bases_dev(dev.data_ptr(), cont.size, bases.data_ptr(), 9)
    assert nbases == 9
    return codec, data, dev, cont.size, bases


# ranges, the blocks they touch
ONE_BLOCK = ([3 * BLOCK + 5, 3 * BLOCK + 700], [100, 20], 1)
THREE_BLOCKS = ([BLOCK - 3, 6 * BLOCK - 1, BLOCK + 40], [7, 1, 50], 3)  # (blocks 0 and 1, 5, 1 again)


@pytest.mark.parametrize("first,count,touched", [ONE_BLOCK, THREE_BLOCKS])
@pytest.mark.parametrize("env,many,one", [({}, "STAGED", "STAGED"), (PAIR, "PAIR", "RING"), (SMALL, "SMALL_RING", "SMALL_RING")])
def test_ranges_decode_the_sub_container_in_the_forced_form(A, torch, ctx, eight_blocks, env, many, one, first, count, touched):
    codec, data, dev, nb, _ = eight_blocks
    total = sum(count)
    out = torch.full((total + 8,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with keys(ctx, env):
        assert codec.decode_ranges_dev(dev.data_ptr(), nb, first, count, out.data_ptr(), total) == total
        torch.cuda.synchronize()
        st = ctx.last_decode_stats()
    exp = np.concatenate([data[a:a + c] for a, c in zip(first, count)])
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:total], exp)
    assert st["nblocks"] == touched and st["decoder"] == (one if touched == 1 else many), st
    assert not st["on_remembered"]  # (a sub-container never runs on a remembered header)


@pytest.mark.parametrize("env,many,one", [(PAIR, "PAIR", "RING"), (SMALL, "SMALL_RING", "SMALL_RING")])
def test_range_sums_decode_the_sub_container_in_the_forced_form(A, torch, ctx, eight_blocks, env, many, one):
    codec, data, dev, nb, bases = eight_blocks
    sums = np.cumsum(data, dtype=np.uint64)
    assert int(sums[-1]) < 1 << 32
    for first, count, touched in (ONE_BLOCK, THREE_BLOCKS):
        total = sum(count)
        out = torch.full((total + 8,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with keys(ctx, env):
            assert codec.decode_ranges_sums_dev(dev.data_ptr(), nb, bases.data_ptr(), 9, first, count, out.data_ptr(), total) == total
            torch.cuda.synchronize()
            st = ctx.last_decode_stats()
        exp = np.concatenate([sums[a:a + c] for a, c in zip(first, count)]).astype(np.uint32)
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[:total], exp)
        assert st["nblocks"] == touched and st["decoder"] == (one if touched == 1 else many), st


def test_batch_passes_of_three_blocks_run_the_pair_decoder(A, torch, ctx):
    """Five containers of 1, 2, 3, 2, 1 blocks in passes of three: an odd count per pass, the last block of every pass
    takes the single-block code inside k_decode_rank2; the stats are those of the last pass."""
    lens = [BLOCK, 2 * BLOCK, 2 * BLOCK + 77, BLOCK + 500, 301]
    whole = lean_list(sum(lens))
    lists, conts, at = [], [], 0
    for n in lens:
        d = whole[at:at + n]
        at += n
        codec, cont, H = encode_pinned(A, ctx, "fold1", d, BLOCK, CKPT)
        lists.append(d)
        t = torch.zeros((cont.size + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        t[:cont.size] = torch.from_numpy(cont.copy()).cuda()
        conts.append((t, cont.size))
    assert sum((n + BLOCK - 1) // BLOCK for n in lens) == 9
    out = torch.full((sum(lens) + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with keys(ctx, dict(PAIR, ANSX_BATCH_PASS_BLOCKS="3")):
        offs = codec.decode_batch_dev([t.data_ptr() for t, _ in conts], [b for _, b in conts], out.data_ptr(), out.numel())
        torch.cuda.synchronize()
        st = ctx.last_decode_stats()
    got = out.cpu().numpy().view(np.uint32)
    for i, d in enumerate(lists):
        assert np.array_equal(got[int(offs[i]):int(offs[i + 1])], d), i
    assert st["nblocks"] == 3 and st["decoder"] == "PAIR" and st["d_grid"] == 2, st


def test_keys_take_their_words_only(A, ctx):
    """ANSX_DECODE_MODE, ANSX_DECODE_PAIR and ANSX_DECODE_SMALL_RING: any other non-empty value is an error, not "auto"."""
    for name, bad in (("ANSX_DECODE_PAIR", "1"), ("ANSX_DECODE_PAIR", "2"), ("ANSX_DECODE_SMALL_RING", "2"), ("ANSX_DECODE_SMALL_RING", "yes"),
                      ("ANSX_DECODE_MODE", "rings"), ("ANSX_DECODE_MODE", "1")):
        with pytest.raises(A.AnsxError) as ei:
            ctx.debug_set(name, bad)
        assert ei.value.status == 1, (name, bad)  # ANSX_ERR_ARG
    for name, ok in (("ANSX_DECODE_PAIR", "always"), ("ANSX_DECODE_PAIR", "never"), ("ANSX_DECODE_SMALL_RING", "always"),
                     ("ANSX_DECODE_MODE", "ring"), ("ANSX_DECODE_MODE", "staged"), ("ANSX_DECODE_MODE", ""), ("ANSX_DECODE_PAIR", "0")):
        ctx.debug_set(name, ok)
        ctx.debug_set(name, None)
