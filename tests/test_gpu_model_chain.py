"""The shortened model chain between histogram and encoder on the GPU (-m gpu), through the C ABI.

By default the call's running maxima (largest frame, alphabet, present symbols, chosen candidate) come from
k_model_maxima behind k_model_finish instead of from four reads by every block of k_model_finish.
ANSX_MODEL_CHAIN=old selects the form before that (every block raises the maxima itself).  Both must write the same
container, byte for byte -- its header carries three of the maxima --; every block must equal the oracle's and decode
back; and the hints a context learns from the maxima must carry the next call (test_hints_learned_from_the_maxima).

Small geometry throughout: block_ints = 1024, ckpt_interval = 256 (the pair encoder's preconditions), lists of 3, about
200 and 64 k + 1 blocks plus a partial last block (the pair encoder's irregular last workgroup, blocks that do
not exist)."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

BI, CK = 1024, 256
FAST = 5  # ansx_encode_stats.path of a hinted call on the fast model path (+ 128: the pair encoder, + 16: repeated)
# 3, about 200, 64 k + 1 blocks (+ a partial block; one of a few ints would be a one-symbol block, which the fast model path
# leaves to the exact one: test_falls_back_to_the_exact_path)
LENGTHS = [3 * BI, 200 * BI + 300, 65 * BI + 517, 129 * BI + 333]


@pytest.fixture(scope="module")
def A(oracle_built):
    import ans_large_alphabet_amd as A_

    try:
        import torch

        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    except ImportError:
        pass
    return A_


def make_codec(A, ctx, kind, f):
    cls = {ol.FOLD: A.ANSfold, ol.RFOLD: A.ANSrfold}[kind]
    return cls(f, ctx=ctx, block_ints=BI, ckpt_interval=CK)


def check_blocks(A, cont, data, kind, f):
    """every block's stream and restart points against the oracle (as tests/test_gpu_parity.py does)"""
    parts = A.parse_container(cont)
    H = parts["header"]
    nblocks = (data.size + BI - 1) // BI
    assert H.n == data.size and H.nblocks == nblocks and H.block_ints == BI
    for b in range(nblocks):
        exp, info, st, off = ol.oracle_encode(kind, f, data[b * BI:(b + 1) * BI], ckpt_interval=CK)
        got = parts["streams"][b]
        assert got.size == exp.size and np.array_equal(got, exp), "block %d differs from the oracle" % b
        nck = st.shape[0]
        assert np.array_equal(parts["ckpt_off"][b][:nck], off), b
        assert np.array_equal(parts["ckpt_state"][b][:nck], st), b


def encode_twice(ctx, codec, data, repeated=False):
    """-> the second call's container; asserts that it took the fast model path (repeated: tried it, missed, and was
    repeated on the exact path)"""
    codec.encode(data)
    cont = codec.encode(data)
    path = ctx.last_encode_stats()["path"]
    if repeated:
        assert path & 16 and path & ~(128 | 16) in (FAST, 1), "path %d: no repeat on the exact path" % path
    else:
        assert path & ~128 == FAST, "path %d: not the fast model path, the comparison would prove nothing" % path
    return cont, path


def run_case(A, data, kind, f, force_pc=False, keys=(), repeated=False, expect_pc=None):
    n = data.size
    conts = {}
    for chain in ("old", None):
        ctx = A.Context(0)
        try:
            ctx.debug_set("ANSX_MODEL_CHAIN", chain)
            if force_pc:
                ctx.debug_set("ANSX_FORCE_PC", "1")
            for k, v in keys:
                ctx.debug_set(k, v)
            codec = make_codec(A, ctx, kind, f)
            cont, path = encode_twice(ctx, codec, data, repeated)
            if expect_pc is not None:
                assert bool(path & 128) == expect_pc, (path, n)
            assert np.array_equal(codec.decode(cont, n), data), (chain, n)
            conts[chain] = cont
        finally:
            ctx.close()
    assert conts[None].size == conts["old"].size and np.array_equal(conts[None], conts["old"]), n
    check_blocks(A, conts[None], data, kind, f)


def sym_value(s):
    """a value whose ANSfold-1 symbol is s (ansx_dev.h: sym = (x >> 8 k) + 255 k)"""
    return s if s < 256 else ((s - 255) << 8 if s < 511 else (s - 510) << 16)


def test_key_values(A):
    ctx = A.Context(0)
    try:
        for ok in ("old", "0", "", None):
            ctx.debug_set("ANSX_MODEL_CHAIN", ok)
        for bad in ("new", "1", "OLD", " old"):
            with pytest.raises(A.AnsxError) as e:
                ctx.debug_set("ANSX_MODEL_CHAIN", bad)
            assert e.value.status == A._lib.ERR_ARG, bad
    finally:
        ctx.close()


@pytest.mark.parametrize("n", LENGTHS)
def test_small_alphabets(A, n):
    """At most 40 symbols and ANSfold-1 on Zipf over 2^20 (the four-symbols-per-thread form of k_model_finish); the pair encoder
    forced (shape A, four pairs) and as the launch site chooses (shape C on the longer lists, none on the 3-block list)."""
    tiny = np.random.default_rng(n).integers(1, 41, size=n, dtype=np.uint32)
    zipf = ol.gen_inputs("zipf20s1.2", n, seed=3 + n)
    for data in (tiny, zipf):
        run_case(A, data, ol.FOLD, 1, force_pc=True, expect_pc=True)
        run_case(A, data, ol.FOLD, 1, expect_pc=n // BI >= 16)


@pytest.mark.parametrize("f", [2, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_large_alphabets(A, f, n):
    """ANSfold-2 and -3 on Zipf over 2^24: alphabets above 640 and above 1024 symbols (the 16-symbols-per-thread form of
    k_model_finish, the pair encoder's two-round shape B), alphabet sizes no multiple of 8."""
    data = ol.gen_inputs("zipf24", n, seed=f + n)
    most = max(ol.oracle_encode(ol.FOLD, f, data[b * BI:(b + 1) * BI])[1].max_sym + 1 for b in range(n // BI))
    assert most > (640 if f == 2 else 1024), most
    run_case(A, data, ol.FOLD, f, expect_pc=n // BI >= 32)


def candidate_top(counts):
    """the candidates' frequencies of a block's most frequent symbol: scale_freqs for the frames M0 * 2^t, t < 8"""
    F = np.sort(counts[counts > 0]).astype(np.float64)
    sigma, n = F.size, F.sum()
    M0 = 1 << int(sigma - 1).bit_length() if sigma > 1 else 1
    tops = []
    for t in range(8):
        M, fs, top = float(M0 << t), n, 0
        for fj in F:
            s = max(1, int(0.5 + M / fs * fj))
            M, fs, top = M - s, fs - fj, s
        if M == 0:
            tops.append(top)
    return tops


def dominant_list(share, nblocks, tail):
    """blocks in which symbol 3 has about `share` of the ints (the count varies by a few from block to block) and every
    other int a symbol of its own, so that the frames are as large as blocks of 1024 ints allow"""
    blocks = []
    for b in range(nblocks + 1):
        n = BI if b < nblocks else tail
        top = min(n - 1, max(1, int(round(share * n)) + (b % 9) - 4))
        rest = np.array([sym_value(4 + i) for i in range(n - top)], dtype=np.uint32)
        blk = np.concatenate([np.full(top, 3, dtype=np.uint32), rest])
        np.random.default_rng(b).shuffle(blk)
        blocks.append(blk)
    return np.concatenate(blocks)


SHARES = [round(0.1 + 0.05 * i, 2) for i in range(18)]  # 0.1 .. 0.95; 0.5 is the one whose last candidate reaches 2^16


def test_dominant_inputs_cross_the_boundaries():
    """CPU only in effect: the inputs of the sweep below have candidate frequencies on both sides of the LDS log2 table's end
    (511 | 512 | 513) and of the u16 exit (65535)."""
    tops = set()
    for share in SHARES:
        data = dominant_list(share, 65, 517)
        for b in range(66):
            blk = data[b * BI:(b + 1) * BI]
            k = (blk >= 256).astype(np.int64) + (blk >= 65536)
            tops.update(candidate_top(np.bincount((blk >> (8 * k)) + 255 * k)))
    for edge in (511, 512, 513, 65535):
        assert any(t >= edge for t in tops) and any(t < edge for t in tops), edge
    assert {511, 512, 513} <= tops and max(tops) >= 65535


@pytest.mark.parametrize("share", SHARES)
def test_dominant_value(A, share):
    """One value's share from 0.1 to 0.95: its candidate frequencies cross the end of k_model_finish's LDS log2 table and
    the u16 exit (see the test above); eight candidates per block, so that the large frames are really computed."""
    data = dominant_list(share, 65, 517)
    run_case(A, data, ol.FOLD, 1, force_pc=True, keys=(("ANSX_T_HINT", "8"),), expect_pc=True)


def test_falls_back_to_the_exact_path(A):
    """A one-value block (H = 0: the fast path leaves it to the exact one) and a block that outgrows ANSX_NS_HINT: the call
    is repeated on the exact path, same bytes with and without the key."""
    n = 65 * BI + 517
    data = ol.gen_inputs("zipf20s1.2", n, seed=9)
    one = data.copy()
    one[7 * BI:8 * BI] = 77
    run_case(A, one, ol.FOLD, 1, force_pc=True, repeated=True)
    grown = data & 63
    grown[40 * BI:41 * BI] = data[40 * BI:41 * BI]
    run_case(A, grown, ol.FOLD, 1, force_pc=True, keys=(("ANSX_NS_HINT", "128"),), repeated=True)


@pytest.mark.parametrize("f,fam", [(1, "zipf20s1.2"), (3, "zipf24")])
def test_hints_learned_from_the_maxima(A, f, fam):
    """The largest alphabet and the largest chosen candidate of a call become the context's hints for the next call of the
    geometry.  The first call runs the fast model path on forced hints (ANSX_NS_HINT, ANSX_T_HINT), so what the context
    learns is what k_model_maxima (or, under the key, the blocks themselves) reported; then the forced hints are taken
    away and the next calls must stay on the fast path without a repeat: a maximum reported too small would send blocks
    past the hint and the call to the exact path (path & 16).  Same bytes, same statistics under both keys."""
    n = 200 * BI + 300
    data = ol.gen_inputs(fam, n, seed=40 + f)
    seen = {}
    for chain in ("old", None):
        ctx = A.Context(0)
        try:
            ctx.debug_set("ANSX_MODEL_CHAIN", chain)
            ctx.debug_set("ANSX_NS_HINT", "4096")
            ctx.debug_set("ANSX_T_HINT", "8")
            codec = make_codec(A, ctx, ol.FOLD, f)
            conts, stats = [codec.encode(data)], [ctx.last_encode_stats()]
            ctx.debug_set("ANSX_NS_HINT", None)
            ctx.debug_set("ANSX_T_HINT", None)
            for _ in range(2):
                conts.append(codec.encode(data))
                stats.append(ctx.last_encode_stats())
            for st in stats:
                assert st["path"] & ~128 == FAST, (chain, stats)
            assert np.array_equal(conts[0], conts[1]) and np.array_equal(conts[0], conts[2])
            seen[chain] = (conts[0], stats)
        finally:
            ctx.close()
    assert np.array_equal(seen[None][0], seen["old"][0])
    assert seen[None][1] == seen["old"][1]
    most = max(ol.oracle_encode(ol.FOLD, f, data[b * BI:(b + 1) * BI])[1].max_sym + 1 for b in range((n + BI - 1) // BI))
    assert seen[None][1][0]["max_nsyms"] == most


def test_back_to_back_encodes_alternating_the_key(A):
    """Two encodes on one context and stream, the key switched between them, one synchronise at the end: the second call's
    model kernels (k_model_maxima among them, on the pipeline's side streams too) must not touch the flag words and block
    records the first call still reads.  Then both are decoded."""
    import torch

    n = 129 * BI + 333
    ctx = A.Context(0)
    try:
        ctx.debug_set("ANSX_FORCE_PC", "1")
        codec = make_codec(A, ctx, ol.FOLD, 1)
        hosts = [ol.gen_inputs("zipf20s1.2", n, seed=s) for s in (21, 22)]
        refs = [encode_twice(ctx, codec, h)[0] for h in hosts]
        devs = [torch.from_numpy(h.view(np.int32)).cuda() for h in hosts]
        outs = [torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda") for _ in hosts]
        for first in ("old", None):
            torch.cuda.synchronize()
            sizes = []
            for i, key in enumerate((first, None if first else "old")):
                ctx.debug_set("ANSX_MODEL_CHAIN", key)
                sizes.append(codec.encode_dev(devs[i].data_ptr(), n, outs[i].data_ptr(), outs[i].numel()))
                assert ctx.last_encode_stats()["path"] == FAST | 128
            torch.cuda.synchronize()
            for i in range(2):
                got = outs[i][:sizes[i]]
                assert np.array_equal(got.cpu().numpy(), refs[i]), (first, i)
                back = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                codec.decode_dev(got.data_ptr(), got.numel(), back.data_ptr(), n)
                torch.cuda.synchronize()
                assert torch.equal(back, devs[i]), (first, i)
                outs[i].zero_()
    finally:
        ctx.close()
