"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against the oracle.

Bit-exact bar: every block stream in the container equals the oracle's encode of that block
(canonical form = zero padding bits), restart points equal the oracle's, and decode
returns the input.  Nothing here reads /root/reference.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import subprocess
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KIND = {"fold": ol.FOLD, "rfold": ol.RFOLD, "msb": ol.MSB}


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module", params=["learned", "hinted", "hinted5", "hinted-exact", "fused"])
def ctx(A, oracle_built, request):
    """"learned": a fresh context -- the first call per geometry discovers the alphabet size with a
    mid-call read-back, later ones are launched back to back on the learned hint.  "hinted": the hint
    is forced from the first call on (ANSX_NS_HINT), so every eligible encode of the suite takes the
    read-back-free path with the fast model kernels (k_candidates / k_model_finish, 8 candidate frame sizes per
    block: ANSX_T_HINT); inputs that outgrow it repeat on the discovery path.  "hinted5": the same with 5
    candidates per block (12 blocks per wave; blocks that need a sixth repeat) and two recurrences per lane.  "hinted-exact": the hinted path
    with the exact model kernels (ANSX_NO_FAST_MODEL).  "fused": the single LDS-resident model kernel
    (k_model_fused, opt-in) instead."""
    # Same order as bench.py: torch (which bundles its own HIP runtime) initialises the device
    # first, libansx then shares that runtime.  On a fresh box the first `import torch` can take
    # minutes while the image pages in; doing it here keeps that out of the individual tests.
    try:
        import torch

        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")
    except ImportError:
        pass
    c = A.Context(0)
    if request.param != "learned":
        c.debug_set("ANSX_NS_HINT", "4096")
    if request.param == "hinted":
        c.debug_set("ANSX_T_HINT", "8")
    if request.param == "hinted5":
        c.debug_set("ANSX_T_HINT", "5")
        c.debug_set("ANSX_CAND_CHAINS", "2")  # two recurrences per lane (what calls of > ~12 K blocks use)
    if request.param == "hinted-exact":
        c.debug_set("ANSX_NO_FAST_MODEL", "1")
    if request.param == "fused":
        c.debug_set("ANSX_MODEL_FUSED", "1")
    return c


def codec_for(A, ctx, kind, f, **kw):
    if kind == ol.MSB:
        return A.ANSmsb(ctx=ctx, **kw)
    if kind == ol.INT:
        return A.ANSint(ctx=ctx, **kw)
    cls = A.ANSfold if kind == ol.FOLD else A.ANSrfold
    return cls(f, ctx=ctx, **kw)


def check_container(A, cont, data, kind, f, block, ckpt):
    parts = A.parse_container(cont)
    H = parts["header"]
    n = data.size
    nblocks = (n + block - 1) // block
    assert H.n == n and H.nblocks == nblocks and H.block_ints == block and (H.kind & ~0x200) == kind and H.fidelity == f  # (bit 9: restart-point format)
    max_lg, max_ns = 0, 0
    for b in range(nblocks):
        blk = data[b * block:(b + 1) * block]
        exp, info, st, off = ol.oracle_encode(kind, f, blk, ckpt_interval=ckpt)
        got = parts["streams"][b]
        assert got.size == exp.size, (b, got.size, exp.size)
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            raise AssertionError("block %d differs at byte %d of %d (prelude %d)" % (b, bad[0], exp.size, info.prelude_bytes))
        nck = st.shape[0]
        assert np.array_equal(parts["ckpt_off"][b][:nck], off), b
        assert np.array_equal(parts["ckpt_state"][b][:nck], st), b
        max_lg = max(max_lg, info.log2_frame)
        max_ns = max(max_ns, info.max_sym + 1)
    if kind == ol.INT and not (H.kind & 0x100):
        # plain ANSint: the header bounds a block's DISTINCT values, whichever model (dense, rank space) the call ran
        max_ns = max(np.unique(data[b * block:(b + 1) * block]).size for b in range(nblocks))
        assert not np.asarray(parts["parse_hints"]).any()
    assert H.max_log2_frame == max_lg and H.max_nsyms == max_ns
    return parts


FAMS = ["uniform256", "uniform12", "uniform20", "geom0.01", "geom0.4", "zipf20s1.2", "zipf24",
        "constant", "distinct", "sparse_large", "boundaries"]


@pytest.mark.parametrize("f", [1, 3, 5])
@pytest.mark.parametrize("fam", FAMS)
def test_fold_blocks_match_oracle(A, ctx, f, fam):
    n = 70001
    data = ol.gen_inputs(fam, n, seed=17 * f)
    codec = codec_for(A, ctx, ol.FOLD, f, block_ints=16384, ckpt_interval=1024)
    cont = codec.encode(data)
    check_container(A, cont, data, ol.FOLD, f, 16384, 1024)
    assert np.array_equal(codec.decode(cont, n), data)


@pytest.mark.parametrize("kind", [ol.FOLD, ol.RFOLD])
@pytest.mark.parametrize("f", [2, 4])
def test_even_fidelities_match_oracle(A, ctx, kind, f):
    """Every accepted fidelity is exercised (the reference harnesses use 1 and 5, BASELINE 1 and 3)."""
    for fam in ("uniform20", "zipf20s1.2", "zipf24", "sparse_large", "boundaries", "constant"):
        n = 40007
        data = ol.gen_inputs(fam, n, seed=31 * f)
        if kind == ol.RFOLD:
            data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
        codec = codec_for(A, ctx, kind, f, block_ints=16384, ckpt_interval=1024)
        cont = codec.encode(data)
        check_container(A, cont, data, kind, f, 16384, 1024)
        assert np.array_equal(codec.decode(cont, n), data), fam


def test_fidelity_8_is_rejected(A, ctx):
    """f = 8 is unsound in the reference itself: ANSX_ERR_ARG, not a HIP error."""
    data = ol.gen_inputs("uniform20", 5000, seed=3)
    for cls in (A.ANSfold, A.ANSrfold):
        with pytest.raises(A.AnsxError) as ei:
            cls(8, ctx=ctx).encode(data)
        assert ei.value.status == 1


@pytest.mark.parametrize("kind", [ol.FOLD, ol.RFOLD])
@pytest.mark.parametrize("f", [6, 7])
def test_fidelities_6_and_7(A, ctx, kind, f):
    """Alphabets of 32 Ki / 64 Ki slots (methods.hpp:529-567 instantiates them): the per-block arrays of the histogram,
    sort, prelude-writer and decode-table stages live in HBM there.  Every block stream, restart point and header field
    against the oracle; round trip; ragged sizes; single-stream mode = the reference's bytes."""
    for fam, n, block, ck in (("zipf24", 70001, 16384, 1024), ("uniform20", 40000, 8192, 2048), ("sparse_large", 33000, 16384, 0),
                              ("zipf20s1.2", 9999, 4096, 512), ("distinct", 20000, 16384, 1024), ("boundaries", 5000, 4096, 1024),
                              ("zipf24", 150000, 65536, 4096)):
        data = ol.gen_inputs(fam, n, seed=13 * f + 1)
        if kind == ol.RFOLD:
            data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
        codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ck if ck else A.NO_CHECKPOINTS)
        cont = codec.encode(data)
        check_container(A, cont, data, kind, f, block, ck)
        assert np.array_equal(codec.decode(cont, n), data), (fam, n)
    data = ol.gen_inputs("zipf24", 30011, seed=f)
    if kind == ol.RFOLD:
        data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
    one = codec_for(A, ctx, kind, f, block_ints=A.SINGLE_STREAM)
    stream = one.encode(data)
    exp = ol.oracle_encode(kind, f, data)[0]
    assert np.array_equal(stream, exp)
    assert np.array_equal(one.decode(exp, data.size), data)


@pytest.mark.parametrize("f", [1, 3, 5])
@pytest.mark.parametrize("fam", ["uniform256", "uniform20", "geom0.01", "zipf20s1.2", "zipf24",
                                 "constant", "distinct", "sparse_large", "boundaries"])
def test_rfold_blocks_match_oracle(A, ctx, f, fam):
    n = 50003
    data = ol.gen_inputs(fam, n, seed=23 * f)
    data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
    codec = codec_for(A, ctx, ol.RFOLD, f, block_ints=16384, ckpt_interval=2048)
    cont = codec.encode(data)
    check_container(A, cont, data, ol.RFOLD, f, 16384, 2048)
    assert np.array_equal(codec.decode(cont, n), data)


def test_rfold_optimistic_hash_table(A, oracle_built):
    """The second ANSrfold call of a geometry sizes its per-block hash tables for 1.5 x the most distinct values a
    block had so far (two workgroups per CU, shorter passes).  Same bytes as the full-size table; a later input
    whose blocks hold more distinct values than the table has slots (uniform over 2^24: every value of a block
    differs) overflows it, and the call repeats itself on the full-size path (stats.path & 16) -- still equal to
    the oracle."""
    own = A.Context(0)  # a context of its own: the hints are per context and geometry
    f, n = 3, 5 * 16384 + 777
    few = ol.gen_inputs("zipf20s1.2", n, seed=3)
    many = ol.gen_inputs("uniform24", n, seed=4)
    codec = codec_for(A, own, ol.RFOLD, f, block_ints=16384, ckpt_interval=1024)
    first = codec.encode(few)                      # discovery: full-size tables
    check_container(A, first, few, ol.RFOLD, f, 16384, 1024)
    second = codec.encode(few)                     # optimistic: small tables
    assert own.last_encode_stats()["path"] & 16 == 0
    assert np.array_equal(first, second)
    cont = codec.encode(many)                      # overflows the small tables
    assert own.last_encode_stats()["path"] & 16
    check_container(A, cont, many, ol.RFOLD, f, 16384, 1024)
    assert np.array_equal(codec.decode(cont, n), many)
    again = codec.encode(many)                     # the hint has grown: full-size tables, no repeat
    assert own.last_encode_stats()["path"] & 16 == 0
    assert np.array_equal(cont, again)
    assert np.array_equal(codec.encode(few), first)


def test_compaction_optimistic_hash_set(A, oracle_built):
    """The compaction layer's remap kernel sizes its hash set and value list like the ANSrfold remap: from the most
    distinct values a block of the geometry had so far.  Same bytes as with the full sizes; blocks with more
    distinct values than that overflow, and the call repeats itself with the full sizes (stats.path & 16)."""
    own = A.Context(0)
    n = 5 * 16384 + 777
    few = ol.gen_inputs("zipf20s1.2", n, seed=5)
    many = np.random.default_rng(6).integers(0, 1 << 15, size=n, dtype=np.uint32)  # ~13 K distinct values per block
                                                                                   # (their sum stays below 2^32)
    codec = A.ANSfold(1, ctx=own, block_ints=16384, ckpt_interval=1024, compact=True)
    first = codec.encode(few)                            # discovery: full sizes
    assert np.array_equal(codec.decode(first, n), few)
    second = codec.encode(few)                           # optimistic: small sizes
    assert own.last_encode_stats()["path"] & 16 == 0
    assert np.array_equal(first, second)
    cont = codec.encode(many)                            # overflows them
    assert own.last_encode_stats()["path"] & 16
    assert np.array_equal(codec.decode(cont, n), many)
    fresh = A.ANSfold(1, ctx=A.Context(0), block_ints=16384, ckpt_interval=1024, compact=True)
    assert np.array_equal(fresh.encode(many), cont)      # equal to a discovery-path encode
    assert np.array_equal(codec.encode(few), first)


@pytest.mark.parametrize("kind", [ol.FOLD, ol.RFOLD])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 313, 1000, 1001, 4096, 4097])
def test_small_and_ragged_sizes(A, ctx, kind, n):
    for f in (1, 3):
        for fam in ("zipf20s1.2", "uniform256"):
            data = ol.gen_inputs(fam, n, seed=n)
            for block, ck in ((4096, 1024), (64, 16), (1024, A.NO_CHECKPOINTS)):
                codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ck)
                cont = codec.encode(data)
                ckv = 0 if ck == A.NO_CHECKPOINTS or ck >= block else ck
                check_container(A, cont, data, kind, f, block, ckv)
                assert np.array_equal(codec.decode(cont, n), data), (n, f, fam, block)


@pytest.mark.parametrize("kind", [ol.FOLD, ol.RFOLD])
def test_single_stream_mode_equals_reference_stream(A, ctx, kind):
    """block_ints = SINGLE_STREAM: output is exactly one reference stream (no container), and the
    decoder accepts reference-made streams."""
    for f in (1, 3, 5):
        for fam, n in (("zipf20s1.2", 9001), ("uniform256", 4096), ("geom0.01", 3)):
            data = ol.gen_inputs(fam, n, seed=f)
            codec = codec_for(A, ctx, kind, f, block_ints=A.SINGLE_STREAM)
            s = codec.encode(data)
            exp, info, _, _ = ol.oracle_encode(kind, f, data)
            assert np.array_equal(s, exp), (f, fam)
            assert np.array_equal(codec.decode(exp, n), data)


def test_single_stream_large_fold(A, ctx):
    data = ol.gen_inputs("zipf20s1.2", 300007, seed=5)
    codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=A.SINGLE_STREAM)
    s = codec.encode(data)
    exp, _, _, _ = ol.oracle_encode(ol.FOLD, 1, data)
    assert np.array_equal(s, exp)
    assert np.array_equal(codec.decode(s, data.size), data)


def test_golden_fixtures_single_stream(A, ctx):
    """The committed reference-made fixtures: GPU single-stream encode must reproduce the bytes,
    GPU decode of the reference bytes must return the input."""
    with open(os.path.join(GOLD, "small.json")) as fh:
        gold = json.load(fh)
    for e in gold[::3]:
        data = np.array(e["input"], dtype=np.uint32)
        kind = KIND[e["kind"]]
        codec = codec_for(A, ctx, kind, e["f"], block_ints=A.SINGLE_STREAM)
        s = codec.encode(data)
        assert s.tobytes().hex() == e["stream_hex"], (e["kind"], e["f"], e.get("family"), e["n"])
        ref_stream = np.frombuffer(bytes.fromhex(e["stream_hex"]), dtype=np.uint8)
        assert np.array_equal(codec.decode(ref_stream, e["n"]), data)


@pytest.mark.parametrize("fixture", ["large.json", "f24.json", "f67.json"])
def test_golden_fixtures_large(A, ctx, fixture):
    with open(os.path.join(GOLD, fixture)) as fh:
        gold = json.load(fh)
    for e in gold:
        data = ol.gen_inputs(e["family"], e["n"], e["seed"])
        if e["kind"] == "rfold":
            data = data % np.uint32(1 << 21)
        codec = codec_for(A, ctx, KIND[e["kind"]], e["f"], block_ints=A.SINGLE_STREAM)
        s = codec.encode(data)
        assert s.size == e["stream_len"]
        assert hashlib.sha256(s.tobytes()).hexdigest() == e["stream_sha256"], (e["kind"], e["f"], e["family"], e["n"])


def test_f3_divergence_is_fixed_in_decode(A, ctx):
    # sigma < T but values >= T; reference decode is off by T, ours round-trips
    d = np.array([5, 1000, 5, 70000, 5, 5, 1000], dtype=np.uint32)
    codec = codec_for(A, ctx, ol.RFOLD, 1, block_ints=A.SINGLE_STREAM)
    s = codec.encode(d)
    exp, info, _, _ = ol.oracle_encode(ol.RFOLD, 1, d)
    assert info.reorder_flag == 0 and np.array_equal(s, exp)
    assert np.array_equal(codec.decode(s, d.size), d)


def test_errors(A, ctx):
    L = A.lib()
    codec = codec_for(A, ctx, ol.FOLD, 1)
    with pytest.raises(A.AnsxError) as ei:
        codec.encode(np.array([1, 2, 1 << 30], dtype=np.uint32))
    assert ei.value.status == 6  # DOMAIN
    with pytest.raises(A.AnsxError) as ei:
        codec.encode(np.zeros(0, dtype=np.uint32))
    assert ei.value.status == 1  # ARG (n == 0 never terminates in the reference)
    data = ol.gen_inputs("zipf20s1.2", 50000, seed=1)
    small = np.empty(1000, dtype=np.uint8)
    with pytest.raises(A.AnsxError) as ei:
        codec.encode(data, out=small)
    assert ei.value.status == 2  # CAPACITY
    cont = codec.encode(data).copy()
    bad = cont.copy()
    bad[0] ^= 0xFF
    with pytest.raises(A.AnsxError) as ei:
        codec.decode(bad, data.size)
    assert ei.value.status == 3  # FORMAT
    bad = cont.copy()
    bad[64 + 8] ^= 0x40  # corrupt the block index
    with pytest.raises(A.AnsxError) as ei:
        codec.decode(bad, data.size)
    assert ei.value.status == 3
    with pytest.raises(A.AnsxError):
        codec.decode(cont, data.size + 1)  # n mismatch
    # the context is still usable afterwards
    assert np.array_equal(codec.decode(cont, data.size), data)


def test_device_log2_bit_identical_to_host(A, ctx):
    """ansx_log2_portable evaluated on the device equals the host evaluation bit for bit on the
    value classes the normaliser feeds it: p = f/n and q = S/2^k."""
    import math

    rng = np.random.default_rng(3)
    n_ = rng.integers(1, 1 << 24, size=40000).astype(np.float64)
    f_ = np.minimum(rng.integers(1, 1 << 24, size=40000), n_).astype(np.float64)
    xs = np.concatenate([f_ / n_, rng.integers(1, 65535, size=40000) / np.exp2(rng.integers(1, 20, size=40000)),
                         np.exp2(-np.arange(0, 40.0)), [1.0, 0.5, 0.999999999, 1e-9]]).astype(np.float64)
    out = np.zeros_like(xs)
    st = A.lib().ansx_selftest_log2(ctx.handle, xs.ctypes.data, out.ctypes.data, xs.size)
    assert st == 0
    host = np.array([A.lib().ansx_host_log2(float(x)) for x in xs])
    assert np.array_equal(out.view(np.uint64), host.view(np.uint64))
    libm = np.array([math.log2(float(x)) for x in xs])
    rel = np.abs(out - libm) / np.maximum(np.abs(libm), 1e-300)
    assert rel[libm != 0].max() <= 2.3e-16  # within 1 ulp of glibc


def test_device_division_helper_is_ieee_exact(A, ctx):
    """The normaliser divides integer-valued doubles below 2^31 (M_rem / fs_rem, count / n) with a
    reciprocal-based sequence instead of the compiler's IEEE expansion; it must round identically
    (proof sketch in csrc/ansx_dev.h).  Random pairs, pairs that make exact quotients, near-ties."""
    rng = np.random.default_rng(11)
    a = [rng.integers(0, 1 << 31, size=400000), rng.integers(0, 1 << 16, size=200000),
         rng.integers(0, 1 << 31, size=200000)]
    b = [rng.integers(1, 1 << 31, size=400000), rng.integers(1, 1 << 31, size=200000),
         rng.integers(1, 1 << 12, size=200000)]
    q = rng.integers(0, 1 << 15, size=100000)
    d = rng.integers(1, 1 << 16, size=100000)
    a.append(q * d)                      # exact quotients
    b.append(d)
    a.append(np.array([0, 1, (1 << 31) - 1, (1 << 31) - 1, 1, 3, (1 << 31) - 2, 16384, 12345678]))
    b.append(np.array([1, (1 << 31) - 1, (1 << 31) - 1, 1, 3, (1 << 31) - 1, (1 << 31) - 1, 3, 7]))
    a = np.concatenate(a).astype(np.float64)
    b = np.concatenate(b).astype(np.float64)
    out = np.zeros_like(a)
    st = A.lib().ansx_selftest_div(ctx.handle, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size)
    assert st == 0
    want = a / b
    bad = np.nonzero(out.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, (bad[:5], a[bad[:5]], b[bad[:5]], out[bad[:5]], want[bad[:5]])


def test_device_log2_matches_host_portable_log2(A, ctx):
    """The normaliser's log2 must be the same function on host and device; exercised indirectly:
    blocks whose XH lands near the threshold would flip otherwise.  Direct check through a
    constant block (M = 32768 exit via the u16 rule) and a two-symbol block."""
    for data in (np.full(5000, 7, dtype=np.uint32), np.array([5, 300] * 2000, dtype=np.uint32)):
        codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=A.SINGLE_STREAM)
        s = codec.encode(data)
        exp, info, _, _ = ol.oracle_encode(ol.FOLD, 1, data)
        assert np.array_equal(s, exp)


def test_device_pointer_api_with_torch(A, ctx):
    torch = pytest.importorskip("torch")
    n = 1 << 20
    data = ol.gen_inputs("zipf20s1.2", n, seed=9)
    d_in = torch.from_numpy(data.view(np.int32)).cuda()
    codec = codec_for(A, ctx, ol.FOLD, 1)
    cap = codec.bound(n)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_back = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    nb = codec.encode_dev(d_in.data_ptr(), n, d_out.data_ptr(), cap, stream=s)
    codec.decode_dev(d_out.data_ptr(), nb, d_back.data_ptr(), n, stream=s)
    torch.cuda.synchronize()
    assert torch.equal(d_back, d_in)
    cont = d_out[:nb].cpu().numpy()
    check_container(A, cont, data, ol.FOLD, 1, A.DEFAULT_BLOCK_INTS, A.DEFAULT_CKPT_INTERVAL)


def test_full_size_roundtrip_properties(A, ctx):
    """BASELINE config-2 shape at a size the oracle cannot cover block by block in seconds:
    encode -> decode round trip on device plus spot-checked blocks against the oracle."""
    torch = pytest.importorskip("torch")
    n = 32 * (1 << 20) + 12345
    g = torch.Generator(device="cuda").manual_seed(1234)
    N = 1 << 20
    w = 1.0 / torch.arange(1, N + 1, dtype=torch.float64, device="cuda") ** 1.2
    cdf = torch.cumsum(w, 0)
    cdf /= cdf[-1].clone()
    u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    d_in = (torch.searchsorted(cdf, u) + 1).clamp_(max=N).to(torch.int32)
    codec = codec_for(A, ctx, ol.FOLD, 1)
    cap = codec.bound(n)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_back = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nb = codec.encode_dev(d_in.data_ptr(), n, d_out.data_ptr(), cap)
    codec.decode_dev(d_out.data_ptr(), nb, d_back.data_ptr(), n)
    torch.cuda.synchronize()
    assert torch.equal(d_back, d_in)
    cont = d_out[:nb].cpu().numpy()
    parts = A.parse_container(cont)
    data = d_in.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(0)
    picks = list(rng.integers(0, parts["header"].nblocks, size=24)) + [0, parts["header"].nblocks - 1]
    for b in picks:
        blk = data[b * 16384:(b + 1) * 16384]
        exp, info, st, off = ol.oracle_encode(ol.FOLD, 1, blk, ckpt_interval=1024)
        assert np.array_equal(parts["streams"][b], exp), b
        assert np.array_equal(parts["ckpt_state"][b][:st.shape[0]], st)
    bpi = 8.0 * nb / n
    assert 8.0 < bpi < 9.6


def test_whole_container_equals_python_builder(A, ctx):
    """Header, block index, restart points and payload — the complete container — against an
    independent Python assembly of oracle block streams (tests/container_py.py)."""
    import container_py as cp

    for kind, f, block, ck, n in ((ol.FOLD, 1, 4096, 1024, 20001), (ol.RFOLD, 3, 4096, 512, 9999),
                                  (ol.FOLD, 5, 16384, 4096, 40000)):
        data = ol.gen_inputs("zipf20s1.2", n, seed=n)
        codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ck)
        got = codec.encode(data)
        exp = cp.build_container(kind, f, data, block, ck)
        assert got.size == exp.size and np.array_equal(got, exp), (kind, f)


def test_restart_point_formats(A):
    """Container v3: packed 29-byte restart points by default (4 x 52-bit states + 24-bit cursor), the wide form (u32 +
    4 x u64) where a frame may exceed 2^16.  Both against the Python builder, both decoded, both merged (native kernel
    and the torch restatement); a call that meets too large a frame half way is repeated with wide restart points and
    the context remembers that for the geometry; parts in different formats do not merge."""
    import container_py as cp
    torch = pytest.importorskip("torch")
    from ans_large_alphabet_amd import dist as adist

    n, block, ck = 70001, 8192, 1024
    data = ol.gen_inputs("zipf20s1.2", n, seed=77)
    exp_packed = cp.build_container(ol.FOLD, 1, data, block, ck)
    exp_wide = cp.build_container(ol.FOLD, 1, data, block, ck, wide=True)
    assert exp_wide.size > exp_packed.size
    # (1) packed is what a fresh context writes; states of frames of exactly 2^16 use all 52 bits
    c0 = A.Context(0)
    codec = A.ANSfold(1, ctx=c0, block_ints=block, ckpt_interval=ck)
    got = codec.encode(data)
    assert np.array_equal(got, exp_packed)
    assert np.array_equal(codec.decode(got, n), data)
    parts = A.parse_container(got)
    assert not (parts["header"].kind & 0x200) and parts["ckpt_state"].shape == (9, 7, 4)
    c0.close()
    # (2) the wide form on request
    c1 = A.Context(0)
    c1.debug_set("ANSX_WIDE_RESTART", "1")
    codec = A.ANSfold(1, ctx=c1, block_ints=block, ckpt_interval=ck)
    for _ in range(2):  # (discovery call, then the hinted fast path)
        got_w = codec.encode(data)
        assert np.array_equal(got_w, exp_wide)
    assert np.array_equal(codec.decode(got_w, n), data)
    pw = A.parse_container(got_w)
    assert pw["header"].kind & 0x200
    assert np.array_equal(pw["ckpt_state"], parts["ckpt_state"]) and np.array_equal(pw["ckpt_off"], parts["ckpt_off"])
    # merge of wide parts: native kernel == torch restatement == whole encode
    shards, sizes, bufs = [], [], []
    for r in range(3):
        lo, cnt = adist.shard_blocks(n, block, r, 3)
        c = codec.encode(data[lo:lo + cnt])
        shards.append(c)
        sizes.append(c.size)
        bufs.append(torch.from_numpy(np.concatenate([c, np.zeros((-c.size) % 16, np.uint8)])).cuda())
    out = torch.empty(exp_wide.size + 64, dtype=torch.uint8, device="cuda:0")
    nb = c1.merge_containers_dev([b.data_ptr() for b in bufs], sizes, out.data_ptr(), out.numel())
    assert np.array_equal(out[:nb].cpu().numpy(), exp_wide)
    pym = adist.merge_containers(torch.cat([torch.from_numpy(c.copy()) for c in shards]), sizes).numpy()
    assert np.array_equal(pym, exp_wide)
    # a packed part among wide ones is refused
    c0 = A.Context(0)
    lo, cnt = adist.shard_blocks(n, block, 1, 3)
    pk = A.ANSfold(1, ctx=c0, block_ints=block, ckpt_interval=ck).encode(data[lo:lo + cnt])
    tb = torch.from_numpy(np.concatenate([pk, np.zeros((-pk.size) % 16, np.uint8)])).cuda()
    with pytest.raises(A.AnsxError) as e:
        c1.merge_containers_dev([bufs[0].data_ptr(), tb.data_ptr(), bufs[2].data_ptr()], [sizes[0], pk.size, sizes[2]], out.data_ptr(), out.numel())
    assert e.value.status == 3  # ANSX_ERR_FORMAT
    c0.close()
    c1.close()
    # (3) a frame "too large" for packed restart points turns up during the call (threshold lowered for the test: the
    # real one, 2^16, is out of reach of the fold codecs' alphabets): repeated wide, then wide from the start
    c2 = A.Context(0)
    c2.debug_set("ANSX_TEST_WIDE_AT", "9")
    codec = A.ANSfold(1, ctx=c2, block_ints=block, ckpt_interval=ck)
    assert np.array_equal(codec.encode(data), exp_wide)
    assert c2.last_encode_stats()["path"] & 32
    assert np.array_equal(codec.encode(data), exp_wide)
    assert not (c2.last_encode_stats()["path"] & 32)
    assert np.array_equal(codec.decode(exp_wide, n), data)
    c2.close()
    # (4) ANSint (32-bit frequencies, frames up to 2^27) always takes the wide form
    c3 = A.Context(0)
    vals = (ol.gen_inputs("zipf20s1.2", 30000, seed=5) % 3000).astype(np.uint32)
    ci = A.ANSint(ctx=c3, block_ints=8192, ckpt_interval=1024, compact=False)
    gi = ci.encode(vals)
    assert A.parse_container(gi)["header"].kind == (ol.INT | 0x200)
    assert np.array_equal(gi, cp.build_container(ol.INT, 0, vals, 8192, 1024))
    assert np.array_equal(ci.decode(gi, vals.size), vals)
    c3.close()


def test_header_bound_on_present_symbols_is_untrusted(A):
    """Header bytes 6, 7 = (most symbols present in a block) - 1 size the decoder's per-present-symbol table in LDS.
    It equals the oracle's count; a container that claims fewer than its blocks hold is a format error -- on a fresh
    context and on one that remembers the honest header of the same shape -- never a write past the table."""
    n, block = 50001, 8192
    data = ol.gen_inputs("zipf24", n, seed=9)
    for kind, f in ((ol.FOLD, 3), (ol.RFOLD, 1), (ol.FOLD, 5)):
        d = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7)))) if kind == ol.RFOLD else data
        c0 = A.Context(0)
        codec = codec_for(A, c0, kind, f, block_ints=block, ckpt_interval=1024)
        cont = codec.encode(d)
        H = A.parse_container(cont)["header"]
        present = max(int(ol.oracle_encode(kind, f, d[b * block:(b + 1) * block])[1].present_syms) for b in range(H.nblocks))
        assert H.max_present_m1 + 1 == present <= H.max_nsyms
        assert np.array_equal(codec.decode(cont, n), d)  # (the context now remembers this header)
        for claim in (0, present // 2, present - 2):
            bad = cont.copy()
            bad[6], bad[7] = claim & 0xFF, claim >> 8
            for ctxx in (c0, A.Context(0)):
                with pytest.raises(A.AnsxError) as e:
                    codec_for(A, ctxx, kind, f, block_ints=block, ckpt_interval=1024).decode(bad, n)
                assert e.value.status == 3  # ANSX_ERR_FORMAT
                if ctxx is not c0:
                    ctxx.close()
        assert np.array_equal(codec.decode(cont, n), d)
        c0.close()


def test_rank_shards_merge_into_one_decodable_container(A, ctx):
    """Multi-GPU data path on one device: encode two contiguous block ranges separately (what
    two ranks do), merge on the 'root' (index rebase), decode the merged container as a whole."""
    torch = pytest.importorskip("torch")
    from ans_large_alphabet_amd import dist as adist

    n, block = 200003, 16384
    data = ol.gen_inputs("zipf20s1.2", n, seed=8)
    codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=block, ckpt_interval=1024)
    parts, sizes = [], []
    for r in range(2):
        lo, cnt = adist.shard_blocks(n, block, r, 2)
        c = codec.encode(data[lo:lo + cnt])
        parts.append(torch.from_numpy(c.copy()))
        sizes.append(c.size)
    merged = adist.merge_containers(torch.cat(parts), sizes).numpy()
    whole = codec.encode(data)
    assert np.array_equal(merged, whole)
    assert np.array_equal(codec.decode(merged, n), data)


@pytest.mark.parametrize("kind,f,block,ckpt,world", [(ol.FOLD, 1, 16384, 1024, 2), (ol.FOLD, 1, 4096, 512, 3),
                                                      (ol.RFOLD, 3, 4096, 0, 5), (ol.MSB, 0, 1024, 256, 8)])
def test_native_merge_equals_whole_encode(A, ctx, kind, f, block, ckpt, world):
    """ansx_merge_containers_dev (one HIP kernel on the root) on rank containers in device memory:
    byte-identical to encoding the whole list at once, for several geometries and rank counts (the
    last rank holds a partial block, parts sit at unaligned payload offsets)."""
    torch = pytest.importorskip("torch")
    from ans_large_alphabet_amd import dist as adist

    n = 37 * block + 777
    data = ol.gen_inputs("zipf20s1.2", n, seed=19)
    codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ckpt if ckpt else A.NO_CHECKPOINTS)
    bufs, ptrs, sizes = [], [], []
    for r in range(world):
        lo, cnt = adist.shard_blocks(n, block, r, world)
        c = codec.encode(data[lo:lo + cnt])
        t = torch.zeros(c.size + 64, dtype=torch.uint8, device="cuda")
        t[:c.size] = torch.from_numpy(c.copy()).cuda()
        bufs.append(t)
        ptrs.append(t.data_ptr())
        sizes.append(c.size)
    whole = codec.encode(data)
    out = torch.zeros(whole.size + 4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = ctx.merge_containers_dev(ptrs, sizes, out.data_ptr(), out.numel())
    torch.cuda.synchronize()
    assert nb == whole.size
    assert np.array_equal(out[:nb].cpu().numpy(), whole)
    # refused: capacity, mismatching geometry, a partial block that is not last
    with pytest.raises(A.AnsxError):
        ctx.merge_containers_dev(ptrs, sizes, out.data_ptr(), whole.size - 1)
    if world >= 2:
        with pytest.raises(A.AnsxError):
            ctx.merge_containers_dev(ptrs[::-1], sizes[::-1], out.data_ptr(), out.numel())


def test_rccl_gather_entry_point_from_cpp(tmp_path):
    """ansx_gather_containers (ncclAllGather of sizes + grouped ncclSend/ncclRecv + merge on the root) driven from
    C++ with one thread per visible GPU: tests/tools/gather_selftest.cpp.  On a one-GPU box this is a one-rank
    communicator (size exchange, local slot copy, merge, decode of the merged container); on a node it is the whole
    path over xGMI."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    exe = str(tmp_path / "gather_selftest")
    cmd = ["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(root, "include"),
           os.path.join(here, "tools", "gather_selftest.cpp"), "-o", exe, "-L" + os.path.join(root, "ans_large_alphabet_amd"), "-lansx",
           "-L/opt/rocm/lib", "-lamdhip64", "-lrccl", "-lpthread", "-Wl,-rpath," + os.path.join(root, "ans_large_alphabet_amd"),
           "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe, "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gather_selftest OK" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_decode_on_a_remembered_header_is_verified(A, oracle_built):
    """The second decode of a container shape (kind, fidelity, n, bytes) is launched on the header remembered from the
    first without waiting for the real one; a kernel compares the two and a difference repeats the call the slow way:
    another container of the same size, a changed but valid header, a corrupt header."""
    n = 6 * 4096 + 17
    a = ol.gen_inputs("zipf20s1.2", n, seed=5)
    c = A.Context(0)
    codec = A.ANSfold(1, ctx=c, block_ints=4096, ckpt_interval=512)
    ca = codec.encode(a)
    assert np.array_equal(codec.decode(ca, n), a)      # remembers the header
    assert np.array_equal(codec.decode(ca, n), a)      # launched on it
    # same bytes and shape, other restart interval in the header of a copy -> a header the cached one does not match
    other = A.ANSfold(1, ctx=c, block_ints=4096, ckpt_interval=1024)
    b = ol.gen_inputs("uniform12", n, seed=6)
    for _ in range(200):                              # a second container with the SAME byte count
        cb = other.encode(b)
        if cb.size == ca.size:
            break
        b = np.concatenate([b[1:], b[:1]])
        if cb.size < ca.size:
            b = b.copy()
            b[0] = (int(b[0]) * 7 + 12345) % (1 << 20)
    if cb.size == ca.size:
        assert np.array_equal(other.decode(cb, n), b)
        assert np.array_equal(codec.decode(ca, n), a)
    bad = ca.copy()
    bad[32] ^= 1                                      # nblocks: no longer the remembered header, and not a valid one
    with pytest.raises(A.AnsxError):
        codec.decode(bad, n)
    grown = ca.copy()
    grown[40] ^= 0xFF                                 # max_nsyms 526 -> 753: another header, still a valid bound
    assert np.array_equal(codec.decode(grown, n), a)
    assert np.array_equal(codec.decode(ca, n), a)
    c.close()


def test_native_merge_of_compacted_containers_and_bad_parts(A, ctx):
    """Containers with per-block alphabet compaction (kind word | 0x100: ANSint, ANSfold + compact) merge like the
    others; a part whose header does not describe its own layout (block count, payload offset) is refused
    before the kernel derives section sizes from it."""
    torch = pytest.importorskip("torch")
    from ans_large_alphabet_amd import dist as adist

    for codec, block in ((A.ANSint(ctx=ctx, block_ints=8192, ckpt_interval=1024), 8192),
                         (A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512, compact=True), 4096)):
        n = 11 * block + 123
        data = ol.gen_inputs("zipf20s1.2", n, seed=29)
        bufs, ptrs, sizes, conts = [], [], [], []
        for r in range(3):
            lo, cnt = adist.shard_blocks(n, block, r, 3)
            c = codec.encode(data[lo:lo + cnt])
            t = torch.zeros(c.size + 64, dtype=torch.uint8, device="cuda")
            t[:c.size] = torch.from_numpy(c.copy()).cuda()
            bufs.append(t)
            conts.append(c)
            ptrs.append(t.data_ptr())
            sizes.append(c.size)
        whole = codec.encode(data)
        out = torch.zeros(whole.size + 4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nb = ctx.merge_containers_dev(ptrs, sizes, out.data_ptr(), out.numel())
        torch.cuda.synchronize()
        assert nb == whole.size and np.array_equal(out[:nb].cpu().numpy(), whole)
        pym = adist.merge_containers(torch.cat([torch.from_numpy(c.copy()) for c in conts]), sizes).numpy()
        assert np.array_equal(pym, whole)  # the Python merge agrees
        # header fields the kernel would trust: nblocks (offset 32) + 1, payload_offset (offset 56) + 8
        for off, delta in ((32, 1), (56, 8)):
            bad = conts[1].copy()
            v = int(bad[off:off + 4].view("<u4")[0]) + delta
            bad[off:off + 4] = np.frombuffer(np.uint32(v).tobytes(), dtype=np.uint8)
            tb = torch.zeros(bad.size + 64, dtype=torch.uint8, device="cuda")
            tb[:bad.size] = torch.from_numpy(bad).cuda()
            torch.cuda.synchronize()
            with pytest.raises(A.AnsxError):
                ctx.merge_containers_dev([ptrs[0], tb.data_ptr(), ptrs[2]], sizes, out.data_ptr(), out.numel())


def test_corrupted_payload_never_faults(A, ctx):
    """Random byte corruption anywhere in the container: the decoder must either report
    ANSX_ERR_FORMAT or return (wrong) data — never fault — and the context stays usable."""
    rng = np.random.default_rng(77)
    data0 = ol.gen_inputs("zipf20s1.2", 60000, seed=4)
    # (plain ANSint twice: values the dense model holds, and values modelled in rank space -- either way its decoder walks the
    # value-range prelude sparsely, csrc/ansx_intsparse.h)
    for kind, f, data in ((ol.FOLD, 1, data0), (ol.RFOLD, 1, data0), (ol.FOLD, 3, data0), (ol.INT, 0, data0 % np.uint32(5000)),
                          (ol.INT, 0, ol.ansint_large_list(60000, 1 << 22, 8, "skew"))):
        codec = A.ANSint(ctx=ctx, block_ints=4096, ckpt_interval=512, compact=False) if kind == ol.INT \
            else codec_for(A, ctx, kind, f, block_ints=4096, ckpt_interval=512)
        cont = codec.encode(data).copy()
        for trial in range(40):
            bad = cont.copy()
            region = trial % 4
            if region == 0:      # header
                pos = rng.integers(8, 64, size=2)
            elif region == 1:    # index + restart points
                pos = rng.integers(64, int(A.parse_container(cont)["header"].payload_offset), size=4)
            else:                # payload (preludes, exception bytes, renorm words, final states)
                pos = rng.integers(int(A.parse_container(cont)["header"].payload_offset), cont.size, size=8)
            bad[pos] ^= rng.integers(1, 256, size=len(pos)).astype(np.uint8)
            try:
                out = codec.decode(bad, data.size)
                assert out.size == data.size
            except A.AnsxError as e:
                assert e.status in (1, 3), e.status
        if kind == ol.INT:  # aimed at the preludes: the first bytes of every block stream (vbyte(max_sym), log2 M, the code's top nodes)
            parts = A.parse_container(cont)
            po = int(parts["header"].payload_offset)
            for trial in range(40):
                bad = cont.copy()
                b = int(rng.integers(0, parts["header"].nblocks))
                start = po + int(parts["block_off"][b])
                pos = start + rng.integers(0, min(160, parts["streams"][b].size), size=int(rng.integers(1, 5)))
                bad[pos] ^= rng.integers(1, 256, size=len(pos)).astype(np.uint8)
                try:
                    out = codec.decode(bad, data.size)
                    assert out.size == data.size
                except A.AnsxError as e:
                    assert e.status in (1, 3), e.status
            assert not parts["parse_hints"].any()  # plain ANSint: no parse hints, whichever model wrote the container
        assert np.array_equal(codec.decode(cont, data.size), data)
    # truncated containers
    data = data0
    codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=4096, ckpt_interval=512)
    cont = codec.encode(data)
    for cut in (0, 10, 63, 64, 200, cont.size // 2, cont.size - 1):
        with pytest.raises(A.AnsxError):
            codec.decode(cont[:cut].copy() if cut else np.zeros(1, dtype=np.uint8), data.size)


def test_crafted_index_is_rejected_not_dereferenced(A):
    """the ring decode path skips k_validate_index and lets every parser check the two index entries of
    its own block.  That check must not depend on a container field: a header with payload_bytes = 0 (once the marker of
    single-stream mode) and a garbage index has to be a format error -- on a fresh context and on one that remembers the
    honest header of the same shape -- never a read at cont + payload_offset + <attacker's 64-bit offset>."""
    n, block = 3 * 16384 + 77, 16384
    data = ol.gen_inputs("zipf20s1.2", n, seed=12)
    for kind, f in ((ol.FOLD, 1), (ol.RFOLD, 1)):
        c0 = A.Context(0)
        codec = codec_for(A, c0, kind, f, block_ints=block, ckpt_interval=1024)
        cont = codec.encode(data)
        H = A.parse_container(cont)["header"]
        assert np.array_equal(codec.decode(cont, n), data)  # (c0 now remembers this header)
        # locate the field by value instead of trusting an offset: it is the only u64 in the header equal to payload_bytes
        hdr64 = cont[:64].view("<u8")
        idx = [i for i in range(8) if int(hdr64[i]) == int(H.payload_bytes)]
        assert len(idx) == 1
        pb_off = 8 * idx[0]
        garbage = [0x7FFFFFFFFFFF0000, 1 << 62, 0xFFFFFFFFFFFFFFF0, 1 << 40]
        variants = []
        a = cont.copy()  # payload_bytes = 0, index untouched
        a[pb_off:pb_off + 8] = 0
        variants.append(a)
        b = cont.copy()  # payload_bytes = 0 and a garbage index
        b[pb_off:pb_off + 8] = 0
        ix = b[64:64 + 8 * (H.nblocks + 1)].view("<u8")
        for i in range(H.nblocks + 1):
            ix[i] = garbage[i % len(garbage)]
        variants.append(b)
        c = cont.copy()  # honest payload_bytes, garbage index
        ix = c[64:64 + 8 * (H.nblocks + 1)].view("<u8")
        for i in range(1, H.nblocks):
            ix[i] = garbage[i % len(garbage)]
        variants.append(c)
        d = cont.copy()  # payload_bytes too small for the block count
        d[pb_off:pb_off + 8] = np.frombuffer(np.uint64(37 * H.nblocks).tobytes(), dtype=np.uint8)
        variants.append(d)
        for bad in variants:
            for ctxx in (c0, A.Context(0)):
                with pytest.raises(A.AnsxError) as e:
                    codec_for(A, ctxx, kind, f, block_ints=block, ckpt_interval=1024).decode(bad, n)
                assert e.value.status == 3  # ANSX_ERR_FORMAT
                if ctxx is not c0:
                    ctxx.close()
        assert np.array_equal(codec.decode(cont, n), data)
        # single-stream mode still decodes (its two index entries are the host's own)
        ss = codec_for(A, c0, kind, f, block_ints=A.SINGLE_STREAM)
        small = data[:5000]
        assert np.array_equal(ss.decode(ss.encode(small), small.size), small)
        c0.close()


@pytest.mark.parametrize("kind,f", [(ol.FOLD, 1), (ol.RFOLD, 1), (ol.FOLD, 3)])
def test_decoder_stream_modes(A, ctx, kind, f):
    """The block decoder reads the stream through per-quad LDS rings, a staged copy of the whole
    block stream, or straight from HBM, with rank/select or slot->symbol tables: every combination
    must return the same ints (the default picks by LDS footprint)."""
    n = 3 * 16384 + 4100  # full blocks + a partial one
    data = ol.gen_inputs("zipf20s1.2", n, seed=91)
    data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
    for block, ckpt in ((16384, 1024), (16384, 256), (8192, 2048)):
        codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ckpt)
        cont = codec.encode(data)
        # (beside every set of keys: the decoders it may end in, as ansx_last_decode_stats names them -- a forced key
        # that fell through to another kernel fails here instead of passing on the default one)
        # Where no key says which rings: the 256-byte ones -- this list takes about 1.2 payload bytes per int -- and
        # by default rings at all, since the codec's worst-case stream of these blocks does not fit the staged form's 52 KiB.
        for env, ran in (({}, ("SMALL_RING",)), ({"ANSX_DECODE_MODE": "ring"}, ("SMALL_RING",)),
                         ({"ANSX_DECODE_MODE": "staged"}, ("STAGED",)),
                         ({"ANSX_DECODE_MODE": "staged", "ANSX_NO_STREAM_LDS": "1"}, ("STAGED",)), ({"ANSX_DECODE_TABLE": "1"}, ("TABLE",)),
                         # ring decoder: one block per workgroup (k_decode_rank) / two blocks in one instruction stream (k_decode_rank2)
                         ({"ANSX_DECODE_MODE": "ring", "ANSX_DECODE_PAIR": "never"}, ("SMALL_RING",)),
                         ({"ANSX_DECODE_MODE": "ring", "ANSX_DECODE_PAIR": "always"}, ("PAIR",)),
                         # 512-byte worst-case rings / 256-byte speculative rings (chosen by the container's bytes per int otherwise)
                         ({"ANSX_DECODE_MODE": "ring", "ANSX_DECODE_SMALL_RING": "never"}, ("RING",)),
                         ({"ANSX_DECODE_MODE": "ring", "ANSX_DECODE_SMALL_RING": "always"}, ("SMALL_RING",))):
            try:
                for k, v in env.items():
                    ctx.debug_set(k, v)
                assert np.array_equal(codec.decode(cont, n), data), (block, ckpt, env)
                st = ctx.last_decode_stats()
                assert st["decoder"] in ran, (block, ckpt, env, st)
                if "ANSX_NO_STREAM_LDS" in env:
                    assert st["stream_cap"] == 0, (block, ckpt, env, st)
                elif env.get("ANSX_DECODE_MODE") == "staged":
                    assert st["stream_cap"] != 0, (block, ckpt, env, st)  # (else the pair of cases is one case twice)
            finally:
                for k in env:
                    ctx.debug_set(k, None)


def test_small_ring_decoder_takes_intervals_back(A, ctx):
    """k_decode_rank<.., 2> (round 4): 256-byte stream rings that do not guarantee an interval's reads stay inside the window
    -- the kernel checks after every four steps and decodes the interval again behind a full window.  Forced onto lists
    that consume up to 28 bytes per step (30-bit values: three exception bytes and a renormalisation word almost every
    symbol), where nearly every interval is taken back, and onto mixtures; restart intervals that leave leftover steps."""
    rng = np.random.default_rng(8)
    n = 5 * 16384 + 1000
    heavy = rng.integers(1 << 24, 1 << 30, size=n, dtype=np.uint32)
    mixed = np.where(rng.random(n) < 0.9, rng.integers(0, 200, size=n), rng.integers(1 << 24, 1 << 30, size=n)).astype(np.uint32)
    bursts = ol.gen_inputs("zipf20s1.2", n, seed=3).copy()
    for a in range(0, n - 200, 3000):  # stretches of maximal consumption inside an otherwise lean stream
        bursts[a:a + 160] = rng.integers(1 << 29, 1 << 30, size=160, dtype=np.uint32)
    for data in (heavy, mixed, bursts):
        for kind, f, block, ck in ((ol.FOLD, 1, 16384, 1024), (ol.RFOLD, 1, 8192, 256), (ol.FOLD, 3, 16384, 1028 - 4), (ol.MSB, 0, 4096, 64)):
            d = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7)))) if kind == ol.RFOLD else data
            codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ck)
            cont = codec.encode(d)
            try:
                ctx.debug_set("ANSX_DECODE_MODE", "ring")
                ctx.debug_set("ANSX_DECODE_SMALL_RING", "always")
                assert np.array_equal(codec.decode(cont, n), d), (kind, f, block, ck)
                assert ctx.last_decode_stats()["decoder"] == "SMALL_RING", (kind, f, block, ck, ctx.last_decode_stats())
            finally:
                ctx.debug_set("ANSX_DECODE_MODE", None)
                ctx.debug_set("ANSX_DECODE_SMALL_RING", None)


def test_random_geometries_round_trip_and_match_oracle(A, ctx):
    """Seeded sweep over block sizes / restart intervals / lengths that exercise the geometry-
    dependent paths: restart intervals that are not a multiple of 16 ints (ring leftover steps),
    blocks that are / are not a multiple of the interval (ring vs staged decoder), partial last
    blocks, fewer segments than a wave, one-int tails.  Every block stream and restart point must
    equal the oracle's and the decoder must return the input."""
    rng = np.random.default_rng(2024)
    fams = ["zipf20s1.2", "uniform256", "uniform20", "geom0.01", "sparse_large"]
    cases = [(4112, 1028, 3 * 4112 + 5), (16448, 1028, 2 * 16448), (8192, 2048, 8192 * 3 + 4095),
             (4096, 4096, 4096 * 5 + 1), (1024, 256, 1024 * 9 + 3), (20480, 1280, 20480 * 2 + 1281),
             (16384, 64, 16384 + 70), (2052, 4, 2052 * 2 + 2), (65536, 1024, 65536 + 1000)]
    for block, ckpt, n in cases:
        fam = fams[int(rng.integers(0, len(fams)))]
        kind, f = [(ol.FOLD, 1), (ol.FOLD, 3), (ol.RFOLD, 1), (ol.MSB, 0)][int(rng.integers(0, 4))]
        data = ol.gen_inputs(fam, n, seed=int(rng.integers(1, 1 << 30)))
        if kind == ol.RFOLD:
            data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
        codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ckpt)
        cont = codec.encode(data)
        check_container(A, cont, data, kind, f, block, ckpt)
        assert np.array_equal(codec.decode(cont, n), data), (block, ckpt, n, fam, kind, f)


def test_harnesses_run_and_stream_bits_equal_the_reference(A, ctx, tmp_path):
    """tools/table_effectiveness --stream writes exactly the reference's streams, so its bits/int
    column must equal 8 * len(reference stream) / n (the oracle stands in for the reference: it is
    pinned byte-identical to it); tools/table_efficiency must run and verify its round trips."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tools = os.path.join(root, "ans_large_alphabet_amd", "tools")
    subprocess.run(["make", "-C", tools], check=True, capture_output=True)
    files = {"a_uniform.u32": ol.gen_inputs("uniform256", 20000, seed=1),
             "b_zipf.u32": ol.gen_inputs("zipf20s1.2", 30001, seed=2)}
    for name, arr in files.items():
        arr.astype(np.uint32).tofile(str(tmp_path / name))
    out = subprocess.run([os.path.join(tools, "table_effectiveness.x"), "-i", str(tmp_path), "--stream"],
                         check=True, capture_output=True, text=True).stdout
    rows = {}
    cur = None
    for line in out.splitlines():
        m = re.match(r"^(ANS\S+)\s+&$", line)
        if m:
            cur = m.group(1)
            rows[cur] = []
        elif cur and re.search(r"\d+\.\d{4}", line):
            rows[cur].append(float(re.search(r"(\d+\.\d{4})", line).group(1)))
    for name, kind, f in (("ANSfold-1", ol.FOLD, 1), ("ANSfold-5", ol.FOLD, 5), ("ANSrfold-3", ol.RFOLD, 3), ("ANSmsb", ol.MSB, 0)):
        want = []
        for key in sorted(files):
            data = files[key].astype(np.uint32)
            stream = ol.oracle_encode(kind, f, data)[0]
            want.append(round(8.0 * stream.size / data.size, 4))
        assert rows[name] == pytest.approx(want, abs=1.01e-4), (name, rows[name], want)
    eff = subprocess.run([os.path.join(tools, "table_efficiency.x"), "-i", str(tmp_path), "--bits"],
                         check=True, capture_output=True, text=True).stdout
    assert "\\method{ANSfold-1}" in eff and "\\method{ANSrfold-5}" in eff and "bits/int" in eff
    # -t: the same lists as decimal text, one number per line (util.hpp:160-170): identical bits/int columns
    tdir = tmp_path / "text"
    tdir.mkdir()
    for name, arr in files.items():
        np.savetxt(str(tdir / name.replace(".u32", ".txt")), arr.astype(np.uint32), fmt="%u")
    out_t = subprocess.run([os.path.join(tools, "table_effectiveness.x"), "-t", "-i", str(tdir), "--stream"],
                           check=True, capture_output=True, text=True).stdout
    assert out_t == out
    # the compacted codecs ("ANS" = ANSint, ANSmsb with per-block alphabets) run and verify their round trips
    blocked = subprocess.run([os.path.join(tools, "table_effectiveness.x"), "-i", str(tmp_path)],
                             check=True, capture_output=True, text=True).stdout
    assert re.search(r"^ANS\s+&$", blocked, re.M) and "ANSmsb" in blocked


def test_default_stream_ordering_without_synchronize(A, ctx):
    """PyTorch's default stream has handle 0, which reaches the C-ABI as NULL = the context's own
    stream.  That stream must be ordered against the legacy default stream: the input below is still
    being produced by torch kernels when encode_dev is called, and the output is consumed by torch
    kernels right after decode_dev, with no explicit synchronisation anywhere."""
    torch = pytest.importorskip("torch")
    n = 48 * (1 << 20)
    codec = codec_for(A, ctx, ol.FOLD, 1)
    cap = codec.bound(n)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(99)
    for rep in range(4):
        d_back = torch.zeros(n, dtype=torch.int32, device="cuda")
        x = torch.randint(0, 1 << 20, (n,), generator=g, device="cuda", dtype=torch.int64)
        for _ in range(6):                      # keep the default stream busy producing the input
            x = (x * 6364136223846793005 + 1442695040888963407) & ((1 << 40) - 1)
        d_in = (x >> 20).to(torch.int32)        # < 2^20
        nb = codec.encode_dev(d_in.data_ptr(), n, d_out.data_ptr(), cap)       # stream = None
        codec.decode_dev(d_out.data_ptr(), nb, d_back.data_ptr(), n)
        assert bool(torch.equal(d_back, d_in)), rep


def test_encoder_table_modes(A, ctx):
    """Alphabets too large for the LDS-table encoder take the compact-table-from-HBM mode (f64 state,
    branch-free step, hand-counted vmcnt waits); ANSX_ENCODE_GTAB16 forces the older 16-byte-entry
    integer-state kernel.  Both must write byte-identical containers (and equal the oracle)."""
    n = 4 * 16384 + 1234
    for fam, f in (("zipf24", 3), ("uniform20", 5), ("sparse_large", 3), ("zipf20s1.2", 1)):
        data = ol.gen_inputs(fam, n, seed=7 + f)
        codec = codec_for(A, ctx, ol.FOLD, f, block_ints=16384, ckpt_interval=1024)
        cont = codec.encode(data)
        check_container(A, cont, data, ol.FOLD, f, 16384, 1024)
        for env in ("ANSX_ENCODE_GTAB16", "ANSX_TEST_TABLE16_FIXUP"):  # 16-byte entries written by the
            try:                                                         # model kernel / rebuilt afterwards
                ctx.debug_set(env, "1")
                cont16 = codec.encode(data)
            finally:
                ctx.debug_set(env, None)
            assert np.array_equal(cont, cont16), (fam, f, env)
        assert np.array_equal(codec.decode(cont, n), data)


def test_encoder_producer_consumer_pairs(A):
    """k_encode_pc (round 4): the LDS-table encoder as a producer wave (fold map, table look-up, reciprocal; a batch ahead,
    16 bytes per symbol through LDS) and a consumer wave (state chain, byte emission) per 16 blocks.  Forced on small lists here (the launch site
    keeps it for grids that fill the chip).  Every block stream, restart point and header field must equal the oracle's,
    the container must equal the one the single-wave kernel writes, on the first call of a geometry (discovery path) and on
    the hinted ones."""
    cases = [  # (family, kind, f, block_ints, ckpt, n)
        ("zipf20s1.2", ol.FOLD, 1, 1024, 256, 64 * 1024 * 2 + 1024 * 5 + 77),   # two pair workgroups + rest + a partial block
        ("uniform256", ol.FOLD, 1, 512, 128, 64 * 512),                          # exactly one pair workgroup, nothing left
        ("geom0.01", ol.FOLD, 1, 2048, 0, 64 * 2048 + 3),                        # no restart points; a 3-int last block
        ("sparse_large", ol.FOLD, 1, 1024, 1024 // 2, 64 * 1024 + 1024),         # exception bytes of every length
        ("zipf20s1.2", ol.RFOLD, 1, 1024, 256, 64 * 1024 * 3),
        ("zipf20s1.2", ol.MSB, 0, 1024, 512, 64 * 1024 + 640),                   # a map that is not a power-of-two fold
        ("uniform20", ol.FOLD, 1, 4096, 1024, 64 * 4096 + 4096 * 2),
        ("const7", ol.FOLD, 1, 1024, 256, 64 * 1024),                            # one symbol, frame 32768
    ]
    for fam, kind, f, block, ck, n in cases:
        expect_pc = True  # (alphabets of ~1000 symbols do not fit 64 LDS tables per CU: the two-round shape takes them)
        if fam == "const7":
            data = np.full(n, 7, dtype=np.uint32)
        else:
            data = ol.gen_inputs(fam, n, seed=31 + f + block)
        if kind == ol.RFOLD:
            data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
        kw = dict(block_ints=block, ckpt_interval=ck if ck else A.NO_CHECKPOINTS)
        c_ref = A.Context(0)
        c_ref.debug_set("ANSX_NO_PC", "1")
        ref = codec_for(A, c_ref, kind, f, **kw).encode(data)
        c_ref.close()
        c_pc = A.Context(0)
        c_pc.debug_set("ANSX_FORCE_PC", "1")
        codec = codec_for(A, c_pc, kind, f, **kw)
        for call in range(3):  # discovery, then hinted (fast model path from the second on)
            got = codec.encode(data)
            assert bool(c_pc.last_encode_stats()["path"] & 128) == expect_pc, (fam, kind, f, block, ck, call)  # the pair kernel really ran
            assert np.array_equal(got, ref), (fam, kind, f, block, ck, call)
        check_container(A, got, data, kind, f, block, ck)
        assert np.array_equal(codec.decode(got, n), data)
        c_pc.close()
    # the two shapes the launch site chooses by itself: (C) short lists -- one pair per workgroup -- and (B) alphabets too
    # large for 64 LDS tables per CU whose tables fit at 32 (two pairs per workgroup, batches of 4 steps; BASELINE config 3)
    auto = [("zipf20s1.2", ol.FOLD, 1, 1024, 256, 16 * 1024 * 3),                    # C: three workgroups
            ("uniform256", ol.MSB, 0, 512, 0, 16 * 512),                           # C: one workgroup, no restart points
            ("zipf24", ol.FOLD, 3, 1024, 256, 32 * 1024 * 2 + 1024 * 3 + 9),        # B: three workgroups, the last one 3 blocks + 9 ints
            ("zipf24", ol.RFOLD, 3, 2048, 512, 32 * 2048),                         # B: exactly one workgroup
            ("uniform24", ol.FOLD, 3, 1024, 16, 32 * 1024 + 1024)]                 # B: a restart point every 4 groups (one batch)
    for fam, kind, f, block, ck, n in auto:
        data = ol.gen_inputs(fam, n, seed=77 + f + block)
        if kind == ol.RFOLD:
            data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
        kw = dict(block_ints=block, ckpt_interval=ck if ck else A.NO_CHECKPOINTS)
        c_ref = A.Context(0)
        c_ref.debug_set("ANSX_NO_PC", "1")
        ref = codec_for(A, c_ref, kind, f, **kw).encode(data)
        assert not (c_ref.last_encode_stats()["path"] & 128)
        c_ref.close()
        c_pc = A.Context(0)
        codec = codec_for(A, c_pc, kind, f, **kw)
        for call in range(3):
            got = codec.encode(data)
            assert c_pc.last_encode_stats()["path"] & 128, (fam, kind, f, block, ck, call)
            assert np.array_equal(got, ref), (fam, kind, f, block, ck, call)
        check_container(A, got, data, kind, f, block, ck)
        assert np.array_equal(codec.decode(got, n), data)
        c_pc.close()


def test_encoder_pairs_take_ragged_lists_whole(A):
    """k_encode_pc takes every block of a call: its last workgroup pads itself with neutral steps where the list ends inside it
    (blocks that do not exist; the partial last block, whose n % 4 tail symbols go to state 0 before its groups).  A frame of
    2^16 has no neutral entry in the 16-bit frequency field: its stand-in lets the state creep and the consumer sets it back
    at the lane's first live step -- so one case must have a partial block with such a frame.  No second encoder launch."""
    cases = [  # (family, kind, f, block_ints, ckpt, n, forced)
        ("geom0.01", ol.FOLD, 1, 512, 128, 512 * 5 + 130, True),               # one workgroup: 5 blocks + 130 ints (tail 2), 58 that are not there
        ("uniform20", ol.FOLD, 1, 1024, 256, 64 * 1024 + 1024 * 17 + 1023, True),  # tail 3
        ("zipf20s1.2", ol.FOLD, 1, 1024, 256, 64 * 1024 * 2 + 1, True),          # a one-int last block
        ("zipf20s1.2", ol.RFOLD, 1, 1024, 128, 64 * 1024 + 517, True),
        ("zipf20s1.2", ol.MSB, 0, 2048, 512, 64 * 2048 + 2048 * 63 + 2047, True),
        ("uniform24", ol.FOLD, 3, 1024, 256, 32 * 1024 * 2 + 1024 * 5 + 1001, False),  # shape B (two pairs, S = 4), frames of 2^16
        ("uniform24", ol.FOLD, 3, 2048, 64, 32 * 2048 + 2048 * 31 + 6, False),
        ("zipf20s1.2", ol.FOLD, 1, 1024, 256, 16 * 1024 * 3 + 1024 * 2 + 333, False),  # shape C (one pair)
        ("const7", ol.FOLD, 1, 1024, 256, 64 * 1024 + 700, True),                # frame 32768: the largest with a true neutral entry
        ("uniform24", ol.FOLD, 3, 1 << 19, 4096, (1 << 19) * 2 + 500001, True),  # frames of 2^16, the partial block's too
    ]
    saw_wide_partial = False
    for fam, kind, f, block, ck, n, forced in cases:
        if fam == "const7":
            data = np.full(n, 7, dtype=np.uint32)
        else:
            data = ol.gen_inputs(fam, n, seed=131 + f + block)
        if kind == ol.RFOLD:
            data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
        last = data[(n // block) * block:]
        if len(last) and kind == ol.FOLD and ol.oracle_encode(kind, f, last)[1].log2_frame == 16:
            saw_wide_partial = True
        kw = dict(block_ints=block, ckpt_interval=ck)
        c_ref = A.Context(0)
        c_ref.debug_set("ANSX_NO_PC", "1")
        ref = codec_for(A, c_ref, kind, f, **kw).encode(data)
        c_ref.close()
        c_pc = A.Context(0)
        if forced:
            c_pc.debug_set("ANSX_FORCE_PC", "1")
        c_pc.profile(True)
        codec = codec_for(A, c_pc, kind, f, **kw)
        for call in range(3):
            got = codec.encode(data)
            assert c_pc.last_encode_stats()["path"] & 128, (fam, kind, f, block, ck, n, call)
            assert np.array_equal(got, ref), (fam, kind, f, block, ck, n, call)
            assert "k_encode_rest" not in [k for k, _, _ in c_pc.profile_get()], (fam, n)
        check_container(A, got, data, kind, f, block, ck)
        assert np.array_equal(codec.decode(got, n), data)
        c_pc.close()
    assert saw_wide_partial


def test_prelude_parser_paths(A, ctx):
    """The decoder's prelude parser has a fast loop (alphabets whose interpolative values fit 16 bits,
    the first 512 prelude bytes staged in LDS), an in-kernel fallback for lanes whose prelude
    outgrows the staged bytes, and a generic kernel.  Valid preludes of such alphabets stay below
    ~420 bytes, so the fallback is forced by shrinking the staged window; all three paths must
    decode the same container identically."""
    rng = np.random.default_rng(5)
    n = 5 * 16384 + 777
    third = n // 3
    data = np.concatenate([rng.integers(0, 256, third), rng.integers(256, 1 << 16, third),
                           rng.integers(1 << 16, 1 << 24, n - 2 * third)]).astype(np.uint32)
    rng.shuffle(data)
    codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=16384, ckpt_interval=1024)
    cont = codec.encode(data)
    parts = check_container(A, cont, data, ol.FOLD, 1, 16384, 1024)
    preludes = [ol.oracle_encode(ol.FOLD, 1, data[b * 16384:(b + 1) * 16384])[1].prelude_bytes
                for b in range(parts["header"].nblocks)]
    assert min(preludes) > 300, preludes
    assert parts["header"].max_nsyms + (1 << parts["header"].max_log2_frame) + 3 <= 65535  # fast kernel eligible
    assert np.array_equal(codec.decode(cont, n), data)             # eight lanes per block on the parse hints (default)
    try:
        ctx.debug_set("ANSX_PARSE_FAST", "1")                      # one lane per block: the E-array fast loop ...
        assert np.array_equal(codec.decode(cont, n), data)
        for words in ("64", "32", "2"):                            # ... 256 / 128 / 8 staged bytes: its fallback lanes
            ctx.debug_set("ANSX_PARSE_STAGE_WORDS", words)
            assert np.array_equal(codec.decode(cont, n), data), words
        ctx.debug_set("ANSX_PARSE_STAGE_WORDS", None)
        ctx.debug_set("ANSX_PARSE_FAST", None)
        ctx.debug_set("ANSX_PARSE_WIN", "1")                       # one lane per block: windowed parser
        assert np.array_equal(codec.decode(cont, n), data)
        ctx.debug_set("ANSX_PARSE_WIN", None)
        ctx.debug_set("ANSX_PARSE_GENERIC", "1")                   # generic kernel
        assert np.array_equal(codec.decode(cont, n), data)
    finally:
        ctx.debug_set("ANSX_PARSE_STAGE_WORDS", None)
        ctx.debug_set("ANSX_PARSE_FAST", None)
        ctx.debug_set("ANSX_PARSE_WIN", None)
        ctx.debug_set("ANSX_PARSE_GENERIC", None)
    # the container's parse hints equal the oracle's (bit offsets of the top right subtrees of every prelude)
    for b in range(parts["header"].nblocks):
        want = ol.prelude_hints(parts["streams"][b], 0)
        assert np.array_equal(parts["parse_hints"][b], want), b
    # a corrupted hint must never fault (the result may be an error or wrong ints)
    for word in (1, 3, 7):
        bad = cont.copy()
        hoff = parts["header"].payload_offset - 32 * parts["header"].nblocks
        bad[hoff + 4 * word: hoff + 4 * word + 4] = np.frombuffer(np.uint32(0x7FFFFFF0).tobytes(), dtype=np.uint8)
        try:
            codec.decode(bad, n)
        except A.AnsxError:
            pass
    # preludes longer than one staged window (alphabets of thousands of symbols): the windowed parser
    # re-stages; cross-checked against the generic kernel
    wide = ol.gen_inputs("uniform24", n, seed=6)
    for f in (3, 5):
        cw = codec_for(A, ctx, ol.FOLD, f, block_ints=16384, ckpt_interval=1024)
        contw = cw.encode(wide)
        assert np.array_equal(cw.decode(contw, n), wide), f
        for knob in ("ANSX_PARSE_GENERIC", "ANSX_PARSE_WIN"):
            try:
                ctx.debug_set(knob, "1")
                assert np.array_equal(cw.decode(contw, n), wide), (f, knob)
            finally:
                ctx.debug_set(knob, None)


@pytest.mark.parametrize("f", [1, 3])
def test_rfold_large_blocks_and_whole_list(A, ctx, f):
    """Blocks longer than one LDS hash table (HBM hash-table path), incl. single-stream mode."""
    n = 200003
    for fam in ("zipf20s1.2", "uniform20", "geom0.01"):
        data = ol.gen_inputs(fam, n, seed=31 * f)
        codec = codec_for(A, ctx, ol.RFOLD, f, block_ints=65536, ckpt_interval=4096)
        cont = codec.encode(data)
        check_container(A, cont, data, ol.RFOLD, f, 65536, 4096)
        assert np.array_equal(codec.decode(cont, n), data)
        codec = codec_for(A, ctx, ol.RFOLD, f, block_ints=A.SINGLE_STREAM)
        s = codec.encode(data)
        exp, info, _, _ = ol.oracle_encode(ol.RFOLD, f, data)
        assert np.array_equal(s, exp), (f, fam)
        assert np.array_equal(codec.decode(s, n), data)


@pytest.mark.parametrize("fam", FAMS)
def test_msb_blocks_match_oracle(A, ctx, fam):
    """ANSmsb: same kernels, fixed-threshold map; per-block parity + round trip."""
    n = 70001
    data = ol.gen_inputs(fam, n, seed=41)
    data[:11] = np.array([0, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1,
                          (1 << 30) - 1], dtype=np.uint32)
    codec = codec_for(A, ctx, ol.MSB, 0, block_ints=16384, ckpt_interval=1024)
    assert codec.name() == "ANSmsb"
    cont = codec.encode(data)
    check_container(A, cont, data, ol.MSB, 0, 16384, 1024)
    assert np.array_equal(codec.decode(cont, n), data)
    if fam in ("zipf20s1.2", "boundaries"):
        codec = codec_for(A, ctx, ol.MSB, 0, block_ints=A.SINGLE_STREAM)
        s = codec.encode(data[:9001])
        exp, _, _, _ = ol.oracle_encode(ol.MSB, 0, data[:9001])
        assert np.array_equal(s, exp)
        assert np.array_equal(codec.decode(exp, 9001), data[:9001])


def _kernels_of(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = fn()
        names = [k for k, _ms, _n in ctx.profile_get()]
    finally:
        ctx.profile(False)
    return out, names


@pytest.mark.parametrize("kind,f,fam", [(ol.FOLD, 1, "zipf20s1.2"), (ol.FOLD, 3, "zipf24"), (ol.RFOLD, 1, "zipf20s1.2"),
                                         (ol.MSB, 0, "sparse_large"), (ol.FOLD, 2, "uniform20")])
def test_hinted_paths_run_and_match(A, kind, f, fam, oracle_built):
    """Alphabet hint: learned on the first call (mid-call read-back), used from the second on (no
    read-back; optionally the fused model kernel); a hint that is too small, or an input that outgrows
    it, repeats on the discovery path.  All byte-identical."""
    n = 5 * 16384 + 333
    data = ol.gen_inputs(fam, n, seed=77)
    if kind == ol.RFOLD:
        data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
    wide = ol.gen_inputs("uniform24" if kind != ol.RFOLD else "uniform20", n, seed=78)
    for fused in (False, True):
        c = A.Context(0)
        if fused:
            c.debug_set("ANSX_MODEL_FUSED", "1")
        codec = codec_for(A, c, kind, f, block_ints=16384, ckpt_interval=1024)
        first, k1 = _kernels_of(c, lambda: codec.encode(data))
        assert "k_fold_hist" in k1 and "k_model_fused" not in k1
        second, k2 = _kernels_of(c, lambda: codec.encode(data))
        if fused:
            assert "k_model_fused" in k2 and "k_fold_hist" not in k2 and "k_scale_attempts" not in k2
        else:
            assert k2.count("k_fold_hist") == 1 and "k_model_fused" not in k2
            # geometries whose blocks settle within 8 candidate frame sizes take the fast model kernels
            took_fast = (c.last_encode_stats()["path"] & 4) != 0
            assert ("k_candidates" in k2) == took_fast and ("k_model_finish" in k2) == took_fast
            if kind == ol.FOLD and f == 1:
                assert took_fast and "k_scale_attempts" not in k2 and "k_write_prelude" not in k2
        assert np.array_equal(first, second)
        check_container(A, second, data, kind, f, 16384, 1024)
        # an input with a larger alphabet than the learned hint: miss -> discovery path, hint grows
        third, k3 = _kernels_of(c, lambda: codec.encode(wide))
        check_container(A, third, wide, kind, f, 16384, 1024)
        assert np.array_equal(codec.decode(third, n), wide)
        # and a forced tiny hint
        c.debug_set("ANSX_NS_HINT", "8")
        fourth, k4 = _kernels_of(c, lambda: codec.encode(data))
        assert np.array_equal(first, fourth)
        assert "k_fold_hist" in k4 and (("k_model_fused" in k4) == fused)  # tried, missed, repeated
        c.close()


def test_fast_model_path_and_its_repeats(A, oracle_built):
    """k_candidates / k_model_finish (ansx_fastmodel.h): taken from the second call of a geometry on, byte-identical
    to the exact kernels; a comparison inside the guard band of the stop rule (forced here by widening the band),
    too few candidate lanes for some block, or an alphabet above the hint repeat the call on the exact path."""
    n = 9 * 16384 + 4321
    for kind, f, fam in ((ol.FOLD, 1, "zipf20s1.2"), (ol.FOLD, 3, "zipf24"), (ol.RFOLD, 3, "zipf24"), (ol.MSB, 0, "zipf20s1.2"),
                         (ol.FOLD, 1, "uniform256"), (ol.FOLD, 5, "geom0.01")):
        data = ol.gen_inputs(fam, n, seed=91)
        if kind == ol.RFOLD:
            data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
        c = A.Context(0)
        codec = codec_for(A, c, kind, f, block_ints=16384, ckpt_interval=1024)
        first = codec.encode(data)                       # discovery: exact kernels, learns the hints
        assert c.last_encode_stats()["path"] & ~128 == 0
        second, k2 = _kernels_of(c, lambda: codec.encode(data))
        st = c.last_encode_stats()
        if f <= 3:                                       # (f = 5: 16384-slot alphabets stay on the exact path)
            assert st["path"] & ~128 == 5 and "k_candidates" in k2 and "k_scale_attempts" not in k2, (kind, f, fam, st)
        assert np.array_equal(first, second)
        check_container(A, second, data, kind, f, 16384, 1024)
        if f > 3:
            c.close()
            continue
        c.debug_set("ANSX_FAST_GUARD", "0.5")            # every comparison counts as too close: repeat
        third, k3 = _kernels_of(c, lambda: codec.encode(data))
        assert c.last_encode_stats()["path"] & 16 and "k_candidates" in k3 and "k_scale_attempts" in k3
        assert np.array_equal(first, third)
        c.debug_set("ANSX_FAST_GUARD", None)
        c.debug_set("ANSX_T_HINT", "4")                  # four candidate lanes: blocks that need a fifth repeat
        fourth = codec.encode(data)
        assert np.array_equal(first, fourth)
        c.debug_set("ANSX_T_HINT", None)
        for _ in range(2):                               # hints recover: the fast path again
            fifth = codec.encode(data)
        assert c.last_encode_stats()["path"] & ~128 == 5 and np.array_equal(first, fifth)
        assert np.array_equal(codec.decode(fifth, n), data)
        c.close()


@pytest.mark.parametrize("kind,f", [(ol.FOLD, 1), (ol.RFOLD, 1), (ol.FOLD, 3), (ol.MSB, 0)])
def test_close_calls_are_decided_again_on_the_host(A, oracle_built, kind, f):
    """The stop rule XH < 1.001 H (ans_util.hpp:149) is evaluated with a portable log2 on the device and with libm's
    in the reference.  Blocks with a comparison inside ANSX_NEAR_BAND of its threshold (1e-12; none ever occurs) are
    decided again on the host with libm, and a differing decision is forced in a repeat of the call.  Here the band
    is widened so that such blocks exist, and then the device is made to decide them the WRONG way: the bytes must
    still be the oracle's."""
    n = 7 * 16384 + 1234
    data = ol.gen_inputs("zipf20s1.2", n, seed=61)
    if kind == ol.RFOLD:
        data = np.minimum(data, np.uint32((1 << 30) - 1 - (1 << (f + 7))))
    c = A.Context(0)
    codec = codec_for(A, c, kind, f, block_ints=16384, ckpt_interval=1024)
    ref = codec.encode(data)
    st = c.last_encode_stats()
    assert st["near_threshold_decisions"] == 0 and st["host_redecided"] == 0
    check_container(A, ref, data, kind, f, 16384, 1024)
    c.debug_set("ANSX_NO_FAST_MODEL", "1")   # (the fast model kernels repeat on the exact ones for anything within 1e-9)
    c.debug_set("ANSX_NEAR_BAND", "2e-2")
    again = codec.encode(data)
    st = c.last_encode_stats()
    assert st["near_threshold_decisions"] > 0 and st["host_redecided"] == 0, st  # the host agrees with the device
    assert np.array_equal(again, ref)
    c.debug_set("ANSX_TEST_NEAR_FLIP", "1")
    fixed = codec.encode(data)
    st = c.last_encode_stats()
    assert st["near_threshold_decisions"] > 0 and st["host_redecided"] > 0, st  # ... and overrules it when it must
    assert np.array_equal(fixed, ref)
    assert np.array_equal(codec.decode(fixed, n), data)
    c.close()


def test_fused_model_many_geometries(A, oracle_built):
    """Fused path over block sizes / lengths incl. partial and tiny blocks, constant blocks (16 frame
    sizes: more than one candidate batch) and blocks that take the reference's degenerate exits."""
    c = A.Context(0)
    c.debug_set("ANSX_NS_HINT", "1024")
    c.debug_set("ANSX_MODEL_FUSED", "1")
    rng = np.random.default_rng(11)
    for block, ckpt, n in ((16384, 1024, 40000), (4096, 512, 12289), (1024, 256, 5000), (64, 0, 1000), (16384, 1024, 3)):
        for fam in ("zipf20s1.2", "uniform256", "geom0.4", "constant", "boundaries", "sparse_large"):
            data = ol.gen_inputs(fam, n, seed=int(rng.integers(1 << 30)))
            for kind, f in ((ol.FOLD, 1), (ol.MSB, 0), (ol.RFOLD, 1)):
                d = np.minimum(data, np.uint32((1 << 30) - 1 - 256)) if kind == ol.RFOLD else data
                kw = dict(block_ints=block, ckpt_interval=ckpt if ckpt else A.NO_CHECKPOINTS)
                codec = codec_for(A, c, kind, f, **kw)
                cont = codec.encode(d)
                check_container(A, cont, d, kind, f, block, ckpt)
                assert np.array_equal(codec.decode(cont, d.size), d), (block, fam, kind)
    c.close()


def test_bwtmtf_fixture_blocks_and_whole_list(A, ctx):
    """Config 5 fallback: BWT-MTF ranks of a local text (tests/golden/bwtmtf.u32, made by
    tools/generate_bwtmtf.x); expected streams were produced by the real reference (oracle/_ref)."""
    with open(os.path.join(GOLD, "bwtmtf.json")) as fh:
        meta = json.load(fh)
    data = np.fromfile(os.path.join(GOLD, "bwtmtf.u32"), dtype=np.uint32)
    assert hashlib.sha256(data.tobytes()).hexdigest() == meta["input_sha256"]
    for kind_name, f in (("fold", 1), ("fold", 5), ("rfold", 1)):
        kind = ol.FOLD if kind_name == "fold" else ol.RFOLD
        want = {(e["first"], e["n"]): e for e in meta["streams"] if e["kind"] == kind_name and e["f"] == f}
        whole = codec_for(A, ctx, kind, f, block_ints=A.SINGLE_STREAM).encode(data)
        e = want[(0, data.size)]
        assert whole.size == e["stream_len"] and hashlib.sha256(whole.tobytes()).hexdigest() == e["stream_sha256"]
        codec = codec_for(A, ctx, kind, f, block_ints=16384, ckpt_interval=1024)
        cont = codec.encode(data)
        parts = A.parse_container(cont)
        for b, stream in enumerate(parts["streams"]):
            e = want[(b * 16384, min(16384, data.size - b * 16384))]
            assert stream.size == e["stream_len"], (kind_name, f, b)
            assert hashlib.sha256(stream.tobytes()).hexdigest() == e["stream_sha256"], (kind_name, f, b)
        assert np.array_equal(codec.decode(cont, data.size), data)
    st = ctx.last_encode_stats()
    assert st["near_threshold_decisions"] == 0 and st["max_nsyms"] > 0


@pytest.mark.parametrize("kind,f,spec", [(ol.FOLD, 3, "zipf24s1.2"), (ol.RFOLD, 3, "zipf24s1.2"), (ol.FOLD, 1, "uniform1-256")])
def test_full_size_configs_roundtrip_and_spot_blocks(A, ctx, kind, f, spec):
    """BASELINE configs 3 (ANSfold-3 / ANSrfold-3 on Zipf over 2^24) and 1's data shape at a size where
    only properties can be checked everywhere: device round trip of the whole list, container header
    sanity, and 24 blocks spread over the list byte-compared with the oracle (streams + restart points)."""
    import torch

    n = 64 * (1 << 20) + 12345
    d_in = torch.empty(n, dtype=torch.int32, device="cuda")
    A.generate_dev(ctx, spec, d_in.data_ptr(), n, seed=2024)
    codec = codec_for(A, ctx, kind, f, block_ints=16384, ckpt_interval=1024)
    cap = codec.bound(n)
    d_out = torch.empty(min(cap, 8 * n + (64 << 20)), dtype=torch.uint8, device="cuda")
    d_back = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nb = codec.encode_dev(d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel())
    codec.decode_dev(d_out.data_ptr(), nb, d_back.data_ptr(), n)
    assert bool(torch.equal(d_back, d_in))
    assert ctx.last_encode_stats()["near_threshold_decisions"] == 0
    parts = A.parse_container(d_out[:nb].cpu().numpy())
    H = parts["header"]
    nblocks = (n + 16383) // 16384
    assert H.n == n and H.nblocks == nblocks and H.payload_offset + H.payload_bytes == nb
    assert np.all(np.diff(parts["block_off"].astype(np.int64)) > 0)
    rng = np.random.default_rng(1)
    picks = sorted(set([0, nblocks - 1, nblocks - 2] + [int(x) for x in rng.integers(0, nblocks, 21)]))
    for b in picks:
        lo, hi = b * 16384, min(n, (b + 1) * 16384)
        blk = d_in[lo:hi].cpu().numpy().view(np.uint32)
        exp, info, st, off = ol.oracle_encode(kind, f, blk, ckpt_interval=1024)
        assert np.array_equal(parts["streams"][b], exp), (spec, b)
        k = st.shape[0]
        assert np.array_equal(parts["ckpt_off"][b][:k], off) and np.array_equal(parts["ckpt_state"][b][:k], st), (spec, b)


@pytest.mark.parametrize("kind,f,spec,mi", [(ol.FOLD, 1, "zipf20s1.2", 256), (ol.FOLD, 3, "zipf24s1.2", 256), (ol.RFOLD, 3, "zipf24s1.2", 48),
                                            (ol.FOLD, 1, "uniform1-256", 96), (ol.FOLD, 5, "zipf20s1.2", 64)])
def test_full_size_every_block_equals_oracle(A, ctx, kind, f, spec, mi):
    """Round 4: full-size parity that is not a sample.  BASELINE config 2 at its 256 Mi ints, config 3a at 256 Mi,
    3b at 48 Mi (the oracle's ANSrfold pass is the slow side), config 1's shape, the harness's fidelity 5: EVERY block's stream
    (size and 64-bit hash), EVERY restart point (digest) and the header's frame / alphabet bounds are compared with the oracle,
    which encodes all blocks on the host's cores (ans_oracle_blocks_digest); then the device round trip."""
    import torch

    n = mi * (1 << 20) + (12345 if mi < 256 else 0)
    block, ck = 16384, 1024
    d_in = torch.empty(n, dtype=torch.int32, device="cuda")
    A.generate_dev(ctx, spec, d_in.data_ptr(), n, seed=4242)
    codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ck)
    d_out = torch.empty(min(codec.bound(n), 8 * n + (64 << 20)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for call in range(2):  # the geometry's first call (discovery) and a hinted one must write the same container
        nb = codec.encode_dev(d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel())
        cont = d_out[:nb].cpu().numpy()
        if call == 0:
            first = cont.copy()
        else:
            assert np.array_equal(cont, first)
    del first
    host = d_in.cpu().numpy().view(np.uint32)
    sizes, shash, cdig, lg, ns = ol.oracle_blocks_digest(kind, f, host, block, ck)
    del host
    parts = A.parse_container(cont)
    H = parts["header"]
    nblocks = (n + block - 1) // block
    assert H.n == n and H.nblocks == nblocks and H.payload_offset + H.payload_bytes == nb
    assert H.max_log2_frame == lg and H.max_nsyms == ns
    boff = parts["block_off"].astype(np.uint64)
    assert np.array_equal(np.diff(boff).astype(np.uint32), sizes)
    got_hash = ol.hash_spans(cont, boff + np.uint64(H.payload_offset))
    bad = np.nonzero(got_hash != shash)[0]
    assert bad.size == 0, (spec, "first differing blocks", bad[:8])
    got_dig = ol.ckpt_digest(parts["ckpt_state"], parts["ckpt_off"])
    bad = np.nonzero(got_dig != cdig)[0]
    assert bad.size == 0, (spec, "restart points differ in blocks", bad[:8])
    del parts, cont
    d_back = torch.zeros(n, dtype=torch.int32, device="cuda")
    codec.decode_dev(d_out.data_ptr(), nb, d_back.data_ptr(), n)
    assert bool(torch.equal(d_back, d_in))
    assert ctx.last_encode_stats()["near_threshold_decisions"] == 0


@pytest.mark.parametrize("mi", [180, 250])
def test_encoder_multi_wave_workgroups_with_ragged_end(A, ctx, mi):
    """The encoder packs 3 resp. 4 waves into a workgroup at these sizes and keeps them in step with a barrier --
    except in the last workgroup, which is only partly filled and ends in a partial block."""
    import torch

    n = mi * (1 << 20) + 4097
    d_in = torch.empty(n, dtype=torch.int32, device="cuda")
    A.generate_dev(ctx, "zipf20s1.2", d_in.data_ptr(), n, seed=77 + mi)
    codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=16384, ckpt_interval=1024)
    d_out = torch.empty(codec.bound(n), dtype=torch.uint8, device="cuda")
    d_back = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nb = codec.encode_dev(d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel())
    codec.decode_dev(d_out.data_ptr(), nb, d_back.data_ptr(), n)
    assert bool(torch.equal(d_back, d_in))
    parts = A.parse_container(d_out[:nb].cpu().numpy())
    nblocks = (n + 16383) // 16384
    assert parts["header"].nblocks == nblocks
    rng = np.random.default_rng(mi)
    for b in sorted(set([0, 63, 64, nblocks - 66, nblocks - 17, nblocks - 2, nblocks - 1] + [int(x) for x in rng.integers(0, nblocks, 9)])):
        lo, hi = b * 16384, min(n, (b + 1) * 16384)
        exp, info, st, off = ol.oracle_encode(ol.FOLD, 1, d_in[lo:hi].cpu().numpy().view(np.uint32), ckpt_interval=1024)
        assert np.array_equal(parts["streams"][b], exp), b
        assert np.array_equal(parts["ckpt_state"][b][:st.shape[0]], st), b


PA_FAMS = ["zipf20s1.2", "uniform256", "geom0.01", "uniform20", "constant", "boundaries_small", "runs"]


def _pa_input(fam, n, seed):
    if fam == "boundaries_small":
        return (ol.gen_inputs("boundaries", n, seed) % np.uint32(1 << 18)).astype(np.uint32)
    if fam == "runs":  # long constant stretches: whole blocks with a single distinct value, low-entropy blocks
        rng = np.random.default_rng(seed)
        out = np.repeat(rng.integers(0, 1000, n // 3000 + 2), 3000)[:n].astype(np.uint32)
        out[rng.integers(0, n, n // 500)] = 7
        return out
    d = ol.gen_inputs(fam, n, seed)
    return (d % np.uint32(1 << 17)).astype(np.uint32) if fam == "uniform20" else d  # running sums must fit 32 bits


@pytest.mark.parametrize("kind,f", [(ol.MSB, 0), (ol.FOLD, 1), (ol.FOLD, 3), (ol.INT, 0)])
@pytest.mark.parametrize("fam", PA_FAMS)
def test_compacted_blocks_match_oracle(A, ctx, kind, f, fam):
    """Per-block alphabet compaction (src/pseudo_adaptive.cpp:85-130): every block stream = alphabet header
    + codec stream of the rank-remapped block, byte-identical to the oracle (itself pinned against the
    reference's bytes in test_oracle.py); restart points; round trip."""
    block, ckpt = (8192, 1024)
    n = 5 * block + 777
    data = _pa_input(fam, n, seed=41)
    codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ckpt, compact=True)
    cont = codec.encode(data)
    parts = A.parse_container(cont)
    H = parts["header"]
    assert H.kind == (kind | 0x100 | (0x200 if kind == ol.INT else 0)) and H.nblocks == 6 and H.n == n  # (ANSint: wide restart points)
    for b in range(H.nblocks):
        blk = data[b * block:(b + 1) * block]
        exp, pinfo, info, st, off = ol.oracle_pa_encode(kind, f, blk, ckpt_interval=ckpt)
        got = parts["streams"][b]
        assert got.size == exp.size and np.array_equal(got, exp), (fam, b, pinfo.sigma)
        k = st.shape[0]
        assert np.array_equal(parts["ckpt_off"][b][:k], off) and np.array_equal(parts["ckpt_state"][b][:k], st), (fam, b)
    assert np.array_equal(codec.decode(cont, n), data), fam
    # other geometries: round trip
    for bl, ck in ((16384 if kind != ol.INT else 16380, 1024), (1024, 256), (64, 0)):
        c2 = codec_for(A, ctx, kind, f, block_ints=bl, ckpt_interval=ck if ck else A.NO_CHECKPOINTS, compact=True)
        m = min(n, 20 * bl + 13)
        cont2 = c2.encode(data[:m])
        assert np.array_equal(c2.decode(cont2, m), data[:m]), (fam, bl)


def test_compaction_argument_and_domain_errors(A, ctx):
    d = ol.gen_inputs("uniform24", 20000, 1)  # 16 Ki distinct values around 2^23: their sum exceeds 32 bits
    with pytest.raises(A.AnsxError) as ei:
        A.ANSmsb(ctx=ctx, compact=True).encode(d)
    assert ei.value.status == 6
    with pytest.raises(A.AnsxError):
        A.ANSrfold(1, ctx=ctx, compact=True).encode(d[:100])          # rfold brings its own remap
    with pytest.raises(A.AnsxError):
        A.ANSint(ctx=ctx, block_ints=16384).encode(d[:100])          # ranks are 1-based: 16380 at most
    with pytest.raises(A.AnsxError):
        A.ANSmsb(ctx=ctx, compact=True, block_ints=32768).encode(d[:100])
    small = (d % np.uint32(4096)).astype(np.uint32)
    codec = A.ANSint(ctx=ctx)
    assert codec.name() == "ANS"                                     # methods.hpp:485
    cont = codec.encode(small)
    assert np.array_equal(codec.decode(cont, small.size), small)
    bad = cont.copy()
    bad[A.parse_container(cont)["header"].payload_offset] ^= 0x5A    # alphabet size of block 0
    with pytest.raises(A.AnsxError):
        codec.decode(bad, small.size)


def _ansint_golden_input(e):
    if e["input"] == "family":
        return np.minimum(ol.gen_inputs(e["family"], e["n"], e["seed"]), np.uint32(e["clip"]))
    d = np.zeros(e["n"], dtype=np.uint32)
    for pos, val in e["pairs"]:
        d[pos] = val
    return d


def test_plain_ansint_is_a_drop_in(A, ctx):
    """ANSint without the compaction layer (methods.hpp:484-497): in single-stream mode the GPU writes exactly the bytes
    of ans_int_compress -- tests/golden/ansint.json, made by the real reference, frames 2^5 .. 2^20 (32-bit frequencies,
    the 64-bit-division encoder step and the wide decoder arithmetic above 2^16) -- decodes reference-made streams, and
    its block container holds the oracle's stream of every block."""
    with open(os.path.join(GOLD, "ansint.json")) as fh:
        gold = json.load(fh)
    wide = 0
    for e in gold:
        d = _ansint_golden_input(e)
        tag = (e.get("family", "sparse"), e["n"], e["log2_frame"])
        codec = A.ANSint(ctx=ctx, block_ints=A.SINGLE_STREAM, compact=False)
        stream = codec.encode(d)
        assert stream.size == e["stream_len"], tag
        if "stream_hex" in e:
            assert stream.tobytes().hex() == e["stream_hex"], tag
            assert np.array_equal(codec.decode(np.frombuffer(bytes.fromhex(e["stream_hex"]), dtype=np.uint8), d.size), d), tag
        else:
            assert hashlib.sha256(stream.tobytes()).hexdigest() == e["stream_sha256"], tag
        assert np.array_equal(codec.decode(stream, d.size), d), tag
        wide += e["log2_frame"] > 16
    assert wide >= 2
    # block container: every block stream is the oracle's (and the reference's) ANSint stream of that block
    for fam, n in (("zipf20s1.2", 70001), ("uniform12", 40000), ("geom0.01", 33000)):
        d = np.minimum(ol.gen_inputs(fam, n, seed=7), np.uint32(16383))
        codec = A.ANSint(ctx=ctx, block_ints=16384, ckpt_interval=1024, compact=False)
        cont = codec.encode(d)
        check_container(A, cont, d, ol.INT, 0, 16384, 1024)
        assert np.array_equal(codec.decode(cont, n), d)


def test_plain_ansint_beyond_the_dense_model(A):
    """ANSint sizes its model by the list's largest value (ans_int.hpp:41-51).  Values from 16384 on are modelled in rank
    space per block (csrc/ansx_intsparse.h) and only the prelude ranges over the values: single-stream bytes equal the
    reference's (tests/golden/ansint_large.json, made by oracle/_ref: max values 2^17, 2^20, 2^22), reference-made streams
    decode, every block of a container is the oracle's stream, and the bytes do not depend on what the context encoded
    before.  The rank-space model has 16384 symbols: a block (in single-stream mode: the list) of any length with at most
    that many DISTINCT values is in reach; beyond, the call is refused, not mis-coded."""
    with open(os.path.join(GOLD, "ansint_large.json")) as fh:
        gold = json.load(fh)
    ctx = A.Context(0)
    for e in gold:
        d = ol.ansint_large_list(e["n"], 1 << e["log2_vmax"], e["seed"], e["shape"])
        tag = (e["shape"], e["n"], e["log2_vmax"])
        assert hashlib.sha256(d.tobytes()).hexdigest() == e["input_sha256"], tag
        codec = A.ANSint(ctx=ctx, block_ints=A.SINGLE_STREAM, compact=False)
        stream = codec.encode(d)
        assert ctx.last_encode_stats()["path"] & 256, tag  # the rank-space model ran
        assert stream.size == e["stream_len"], tag
        assert hashlib.sha256(stream.tobytes()).hexdigest() == e["stream_sha256"], tag
        if "stream_hex" in e:
            assert stream.tobytes().hex() == e["stream_hex"], tag
            assert np.array_equal(codec.decode(np.frombuffer(bytes.fromhex(e["stream_hex"]), dtype=np.uint8), d.size), d), tag
        assert np.array_equal(codec.decode(stream, d.size), d), tag
    ctx.close()
    # block containers: blocks of 16384 / 4096 / 512 ints, ragged ends, restart points
    for shape, n, lg, block, ck in (("skew", 70001, 20, 16384, 1024), ("uniform", 40000, 22, 4096, 256), ("cluster", 33333, 17, 16384, 1024),
                                    ("uniform", 3000, 24, 512, 0), ("skew", 16384 * 3, 22, 16384, 4096)):
        d = ol.ansint_large_list(n, 1 << lg, 9 + lg, shape)
        c1 = A.Context(0)
        codec = A.ANSint(ctx=c1, block_ints=block, ckpt_interval=ck if ck else A.NO_CHECKPOINTS, compact=False)
        cont = codec.encode(d)
        assert c1.last_encode_stats()["path"] & 256
        check_container(A, cont, d, ol.INT, 0, block, ck)
        assert np.array_equal(codec.decode(cont, n), d)
        assert np.array_equal(codec.encode(d), cont)  # (second call: rank space from the start)
        # the same context, a list the dense model holds: the bytes a fresh context writes (parse hints included)
        small = d % np.uint32(16384)
        got = codec.encode(small)
        assert not (c1.last_encode_stats()["path"] & 256)
        c2 = A.Context(0)
        fresh = A.ANSint(ctx=c2, block_ints=block, ckpt_interval=ck if ck else A.NO_CHECKPOINTS, compact=False).encode(small)
        assert np.array_equal(got, fresh)
        assert np.array_equal(codec.decode(got, n), small)
        # ... and back
        assert np.array_equal(codec.encode(d), cont)
        c1.close()
        c2.close()
    # the prelude writer sizes its bit buffer from the call's distinct-value maximum (two words per value) and the call is
    # repeated with the full size when a block's code is longer: forced here, same bytes
    d = ol.ansint_large_list(30000, 1 << 22, 41, "skew")
    c3 = A.Context(0)
    ref = A.ANSint(ctx=c3, block_ints=8192, ckpt_interval=1024, compact=False).encode(d)
    assert not (c3.last_encode_stats()["path"] & 512)
    c3.close()
    c3 = A.Context(0)
    c3.debug_set("ANSX_TEST_SP_BITS", "40")
    got = A.ANSint(ctx=c3, block_ints=8192, ckpt_interval=1024, compact=False).encode(d)
    assert c3.last_encode_stats()["path"] & 512 and np.array_equal(got, ref)
    c3.close()
    # a block in which every int is a different large value (16384 ranks: the model's last symbol is used)
    ctx = A.Context(0)
    d = (np.arange(16384, dtype=np.uint32) * np.uint32(977) + np.uint32(50000))
    codec = A.ANSint(ctx=ctx, block_ints=16384, ckpt_interval=1024, compact=False)
    cont = codec.encode(d)
    check_container(A, cont, d, ol.INT, 0, 16384, 1024)
    assert np.array_equal(codec.decode(cont, d.size), d)
    # a small case, as before: 16384 itself
    d = np.array([1, 2, 16384, 3] * 100, dtype=np.uint32)
    codec = A.ANSint(ctx=ctx, compact=False)
    cont = codec.encode(d)
    check_container(A, cont, d, ol.INT, 0, 16384, 1024)
    assert np.array_equal(codec.decode(cont, d.size), d)
    # long blocks with few distinct large values: a 65536-int block geometry and a whole list as one stream
    d = ol.ansint_large_list(200000, 1 << 21, 77, "cluster")
    codec = A.ANSint(ctx=ctx, block_ints=65536, ckpt_interval=1024, compact=False)
    cont = codec.encode(d)
    assert ctx.last_encode_stats()["path"] & 256
    check_container(A, cont, d, ol.INT, 0, 65536, 1024)
    assert np.array_equal(codec.decode(cont, d.size), d)
    # shards of one list, one with small values only (dense model), one with large ones (rank space): the merged container is the
    # whole list's (no parse hints for plain ANSint, max_nsyms bounds the distinct values: nothing tells the two models apart)
    torch = pytest.importorskip("torch")
    block = 4096
    small_part = (ol.gen_inputs("zipf20s1.2", 5 * block, seed=3) % np.uint32(9000)).astype(np.uint32)
    large_part = ol.ansint_large_list(3 * block + 123, 1 << 21, 5, "skew")
    whole_data = np.concatenate([small_part, large_part])
    bufs, ptrs, sizes = [], [], []
    for part in (small_part, large_part):
        cs = A.Context(0)
        cpart = A.ANSint(ctx=cs, block_ints=block, ckpt_interval=512, compact=False).encode(part)
        cs.close()
        t = torch.zeros(cpart.size + 64, dtype=torch.uint8, device="cuda")
        t[:cpart.size] = torch.from_numpy(cpart.copy()).cuda()
        bufs.append(t), ptrs.append(t.data_ptr()), sizes.append(cpart.size)
    wcodec = A.ANSint(ctx=ctx, block_ints=block, ckpt_interval=512, compact=False)
    whole = wcodec.encode(whole_data)
    outb = torch.zeros(whole.size + 4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nbm = ctx.merge_containers_dev(ptrs, sizes, outb.data_ptr(), outb.numel())
    torch.cuda.synchronize()
    assert nbm == whole.size and np.array_equal(outb[:nbm].cpu().numpy(), whole)
    assert np.array_equal(wcodec.decode(whole, whole_data.size), whole_data)
    # out of reach (more than 16384 distinct values in a block): refused, not mis-coded
    big = ol.ansint_large_list(40000, 1 << 20, 3, "uniform")
    for kw in (dict(block_ints=A.SINGLE_STREAM), dict(block_ints=32768, ckpt_interval=1024)):
        with pytest.raises(A.AnsxError) as ei:
            A.ANSint(ctx=ctx, compact=False, **kw).encode(big)
        assert ei.value.status == 6  # ANSX_ERR_DOMAIN
    with pytest.raises(A.AnsxError) as ei:
        A.ANSint(ctx=ctx, compact=False).encode(np.array([5, 1 << 30, 7], dtype=np.uint32))
    assert ei.value.status == 6
    ctx.close()


def test_golden_compaction_fixtures(A, ctx):
    """tests/golden/pa.json: bytes made by the real reference (pseudo_adaptive blocks); the GPU container of a
    one-block list holds exactly that stream."""
    with open(os.path.join(GOLD, "pa.json")) as fh:
        gold = [e for e in json.load(fh) if e["mode"] == "pa"]
    kinds = {"fold": ol.FOLD, "msb": ol.MSB, "int": ol.INT}
    for e in gold:
        d = ol.gen_inputs(e["family"], e["n"], e["seed"])
        block = 16380 if e["kind"] == "int" else 16384
        codec = codec_for(A, ctx, kinds[e["kind"]], e["f"], block_ints=block, ckpt_interval=A.NO_CHECKPOINTS, compact=True)
        cont = codec.encode(d)
        stream = A.parse_container(cont)["streams"][0]
        tag = (e["kind"], e["f"], e["family"], e["n"])
        assert stream.size == e["stream_len"], tag
        assert hashlib.sha256(stream.tobytes()).hexdigest() == e["stream_sha256"], tag
        assert np.array_equal(codec.decode(cont, e["n"]), d), tag
