"""Block-range pipeline of the fast model path on the GPU (-m gpu), through the C ABI.

ANSX_MODEL_PIPELINE = always | a range count runs k_fold_hist -> k_sort_entropy -> k_candidates -> k_model_finish per
range of blocks: the histograms one after the other on the caller's stream, the model kernels of every range but the
last on two side streams of the context (alternating), the last range's behind its histogram; `never` is the serial form.  Every form must write the same container, byte for byte: `never` is the expected answer
throughout (pinned to the oracle by test_gpu_parity.py), and every decode must give the input back.

No call here reports WHETHER it was pipelined (there is no such field in ansx_encode_stats): the forced modes
pipeline every call that takes the fast model path outside profile mode, and the tests assert that path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BI = 16384
MODES = ["always", "2", "3", "7"]
CODECS = [("fold", 1), ("fold", 3), ("fold", 5), ("rfold", 3), ("msb", 0)]
DISTS = ["zipf20s1.2", "uniform12", "geom0.01"]
FAST = 5  # ansx_encode_stats.path of a hinted call on the fast model path (+ 128: the producer / consumer encoder)


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def torch():
    torch_ = pytest.importorskip("torch")
    torch_.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return torch_


@pytest.fixture()
def ctx(A, torch):
    c = A.Context(0)
    yield c
    c.close()


def make_codec(A, ctx, name, f, **kw):
    if name == "msb":
        return A.ANSmsb(ctx=ctx, **kw)
    return {"fold": A.ANSfold, "rfold": A.ANSrfold}[name](f, ctx=ctx, **kw)


def gen(A, torch, ctx, spec, n, seed=11):
    d = torch.empty(n, dtype=torch.int32, device="cuda")
    A.generate_dev(ctx, spec, d.data_ptr(), n, seed=seed)
    torch.cuda.synchronize()
    return d


def encode(torch, ctx, codec, d, fast=True):
    """-> the container's bytes as a device tensor; asserts the call took the fast model path."""
    n = d.numel()
    out = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = codec.encode_dev(d.data_ptr(), n, out.data_ptr(), out.numel())
    if fast:
        path = ctx.last_encode_stats()["path"]
        assert path & ~128 == FAST, "path %d: not the fast model path, the comparison would prove nothing" % path
    return out[:nb]


def decode(torch, codec, cont, n):
    back = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_dev(cont.data_ptr(), cont.numel(), back.data_ptr(), n)
    torch.cuda.synchronize()
    return back


def compare_modes(A, torch, ctx, codec, d, modes=MODES):
    n = d.numel()
    ctx.debug_set("ANSX_MODEL_PIPELINE", "never")
    encode(torch, ctx, codec, d, fast=False)  # the geometry's hints (alphabet, candidates per block)
    ref = encode(torch, ctx, codec, d)
    assert torch.equal(decode(torch, codec, ref, n), d)
    for mode in modes:
        ctx.debug_set("ANSX_MODEL_PIPELINE", mode)
        got = encode(torch, ctx, codec, d)
        assert got.numel() == ref.numel() and torch.equal(got, ref), (mode, n)
        assert torch.equal(decode(torch, codec, got, n), d), (mode, n)
    return ref


# (a) a multiple of every range size, (b) a block count that is no multiple of 64 or of a range count, (c) a partial
# last block, (d) fewer blocks than ranges (three blocks, one block)
LENGTHS = [768 * BI, 333 * BI, 200 * BI + 777, 2 * BI + 5, 1000]


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name,f", CODECS)
def test_pipelined_bytes_equal_serial(A, torch, ctx, name, f, dist):
    codec = make_codec(A, ctx, name, f)
    for n in LENGTHS:
        compare_modes(A, torch, ctx, codec, gen(A, torch, ctx, dist, n))


@pytest.mark.parametrize("name,f,dist", [("fold", 1, "zipf20s1.2"), ("rfold", 3, "geom0.01"), ("msb", 0, "uniform12"),
                                         ("fold", 3, "zipf20s1.2")])
def test_small_blocks_many_ranges(A, torch, ctx, name, f, dist):
    """block_ints = 1024: a few hundred thousand ints are hundreds of blocks and many ranges."""
    codec = make_codec(A, ctx, name, f, block_ints=1024, ckpt_interval=256)
    # (a last block of a handful of ints would choose a frame far above its neighbours' and send the whole geometry to the
    # exact model kernels: the partial blocks here are a few hundred ints)
    for n in (448 * 1024, 300 * 1024 + 300, 131 * 1024 + 517):
        compare_modes(A, torch, ctx, codec, gen(A, torch, ctx, dist, n), modes=MODES + ["16", "64"])


def test_key_values(A, torch, ctx):
    for ok in ("never", "always", "1", "2", "64", "0", "", None):
        ctx.debug_set("ANSX_MODEL_PIPELINE", ok)
    for bad in ("sometimes", "65", "-1", "3x", "0x4", " 2"):
        with pytest.raises(A.AnsxError) as e:
            ctx.debug_set("ANSX_MODEL_PIPELINE", bad)
        assert e.value.status == A._lib.ERR_ARG, bad


def test_capacity_error_joins(A, torch, ctx):
    """Too small an output: the capacity error comes back with the pipeline forced, and the next call on the same context
    and stream is right (the side streams were joined on the error path too)."""
    codec = make_codec(A, ctx, "fold", 1)
    n = 333 * BI + 99
    d = gen(A, torch, ctx, "zipf20s1.2", n)
    ref = compare_modes(A, torch, ctx, codec, d, modes=["3"])
    ctx.debug_set("ANSX_MODEL_PIPELINE", "3")
    small = torch.zeros(ref.numel() // 2 // 16 * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        with pytest.raises(A.AnsxError) as e:
            codec.encode_dev(d.data_ptr(), n, small.data_ptr(), small.numel())
        assert e.value.status == A._lib.ERR_CAPACITY
        assert ctx.last_encode_stats()["path"] & ~128 == FAST
        got = encode(torch, ctx, codec, d)
        assert torch.equal(got, ref)
        assert torch.equal(decode(torch, codec, got, n), d)


def test_first_call_and_outgrown_hint(A, torch):
    """A first call of a geometry (discovery path, then the hints exist) and a call whose blocks outgrow a forced small
    hint (the pipelined attempt raises the violation and the call repeats on the discovery path), pipeline forced: the
    serial context's bytes."""
    n = 150 * BI + 1234
    serial, piped = A.Context(0), A.Context(0)
    try:
        serial.debug_set("ANSX_MODEL_PIPELINE", "never")
        piped.debug_set("ANSX_MODEL_PIPELINE", "3")
        d = gen(A, torch, serial, "zipf20s1.2", n)
        cs, cp = make_codec(A, serial, "fold", 1), make_codec(A, piped, "fold", 1)
        for call in range(3):  # first call of the geometry, then two hinted ones
            a = encode(torch, serial, cs, d, fast=call > 0)
            b = encode(torch, piped, cp, d, fast=call > 0)
            assert torch.equal(a, b), call
        for c in (serial, piped):
            c.debug_set("ANSX_NS_HINT", "64")  # every block of this input has more symbols than that
            c.debug_set("ANSX_T_HINT", "8")
        for call in range(2):
            a = encode(torch, serial, cs, d, fast=False)
            b = encode(torch, piped, cp, d, fast=False)
            for c in (serial, piped):
                assert c.last_encode_stats()["path"] & ~128 == FAST | 16  # tried on the fast path, missed, repeated
            assert torch.equal(a, b), call
            assert torch.equal(decode(torch, cp, b, n), d)
        # a hint that only SOME blocks outgrow: the others of their ranges are modelled, then the call repeats
        w = gen(A, torch, serial, "zipf20s1.2", n, seed=5)
        w[: 70 * BI] &= 63
        torch.cuda.synchronize()
        for c in (serial, piped):
            c.debug_set("ANSX_NS_HINT", "128")
        a = encode(torch, serial, cs, w, fast=False)
        b = encode(torch, piped, cp, w, fast=False)
        assert piped.last_encode_stats()["path"] & 16
        assert torch.equal(a, b)
        assert torch.equal(decode(torch, cp, b, n), w)
    finally:
        serial.close()
        piped.close()


def test_profile_mode_stays_serial(A, torch, ctx):
    """Per-kernel profile mode: one record per launch of the serial form (event pairs around overlapped kernels would
    time nothing), same bytes."""
    codec = make_codec(A, ctx, "fold", 1)
    n = 333 * BI
    d = gen(A, torch, ctx, "zipf20s1.2", n)
    ref = compare_modes(A, torch, ctx, codec, d, modes=["7"])
    ctx.debug_set("ANSX_MODEL_PIPELINE", "7")
    ctx.profile(True)
    ctx.profile_reset()
    try:
        got = encode(torch, ctx, codec, d)
        recs = {k: (ms, cnt) for k, ms, cnt in ctx.profile_get()}
    finally:
        ctx.profile(False)
    assert torch.equal(got, ref)
    for k in ("k_fold_hist", "k_sort_entropy", "k_candidates", "k_model_finish"):
        assert k in recs and recs[k][1] == 1 and recs[k][0] > 0.0, (k, recs.get(k))
    assert torch.equal(encode(torch, ctx, codec, d), ref)  # and pipelined again afterwards


def test_two_encodes_back_to_back(A, torch, ctx):
    """Two encodes on one stream into different outputs, one synchronise at the end: a range of the second call must not
    start before the first call's encoder has read the shared workspace."""
    codec = make_codec(A, ctx, "fold", 1)
    n = 400 * BI + 3
    d1 = gen(A, torch, ctx, "zipf20s1.2", n, seed=1)
    d2 = gen(A, torch, ctx, "zipf20s1.2", n, seed=2)
    r1 = compare_modes(A, torch, ctx, codec, d1, modes=[])
    r2 = compare_modes(A, torch, ctx, codec, d2, modes=[])
    assert not torch.equal(r1[: min(r1.numel(), r2.numel())], r2[: min(r1.numel(), r2.numel())])
    side = torch.cuda.Stream()
    for mode in MODES:
        ctx.debug_set("ANSX_MODEL_PIPELINE", mode)
        o1 = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
        o2 = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for stream in (None, side.cuda_stream):
            n1 = codec.encode_dev(d1.data_ptr(), n, o1.data_ptr(), o1.numel(), stream=stream)
            n2 = codec.encode_dev(d2.data_ptr(), n, o2.data_ptr(), o2.numel(), stream=stream)
            assert ctx.last_encode_stats()["path"] & ~128 == FAST
            torch.cuda.synchronize()
            assert torch.equal(o1[:n1], r1) and torch.equal(o2[:n2], r2), (mode, stream)
            o1.zero_()
            o2.zero_()
            torch.cuda.synchronize()
