"""CPU tests of the calls over a batch of gap-coded lists (ansx_encode_batch_gaps_bases_dev,
ansx_decode_batch_ranges_sums_dev, ansx_next_geq_batch_dev): they are exported and bound, and the argument checks that
come before anything touches the context answer without a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_batch_ranges_cpu import INS, OUT, UNSET, _StandIn

BASES = (20480, 24576, 28672)  # fake device addresses of the three containers' bases, 4-byte aligned
TGT, POS, IDS = 32768, 36864, 40960


@pytest.fixture(scope="module")
def A():
    import os

    import ans_large_alphabet_amd as A_

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "ans_large_alphabet_amd", "libansx.so")):
        A_.build_library()
    return A_


def ptr_array(values):
    return (C.c_void_p * max(len(values), 1))(*[C.c_void_p(p) if p else None for p in values])


def sums_call(A, ctx, ins=INS, bases=BASES, nbases=(2, 2, 2), count=None, src=(0, 1, 2), first=None, cnt=None, nranges=None,
              out=OUT, cap=16, offsets=None, total=None, null=()):
    """ansx_decode_batch_ranges_sums_dev -> (status, bad_container, bad_range); null: names of arrays passed as NULL"""
    count = len(ins) if count is None else count
    nranges = len(src) if nranges is None else nranges
    first = [0] * len(src) if first is None else first
    cnt = [1] * len(src) if cnt is None else cnt
    arr = {"d_ins": ptr_array(ins), "in_bytes": (C.c_size_t * max(len(ins), 1))(*([4096] * len(ins))),
           "d_bases": ptr_array(bases), "nbases": (C.c_size_t * max(len(nbases), 1))(*nbases),
           "src": (C.c_uint32 * max(len(src), 1))(*src), "first": (C.c_uint64 * max(len(first), 1))(*first),
           "cnt": (C.c_uint32 * max(len(cnt), 1))(*cnt)}
    for k in null:
        arr[k] = None
    bad_c, bad_r = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_decode_batch_ranges_sums_dev(
        ctx, A.FOLD, 1, arr["d_ins"], arr["in_bytes"], arr["d_bases"], arr["nbases"], count, arr["src"], arr["first"],
        arr["cnt"], nranges, None if out is None else C.c_void_p(out), cap, offsets, total, C.byref(bad_c), C.byref(bad_r), None)
    return st, bad_c.value, bad_r.value


def geq_call(A, ctx, ins=INS, bases=BASES, nbases=(2, 2, 2), count=None, src=(0, 1, 2), ntargets=None, targets=TGT, pos=POS,
             ids=IDS, found=None, null=()):
    """ansx_next_geq_batch_dev -> (status, bad_container, bad_target)"""
    count = len(ins) if count is None else count
    ntargets = len(src) if ntargets is None else ntargets
    arr = {"d_ins": ptr_array(ins), "in_bytes": (C.c_size_t * max(len(ins), 1))(*([4096] * len(ins))),
           "d_bases": ptr_array(bases), "nbases": (C.c_size_t * max(len(nbases), 1))(*nbases),
           "src": (C.c_uint32 * max(len(src), 1))(*src)}
    for k in null:
        arr[k] = None
    p = lambda v: None if v is None else C.c_void_p(v)
    bad_c, bad_t = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_next_geq_batch_dev(ctx, A.FOLD, 1, arr["d_ins"], arr["in_bytes"], arr["d_bases"], arr["nbases"], count,
                                         arr["src"], p(targets), ntargets, p(pos), p(ids), found, C.byref(bad_c),
                                         C.byref(bad_t), None)
    return st, bad_c.value, bad_t.value


def writer_call(A, ctx, offsets=(0, 5, 9), d_in=4096, out=8192, bases=BASES[0], cap=16, base_offsets=None, total=None,
                block_ints=0):
    """ansx_encode_batch_gaps_bases_dev -> status"""
    offs = (C.c_uint64 * len(offsets))(*offsets)
    opts = A._lib.Opts(block_ints, 0, 0, 0)
    return A.lib().ansx_encode_batch_gaps_bases_dev(ctx, A.FOLD, 1, C.c_void_p(d_in), offs, len(offsets) - 1, C.c_void_p(out),
                                                    1 << 20, None, None, None, None, C.byref(opts),
                                                    None if bases is None else C.c_void_p(bases), cap, base_offsets, total, None)


def test_symbols_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    for name, nargs in (("ansx_encode_batch_gaps_bases_dev", 18), ("ansx_decode_batch_ranges_sums_dev", 19),
                        ("ansx_next_geq_batch_dev", 17)):
        assert name in _lib.EXPORTS
        fn = getattr(A.lib(), name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        for m in ("encode_batch_gaps_bases_dev", "decode_batch_ranges_sums_dev", "next_geq_batch_dev"):
            assert callable(getattr(codec, m))


# ---------------------------------------------------------------------------------------------------- ids of ranges
def test_sums_null_context_and_null_arrays(A):
    ctx = _StandIn()
    assert sums_call(A, None)[0] == A._lib.ERR_ARG
    for k in ("d_ins", "in_bytes", "d_bases", "nbases", "src", "first", "cnt"):
        assert sums_call(A, ctx.handle, null=(k,))[0] == A._lib.ERR_ARG, k
    assert sums_call(A, ctx.handle, count=1 << 32)[0] == A._lib.ERR_ARG
    assert sums_call(A, ctx.handle, nranges=1 << 32)[0] == A._lib.ERR_ARG
    assert sums_call(A, ctx.handle, out=OUT + 2)[0] == A._lib.ERR_ARG
    assert sums_call(A, ctx.handle, out=None, cap=1)[0] == A._lib.ERR_ARG


@pytest.mark.parametrize("delta", [None, 1, 2, 3])
def test_sums_bad_bases_of_a_referenced_container(A, delta):
    """delta None: a null pointer.  bad_range: the first range that names the container, count 0 included."""
    ctx = _StandIn()
    bases = list(BASES)
    bases[1] = 0 if delta is None else bases[1] + delta
    st, bad_c, bad_r = sums_call(A, ctx.handle, bases=bases, src=(2, 0, 1, 1), cnt=(1, 1, 0, 5))
    assert st == A._lib.ERR_ARG and bad_r == 2 and bad_c == UNSET
    ins = list(INS)
    ins[1] += 8
    st, bad_c, bad_r = sums_call(A, ctx.handle, ins=ins, src=(2, 0, 1, 1))
    assert st == A._lib.ERR_ARG and bad_r == 2 and bad_c == UNSET


def test_sums_a_container_past_the_batch_wins_over_a_bad_pointer(A):
    ctx = _StandIn()
    bases = list(BASES)
    bases[0] += 2
    st, _, bad_r = sums_call(A, ctx.handle, bases=bases, src=(0, 5))
    assert st == A._lib.ERR_ARG and bad_r == 1


def test_sums_an_unreferenced_container_is_not_examined(A):
    """Container 1 -- null input, null bases -- is named by no range: the argument checks pass and the call goes on to
    the context, where the stand-in stops it."""
    ctx = _StandIn()
    ins, bases = list(INS), list(BASES)
    ins[1], bases[1] = 0, 0
    st, bad_c, bad_r = sums_call(A, ctx.handle, ins=ins, bases=bases, src=(2, 0, 2))
    assert st == A._lib.ERR_HIP and bad_c == UNSET and bad_r == UNSET
    st, _, bad_r = sums_call(A, ctx.handle, ins=ins, bases=bases, src=(2, 0, 2, 1))
    assert st == A._lib.ERR_ARG and bad_r == 3


def test_sums_no_ranges_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    total = C.c_uint64(12345)
    offsets = (C.c_uint64 * 1)(777)
    st = sums_call(A, ctx.handle, src=(), null=("src", "first", "cnt", "d_bases", "nbases"), offsets=offsets,
                   total=C.byref(total))[0]
    assert st == A._lib.OK and total.value == 0 and offsets[0] == 0
    codec = A.ANSfold(1, ctx=ctx)
    assert codec.decode_batch_ranges_sums_dev([], [], [], [], [], [], [], None, 0).tolist() == [0]
    assert codec.decode_batch_ranges_sums_dev(INS, [4096] * 3, BASES, [2] * 3, [], [], [], OUT, 16).tolist() == [0]


# ---------------------------------------------------------------------------------------------------- search by value
def test_geq_null_and_misaligned_arguments(A):
    ctx = _StandIn()
    E = A._lib
    assert geq_call(A, None)[0] == E.ERR_ARG
    for k in ("d_ins", "in_bytes", "d_bases", "nbases", "src"):
        assert geq_call(A, ctx.handle, null=(k,))[0] == E.ERR_ARG, k
    assert geq_call(A, ctx.handle, targets=None)[0] == E.ERR_ARG
    assert geq_call(A, ctx.handle, pos=None, ids=None)[0] == E.ERR_ARG
    for kw in ({"targets": TGT + 2}, {"pos": POS + 4}, {"ids": IDS + 1}):
        assert geq_call(A, ctx.handle, **kw)[0] == E.ERR_ARG, kw
    assert geq_call(A, ctx.handle, count=1 << 32)[0] == E.ERR_ARG
    assert geq_call(A, ctx.handle, ntargets=1 << 32)[0] == E.ERR_ARG
    # either output alone passes the checks: the stand-in stops the call at the context
    assert geq_call(A, ctx.handle, pos=None)[0] == E.ERR_HIP
    assert geq_call(A, ctx.handle, ids=None)[0] == E.ERR_HIP


@pytest.mark.parametrize("src,want", [((0, 3, 1), 1), ((2, 1, 0, 7, 9), 3), ((0xFFFFFFFF,), 0)])
def test_geq_a_target_of_a_list_past_the_batch(A, src, want):
    ctx = _StandIn()
    st, bad_c, bad_t = geq_call(A, ctx.handle, src=src)
    assert st == A._lib.ERR_ARG and bad_t == want and bad_c == UNSET


@pytest.mark.parametrize("which,delta", [("ins", None), ("ins", 8), ("bases", None), ("bases", 2)])
def test_geq_bad_pointer_of_a_referenced_list(A, which, delta):
    ctx = _StandIn()
    ins, bases = list(INS), list(BASES)
    v = ins if which == "ins" else bases
    v[1] = 0 if delta is None else v[1] + delta
    st, bad_c, bad_t = geq_call(A, ctx.handle, ins=ins, bases=bases, src=(2, 0, 1, 1))
    assert st == A._lib.ERR_ARG and bad_t == 2 and bad_c == UNSET
    # ... a list past the batch wins over it
    st, _, bad_t = geq_call(A, ctx.handle, ins=ins, bases=bases, src=(1, 5))
    assert st == A._lib.ERR_ARG and bad_t == 1
    # ... and unreferenced it is not examined
    st, bad_c, bad_t = geq_call(A, ctx.handle, ins=ins, bases=bases, src=(2, 0, 2))
    assert st == A._lib.ERR_HIP and bad_c == UNSET and bad_t == UNSET


def test_geq_no_targets_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    found = C.c_uint64(99)
    st = geq_call(A, ctx.handle, src=(), null=("src",), targets=None, pos=None, ids=None, found=C.byref(found))[0]
    assert st == A._lib.OK and found.value == 0
    assert A.ANSfold(1, ctx=ctx).next_geq_batch_dev(INS, [4096] * 3, BASES, [2] * 3, [], TGT, POS, IDS) == 0


# ---------------------------------------------------------------------------------------------------- the writer
def test_writer_argument_errors_and_size_query(A):
    ctx = _StandIn()
    E = A._lib
    assert writer_call(A, None) == E.ERR_ARG
    assert writer_call(A, ctx.handle, bases=BASES[0] + 2) == E.ERR_ARG
    assert writer_call(A, ctx.handle, bases=None, cap=1) == E.ERR_ARG
    assert writer_call(A, ctx.handle, out=8200) == E.ERR_ARG  # (the checks of ansx_encode_batch_gaps_dev)
    assert writer_call(A, ctx.handle, offsets=(0, 5, 5)) == E.ERR_ARG
    # the size query and a short capacity: decided on the host, base_offsets and the total written
    for bases, cap in ((None, 0), (BASES[0], 6)):
        boffs = (C.c_uint64 * 4)(7, 7, 7, 7)
        total = C.c_size_t(0)
        st = writer_call(A, ctx.handle, offsets=(0, 5, 9, 18), block_ints=4, bases=bases, cap=cap, base_offsets=boffs,
                         total=C.byref(total))
        assert st == E.ERR_CAPACITY
        assert list(boffs) == [0, 3, 5, 9] and total.value == 9  # blocks 2, 1, 3 -> 3, 2, 4 bases
    # enough capacity: on to the context
    assert writer_call(A, ctx.handle, offsets=(0, 5, 9, 18), block_ints=4, cap=9) == E.ERR_HIP
    codec = A.ANSfold(1, ctx=ctx, block_ints=4, ckpt_interval=A.NO_CHECKPOINTS)
    assert codec.encode_batch_gaps_bases_dev(4096, [0, 5, 9, 18], 8192, 1 << 20, None, 0).tolist() == [0, 3, 5, 9]
    with pytest.raises(A.AnsxError) as e:
        codec.encode_batch_gaps_bases_dev(4096, [0, 5, 9, 18], 8192, 1 << 20, BASES[0], 8)
    assert e.value.status == E.ERR_CAPACITY and e.value.needed == 9 and e.value.base_offsets.tolist() == [0, 3, 5, 9]


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    E = A._lib
    with pytest.raises(ValueError):
        codec.decode_batch_ranges_sums_dev(INS, [4096, 4096], BASES, [2] * 3, [0], [0], [1], OUT, 16)
    with pytest.raises(ValueError):
        codec.decode_batch_ranges_sums_dev(INS, [4096] * 3, BASES[:2], [2] * 3, [0], [0], [1], OUT, 16)
    with pytest.raises(ValueError):
        codec.decode_batch_ranges_sums_dev(INS, [4096] * 3, BASES, [2] * 2, [0], [0], [1], OUT, 16)
    for src, first, cnt in (([0, 1], [0], [1]), ([0], [0, 0], [1]), ([0], [0], [1, 1])):
        with pytest.raises(ValueError):
            codec.decode_batch_ranges_sums_dev(INS, [4096] * 3, BASES, [2] * 3, src, first, cnt, OUT, 16)
    with pytest.raises(ValueError):
        codec.next_geq_batch_dev(INS, [4096] * 2, BASES, [2] * 3, [0], TGT, POS, IDS)
    with pytest.raises(ValueError):
        codec.next_geq_batch_dev(INS, [4096] * 3, BASES, [2], [0], TGT, POS, IDS)
    with pytest.raises(ValueError):
        codec.next_geq_batch_dev(INS, [4096] * 3, BASES, [2] * 3, np.array([0.5]), TGT, POS, IDS)
    with pytest.raises(ValueError):
        codec.encode_batch_gaps_bases_dev(4096, [], 8192, 1 << 20, BASES[0], 8)
    # the C checks behind the wrappers, with what they set
    with pytest.raises(A.AnsxError) as e:
        codec.decode_batch_ranges_sums_dev(INS, [4096] * 3, BASES, [2] * 3, [0, 1, 3], [0, 0, 0], [1, 1, 1], OUT, 16)
    assert e.value.status == E.ERR_ARG and e.value.range == 2 and e.value.bad_range == 2 and e.value.container is None
    with pytest.raises(A.AnsxError) as e:
        codec.decode_batch_ranges_sums_dev(INS, [4096] * 3, [BASES[0], BASES[1] + 2, BASES[2]], [2] * 3, [0, 2, 1], [0] * 3,
                                           [1] * 3, OUT, 16)
    assert e.value.status == E.ERR_ARG and e.value.range == 2
    with pytest.raises(A.AnsxError) as e:
        codec.next_geq_batch_dev(INS, [4096] * 3, BASES, [2] * 3, [0, 4, 1], TGT, POS, IDS)
    assert e.value.status == E.ERR_ARG and e.value.target == 1 and e.value.container is None
    with pytest.raises(A.AnsxError) as e:
        codec.next_geq_batch_dev(INS, [4096] * 3, BASES, [2] * 3, [0, 1], TGT, None, None)
    assert e.value.status == E.ERR_ARG and e.value.target is None
