"""Host-side mirror of the reference's codec concept for this path.

The reference exposes ``ANSfold<f>`` / ``ANSrfold<f>`` as structs with static ``name()``,
``encode(in, n, out, cap)`` -> bytes written and ``decode(in, bytes, out, n)``
(/root/reference/include/methods.hpp:529-567).  The classes below keep those names and argument
meanings on top of the C-ABI (include/ansx.h); the C++17 mirror with the exact static
signatures is ans_large_alphabet_amd/include/ansx_methods.hpp.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def make_opts(block_ints=0, ckpt_interval=0, flags=0):
    return L.Opts(block_ints, ckpt_interval, flags, 0)


class Context:
    """One per (process, device): owns the HIP stream and the device workspace."""

    def __init__(self, device=-1):
        self._h = C.c_void_p()
        st = L.lib().ansx_init(device, C.byref(self._h))
        if st != L.OK:
            raise L.AnsxError(st, "ansx_init")

    def close(self):
        if self._h:
            L.lib().ansx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def workspace_bytes(self):
        return L.lib().ansx_workspace_bytes(self._h)

    def merge_containers_dev(self, part_ptrs, part_bytes, out_ptr, out_capacity, stream=None):
        """Native root-side concatenation of rank containers (device pointers, list order) -> bytes written."""
        k = len(part_ptrs)
        ptrs = (C.c_void_p * k)(*part_ptrs)
        sizes = (C.c_size_t * k)(*part_bytes)
        nb = C.c_size_t(0)
        st = L.lib().ansx_merge_containers_dev(self._h, ptrs, sizes, k, out_ptr, out_capacity, C.byref(nb), stream)
        if st != L.OK:
            raise L.AnsxError(st, "ansx_merge_containers_dev")
        return nb.value

    def last_encode_stats(self):
        """dict(max_nsyms, max_log2_frame, near_threshold_decisions, path, host_redecided) of the most recent encode."""
        st = L.EncodeStats()
        L.lib().ansx_last_encode_stats(self._h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in L.EncodeStats._fields_}

    def last_encode_form(self):
        """The forms of the most recent encode as they were launched (ansx_encode_form_report in include/ansx.h): a dict
        of the struct's fields as ints, the enumerations as names ("hist", "sort", "fin", "rf", "prelude", "enc",
        "criterion": _lib.FORM_*) and the bits of "attempt" as bools "optimistic", "fast_model", "fused", "rank_space",
        "sp_full_lds", "batch_pass"."""
        st = L.EncodeFormReport()
        rc = L.lib().ansx_last_encode_form(self._h, C.byref(st))
        if rc != L.OK:
            raise L.AnsxError(rc, "ansx_last_encode_form")
        d = {k: int(getattr(st, k)) for k, _ in L.EncodeFormReport._fields_}
        for k, names in (("hist", L.FORM_HIST), ("sort", L.FORM_SORT), ("fin", L.FORM_FIN), ("rf", L.FORM_RF),
                         ("prelude", L.FORM_PRELUDE), ("enc", L.FORM_ENC), ("criterion", L.FORM_PC)):
            d[k] = names[d[k]]
        for k, bit in L.FORM_ATTEMPT_BITS:
            d[k] = bool(d["attempt"] & bit)
        return d

    def last_decode_stats(self):
        """The form of the most recent decode as it ran (ansx_decode_stats in include/ansx.h): a dict of the struct's
        fields as ints, "parser" and "decoder" as names ("PAR", "SMALL_RING", ...; _lib.PARSERS / _lib.DECODERS) and the
        three flags as bools "index_validated", "on_remembered", "repeated"."""
        st = L.DecodeStats()
        rc = L.lib().ansx_last_decode_stats(self._h, C.byref(st))
        if rc != L.OK:
            raise L.AnsxError(rc, "ansx_last_decode_stats")
        d = {k: int(getattr(st, k)) for k, _ in L.DecodeStats._fields_}
        d["parser"] = L.PARSERS[d["parser"]]
        d["decoder"] = L.DECODERS[d["decoder"]]
        d["index_validated"] = bool(d["flags"] & L.DECODE_INDEX_VALIDATED)
        d["on_remembered"] = bool(d["flags"] & L.DECODE_ON_REMEMBERED)
        d["repeated"] = bool(d["flags"] & L.DECODE_REPEATED)
        return d

    def debug_set(self, name, value=None):
        """Select one of the equivalent internal code paths (tests / experiments); value None or "" = default."""
        st = L.lib().ansx_debug_set(self._h, name.encode(), None if value is None else str(value).encode())
        if st != L.OK:
            raise L.AnsxError(st, "ansx_debug_set(%s)" % name)

    # -- per-kernel timing (hipEvents inside the library)
    def profile(self, on=True):
        L.lib().ansx_profile_enable(self._h, int(on))

    def profile_reset(self):
        L.lib().ansx_profile_reset(self._h)

    def profile_get(self):
        arr = (L.KernelTime * 64)()
        cnt = C.c_int(0)
        L.lib().ansx_profile_get(self._h, arr, 64, C.byref(cnt))
        return [(arr[i].name.decode(), arr[i].total_ms, int(arr[i].launches)) for i in range(min(cnt.value, 64))]


class _Codec:
    KIND = L.FOLD
    PREFIX = "ANSfold"

    def __init__(self, fidelity, ctx=None, block_ints=0, ckpt_interval=0, compact=False):
        """compact=True: per-block alphabet compaction (src/pseudo_adaptive.cpp:85-130, ANSX_FLAG_COMPACT_ALPHABET)."""
        self.f = int(fidelity)
        self.ctx = ctx
        self.opts = make_opts(block_ints, ckpt_interval, L.FLAG_COMPACT_ALPHABET if compact else 0)

    def _ctx(self):
        if self.ctx is None:
            self.ctx = Context()
        return self.ctx

    def name(self):  # methods.hpp:530-533 / 550-553
        buf = C.create_string_buffer(32)
        L.lib().ansx_codec_name(self.KIND, self.f, buf, 32)
        return buf.value.decode()

    def bound(self, n):
        return L.lib().ansx_bound(self.KIND, self.f, n, C.byref(self.opts))

    # ---- host buffers (numpy), signature meaning as methods.hpp encode()/decode()
    def encode(self, data, out=None):
        data = np.ascontiguousarray(data, dtype=np.uint32)
        n = data.size
        if out is None:
            out = np.empty(max(self.bound(n), 64), dtype=np.uint8)
        nb = C.c_size_t(0)
        st = L.lib().ansx_encode(self._ctx().handle, self.KIND, self.f, data.ctypes.data, n,
                                 out.ctypes.data, out.size, C.byref(nb), C.byref(self.opts))
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".encode")
        return out[: nb.value]

    def decode(self, stream, n, out=None):
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        if out is None:
            out = np.empty(n, dtype=np.uint32)
        st = L.lib().ansx_decode(self._ctx().handle, self.KIND, self.f, stream.ctypes.data, stream.size,
                                 out.ctypes.data, n, C.byref(self.opts))
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".decode")
        return out

    # ---- device pointers (HBM resident); ptrs are integers (e.g. torch.Tensor.data_ptr())
    def encode_dev(self, in_ptr, n, out_ptr, out_capacity, stream=None):
        nb = C.c_size_t(0)
        st = L.lib().ansx_encode_dev(self._ctx().handle, self.KIND, self.f, in_ptr, n, out_ptr,
                                     out_capacity, C.byref(nb), C.byref(self.opts), stream)
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".encode_dev")
        return nb.value

    def decode_dev(self, in_ptr, in_bytes, out_ptr, n, stream=None):
        st = L.lib().ansx_decode_dev(self._ctx().handle, self.KIND, self.f, in_ptr, in_bytes, out_ptr, n,
                                     C.byref(self.opts), stream)
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".decode_dev")

    def decode_ranges_dev(self, in_ptr, in_bytes, first, count, out_ptr, out_capacity, stream=None):
        """Random access: ints [first[i], first[i] + count[i]) of the container at in_ptr, range after range, to
        out_ptr (out_capacity ints); decodes only the blocks the ranges touch.  first / count: anything numpy turns
        into uint64 / uint32 arrays of one length.  Returns sum(count)."""
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
        count = np.ascontiguousarray(count, dtype=np.uint32).reshape(-1)
        if first.size != count.size:
            raise ValueError("first and count differ in length (%d, %d)" % (first.size, count.size))
        st = L.lib().ansx_decode_ranges_dev(self._ctx().handle, self.KIND, self.f, in_ptr, in_bytes, first.ctypes.data,
                                            count.ctypes.data, first.size, out_ptr, out_capacity, stream)
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".decode_ranges_dev")
        return int(count.sum(dtype=np.uint64))

    def decode_device_ranges_dev(self, in_ptr, in_bytes, first_ptr, count_ptr, nranges, out_ptr, out_capacity,
                                 offsets_ptr=None, stream=None):
        """Random access with the ranges in device memory: first_ptr -> nranges uint64 firsts, count_ptr -> nranges
        uint32 counts, both device pointers read on `stream` (e.g. an int64 / int32 tensor's data_ptr()).  Writes the
        ranges back to back to out_ptr (out_capacity ints) and, if offsets_ptr is given, the nranges + 1 exclusive
        prefix sums of count there.  Returns sum(count); ANSX_ERR_CAPACITY raises AnsxError with .needed = sum(count)."""
        for name, v in (("nranges", nranges), ("out_capacity", out_capacity), ("in_bytes", in_bytes)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
        total = C.c_uint64(0)
        st = L.lib().ansx_decode_device_ranges_dev(self._ctx().handle, self.KIND, self.f, in_ptr, int(in_bytes),
                                                   first_ptr, count_ptr, int(nranges), out_ptr, int(out_capacity),
                                                   offsets_ptr, C.byref(total), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".decode_device_ranges_dev")
            if st == L.ERR_CAPACITY:
                err.needed = int(total.value)
            raise err
        return int(total.value)

    def decode_batch_dev(self, in_ptrs, in_bytes, out_ptr, out_capacity, stream=None):
        """A batch of containers in one call: in_ptrs / in_bytes (sequences or numpy arrays of ints) are the device
        addresses (16-byte aligned) and sizes of the containers; container i decodes to ints [offsets[i],
        offsets[i + 1]) of out_ptr (out_capacity ints).  Returns offsets, np.uint64 of len(in_ptrs) + 1 (the last is the
        total).  out_ptr=None with out_capacity=0 is a size query: it decodes nothing and returns the offsets.
        ERR_CAPACITY raises AnsxError with .needed = the total (and .offsets); a host-side ERR_FORMAT carries .index,
        the first container that failed its checks, one found on the device .index = None."""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        count = ptrs.size
        offsets = np.zeros(count + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        bad = C.c_size_t(count)
        st = L.lib().ansx_decode_batch_dev(self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if count else None,
                                           sizes.ctypes.data if count else None, count, out_ptr, int(out_capacity),
                                           offsets.ctypes.data, C.byref(total), C.byref(bad), stream)
        if st == L.ERR_CAPACITY and out_ptr is None and int(out_capacity) == 0:
            return offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".decode_batch_dev")
            if st == L.ERR_CAPACITY:
                err.needed = int(total.value)
                err.offsets = offsets
            if st == L.ERR_FORMAT:
                err.index = int(bad.value) if bad.value < count else None
            raise err
        return offsets

    def decode_batch_ranges_dev(self, in_ptrs, in_bytes, src, first, count, out_ptr, out_capacity, stream=None):
        """Ranges of a batch of containers in one call: range i is ints [first[i], first[i] + count[i]) of container
        src[i] of the batch in_ptrs / in_bytes (as decode_batch_dev; a container no range names is not looked at, its
        pointer may be 0) and goes to ints [offsets[i], offsets[i + 1]) of out_ptr (out_capacity ints).  Decodes only
        the blocks the ranges touch.  Returns offsets, np.uint64 of len(src) + 1 (the last is the total).  out_ptr=None
        with out_capacity=0 is a size query.  An AnsxError carries .bad_container / .bad_range where the call set
        them (None otherwise; a format error found on the device has .bad_container = len(in_ptrs)); ERR_CAPACITY
        also .needed = the total and .offsets."""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        src = np.ascontiguousarray(src, dtype=np.uint32).reshape(-1)
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
        count = np.ascontiguousarray(count, dtype=np.uint32).reshape(-1)
        if not src.size == first.size == count.size:
            raise ValueError("src, first and count differ in length (%d, %d, %d)" % (src.size, first.size, count.size))
        nc, nr = ptrs.size, src.size
        offsets = np.zeros(nr + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_r = C.c_size_t(unset), C.c_size_t(unset)
        st = L.lib().ansx_decode_batch_ranges_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None, nc,
            src.ctypes.data if nr else None, first.ctypes.data if nr else None, count.ctypes.data if nr else None, nr,
            out_ptr, int(out_capacity), offsets.ctypes.data, C.byref(total), C.byref(bad_c), C.byref(bad_r), stream)
        if st == L.ERR_CAPACITY and out_ptr is None and int(out_capacity) == 0:
            return offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".decode_batch_ranges_dev")
            err.bad_container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_range = int(bad_r.value) if bad_r.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(total.value)
                err.offsets = offsets
            raise err
        return offsets

    def encode_batch_dev(self, in_ptr, offsets, out_ptr, out_capacity, stream=None):
        """A batch of lists in one call: list i is ints [offsets[i], offsets[i + 1]) of the device array at in_ptr
        (offsets: len(lists) + 1 non-decreasing ints, the layout decode_batch_dev returns; no list may be empty).
        Container i -- byte for byte what encode_dev writes for list i -- goes to out_ptr + out_offsets[i] (16-byte
        aligned, back to back, zero padding in between) with out_bytes[i] bytes; sum(rup16(bound(n_i))) is always enough
        out_capacity.  Returns (out_offsets, out_bytes): np.uint64 of len(lists) + 1 (the last is the total) and of
        len(lists).  An AnsxError carries .index: the list an argument check or a per-list encode refused, None when
        the error was found on the device in a pass over many lists."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if offsets.size == 0:
            raise ValueError("offsets needs at least one entry (count + 1)")
        count = offsets.size - 1
        out_offsets = np.zeros(count + 1, dtype=np.uint64)
        out_bytes = np.zeros(count, dtype=np.uint64)
        total = C.c_size_t(0)
        bad = C.c_size_t(count)
        st = L.lib().ansx_encode_batch_dev(self._ctx().handle, self.KIND, self.f, in_ptr, offsets.ctypes.data, count, out_ptr,
                                           int(out_capacity), out_offsets.ctypes.data,
                                           out_bytes.ctypes.data if count else None, C.byref(total), C.byref(bad),
                                           C.byref(self.opts), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".encode_batch_dev")
            err.index = int(bad.value) if bad.value < count else None
            raise err
        return out_offsets, out_bytes

    # ---- docids: running sums behind the decoders, gaps in front of the encoders (include/ansx.h)
    def decode_sums_dev(self, in_ptr, in_bytes, out_ptr, n, stream=None):
        """decode_dev, then the n ints at out_ptr (4-byte aligned) are replaced by their inclusive running sums: gaps
        in, docids out.  ERR_DOMAIN if a running sum exceeds 2^32 - 1."""
        st = L.lib().ansx_decode_sums_dev(self._ctx().handle, self.KIND, self.f, in_ptr, in_bytes, out_ptr, n,
                                          C.byref(self.opts), stream)
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".decode_sums_dev")

    def decode_batch_sums_dev(self, in_ptrs, in_bytes, out_ptr, out_capacity, stream=None):
        """decode_batch_dev, then every list out[offsets[i] : offsets[i + 1]] is replaced by its own running sums.
        Arguments, return value and error attributes are those of decode_batch_dev; ERR_DOMAIN (the sum of a list
        exceeds 2^32 - 1) carries .index, the first such list."""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        count = ptrs.size
        offsets = np.zeros(count + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        bad = C.c_size_t(count)
        st = L.lib().ansx_decode_batch_sums_dev(self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if count else None,
                                                sizes.ctypes.data if count else None, count, out_ptr, int(out_capacity),
                                                offsets.ctypes.data, C.byref(total), C.byref(bad), stream)
        if st == L.ERR_CAPACITY and out_ptr is None and int(out_capacity) == 0:
            return offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".decode_batch_sums_dev")
            if st == L.ERR_CAPACITY:
                err.needed = int(total.value)
                err.offsets = offsets
            if st in (L.ERR_FORMAT, L.ERR_DOMAIN):
                err.index = int(bad.value) if bad.value < count else None
            raise err
        return offsets

    def encode_gaps_dev(self, in_ptr, n, out_ptr, out_capacity, stream=None):
        """encode_dev of the gaps of the n non-decreasing ids at in_ptr (which is only read) -> bytes written.
        ERR_DOMAIN if an id is smaller than the one before it."""
        nb = C.c_size_t(0)
        st = L.lib().ansx_encode_gaps_dev(self._ctx().handle, self.KIND, self.f, in_ptr, n, out_ptr,
                                          out_capacity, C.byref(nb), C.byref(self.opts), stream)
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".encode_gaps_dev")
        return nb.value

    def encode_batch_gaps_dev(self, in_ptr, offsets, out_ptr, out_capacity, stream=None):
        """encode_batch_dev of the gaps of every list of non-decreasing ids (a list's first gap is its first id).
        Arguments, return value and .index are those of encode_batch_dev; ERR_DOMAIN for a decrease carries .index,
        the first list that holds one."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if offsets.size == 0:
            raise ValueError("offsets needs at least one entry (count + 1)")
        count = offsets.size - 1
        out_offsets = np.zeros(count + 1, dtype=np.uint64)
        out_bytes = np.zeros(count, dtype=np.uint64)
        total = C.c_size_t(0)
        bad = C.c_size_t(count)
        st = L.lib().ansx_encode_batch_gaps_dev(self._ctx().handle, self.KIND, self.f, in_ptr, offsets.ctypes.data, count,
                                                out_ptr, int(out_capacity), out_offsets.ctypes.data,
                                                out_bytes.ctypes.data if count else None, C.byref(total), C.byref(bad),
                                                C.byref(self.opts), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".encode_batch_gaps_dev")
            err.index = int(bad.value) if bad.value < count else None
            raise err
        return out_offsets, out_bytes

    # ---- docids of ranges: block bases beside the container (include/ansx.h)
    def block_bases_dev(self, in_ptr, in_bytes, bases_ptr, capacity, stream=None):
        """The block bases of the container at in_ptr -> the nblocks + 1 uint32 at bases_ptr (capacity entries):
        bases[b] is the sum of the ints in front of block b.  Returns nbases = nblocks + 1.  bases_ptr=None with
        capacity=0 is a size query: nothing is decoded.  ERR_CAPACITY raises AnsxError with .needed = nbases;
        ERR_DOMAIN if the list sums to more than 2^32 - 1."""
        nb = C.c_size_t(0)
        st = L.lib().ansx_block_bases_dev(self._ctx().handle, self.KIND, self.f, in_ptr, int(in_bytes), bases_ptr,
                                          int(capacity), C.byref(nb), stream)
        if st == L.ERR_CAPACITY and bases_ptr is None and int(capacity) == 0:
            return int(nb.value)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".block_bases_dev")
            if st == L.ERR_CAPACITY:
                err.needed = int(nb.value)
            raise err
        return int(nb.value)

    def encode_gaps_bases_dev(self, in_ptr, n, out_ptr, out_capacity, bases_ptr, bases_capacity, stream=None):
        """encode_gaps_dev that also writes the block bases of its container to bases_ptr (bases_capacity uint32
        entries) -> (bytes written, nbases).  A bases_capacity below nblocks + 1 raises AnsxError(ERR_CAPACITY) with
        .needed = nbases before anything is encoded."""
        nb, nbases = C.c_size_t(0), C.c_size_t(0)
        st = L.lib().ansx_encode_gaps_bases_dev(self._ctx().handle, self.KIND, self.f, in_ptr, n, out_ptr, out_capacity,
                                                C.byref(nb), C.byref(self.opts), bases_ptr, int(bases_capacity),
                                                C.byref(nbases), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".encode_gaps_bases_dev")
            if st == L.ERR_CAPACITY and nbases.value > int(bases_capacity):
                err.needed = int(nbases.value)
            raise err
        return nb.value, int(nbases.value)

    def decode_ranges_sums_dev(self, in_ptr, in_bytes, bases_ptr, nbases, first, count, out_ptr, out_capacity, stream=None):
        """decode_ranges_dev returning docids: range i is sums[first[i] : first[i] + count[i]] of the container's
        running sums, computed from the touched blocks and their entries of the nbases block bases at bases_ptr.
        ERR_FORMAT if the bases of a touched block are not this container's.  Returns sum(count)."""
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
        count = np.ascontiguousarray(count, dtype=np.uint32).reshape(-1)
        if first.size != count.size:
            raise ValueError("first and count differ in length (%d, %d)" % (first.size, count.size))
        st = L.lib().ansx_decode_ranges_sums_dev(self._ctx().handle, self.KIND, self.f, in_ptr, in_bytes, bases_ptr,
                                                 int(nbases), first.ctypes.data, count.ctypes.data, first.size, out_ptr,
                                                 out_capacity, stream)
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".decode_ranges_sums_dev")
        return int(count.sum(dtype=np.uint64))

    def decode_device_ranges_sums_dev(self, in_ptr, in_bytes, bases_ptr, nbases, first_ptr, count_ptr, nranges, out_ptr,
                                      out_capacity, offsets_ptr=None, stream=None):
        """decode_device_ranges_dev returning docids (see decode_ranges_sums_dev); arguments, return value and
        .needed on ERR_CAPACITY are those of decode_device_ranges_dev, with bases_ptr, nbases behind in_bytes."""
        for name, v in (("nranges", nranges), ("out_capacity", out_capacity), ("in_bytes", in_bytes), ("nbases", nbases)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
        total = C.c_uint64(0)
        st = L.lib().ansx_decode_device_ranges_sums_dev(self._ctx().handle, self.KIND, self.f, in_ptr, int(in_bytes),
                                                        bases_ptr, int(nbases), first_ptr, count_ptr, int(nranges),
                                                        out_ptr, int(out_capacity), offsets_ptr, C.byref(total), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".decode_device_ranges_sums_dev")
            if st == L.ERR_CAPACITY:
                err.needed = int(total.value)
            raise err
        return int(total.value)

    # ---- search by value (include/ansx.h)
    def next_geq_dev(self, in_ptr, in_bytes, bases_ptr, nbases, targets_ptr, ntargets, pos_ptr, ids_ptr, stream=None):
        """For each of the ntargets uint32 at targets_ptr (device), the first docid >= it of the container at in_ptr:
        its position -> the uint64 at pos_ptr, the id -> the uint32 at ids_ptr (device arrays of ntargets; either may be
        None).  A target above the last id gives position n -- the authoritative "not found" -- and id NO_ID.  Only the
        blocks some target lands in are read, located through the nbases block bases at bases_ptr; ERR_FORMAT if the
        bases of such a block are not this container's, and then neither array is written.  Returns the number of
        targets found."""
        for name, v in (("ntargets", ntargets), ("in_bytes", in_bytes), ("nbases", nbases)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
        found = C.c_uint64(0)
        st = L.lib().ansx_next_geq_dev(self._ctx().handle, self.KIND, self.f, in_ptr, int(in_bytes), bases_ptr, int(nbases),
                                       targets_ptr, int(ntargets), pos_ptr, ids_ptr, C.byref(found), stream)
        if st != L.OK:
            raise L.AnsxError(st, self.name() + ".next_geq_dev")
        return int(found.value)

    # ---- batches of gap-coded lists: bases, ids of ranges, search by value (include/ansx.h)
    def encode_batch_gaps_bases_dev(self, in_ptr, offsets, out_ptr, out_capacity, bases_ptr, bases_capacity, stream=None):
        """encode_batch_gaps_dev that also writes the block bases of every list: list i's nb_i + 1 bases go to uint32
        entries [base_offsets[i], base_offsets[i + 1]) of bases_ptr (bases_capacity entries).  Returns (out_offsets,
        out_bytes, base_offsets), base_offsets np.uint64 of len(lists) + 1 (the last is the total).  bases_ptr=None
        with bases_capacity=0 is a size query: nothing is encoded and only base_offsets is returned.  A smaller
        bases_capacity raises AnsxError(ERR_CAPACITY) with .needed = the total and .base_offsets before anything is
        encoded; .index is that of encode_batch_gaps_dev."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if offsets.size == 0:
            raise ValueError("offsets needs at least one entry (count + 1)")
        count = offsets.size - 1
        out_offsets = np.zeros(count + 1, dtype=np.uint64)
        out_bytes = np.zeros(count, dtype=np.uint64)
        base_offsets = np.zeros(count + 1, dtype=np.uint64)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        total, nbases = C.c_size_t(0), C.c_size_t(unset)
        bad = C.c_size_t(count)
        st = L.lib().ansx_encode_batch_gaps_bases_dev(
            self._ctx().handle, self.KIND, self.f, in_ptr, offsets.ctypes.data, count, out_ptr, int(out_capacity),
            out_offsets.ctypes.data, out_bytes.ctypes.data if count else None, C.byref(total), C.byref(bad),
            C.byref(self.opts), bases_ptr, int(bases_capacity), base_offsets.ctypes.data, C.byref(nbases), stream)
        short = nbases.value != unset and nbases.value > int(bases_capacity)
        if st == L.ERR_CAPACITY and short and bases_ptr is None and int(bases_capacity) == 0:
            return base_offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".encode_batch_gaps_bases_dev")
            err.index = int(bad.value) if bad.value < count else None
            if st == L.ERR_CAPACITY and short:
                err.needed = int(nbases.value)
                err.base_offsets = base_offsets
            raise err
        return out_offsets, out_bytes, base_offsets

    @staticmethod
    def _batch_bases(ptrs, bases_ptrs, nbases):
        bptrs = np.ascontiguousarray(bases_ptrs, dtype=np.uint64).reshape(-1)
        nb = np.ascontiguousarray(nbases, dtype=np.uint64).reshape(-1)
        if not ptrs.size == bptrs.size == nb.size:
            raise ValueError("in_ptrs, bases_ptrs and nbases differ in length (%d, %d, %d)" % (ptrs.size, bptrs.size, nb.size))
        return bptrs, nb

    def decode_batch_ranges_sums_dev(self, in_ptrs, in_bytes, bases_ptrs, nbases, src, first, count, out_ptr, out_capacity,
                                     stream=None):
        """decode_batch_ranges_dev returning docids: range i is sums[first[i] : first[i] + count[i]] of the running
        sums of container src[i], computed from the touched blocks and their entries of that container's block bases,
        the nbases[j] uint32 at bases_ptrs[j] (arrays as long as in_ptrs; those of a container no range names are not
        looked at).  Arguments, return value and error attributes are otherwise those of decode_batch_ranges_dev;
        ERR_ARG with .bad_container for an nbases[j] that is not nblocks + 1, ERR_FORMAT with .bad_container =
        len(in_ptrs) if the bases of a touched block are not its container's.  (.container / .range repeat
        .bad_container / .bad_range.)"""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        bptrs, nb = self._batch_bases(ptrs, bases_ptrs, nbases)
        src = np.ascontiguousarray(src, dtype=np.uint32).reshape(-1)
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
        count = np.ascontiguousarray(count, dtype=np.uint32).reshape(-1)
        if not src.size == first.size == count.size:
            raise ValueError("src, first and count differ in length (%d, %d, %d)" % (src.size, first.size, count.size))
        nc, nr = ptrs.size, src.size
        offsets = np.zeros(nr + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_r = C.c_size_t(unset), C.c_size_t(unset)
        st = L.lib().ansx_decode_batch_ranges_sums_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None,
            bptrs.ctypes.data if nc else None, nb.ctypes.data if nc else None, nc,
            src.ctypes.data if nr else None, first.ctypes.data if nr else None, count.ctypes.data if nr else None, nr,
            out_ptr, int(out_capacity), offsets.ctypes.data, C.byref(total), C.byref(bad_c), C.byref(bad_r), stream)
        if st == L.ERR_CAPACITY and out_ptr is None and int(out_capacity) == 0:
            return offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".decode_batch_ranges_sums_dev")
            err.bad_container = err.container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_range = err.range = int(bad_r.value) if bad_r.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(total.value)
                err.offsets = offsets
            raise err
        return offsets

    def decode_batch_device_ranges_dev(self, in_ptrs, in_bytes, src_ptr, first_ptr, count_ptr, nranges, out_ptr, out_capacity,
                                       offsets_ptr=None, stream=None):
        """decode_batch_ranges_dev with the ranges in device memory and the plan built on the device: src_ptr ->
        nranges uint32 container numbers, first_ptr -> nranges uint64 firsts, count_ptr -> nranges uint32 counts, all
        device pointers read on `stream`.  in_ptrs / in_bytes are host sequences as in decode_batch_dev (a container no
        range names may be 0).  Writes the ranges back to back to out_ptr (out_capacity ints) and, if offsets_ptr (a
        device pointer) is given, the nranges + 1 exclusive prefix sums of count there.  Returns sum(count);
        out_ptr=None with out_capacity=0 is a size query.  An AnsxError carries .bad_container / .bad_range where the
        call set them (None otherwise); ERR_CAPACITY also .needed = sum(count)."""
        return self._batch_device_ranges("decode_batch_device_ranges_dev", in_ptrs, in_bytes, None, None, src_ptr, first_ptr,
                                         count_ptr, nranges, out_ptr, out_capacity, offsets_ptr, stream)

    def decode_batch_device_ranges_sums_dev(self, in_ptrs, in_bytes, bases_ptrs, nbases, src_ptr, first_ptr, count_ptr, nranges,
                                            out_ptr, out_capacity, offsets_ptr=None, stream=None):
        """decode_batch_device_ranges_dev returning docids, as decode_batch_ranges_sums_dev does: bases_ptrs / nbases
        are host sequences as long as in_ptrs (those of a container no range names are not looked at)."""
        return self._batch_device_ranges("decode_batch_device_ranges_sums_dev", in_ptrs, in_bytes, bases_ptrs, nbases, src_ptr,
                                         first_ptr, count_ptr, nranges, out_ptr, out_capacity, offsets_ptr, stream)

    def _batch_device_ranges(self, what, in_ptrs, in_bytes, bases_ptrs, nbases, src_ptr, first_ptr, count_ptr, nranges, out_ptr,
                             out_capacity, offsets_ptr, stream):
        for name, v in (("nranges", nranges), ("out_capacity", out_capacity)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        nc = ptrs.size
        head = [self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None]
        if bases_ptrs is not None:
            bptrs, nb = self._batch_bases(ptrs, bases_ptrs, nbases)
            # (the arrays themselves must not be null, even for an empty batch)
            head += [bptrs.ctypes.data if nc else np.zeros(1, np.uint64).ctypes.data,
                     nb.ctypes.data if nc else np.zeros(1, np.uint64).ctypes.data]
        total = C.c_uint64(0)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_r = C.c_size_t(unset), C.c_size_t(unset)
        st = getattr(L.lib(), "ansx_" + what)(*head, nc, src_ptr, first_ptr, count_ptr, int(nranges), out_ptr, int(out_capacity),
                                              offsets_ptr, C.byref(total), C.byref(bad_c), C.byref(bad_r), stream)
        if st == L.ERR_CAPACITY and out_ptr is None and int(out_capacity) == 0:
            return int(total.value)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + "." + what)
            err.bad_container = err.container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_range = err.range = int(bad_r.value) if bad_r.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(total.value)
            raise err
        return int(total.value)

    def next_geq_batch_dev(self, in_ptrs, in_bytes, bases_ptrs, nbases, src, targets_ptr, pos_ptr, ids_ptr, stream=None):
        """next_geq_dev over a batch: target i, the uint32 at targets_ptr + 4 i (device), is looked up in the list of
        container src[i] (host array; its length is the number of targets) of the batch in_ptrs / in_bytes /
        bases_ptrs / nbases (as decode_batch_ranges_sums_dev).  Position -> the uint64 at pos_ptr, id -> the uint32 at
        ids_ptr (device arrays of len(src); either may be None); a target above its list's last id gives that list's n
        and NO_ID.  Returns the number of targets found.  An AnsxError carries .bad_container / .bad_target where the
        call set them (None otherwise; .container / .target repeat them)."""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        bptrs, nb = self._batch_bases(ptrs, bases_ptrs, nbases)
        src = np.asarray(src)
        if src.size and src.dtype.kind not in "ui":
            raise ValueError("src must hold integers, got dtype %s" % src.dtype)
        src = np.ascontiguousarray(src, dtype=np.uint32).reshape(-1)
        nc, nt = ptrs.size, src.size
        found = C.c_uint64(0)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_t = C.c_size_t(unset), C.c_size_t(unset)
        st = L.lib().ansx_next_geq_batch_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None,
            bptrs.ctypes.data if nc else None, nb.ctypes.data if nc else None, nc, src.ctypes.data if nt else None,
            targets_ptr, nt, pos_ptr, ids_ptr, C.byref(found), C.byref(bad_c), C.byref(bad_t), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".next_geq_batch_dev")
            err.bad_container = err.container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_target = err.target = int(bad_t.value) if bad_t.value != unset else None
            raise err
        return int(found.value)

    # ---- intersection (include/ansx.h)
    def intersect_ids_dev(self, in_ptr, in_bytes, bases_ptr, nbases, cand_ptr, ncand, out_ids_ptr, out_idx_ptr, out_pos_ptr,
                          out_capacity, stream=None):
        """Which of the ncand uint32 at cand_ptr (device, any order, repeats allowed) are docids of the container at
        in_ptr: the members, in candidate order and back to back, go to the device arrays of out_capacity entries
        out_ids_ptr (uint32: the value), out_idx_ptr (uint32: its index among the candidates) and out_pos_ptr (uint64:
        its first position in the list); any may be None, not all.  Returns the number of members; more than
        out_capacity raises AnsxError(ERR_CAPACITY) with .needed = that number and writes nothing.  ERR_FORMAT if the
        bases of a block some candidate was sent to are not this container's; nothing is written then either."""
        for name, v in (("ncand", ncand), ("in_bytes", in_bytes), ("nbases", nbases), ("out_capacity", out_capacity)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
        found = C.c_uint64(0)
        st = L.lib().ansx_intersect_ids_dev(self._ctx().handle, self.KIND, self.f, in_ptr, int(in_bytes), bases_ptr,
                                            int(nbases), cand_ptr, int(ncand), out_ids_ptr, out_idx_ptr, out_pos_ptr,
                                            int(out_capacity), C.byref(found), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".intersect_ids_dev")
            if st == L.ERR_CAPACITY:
                err.needed = int(found.value)
            raise err
        return int(found.value)

    def intersect_dev(self, in_ptrs, in_bytes, bases_ptrs, nbases, out_ids_ptr, out_capacity, stream=None):
        """The docids common to the lists of the batch in_ptrs / in_bytes / bases_ptrs / nbases (as
        decode_batch_ranges_sums_dev): those of the shortest list (of equal ones the first) that occur in every other
        one, ascending, to the uint32 array of out_capacity entries at out_ids_ptr (device).  Returns their number; more
        than out_capacity raises AnsxError(ERR_CAPACITY) with .needed = that number and writes nothing, so
        out_ids_ptr=None, out_capacity=0 asks for the size.  An AnsxError carries .bad_container where the call set it
        (None otherwise)."""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        bptrs, nb = self._batch_bases(ptrs, bases_ptrs, nbases)
        nc = ptrs.size
        found = C.c_uint64(0)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c = C.c_size_t(unset)
        st = L.lib().ansx_intersect_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None,
            bptrs.ctypes.data if nc else None, nb.ctypes.data if nc else None, nc, out_ids_ptr, int(out_capacity),
            C.byref(found), C.byref(bad_c), stream)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".intersect_dev")
            err.bad_container = err.container = int(bad_c.value) if bad_c.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(found.value)
            raise err
        return int(found.value)

    @staticmethod
    def _batch_queries(in_ptrs, in_bytes, queries, out_capacity):
        """The checked host arrays of a call over queries of a batch -> (ptrs, sizes, terms, qoff)"""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        if isinstance(out_capacity, bool) or not isinstance(out_capacity, (int, np.integer)) or out_capacity < 0:
            raise ValueError("out_capacity must be a non-negative integer, got %r" % (out_capacity,))
        terms, qoff = _Codec._flatten_queries(queries, "queries", "query")
        return ptrs, sizes, terms, qoff

    @staticmethod
    def _flatten_queries(queries, what, one):
        """A sequence of sequences of batch indices -> (terms, qoff), the flat uint32 and uint64 host arrays of a call"""
        if isinstance(queries, (str, bytes)) or not hasattr(queries, "__len__"):
            raise ValueError("%s must be a sequence of sequences of batch indices" % what)
        qoff = np.zeros(len(queries) + 1, dtype=np.uint64)
        flat = []
        for q, terms in enumerate(queries):
            if isinstance(terms, (str, bytes)) or not hasattr(terms, "__len__"):
                raise ValueError("%s %d is not a sequence of batch indices" % (one, q))
            t = np.asarray(terms)
            if t.ndim != 1 or (t.size and t.dtype.kind not in "ui"):
                raise ValueError("%s %d must be a flat sequence of integers" % (one, q))
            if t.size and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
                raise ValueError("%s %d names a list outside [0, 2^32)" % (one, q))
            flat.append(t.astype(np.uint32))
            qoff[q + 1] = qoff[q] + np.uint64(t.size)
        # (never empty, so that the library and not a null array answers queries that are all empty)
        terms = np.ascontiguousarray(np.concatenate(flat + [np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)
        return terms, qoff

    def intersect_batch_dev(self, in_ptrs, in_bytes, queries, out_ids_ptr, out_capacity, stream=None):
        """intersect_dev for many queries over the batch in_ptrs / in_bytes in one call (no bases
        are needed).  queries: a sequence of non-empty sequences of batch indices.  The result of query q, exactly what
        intersect_dev gives for its lists in that order, goes to uint32 entries [offsets[q], offsets[q + 1]) of
        out_ids_ptr (device, out_capacity entries); returns offsets, np.uint64 of len(queries) + 1.  A total above
        out_capacity raises AnsxError(ERR_CAPACITY) with .needed = the total and .offsets, except that out_ids_ptr=None,
        out_capacity=0 is a size query and returns the offsets.  A container no query names is not looked at and may be
        0.  An AnsxError carries .bad_container / .bad_query where the call set them (None otherwise)."""
        ptrs, sizes, terms, qoff = self._batch_queries(in_ptrs, in_bytes, queries, out_capacity)
        nc, nq = ptrs.size, len(queries)
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_q = C.c_size_t(unset), C.c_size_t(unset)
        st = L.lib().ansx_intersect_batch_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None, nc,
            terms.ctypes.data, qoff.ctypes.data, nq, out_ids_ptr, int(out_capacity),
            offsets.ctypes.data, C.byref(bad_c), C.byref(bad_q), stream)
        if st == L.ERR_CAPACITY and out_ids_ptr is None and int(out_capacity) == 0:
            return offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".intersect_batch_dev")
            err.bad_container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_query = int(bad_q.value) if bad_q.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(offsets[nq])
                err.offsets = offsets
            raise err
        return offsets

    # ---- union (include/ansx.h)
    def union_batch_dev(self, in_ptrs, in_bytes, queries, out_ids_ptr, out_capacity, out_cnt_ptr=None, stream=None):
        """Many disjunctive queries over the batch in_ptrs / in_bytes in one call (no bases are needed).  queries: a
        sequence of non-empty sequences of batch indices.  The distinct docids that occur in any list of query q,
        ascending, go to uint32 entries [offsets[q], offsets[q + 1]) of out_ids_ptr (device, out_capacity entries) and,
        when out_cnt_ptr is given (device, uint32, the same capacity and offsets), how often each occurs in the query's
        lists as named; returns offsets, np.uint64 of len(queries) + 1.  A total above out_capacity raises
        AnsxError(ERR_CAPACITY) with .needed = the total and .offsets, except that out_ids_ptr=None, out_capacity=0 is a
        size query and returns the offsets.  A container no query names is not looked at and may be 0.  An AnsxError
        carries .bad_container / .bad_query where the call set them (None otherwise)."""
        ptrs, sizes, terms, qoff = self._batch_queries(in_ptrs, in_bytes, queries, out_capacity)
        nc, nq = ptrs.size, len(queries)
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_q = C.c_size_t(unset), C.c_size_t(unset)
        st = L.lib().ansx_union_batch_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None, nc,
            terms.ctypes.data, qoff.ctypes.data, nq, out_ids_ptr, out_cnt_ptr, int(out_capacity),
            offsets.ctypes.data, C.byref(bad_c), C.byref(bad_q), stream)
        if st == L.ERR_CAPACITY and out_ids_ptr is None and int(out_capacity) == 0:
            return offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".union_batch_dev")
            err.bad_container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_query = int(bad_q.value) if bad_q.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(offsets[nq])
                err.offsets = offsets
            raise err
        return offsets

    # ---- Boolean queries with exclusion (include/ansx.h)
    def bool_batch_dev(self, in_ptrs, in_bytes, queries, excludes, out_ids_ptr, out_capacity, op="all", stream=None):
        """Many Boolean queries over the batch in_ptrs / in_bytes in one call.  queries: as for intersect_batch_dev;
        op "all" intersects a query's lists (intersect_batch_dev's result), "any" unites them (union_batch_dev's ids).
        excludes: None, or a sequence as long as queries of (possibly empty) sequences of batch indices: every docid
        that occurs in one of query q's excluded lists is removed from its result.  Outputs, offsets (np.uint64 of
        len(queries) + 1), the size query and the errors are intersect_batch_dev's; an AnsxError carries .bad_container
        / .bad_query where the call set them (None otherwise)."""
        ops = {"all": L.BOOL_ALL, "any": L.BOOL_ANY}
        if op not in ops:
            raise ValueError("op must be 'all' or 'any', got %r" % (op,))
        ptrs, sizes, terms, qoff = self._batch_queries(in_ptrs, in_bytes, queries, out_capacity)
        nc, nq = ptrs.size, len(queries)
        xterms = xqoff = None
        if excludes is not None:
            xterms, xqoff = self._flatten_queries(excludes, "excludes", "excludes of query")
            if xqoff.size != nq + 1:
                raise ValueError("excludes and queries differ in length (%d, %d)" % (xqoff.size - 1, nq))
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_q = C.c_size_t(unset), C.c_size_t(unset)
        st = L.lib().ansx_bool_batch_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None, nc,
            ops[op], terms.ctypes.data, qoff.ctypes.data, None if xterms is None else xterms.ctypes.data,
            None if xqoff is None else xqoff.ctypes.data, nq, out_ids_ptr, int(out_capacity),
            offsets.ctypes.data, C.byref(bad_c), C.byref(bad_q), stream)
        if st == L.ERR_CAPACITY and out_ids_ptr is None and int(out_capacity) == 0:
            return offsets
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".bool_batch_dev")
            err.bad_container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_query = int(bad_q.value) if bad_q.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(offsets[nq])
                err.offsets = offsets
            raise err
        return offsets

    # ---- ranked disjunctive queries (include/ansx.h)
    def topk_batch_dev(self, in_ptrs, in_bytes, queries, weights, k, out_ids_ptr, out_scores_ptr=None, pay_ptrs=None,
                       pay_sizes=None, stream=None):
        """Many ranked disjunctive queries over the batch in_ptrs / in_bytes in one call.  queries: as for
        union_batch_dev; weights: a sequence as long as queries of sequences of integers in [0, 2^32), weights[q][i] the
        weight of queries[q][i].  pay_ptrs / pay_sizes: None (every payload is 1), or per list of the batch a container
        of this codec with a value per posting.  The k ids of query q's union with the largest scores -- the sum over
        its postings of weight * payload -- ordered by (score descending, id ascending) go to uint32 entries
        [q * k, q * k + counts[q]) of out_ids_ptr (device, len(queries) * k entries) and their scores to out_scores_ptr
        when given; the entries behind are ANSX_NO_ID / 0.  Returns counts, np.uint32 of len(queries): min(k, distinct
        ids).  A score of 2^32 - 1 or more raises AnsxError(ERR_DOMAIN) with .bad_query.  An AnsxError carries
        .bad_container / .bad_query where the call set them (None otherwise)."""
        return self._topk_call("topk_batch_dev", in_ptrs, in_bytes, queries, weights, None, k, out_ids_ptr, None, out_scores_ptr,
                               pay_ptrs, pay_sizes, stream)

    # ---- ranked Boolean queries (include/ansx.h)
    def topk_bool_batch_dev(self, in_ptrs, in_bytes, queries, weights, excludes, k, out_ids_ptr, op="all", out_scores_ptr=None,
                            pay_ptrs=None, pay_sizes=None, stream=None):
        """topk_batch_dev over the ids of ALL of a query's lists (op "all") or of ANY of them (op "any"), less every id that
        occurs in one of the query's excluded lists.  excludes: None, or a sequence as long as queries of (possibly empty)
        sequences of batch indices, as for bool_batch_dev.  Scores, the order, the outputs and counts (np.uint32 of
        len(queries): min(k, ids in the result)) are topk_batch_dev's; every posting of a result's id is scored, and the
        id appears once.  A list that is only excluded needs no payload (its pay_ptrs entry may be 0).  A score of
        2^32 - 1 or more of an id of the result raises AnsxError(ERR_DOMAIN) with .bad_query.  An AnsxError carries
        .bad_container / .bad_query where the call set them (None otherwise)."""
        ops = {"all": L.BOOL_ALL, "any": L.BOOL_ANY}
        if op not in ops:
            raise ValueError("op must be 'all' or 'any', got %r" % (op,))
        return self._topk_call("topk_bool_batch_dev", in_ptrs, in_bytes, queries, weights, excludes, k, out_ids_ptr, ops[op],
                               out_scores_ptr, pay_ptrs, pay_sizes, stream)

    # ---- ranked queries with required, optional and excluded terms (include/ansx.h)
    def topk_query_batch_dev(self, in_ptrs, in_bytes, queries, weights, occurs, min_should, excludes, k, out_ids_ptr,
                             out_scores_ptr=None, pay_ptrs=None, pay_sizes=None, stream=None):
        """topk_bool_batch_dev with a role per term and a threshold per query instead of one op.  occurs: None (every term
        is optional), or a sequence as long as queries of sequences of OCCUR_MUST (1, required) / OCCUR_SHOULD (0, optional),
        occurs[q][i] the role of queries[q][i].  min_should: None (all zero), or a sequence of len(queries) integers in
        [0, 2^32).  The result of query q: the ids that occur in every required list, have at least min_should[q] entries
        in its optional lists as named (at least one where it has no required term) and occur in none of its excluded
        lists; every posting of a result's id, in required and optional lists, is scored.  Outputs, counts and errors are
        topk_bool_batch_dev's."""
        return self._topk_call("topk_query_batch_dev", in_ptrs, in_bytes, queries, weights, excludes, k, out_ids_ptr, None,
                               out_scores_ptr, pay_ptrs, pay_sizes, stream, query=(occurs, min_should))

    # ---- ranked queries with length-normalised scores (include/ansx.h)
    def topk_scored_batch_dev(self, in_ptrs, in_bytes, queries, weights, occurs, min_should, excludes, k, out_ids_ptr,
                              out_scores_ptr=None, pay_ptrs=None, pay_sizes=None, stream=None, scorer=None):
        """topk_query_batch_dev in which a posting contributes weight * table[min(payload, tf_rows - 1)][norms[id]] -- a
        quantised impact, BM25 among them -- and not weight * payload.  scorer: None (topk_query_batch_dev itself, the same
        bytes and launches), or (norms_ptr, ndocs, table_ptr, tf_rows): the device address of ndocs uint8 norms, one per
        document id, and of tf_rows * 256 uint32 impacts, row-major; bm25_norms and bm25_table make both for BM25, the IDF
        being the weights.  A scorer needs pay_ptrs (the term frequencies).  An id of ndocs or more in a list that is a term
        raises AnsxError(ERR_DOMAIN) with .bad_container; everything else is topk_query_batch_dev's."""
        return self._topk_call("topk_scored_batch_dev", in_ptrs, in_bytes, queries, weights, excludes, k, out_ids_ptr, None,
                               out_scores_ptr, pay_ptrs, pay_sizes, stream, query=(occurs, min_should), scorer=scorer, scored=True)

    # ---- ranked queries with total hits and facet counts (include/ansx.h)
    def topk_facets_batch_dev(self, in_ptrs, in_bytes, queries, weights, occurs, min_should, excludes, k, out_ids_ptr,
                              out_scores_ptr=None, pay_ptrs=None, pay_sizes=None, stream=None, scorer=None, facets=None, totals=True):
        """topk_scored_batch_dev that also says how many documents matched and how they fall over one column.  facets: None,
        or (values_ptr, ndocs, nvalues, counts_ptr): the device address of ndocs uint32 values, one per document id, and of
        len(queries) * nvalues uint32 counts, which the call zeroes and fills: counts[q * nvalues + v] = the ids of query
        q's whole result with value v; a value of nvalues or more is counted nowhere.  Returns (counts, totals): what
        topk_scored_batch_dev returns, and np.uint32 of len(queries), the size of every query's result, not cut to k
        (totals=False: None, and the library is handed no array).  An id of ndocs or more in a result raises
        AnsxError(ERR_DOMAIN) with .bad_query; everything else is topk_scored_batch_dev's.  With facets=None and
        totals=False it is that call: the same bytes and launches."""
        return self._topk_call("topk_facets_batch_dev", in_ptrs, in_bytes, queries, weights, excludes, k, out_ids_ptr, None,
                               out_scores_ptr, pay_ptrs, pay_sizes, stream, query=(occurs, min_should), scorer=scorer, scored=True,
                               facets=(facets, bool(totals)))

    # ---- ranked queries with range filters over document columns (include/ansx.h)
    def topk_filter_batch_dev(self, in_ptrs, in_bytes, queries, weights, occurs, min_should, excludes, k, out_ids_ptr,
                              out_scores_ptr=None, pay_ptrs=None, pay_sizes=None, stream=None, scorer=None, facets=None, totals=True,
                              filters=None):
        """topk_facets_batch_dev over the ids of every query's result that pass the query's clauses, applied before the
        ranking, the totals and the facet counts.  filters: None (that call itself, the same bytes and launches), or
        (column_ptrs, ndocs, clauses_per_query): the device addresses of the columns, each ndocs uint32 values, one per
        document id (None / 0 for a column no clause names), and a sequence as long as queries of (possibly empty) sequences
        of clauses (column, lo, hi) or (column, lo, hi, negate): the clause passes for document d iff
        (lo <= column[d] <= hi) != negate; lo > hi is the empty range.  A query's clauses are conjunctive; a query without
        clauses is not filtered.  sortable_u32 maps int32 and float32 columns and bounds to uint32, order-preserving.
        Returns what topk_facets_batch_dev returns, over the filtered results.  An id of ndocs or more in the result of a
        query with a clause raises AnsxError(ERR_DOMAIN) with .bad_query."""
        return self._topk_call("topk_filter_batch_dev", in_ptrs, in_bytes, queries, weights, excludes, k, out_ids_ptr, None,
                               out_scores_ptr, pay_ptrs, pay_sizes, stream, query=(occurs, min_should), scorer=scorer, scored=True,
                               facets=(facets, bool(totals)), filters=(filters,))

    @staticmethod
    def _filters_struct(fl, nq):
        """filters = (column_ptrs, ndocs, clauses_per_query) -> (L.Filters, the arrays it points into); what can be
        checked before the library is checked here"""
        if isinstance(fl, (str, bytes)) or not hasattr(fl, "__len__") or len(fl) != 3:
            raise ValueError("filters must be (column_ptrs, ndocs, clauses_per_query)")
        cols, ndocs, per = fl
        if isinstance(cols, (str, bytes)) or not hasattr(cols, "__len__"):
            raise ValueError("filters: column_ptrs must be a sequence of device addresses")
        for v in cols:
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 1 << 64):
                raise ValueError("filters: a column pointer must be a non-negative integer or None, got %r" % (v,))
        if isinstance(ndocs, bool) or not isinstance(ndocs, (int, np.integer)) or not 0 <= ndocs < 1 << 64:
            raise ValueError("filters: ndocs must be a non-negative integer, got %r" % (ndocs,))
        if isinstance(per, (str, bytes)) or not hasattr(per, "__len__") or len(per) != nq:
            raise ValueError("filters: clauses_per_query must be a sequence as long as queries")
        colarr = np.array([int(v or 0) for v in cols] + [0], dtype=np.uint64)  # (never empty)
        fqoff = np.zeros(nq + 1, dtype=np.uint64)
        rows = []
        for q, cl in enumerate(per):
            if isinstance(cl, (str, bytes)) or not hasattr(cl, "__len__"):
                raise ValueError("filters: the clauses of query %d are not a sequence" % q)
            for c in cl:
                if isinstance(c, (str, bytes)) or not hasattr(c, "__len__") or len(c) not in (3, 4):
                    raise ValueError("filters: a clause of query %d is not (column, lo, hi[, negate])" % q)
                for v in c[:3]:
                    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 0xFFFFFFFF:
                        raise ValueError("filters: a clause of query %d holds %r, not an integer in [0, 2^32)" % (q, v))
                rows.append((int(c[0]), int(c[1]), int(c[2]), L.FILTER_NOT if len(c) == 4 and c[3] else 0))
            fqoff[q + 1] = len(rows)
        clauses = np.array(rows + [(0, 0, 0, 0)], dtype=np.uint32).reshape(-1, 4)  # (never empty)
        st = L.Filters(colarr.ctypes.data, len(cols), int(ndocs), clauses.ctypes.data, fqoff.ctypes.data)
        return st, (colarr, fqoff, clauses)

    def _topk_call(self, what, in_ptrs, in_bytes, queries, weights, excludes, k, out_ids_ptr, op, out_scores_ptr, pay_ptrs,
                   pay_sizes, stream, query=None, scorer=None, scored=False, facets=None, filters=None):
        """What the ranked calls share: the checks of their arguments and the call; op None: ansx_topk_batch_dev or, with
        query = (occurs, min_should), ansx_topk_query_batch_dev -- with scored, ansx_topk_scored_batch_dev, scorer its
        (norms_ptr, ndocs, table_ptr, tf_rows) or None -- with facets = ((values_ptr, ndocs, nvalues, counts_ptr) or None,
        whether the totals are wanted), ansx_topk_facets_batch_dev, which returns (counts, totals or None) -- with filters =
        ((column_ptrs, ndocs, clauses_per_query) or None,) as well, ansx_topk_filter_batch_dev"""
        fc = None
        if facets is not None and facets[0] is not None:
            fa = facets[0]
            if isinstance(fa, (str, bytes)) or not hasattr(fa, "__len__") or len(fa) != 4:
                raise ValueError("facets must be (values_ptr, ndocs, nvalues, counts_ptr)")
            for name, v, top in zip(("values_ptr", "ndocs", "nvalues", "counts_ptr"), fa, (1 << 64, 1 << 64, 1 << 32, 1 << 64)):
                if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < top):
                    raise ValueError("facets: %s must be a non-negative integer, got %r" % (name, v))
            fc = L.Facets(fa[0], int(fa[1] or 0), int(fa[2] or 0), fa[3])
        sc = None
        if scorer is not None:
            if isinstance(scorer, (str, bytes)) or not hasattr(scorer, "__len__") or len(scorer) != 4:
                raise ValueError("scorer must be (norms_ptr, ndocs, table_ptr, tf_rows)")
            for name, v, top in zip(("norms_ptr", "ndocs", "table_ptr", "tf_rows"), scorer, (1 << 64, 1 << 64, 1 << 64, 1 << 32)):
                if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < top):
                    raise ValueError("scorer: %s must be a non-negative integer, got %r" % (name, v))
            sc = L.Scorer(scorer[0], int(scorer[1] or 0), scorer[2], int(scorer[3] or 0))
        ptrs, sizes, terms, qoff = self._batch_queries(in_ptrs, in_bytes, queries, 0)
        nc, nq = ptrs.size, len(queries)
        occ = msm = None
        if query is not None and query[0] is not None:
            occurs = query[0]
            if isinstance(occurs, (str, bytes)) or not hasattr(occurs, "__len__") or len(occurs) != nq:
                raise ValueError("occurs must be a sequence as long as queries")
            # (one conversion for all queries: a conversion per query costs microseconds each, which a batch of
            # thousands of short queries would see)
            lens = qoff[1:] - qoff[:-1]
            for q, oc in enumerate(occurs):
                if isinstance(oc, (str, bytes)) or not hasattr(oc, "__len__"):
                    raise ValueError("occurs of query %d are not a sequence of integers" % q)
                if len(oc) != lens[q]:
                    raise ValueError("occurs of query %d must be a flat sequence of integers, one per term" % q)
            flat = np.array([o for oc in occurs for o in oc] + [0])  # (never empty)
            if flat.ndim != 1 or flat.dtype.kind not in "uib":
                raise ValueError("occurs must be flat sequences of integers, one per term")
            if int(flat.min()) < 0 or int(flat.max()) > 0xFF:
                raise ValueError("occurs lie outside [0, 256)")
            occ = np.ascontiguousarray(flat, dtype=np.uint8)
        if query is not None and query[1] is not None:
            ms = query[1]
            if isinstance(ms, (str, bytes)) or not hasattr(ms, "__len__") or len(ms) != nq:
                raise ValueError("min_should must be a sequence as long as queries")
            ms = np.asarray(ms).reshape(-1)
            if ms.size and (ms.dtype.kind not in "ui" or int(ms.min()) < 0 or int(ms.max()) > 0xFFFFFFFF):
                raise ValueError("min_should must hold integers in [0, 2^32)")
            msm = np.ascontiguousarray(np.concatenate([ms.astype(np.uint32), np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)
        xterms = xqoff = None
        if excludes is not None:
            xterms, xqoff = self._flatten_queries(excludes, "excludes", "excludes of query")
            if xqoff.size != nq + 1:
                raise ValueError("excludes and queries differ in length (%d, %d)" % (xqoff.size - 1, nq))
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k <= 0xFFFFFFFF:
            raise ValueError("k must be an integer in [0, 2^32), got %r" % (k,))
        if isinstance(weights, (str, bytes)) or not hasattr(weights, "__len__") or len(weights) != nq:
            raise ValueError("weights must be a sequence as long as queries")
        flat = []
        for q, w in enumerate(weights):
            if isinstance(w, (str, bytes)) or not hasattr(w, "__len__"):
                raise ValueError("weights of query %d are not a sequence of integers" % q)
            w = np.asarray(w)
            if w.ndim != 1 or w.size != int(qoff[q + 1] - qoff[q]) or (w.size and w.dtype.kind not in "ui"):
                raise ValueError("weights of query %d must be a flat sequence of integers, one per term" % q)
            if w.size and (int(w.min()) < 0 or int(w.max()) > 0xFFFFFFFF):
                raise ValueError("weights of query %d lie outside [0, 2^32)" % q)
            flat.append(w.astype(np.uint32))
        wts = np.ascontiguousarray(np.concatenate(flat + [np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)  # (never empty)
        pays = psizes = None
        if (pay_ptrs is None) != (pay_sizes is None):
            raise ValueError("pay_ptrs and pay_sizes go together")
        if pay_ptrs is not None:
            pays = np.ascontiguousarray(pay_ptrs, dtype=np.uint64).reshape(-1)
            psizes = np.ascontiguousarray(pay_sizes, dtype=np.uint64).reshape(-1)
            if pays.size != nc or psizes.size != nc:
                raise ValueError("pay_ptrs / pay_sizes and in_ptrs differ in length (%d, %d, %d)" % (pays.size, psizes.size, nc))
            if nc == 0:  # (never a null array: the library answers)
                pays, psizes = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        counts = np.zeros(nq, dtype=np.uint32)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c, bad_q = C.c_size_t(unset), C.c_size_t(unset)
        head = (self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None,
                None if pays is None else pays.ctypes.data, None if psizes is None else psizes.ctypes.data, nc)
        tail = (nq, int(k), out_ids_ptr, out_scores_ptr, counts.ctypes.data if nq else None, C.byref(bad_c), C.byref(bad_q), stream)
        totals = np.zeros(nq, dtype=np.uint32) if facets is not None and facets[1] else None
        if filters is not None:
            fl, keep = (None, None) if filters[0] is None else self._filters_struct(filters[0], nq)
            st = L.lib().ansx_topk_filter_batch_dev(
                *head, terms.ctypes.data, wts.ctypes.data, None if occ is None else occ.ctypes.data, qoff.ctypes.data,
                None if msm is None else msm.ctypes.data, None if xterms is None else xterms.ctypes.data,
                None if xqoff is None else xqoff.ctypes.data, None if sc is None else C.byref(sc), None if fc is None else C.byref(fc),
                None if fl is None else C.byref(fl), *tail[:5], totals.ctypes.data if totals is not None and nq else None, *tail[5:])
            del keep
        elif facets is not None:
            st = L.lib().ansx_topk_facets_batch_dev(
                *head, terms.ctypes.data, wts.ctypes.data, None if occ is None else occ.ctypes.data, qoff.ctypes.data,
                None if msm is None else msm.ctypes.data, None if xterms is None else xterms.ctypes.data,
                None if xqoff is None else xqoff.ctypes.data, None if sc is None else C.byref(sc), None if fc is None else C.byref(fc),
                *tail[:5], totals.ctypes.data if totals is not None and nq else None, *tail[5:])
        elif scored:
            st = L.lib().ansx_topk_scored_batch_dev(
                *head, terms.ctypes.data, wts.ctypes.data, None if occ is None else occ.ctypes.data, qoff.ctypes.data,
                None if msm is None else msm.ctypes.data, None if xterms is None else xterms.ctypes.data,
                None if xqoff is None else xqoff.ctypes.data, None if sc is None else C.byref(sc), *tail)
        elif query is not None:
            st = L.lib().ansx_topk_query_batch_dev(
                *head, terms.ctypes.data, wts.ctypes.data, None if occ is None else occ.ctypes.data, qoff.ctypes.data,
                None if msm is None else msm.ctypes.data, None if xterms is None else xterms.ctypes.data,
                None if xqoff is None else xqoff.ctypes.data, *tail)
        elif op is None:
            st = L.lib().ansx_topk_batch_dev(*head, terms.ctypes.data, wts.ctypes.data, qoff.ctypes.data, *tail)
        else:
            st = L.lib().ansx_topk_bool_batch_dev(
                *head, op, terms.ctypes.data, wts.ctypes.data, qoff.ctypes.data, None if xterms is None else xterms.ctypes.data,
                None if xqoff is None else xqoff.ctypes.data, *tail)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + "." + what)
            err.bad_container = int(bad_c.value) if bad_c.value != unset else None
            err.bad_query = int(bad_q.value) if bad_q.value != unset else None
            raise err
        return counts if facets is None else (counts, totals)

    def union_dev(self, in_ptrs, in_bytes, out_ids_ptr, out_capacity, out_cnt_ptr=None, stream=None):
        """union_batch_dev's single query over all the lists of the batch in_ptrs / in_bytes, in batch order.  Returns the
        number of distinct docids; more than out_capacity raises AnsxError(ERR_CAPACITY) with .needed = that number,
        except that out_ids_ptr=None, out_capacity=0 is a size query and returns the number.  An AnsxError carries
        .bad_container where the call set it (None otherwise)."""
        ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(in_bytes, dtype=np.uint64).reshape(-1)
        if ptrs.size != sizes.size:
            raise ValueError("in_ptrs and in_bytes differ in length (%d, %d)" % (ptrs.size, sizes.size))
        if isinstance(out_capacity, bool) or not isinstance(out_capacity, (int, np.integer)) or out_capacity < 0:
            raise ValueError("out_capacity must be a non-negative integer, got %r" % (out_capacity,))
        nc = ptrs.size
        found = C.c_uint64(0)
        unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
        bad_c = C.c_size_t(unset)
        st = L.lib().ansx_union_dev(
            self._ctx().handle, self.KIND, self.f, ptrs.ctypes.data if nc else None, sizes.ctypes.data if nc else None, nc,
            out_ids_ptr, out_cnt_ptr, int(out_capacity), C.byref(found), C.byref(bad_c), stream)
        if st == L.ERR_CAPACITY and out_ids_ptr is None and int(out_capacity) == 0:
            return int(found.value)
        if st != L.OK:
            err = L.AnsxError(st, self.name() + ".union_dev")
            err.bad_container = err.container = int(bad_c.value) if bad_c.value != unset else None
            if st == L.ERR_CAPACITY:
                err.needed = int(found.value)
            raise err
        return int(found.value)


class ANSfold(_Codec):
    """methods.hpp:529-547"""
    KIND = L.FOLD
    PREFIX = "ANSfold"


class ANSrfold(_Codec):
    """methods.hpp:549-567"""
    KIND = L.RFOLD
    PREFIX = "ANSrfold"


class ANSmsb(_Codec):
    """methods.hpp:499-515 (include/ans_msb.hpp): the fixed-threshold MSB fold; no fidelity."""
    KIND = L.MSB
    PREFIX = "ANSmsb"

    def __init__(self, ctx=None, block_ints=0, ckpt_interval=0, compact=False):
        super().__init__(0, ctx=ctx, block_ints=block_ints, ckpt_interval=ckpt_interval, compact=compact)


class ANSint(_Codec):
    """methods.hpp:484-497 (include/ans_int.hpp), name() == "ANS".  compact=True (default): per-block alphabet
    compaction, any values.  compact=False: the values themselves are the symbols and must be below 16384;
    block_ints=SINGLE_STREAM then gives exactly the bytes of ANSint::encode (ans_int_compress)."""
    KIND = L.INT
    PREFIX = "ANS"

    def __init__(self, ctx=None, block_ints=0, ckpt_interval=0, compact=True):
        super().__init__(0, ctx=ctx, block_ints=block_ints, ckpt_interval=ckpt_interval, compact=compact)


# ---------------------------------------------------------------- container parsing (host)

# ---- BM25 as quantised integer impacts for topk_scored_batch_dev; pure numpy, no device
# The lower edge of every length class: lengths 0 .. 31 have a class each, and from 32 on every octave [2^e, 2^(e + 1))
# is cut into 16 classes of equal width (sixteenth-octaves), up to 2^19; class 255 holds every length from 507904 on.
# Written out as literals, so that no floating-point rounding ever decides a class.
BM25_LENGTH_EDGES = (
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
    16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
    32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62,
    64, 68, 72, 76, 80, 84, 88, 92, 96, 100, 104, 108, 112, 116, 120, 124,
    128, 136, 144, 152, 160, 168, 176, 184, 192, 200, 208, 216, 224, 232, 240, 248,
    256, 272, 288, 304, 320, 336, 352, 368, 384, 400, 416, 432, 448, 464, 480, 496,
    512, 544, 576, 608, 640, 672, 704, 736, 768, 800, 832, 864, 896, 928, 960, 992,
    1024, 1088, 1152, 1216, 1280, 1344, 1408, 1472, 1536, 1600, 1664, 1728, 1792, 1856, 1920, 1984,
    2048, 2176, 2304, 2432, 2560, 2688, 2816, 2944, 3072, 3200, 3328, 3456, 3584, 3712, 3840, 3968,
    4096, 4352, 4608, 4864, 5120, 5376, 5632, 5888, 6144, 6400, 6656, 6912, 7168, 7424, 7680, 7936,
    8192, 8704, 9216, 9728, 10240, 10752, 11264, 11776, 12288, 12800, 13312, 13824, 14336, 14848, 15360, 15872,
    16384, 17408, 18432, 19456, 20480, 21504, 22528, 23552, 24576, 25600, 26624, 27648, 28672, 29696, 30720, 31744,
    32768, 34816, 36864, 38912, 40960, 43008, 45056, 47104, 49152, 51200, 53248, 55296, 57344, 59392, 61440, 63488,
    65536, 69632, 73728, 77824, 81920, 86016, 90112, 94208, 98304, 102400, 106496, 110592, 114688, 118784, 122880, 126976,
    131072, 139264, 147456, 155648, 163840, 172032, 180224, 188416, 196608, 204800, 212992, 221184, 229376, 237568, 245760,
    253952, 262144, 278528, 294912, 311296, 327680, 344064, 360448, 376832, 393216, 409600, 425984, 442368, 458752, 475136,
    491520, 507904,
)


def bm25_norms(doc_lens):
    """The norm byte of every document for topk_scored_batch_dev: doc_lens (non-negative integers, one per document id)
    -> np.uint8, the class c of a length l being the last one with BM25_LENGTH_EDGES[c] <= l (np.searchsorted over the
    edges, integers throughout).  Longer documents never get a smaller class; bm25_table takes the class's lower edge as
    the length of all of its documents."""
    lens = np.asarray(doc_lens)
    if lens.ndim != 1 or (lens.size and lens.dtype.kind not in "ui"):
        raise ValueError("doc_lens must be a flat sequence of integers")
    if lens.size and int(lens.min()) < 0:
        raise ValueError("doc_lens must not be negative")
    edges = np.array(BM25_LENGTH_EDGES, dtype=np.uint64)
    return (np.searchsorted(edges, lens.astype(np.uint64), side="right") - 1).astype(np.uint8)


def sortable_u32(array):
    """An int32 or float32 array -> np.uint32 of the same shape whose unsigned order is the order of the values, so that
    the one uint32 comparison of topk_filter_batch_dev serves dates, prices and floats; bounds go through the same map.
    int32: the sign bit flipped.  float32: a set sign bit flips every bit, a clear one only the sign bit -- so
    -inf < ... < -0.0 < +0.0 < ... < +inf -- and every NaN, whatever its sign and payload, goes to 0xFFFFFFFF, above
    +inf (where np.sort puts it)."""
    a = np.asarray(array)
    if a.dtype == np.int32:
        return a.view(np.uint32) ^ np.uint32(0x80000000)
    if a.dtype == np.float32:
        b = np.ascontiguousarray(a).view(np.uint32)
        out = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
        return np.where(np.isnan(a), np.uint32(0xFFFFFFFF), out).astype(np.uint32)
    raise ValueError("sortable_u32 takes an int32 or float32 array, got %s" % (a.dtype,))


def bm25_table(avgdl, k1=1.2, b=0.75, tf_rows=64, bits=16):
    """The impact table of BM25 for topk_scored_batch_dev: np.uint32 of shape (tf_rows, 256), table[t][c] the quantised
    term-frequency part of a posting with payload t in a document of class c (bm25_norms).  Row 0 is zero, and for t >= 1
      table[t][c] = round((2^bits - 1) / (k1 + 1) * t * (k1 + 1) / (t + k1 * (1 - b + b * rep(c) / avgdl)))
    in float64, rep(c) = BM25_LENGTH_EDGES[c], the class's lower edge.  The BM25 factor t (k1 + 1) / (t + ...) lies below
    k1 + 1, so every entry lies below 2^bits; bits <= 24, so that an IDF weight of up to 8 bits cannot saturate one
    posting.  The IDF is not in the table: it is the caller's weight of the term.  A payload of tf_rows or more scores as
    tf_rows - 1 (the factor is within k1 / (tf_rows + k1) of its limit there)."""
    for name, v, lo, hi in (("tf_rows", tf_rows, 1, 256), ("bits", bits, 1, 24)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    avgdl, k1, b = float(avgdl), float(k1), float(b)
    if not (avgdl > 0 and np.isfinite(avgdl)) or not (k1 >= 0 and np.isfinite(k1)) or not 0 <= b <= 1:
        raise ValueError("bm25_table needs avgdl > 0, k1 >= 0 and b in [0, 1]")
    t = np.arange(tf_rows, dtype=np.float64)[:, None]
    rep = np.array(BM25_LENGTH_EDGES, dtype=np.float64)[None, :]
    scale = (2.0 ** bits - 1.0) / (k1 + 1.0)
    table = np.zeros((tf_rows, 256), dtype=np.float64)
    table[1:] = np.floor(scale * t[1:] * (k1 + 1.0) / (t[1:] + k1 * (1.0 - b + b * rep / avgdl)) + 0.5)
    return table.astype(np.uint32)


def unpack_restart_points(raw):
    """29-byte restart points -> (cursors u32[n], states u64[n * 4]): states 0, 1 as one 104-bit little-endian
    integer in bytes 0..12, states 2, 3 in bytes 13..25 (52 bits each), the cursor in bytes 26..28."""
    rec = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, 29).astype(np.uint64)
    n = rec.shape[0]
    st = np.zeros((n, 4), dtype=np.uint64)
    m52 = np.uint64((1 << 52) - 1)
    for pair in range(2):
        b = rec[:, 13 * pair: 13 * pair + 13]
        lo = np.zeros(n, dtype=np.uint64)
        for i in range(8):
            lo |= b[:, i] << np.uint64(8 * i)
        hi = np.zeros(n, dtype=np.uint64)
        for i in range(5):
            hi |= b[:, 8 + i] << np.uint64(8 * i)
        st[:, 2 * pair] = lo & m52
        st[:, 2 * pair + 1] = (lo >> np.uint64(52)) | (hi << np.uint64(12))
    off = (rec[:, 26] | (rec[:, 27] << np.uint64(8)) | (rec[:, 28] << np.uint64(16))).astype(np.uint32)
    return off, st.reshape(-1)


def parse_container(buf):
    """Split a container (np.uint8) into header fields, per-block streams and restart points."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    H = L.ContainerHeader()
    st = L.lib().ansx_container_info(buf.ctypes.data, buf.size, C.byref(H))
    if st != L.OK:
        raise L.AnsxError(st, "ansx_container_info")
    nb = H.nblocks
    idx_off = C.sizeof(L.ContainerHeader)
    boff = np.frombuffer(buf[idx_off: idx_off + 8 * (nb + 1)].tobytes(), dtype=np.uint64)
    ck_off_off = idx_off + 8 * (nb + 1)
    nck = nb * H.ckpts_per_block
    if H.kind & 0x200:  # wide restart points: u32 cursors, then 4 x u64 states (the v2 form)
        ck_off = np.frombuffer(buf[ck_off_off: ck_off_off + 4 * nck].tobytes(), dtype=np.uint32)
        ck_state_off = (ck_off_off + 4 * nck + 7) // 8 * 8
        ck_state = np.frombuffer(buf[ck_state_off: ck_state_off + 32 * nck].tobytes(), dtype=np.uint64)
        hint_off = (ck_state_off + 32 * nck + 15) // 16 * 16
    else:  # packed 29-byte records
        ck_off, ck_state = unpack_restart_points(buf[ck_off_off: ck_off_off + 29 * nck])
        hint_off = (ck_off_off + 29 * nck + 15) // 16 * 16
    hints = np.frombuffer(buf[hint_off: hint_off + 32 * nb].tobytes(), dtype=np.uint32).reshape(nb, 8)
    p0 = int(H.payload_offset)
    streams = [buf[p0 + int(boff[i]): p0 + int(boff[i + 1])] for i in range(nb)]
    return {
        "header": H, "block_off": boff, "streams": streams, "parse_hints": hints,
        "ckpt_off": ck_off.reshape(nb, H.ckpts_per_block) if nck else ck_off.reshape(nb, 0),
        "ckpt_state": ck_state.reshape(nb, H.ckpts_per_block, 4) if nck else ck_state.reshape(nb, 0, 4),
    }


# ---------------------------------------------------------------- synthetic inputs (generate_inputs.cpp)

def parse_dist(spec):
    """'uniform<lo>-<hi>' | 'uniform<bits>' (0 .. 2^bits - 1, generate_inputs.cpp:94-101) | 'geom<p>' |
    'zipf<log2 n>[s<q>]' (values 1 .. 2^log2n, exponent q, default 1.0 as zipf_dist.hpp:39-40)
    -> (dist, a, b)"""
    if spec.startswith("uniform"):
        body = spec[7:]
        if "-" in body:
            lo, hi = body.split("-")
            return L.GEN_UNIFORM, float(int(lo)), float(int(hi))
        return L.GEN_UNIFORM, 0.0, float((1 << int(body)) - 1)
    if spec.startswith("geom"):
        return L.GEN_GEOMETRIC, float(spec[4:]), 0.0
    if spec.startswith("zipf"):
        body = spec[4:]
        lg, q = (body.split("s") + ["1.0"])[:2] if "s" in body else (body, "1.0")
        return L.GEN_ZIPF, float(1 << int(lg)), float(q)
    raise ValueError("unknown distribution %r" % (spec,))


def generate_host(spec, n, seed=0, first_index=0):
    """n values of the named distribution on the CPU (same values as generate_dev)."""
    dist, a, b = parse_dist(spec)
    out = np.empty(n, dtype=np.uint32)
    st = L.lib().ansx_generate_host(dist, a, b, seed, first_index, out.ctypes.data, n)
    if st != L.OK:
        raise L.AnsxError(st, "ansx_generate_host")
    return out


def zipf_from_uniform(n, q, u01):
    """(value, accepted) of one pass of the Zipf generator's rejection loop for the canonical uniform u01."""
    import ctypes as C

    k, acc = C.c_uint32(0), C.c_int(0)
    st = L.lib().ansx_zipf_from_uniform(float(n), float(q), float(u01), C.byref(k), C.byref(acc))
    if st != L.OK:
        raise L.AnsxError(st, "ansx_zipf_from_uniform")
    return int(k.value), bool(acc.value)


def generate_dev(ctx, spec, out_ptr, n, seed=0, first_index=0, stream=None):
    """Fill device memory at out_ptr (n x uint32) with the named distribution; asynchronous on `stream`."""
    dist, a, b = parse_dist(spec)
    st = L.lib().ansx_generate_dev(ctx.handle, dist, a, b, seed, first_index, out_ptr, n, stream)
    if st != L.OK:
        raise L.AnsxError(st, "ansx_generate_dev")
