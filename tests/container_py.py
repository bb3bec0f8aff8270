"""Pure-Python builder of the ansx container from ORACLE block streams (test infrastructure):
an independent statement of the container layout documented in DESIGN.md section 3."""
import struct

import numpy as np

import oracle_lib as ol

MAGIC = b"ANSXv3"


def nseg(nb, ckpt):
    nfull = nb - (nb & 3)
    if ckpt == 0 or nfull == 0:
        return 1
    return (nfull + ckpt - 1) // ckpt


NSP = {0: lambda f: 1 << (f + 9), 1: lambda f: 1 << (f + 9), 2: lambda f: 2048, 3: lambda f: 16384}  # symbol-row stride per codec


def block_bound(kind, f, block, compact=False):
    """Worst-case bytes of one block stream: hdr + 8 + 4 NSP + 7 block + 32, where ANSrfold's hdr is
    its most-frequent table, 4 + 4 T with T = 2^(f + 7), and compaction adds the alphabet header, 8 + 4 block + 8."""
    k = kind & 0xFF
    hdr = 4 + 4 * (1 << (f + 7)) if k == 1 else 0
    if compact:
        hdr += 8 + 4 * block + 8
    return hdr + 8 + 4 * NSP[k](f) + 7 * block + 32


def wide_by_geometry(kind, f, block, compact=False):
    """The cursor rule: a restart cursor has 24 bits in the packed form, so a geometry whose worst-case block stream
    (+ 16 bytes of slack) reaches 2^24 takes the wide form -- decided from block_ints alone, never from the streams."""
    return block_bound(kind, f, block, compact) + 16 >= 1 << 24


def scratch_stride(kind, f, block, compact=False):
    """Bytes between two blocks' slots in the encoder's stream scratch: the bound + 16, rounded up to 256."""
    return (block_bound(kind, f, block, compact) + 16 + 255) // 256 * 256


def first_block_ints(reached, multiple=4):
    """The smallest block_ints (a multiple of `multiple`) at which the monotone predicate reached(block_ints) holds."""
    lo, hi = 0, 1 << 31
    while hi - lo > multiple:
        mid = (lo + hi) // 2 // multiple * multiple
        lo, hi = (lo, mid) if reached(mid) else (mid, hi)
    return hi


def layout(nblocks, nckf, wide):
    """Section offsets of a container: (index, restart cursors / records, wide states, parse hints, payload)."""
    index_off = 64
    ckoff_off = index_off + 8 * (nblocks + 1)
    if wide:
        ckstate_off = (ckoff_off + 4 * nblocks * nckf + 7) // 8 * 8
        hint_off = (ckstate_off + 32 * nblocks * nckf + 15) // 16 * 16
    else:
        ckstate_off = ckoff_off
        hint_off = (ckoff_off + 29 * nblocks * nckf + 15) // 16 * 16
    return index_off, ckoff_off, ckstate_off, hint_off, hint_off + 32 * nblocks


def pack_restart_points(states, offs):
    """(n, 4) u64 states + n u32 cursors -> n records of 29 bytes: states 0, 1 as one 104-bit little-endian integer
    (state 0 in the low 52 bits), states 2, 3 likewise, then the cursor in 24 bits."""
    out = bytearray()
    for st, off in zip(states.tolist(), offs.tolist()):
        assert all(x < (1 << 52) for x in st) and off < (1 << 24)
        out += (st[0] | (st[1] << 52)).to_bytes(13, "little")
        out += (st[2] | (st[3] << 52)).to_bytes(13, "little")
        out += off.to_bytes(3, "little")
    return np.frombuffer(bytes(out), dtype=np.uint8)


def build_container(kind, f, data, block, ckpt, wide=None):
    """wide: restart-point format; None = what the library picks: wide for ANSint, for a geometry whose worst-case block
    stream reaches 2^24 bytes (wide_by_geometry) and once a frame exceeds 2^16."""
    data = np.ascontiguousarray(data, dtype=np.uint32)
    n = data.size
    if ckpt >= block:
        ckpt = 0
    nblocks = (n + block - 1) // block
    nckf = nseg(block, ckpt) - 1
    streams, cks, cko, hints, maxlg, maxns, maxsig = [], [], [], [], 0, 0, 0
    for b in range(nblocks):
        s, info, st, off = ol.oracle_encode(kind, f, data[b * block:(b + 1) * block], ckpt_interval=ckpt)
        streams.append(s)
        hints.append(ol.prelude_hints(s, info.header_bytes))
        pad_s = np.zeros((nckf, 4), dtype=np.uint64)
        pad_o = np.zeros(nckf, dtype=np.uint32)
        pad_s[:st.shape[0]] = st
        pad_o[:off.shape[0]] = off
        cks.append(pad_s)
        cko.append(pad_o)
        maxlg = max(maxlg, info.log2_frame)
        maxns = max(maxns, info.max_sym + 1)
        maxsig = max(maxsig, int(info.present_syms))  # symbols present in the block's model
    if (kind & 0x1FF) == 3:  # plain ANSint: no parse hints, max_nsyms bounds a block's distinct values (dense and rank-space model alike)
        hints = [np.zeros(8, dtype=np.uint32) for _ in hints]
        maxns = maxsig
    if wide is None:
        wide = (kind & 0xFF) == 3 or wide_by_geometry(kind, f, block, bool(kind & 0x100)) or maxlg > 16
    index_off, ckoff_off, ckstate_off, hint_off, payload_off = layout(nblocks, nckf, wide)
    sizes = np.array([s.size for s in streams], dtype=np.uint64)
    boff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    payload = np.concatenate(streams)
    out = np.zeros(payload_off + payload.size, dtype=np.uint8)
    hdr = MAGIC + struct.pack("<HIIQIIIIIIQQ", max(maxsig, 1) - 1, kind | (0x200 if wide else 0), f, n, block, ckpt, nblocks, maxlg, maxns, nckf,
                              int(payload.size), payload_off)
    out[:64] = np.frombuffer(hdr, dtype=np.uint8)
    out[index_off:index_off + 8 * (nblocks + 1)] = boff.view(np.uint8)
    if nckf and wide:
        out[ckoff_off:ckoff_off + 4 * nblocks * nckf] = np.concatenate(cko).view(np.uint8)
        out[ckstate_off:ckstate_off + 32 * nblocks * nckf] = np.concatenate(cks).reshape(-1).view(np.uint8)
    elif nckf:
        out[ckoff_off:ckoff_off + 29 * nblocks * nckf] = pack_restart_points(np.concatenate(cks), np.concatenate(cko))
    out[hint_off:hint_off + 32 * nblocks] = np.concatenate(hints).view(np.uint8)
    out[payload_off:] = payload
    return out
