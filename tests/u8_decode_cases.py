"""Decode to UTF-16 on the device (tkz_decode_batch_utf16 / _device: the k_dec_* family, then k_u8_len / k_u8_write / k_u8_docoffs) at the tile, lane-group
and bitmap-word edges of the BYTES: a plain reference in pure Python, the positioned case generators and the comparisons the emulated (CPU) and the GPU test
modules share.  Every comparison is exact equality of code units and unit offsets.

The reference restates Encoding.UTF8.GetString (.NET Core 3.0+; WHATWG TextDecoder("utf-8")) one byte at a time and knows nothing of tiles:
  get_string(bytes)      the code units of ONE document: a well-formed sequence (Unicode table 3-7) is one unit, a 4-byte one a pair; every maximal subpart of
                         an ill-formed sequence is one U+FFFD
  python_codec(bytes)    what Python's own codec makes of the same bytes: the check that keeps get_string from drifting
The expected result of a batch is u16_cases.decode_ids(...) of every document followed by get_string.

The constants are the kernels' (tests/test_emu_u8_decode.py::test_constants_are_the_kernels reads them back out of the sources):
  TILE   1024   tkz_kernels.hip: kU8Tile -- bytes per wavefront
  GROUP    16   tkz_kernels.hip: kU8Lane -- ... per lane; grp_prefix holds one entry per group, k_u8_docoffs walks the rest
WORD, WG_TILES and SCAN_BLOCK are u16_cases': the bitmap word of the document starts, the tiles of a workgroup, the tiles of a scan workgroup.

The positioned sweeps.  Both tables hold all 256 single-byte keys, so a batch of single-byte ids puts byte q at id q.  A sweep case places ONE probe, at one
distance in front of the edge and with one kind of document boundary, at EVERY edge e of the sweep inside one batch: the edges are at least 16 bytes apart and a
probe reaches at most 3 bytes either side of its edge, so the probes never meet, and the filler between them (period 55) faces every edge in another phase.
"""
import ctypes as C
import functools
import random
import zlib

import numpy as np

import u16_cases as U
from tokenizer_amd import _native as N

TILE, GROUP = 1024, 16
WORD, WG_TILES, SCAN_BLOCK = U.WORD, U.WG_TILES, U.SCAN_BLOCK
WG_BYTES = WG_TILES * TILE
# 1-, 2- and 3-byte chars; 55 bytes: a period that shares no factor with 16
FILLER = "the quïck bröwn 中文 fox it's 12 €, naïve →x\n!".encode("utf-8")
assert len(FILLER) == 55 and {1, 2, 3} == {len(c.encode("utf-8")) for c in FILLER.decode("utf-8")}
# the bytes at which table 3-7 changes its answer, and ASCII
BOUNDARY = bytes.fromhex("80 8F 90 9F A0 BF C0 C1 C2 DF E0 E1 ED EF F0 F1 F4 F5 FF") + b"Az"
PROBES = [bytes.fromhex(h) for h in ("C3 A9", "E4 B8 AD", "F0 9F 98 80", "E4 B8 41", "F0 9F 98 41", "E0 80 80", "ED A0 80", "F0 8F 80 80", "F4 90 80 80",
                                     "C0 80", "F5 80", "80 80")]
BACKS = (1, 2, 3)                  # the probe's first byte is at e - 1, e - 2, e - 3
KINDS = U.PAIR_KINDS               # inside one document; a document boundary at e; an empty document at e
# the issue's examples and the Unicode standard's own (3.9, table 3-11), as literals
HAND = [("F0 90 41", [0xFFFD, 0x41]), ("E0 80", [0xFFFD, 0xFFFD]), ("ED A0 80", [0xFFFD] * 3), ("F4 90 80 80", [0xFFFD] * 4), ("E4 B8", [0xFFFD]),
        ("C0", [0xFFFD]), ("C1", [0xFFFD]), ("F5", [0xFFFD]), ("FF", [0xFFFD]), ("80", [0xFFFD]), ("BF", [0xFFFD]),
        ("41 C3 A9 E4 B8 AD F0 9F 98 80", [0x41, 0xE9, 0x4E2D, 0xD83D, 0xDE00]), ("F4 8F BF BF", [0xDBFF, 0xDFFF]), ("F0 90 80 80", [0xD800, 0xDC00]),
        ("EF BF BD", [0xFFFD]), ("ED 9F BF EE 80 80", [0xD7FF, 0xE000]),
        ("61 F1 80 80 E1 80 C2 62 80 63 80 BF 64", [0x61, 0xFFFD, 0xFFFD, 0xFFFD, 0x62, 0xFFFD, 0x63, 0xFFFD, 0xFFFD, 0x64])]


# ---- the plain reference --------------------------------------------------------------------------------------------------------------------------------

def _need(b):
    return 1 if 0xC2 <= b <= 0xDF else 2 if 0xE0 <= b <= 0xEF else 3 if 0xF0 <= b <= 0xF4 else 0


def _second(lead):
    return {0xE0: (0xA0, 0xBF), 0xED: (0x80, 0x9F), 0xF0: (0x90, 0xBF), 0xF4: (0x80, 0x8F)}.get(lead, (0x80, 0xBF))


def get_string(data):
    """Encoding.UTF8.GetString, one byte at a time, on the bytes of ONE document: the list of code units."""
    out = []
    n = len(data)
    i = 0
    while i < n:
        b = data[i]
        i += 1
        if b < 0x80:
            out.append(b)
            continue
        need = _need(b)
        cp, got = b & (0x3F >> need), 0
        while got < need and i < n:                  # the longest prefix of a well-formed sequence that is present
            lo, hi = _second(b) if got == 0 else (0x80, 0xBF)
            if not lo <= data[i] <= hi:
                break
            cp = (cp << 6) | (data[i] & 0x3F)
            i += 1
            got += 1
        if need == 0 or got < need:                  # a byte that starts nothing, or a maximal subpart: one U+FFFD, and on right behind it
            out.append(0xFFFD)
        elif cp >= 0x10000:
            out += [0xD800 + ((cp - 0x10000) >> 10), 0xDC00 + ((cp - 0x10000) & 0x3FF)]
        else:
            out.append(cp)
    return out


def python_codec(data):
    return np.frombuffer(bytes(data).decode("utf-8", "replace").encode("utf-16-le"), "<u2").tolist()


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------------

def byte_ids(S):
    """byte value -> the id of its single-byte key, as an int32 lookup array"""
    one = {k[0]: i for i, k in S.key_of.items() if len(k) == 1}
    assert len(one) == 256, "the table does not hold all 256 single-byte keys"
    return np.asarray([one[b] for b in range(256)], np.int32)


def filler(n, phase=0):
    return bytearray(FILLER[(phase + i) % len(FILLER)] for i in range(n))


def offsets_of(n, starts):
    """starts: the position of every document start BEHIND the first one, in order; a position that repeats is an empty document"""
    offs = [0] + list(starts) + [n]
    assert all(a <= b for a, b in zip(offs, offs[1:])), offs
    return offs


def bytes_case(S, name, flat, starts=()):
    """a batch of single-byte ids: byte position = id position"""
    return U.DecodeCase(name, byte_ids(S)[np.frombuffer(bytes(flat), np.uint8)], offsets_of(len(flat), starts))


def sweep_edges(step):
    """step 64: every multiple of 64 up to a workgroup and a word beyond it, and the group edges 16, 32 and 48 inside the first and the last word of a tile
    and of a workgroup.  step 16: every multiple of 16 up to a workgroup and a group beyond it."""
    if step == WORD:
        inner = {w + g for w in (0, TILE - WORD, TILE, WG_BYTES - WORD, WG_BYTES) for g in (16, 32, 48)}
        return sorted(set(range(WORD, WG_BYTES + WORD + 1, WORD)) | inner)
    assert step == GROUP
    return list(range(GROUP, WG_BYTES + GROUP + 1, GROUP))


def sweep_case(S, probe, back, kind, edges):
    n = edges[-1] + 40
    flat = filler(n, phase=len(probe) + back)
    starts = []
    for e in edges:
        flat[e - back:e - back + len(probe)] = probe
        starts += {"inside": [], "boundary": [e], "empty": [e, e]}[kind]
    return bytes_case(S, "probe_%s_first_byte_at_edge_minus_%d_%s_at_%d_edges_up_to_%d" % (probe.hex(), back, kind, len(edges), edges[-1]), flat, starts)


def sweep_cases(S, kind, step):
    edges = sweep_edges(step)
    return [sweep_case(S, p, back, kind, edges) for p in PROBES for back in BACKS]


def split_keys(S):
    """(prefix id, rest ids, the char's bytes) for a 3- and a 4-byte char: a multi-byte key that is a proper prefix of the char, then the rest -- one key when the
    table has it, single-byte keys otherwise."""
    ids_of = {k: i for i, k in S.key_of.items()}
    out = {}
    for k, i in sorted(ids_of.items()):
        if len(k) in (2, 3) and _need(k[0]) > len(k) - 1 and get_string(k) == [0xFFFD]:          # a proper prefix, 2 or 3 bytes long, of a well-formed char
            rest = bytes([0xAD] * (_need(k[0]) + 1 - len(k)))
            assert len(get_string(k + rest)) in (1, 2) and get_string(k + rest)[0] != 0xFFFD
            out.setdefault(_need(k[0]) + 1, (i, [ids_of[rest]] if rest in ids_of else [ids_of[bytes([b])] for b in rest], k + rest))
    return out


def split_char_cases(S):
    """The ordinary cause of ill-formed bytes: a char split across two keys.  The prefix key ends at the tile edge / one byte into the next tile; in one document
    (the char is whole), and as the last ids of a document (a prefix, then stray continuation bytes)."""
    lut = byte_ids(S)
    out = []
    for nbytes, (pid, rest, char) in sorted(split_keys(S).items()):
        plen = len(S.key_of[pid])
        for edge in (TILE, TILE + 1, 2 * TILE - 1):
            head = lut[np.frombuffer(bytes(filler(edge - plen, phase=nbytes)), np.uint8)].tolist()
            tail = lut[np.frombuffer(bytes(filler(TILE + 7, phase=3)), np.uint8)].tolist()
            ids = head + [pid] + rest + tail
            cut = len(head) + 1
            out.append(U.DecodeCase("split_%d_byte_char_prefix_key_ends_at_%d_one_document" % (nbytes, edge), ids, [0, len(ids)]))
            out.append(U.DecodeCase("split_%d_byte_char_prefix_key_ends_at_%d_last_id_of_its_document" % (nbytes, edge), ids, [0, cut, len(ids)]))
            out.append(U.DecodeCase("split_%d_byte_char_prefix_key_ends_at_%d_empty_document_behind_it" % (nbytes, edge), ids, [0, cut, cut, len(ids)]))
        out.append(U.DecodeCase("split_%d_byte_char_prefix_key_is_the_last_id" % nbytes, head + [pid], [0, 5, len(head) + 1]))
    return out


RAGGED_TOTALS = (1, 15, 16, 17, 1023, 1024, 1025, 4095, 4097)


def ragged_tail_cases(S):
    """totals that end in a truncated 4-byte prefix of 1, 2 or 3 bytes"""
    out = []
    for t in RAGGED_TOTALS:
        cut = min(t, 1 + t % 3)
        flat = filler(t, phase=t)
        flat[t - cut:] = bytes.fromhex("F0 9F 98")[:cut]
        out.append(bytes_case(S, "ragged_tail_%d_bytes_ends_in_%d_of_4" % (t, cut), flat, [] if t % 2 else [t // 2]))
    assert {c.ids.size for c in out} == set(RAGGED_TOTALS)
    return out


def unit_extreme_cases(S):
    """A tile of 256 four-byte chars (1024 four-byte-sequence bytes: 512 units) between two tiles of ASCII (1024 units each); and the most a tile can yield:
    1023 ASCII bytes and the lead of a 4-byte char, whose pair counts for the tile of the lead (1025 units)."""
    emoji = bytes.fromhex("F0 9F 98 80")
    a = bytearray(b"ab" * (TILE // 2)) + bytearray(emoji * (TILE // 4)) + bytearray(b"cd" * (TILE // 2 + 3))
    b = bytearray(b"x" * (TILE - 1)) + bytearray(emoji) + bytearray(b"y" * (TILE - 4)) + bytearray(emoji) + bytearray(b"z" * 5)
    return [bytes_case(S, "tile_of_four_byte_chars_between_tiles_of_ascii", a, [TILE, TILE + 6, 2 * TILE]),
            bytes_case(S, "tile_of_1025_units_lead_in_its_last_byte", b), bytes_case(S, "tile_of_1025_units_lead_cut_off_by_a_boundary", b, [TILE])]


def odd_shape_cases(S):
    unknown, one_in_last = U.odd_shape_cases(S)
    return [unknown, one_in_last, U.DecodeCase("all_documents_empty", [], [0, 0, 0, 0]), U.DecodeCase("one_empty_document", [], [0, 0])]


def scan_edge_case(S):
    """SCAN_BLOCK + 1 byte tiles: a second workgroup takes part in the scan of the tile sums.  A block of soup and filler (1021 bytes: no multiple of a group)
    repeated, cut into documents inside groups."""
    rng = random.Random(7)
    block = filler(1021, phase=9)
    for q in range(0, 1021, 29):
        block[q:q + 3] = bytes(rng.choice(BOUNDARY) for _ in range(3))
    total = SCAN_BLOCK * TILE + 3
    flat = np.resize(np.frombuffer(bytes(block), np.uint8), total)
    offs = [0, 5, SCAN_BLOCK * TILE // 2 + 9, total - TILE - 1, total - 2, total]
    return U.DecodeCase("scan_block_edge_%d_byte_tiles" % (SCAN_BLOCK + 1), byte_ids(S)[flat], offs)


def soup_cases(S, seed=20250117):
    """the boundary alphabet everywhere, cut into documents of 0..40 bytes: three tiles"""
    rng = random.Random(seed)
    flat = bytes(rng.choice(BOUNDARY) for _ in range(3 * TILE + 5))
    starts, p = [], 0
    while True:
        p += rng.choice((0, 1, 2, 3, 5, 16, 17, 40))
        if p >= len(flat): break
        starts.append(p)
    return [bytes_case(S, "boundary_soup_one_document", flat), bytes_case(S, "boundary_soup_cut_into_short_documents", flat, starts)]


def quick_cases(S):
    """what the mirrors and the capacity checks run on: a few of every kind"""
    edges = sweep_edges(WORD)
    return [sweep_case(S, PROBES[2], 1, "boundary", edges), sweep_case(S, PROBES[4], 3, "inside", edges)] + ragged_tail_cases(S)[3:7] + soup_cases(S) + \
        unit_extreme_cases(S)[:2]


# ---- the comparisons --------------------------------------------------------------------------------------------------------------------------------------

def documents(S, case):
    """the decoded bytes of every document"""
    return [U.decode_ids(case.ids[int(a):int(b)], S.key_of, S.specials) for a, b in zip(case.offs, case.offs[1:])]


def expect(S, case):
    """(units uint16, unit offsets) of the reference, computed once per table and case"""
    cache = S.__dict__.setdefault("_u8_expect", {})
    key = (case.name, zlib.crc32(case.ids.tobytes()), zlib.crc32(case.offs.tobytes()))          # (the batch itself: two cases may share a name)
    if key not in cache:
        parts = [get_string(d) for d in documents(S, case)]
        cache[key] = (np.asarray([u for p in parts for u in p], np.uint16), np.cumsum([0] + [len(p) for p in parts]).tolist())
    return cache[key]


def decode_raw(enc, ids, offs, cap):
    """tkz_decode_batch_utf16 with room for `cap` units: (status, needed, units, offsets)."""
    ids = np.ascontiguousarray(ids, np.int32)
    offs = np.ascontiguousarray(offs, np.int64)
    out = np.full(max(1, cap) + 8, 0xAAAA, np.uint16)
    ooff = np.empty(len(offs), np.int64)
    needed = C.c_int64(0)
    st = enc.lib.L.tkz_decode_batch_utf16(enc._h, ids.ctypes.data if len(ids) else None, offs.ctypes.data, len(offs) - 1, out.ctypes.data, cap, ooff.ctypes.data,
                                          C.byref(needed))
    return st, needed.value, out, ooff


def check_case(enc, S, case, device=None):
    """Units and offsets against decode_ids + get_string; device(ids, offs, cap) -> (units, offsets), when given, is a second entry that must agree."""
    want, woffs = expect(S, case)
    st, needed, out, ooff = decode_raw(enc, case.ids, case.offs, len(want))                      # (a capacity of exactly the reference length)
    assert (st, needed) == (N.OK, len(want)), (case, st, needed, len(want))
    assert ooff.tolist() == woffs, "%r: unit offsets differ at document %d" % (case, U.first_diff(ooff.tolist(), woffs))
    got = out[:needed]
    assert np.array_equal(got, want), "%r: units differ at %d" % (case, U.first_diff(got.tolist(), want.tolist()))
    assert (out[needed:] == 0xAAAA).all(), "%r: units behind the result were written" % (case,)
    out2, ooff2 = enc.decode_batch_utf16(case.ids, case.offs)                                    # (the wrapper's own capacity: a hint larger than the result)
    assert np.array_equal(out2, want) and ooff2.tolist() == woffs, case
    if device is not None:
        out3, ooff3 = device(case.ids, case.offs, len(want) + 3)
        assert ooff3.tolist() == woffs and np.array_equal(out3, want), "%r: the device entry differs" % (case,)
    return len(want)


def check_capacity(enc, S, case):
    """one unit short, half, none: E_CAPACITY and the exact unit total; then the call with exactly that many succeeds"""
    want, woffs = expect(S, case)
    assert len(want) > TILE
    for cap in (len(want) - 1, len(want) // 2, 0):
        st, needed, out, _ = decode_raw(enc, case.ids, case.offs, cap)
        assert (st, needed) == (N.E_CAPACITY, len(want)), (case, cap, st, needed, len(want))
        assert (out[cap:] == 0xAAAA).all()
    st, needed, out, ooff = decode_raw(enc, case.ids, case.offs, needed)
    assert (st, needed) == (N.OK, len(want)) and np.array_equal(out[:needed], want) and ooff.tolist() == woffs
    try:
        enc.decode_batch_utf16(case.ids, case.offs, out_cap=len(want) - 1)
        raise AssertionError("one unit short did not raise")
    except N.TkzError as ex:
        assert ex.code == N.E_CAPACITY


def check_bad_offsets(enc, S):
    ids = byte_ids(S)[np.frombuffer(bytes(filler(40)), np.uint8)]
    for offs in ([1, 40], [0, 30, 20, 40], [0, -1, 40], [0, 41, 40]):
        st, _, _, _ = decode_raw(enc, ids, offs, 64)
        assert st == N.E_ARG, (offs, st)
    check_case(enc, S, bytes_case(S, "after_bad_offsets", filler(40), [7]))                     # (and the encoder serves the next call as before)
