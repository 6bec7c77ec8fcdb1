"""Packed rows (tkz_encode_batch_packed_device / _utf8 / _utf16; k_pack_count, k_pack_write): the cases and comparisons the emulated (CPU) and the GPU test modules
share.  Every comparison is exact.

No expected value comes from the code under test.  The model (`Model`) is numpy over the ORACLE's ids -- oracle.Encoder, the special-token form where literals are
allowed; TrimOracle's literal search for UTF-16 text with lone surrogates (u16_special_cases.Expect) -- and builds the stream, s, the rows, the segment starts and
pos from the rule of tkz.h.  It never reads the library's own encode output.

The kernel cases go through tkz_encode_batch_packed_device.  `upload(np_array) -> (owner, pointer)` as in count_cases: identity for the emulated build, a device
tensor on the hardware.  Every output buffer carries GUARD words behind the capacity the call is told, and they must be intact afterwards.

Geometry (tkz_kernels.h): a wavefront per tile of K = kPackTile stream positions, four wavefronts a workgroup, at most GRID workgroups.  Documents are short words
of one token each (" the", " of" ...: keys of the tables the tests use), so a case is a few tens of KB.
"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import count_cases as CC
import parity
import spans_cases as SP
import special_cases as SC
import u16_cases as U16
import u16_special_cases as U16S
from conftest import ROOT
from tokenizer_amd import _native as N

_HEAD = open(os.path.join(ROOT, "tokenizer_amd", "csrc", "tkz_kernels.h")).read()
K = int(re.search(r"\bkPackTile = (\d+)\b", _HEAD).group(1))
GRID = int(re.search(r"\bkPackGridMax = (\d+)\b", _HEAD).group(1))
EOT = SC.EOT
EOT_ID = SP.EOT_ID
EMOJI = "\U0001F600"
GUARD = 8
FORMS = ((-1, -1), (7, -1), (-1, 9), (7, 9))          # none, bos only, eos only, both


def words(rng, n):
    """a document of exactly n tokens: n words with the blank in front of each"""
    return "".join(" " + rng.choice(CC.WORDS) for _ in range(n)).encode()


class Model:
    """the rule of tkz.h over the oracle's ids of every document"""

    def __init__(self, ids_per_doc, L, bos=-1, eos=-1, pad=0):
        fb, fe = bos >= 0, eos >= 0
        stream, s = [], [0]
        for di in ids_per_doc:
            stream += ([bos] if fb else []) + list(di) + ([eos] if fe else [])
            s.append(len(stream))
        self.T, self.offs = len(stream), s
        self.n_rows = -(-self.T // L)
        self.ids = np.full(self.n_rows * L, pad, np.int64)
        self.ids[:self.T] = stream
        starts = set(range(0, self.T, L)) | {s[d] for d in range(len(ids_per_doc)) if s[d + 1] > s[d]}
        self.seg = sorted(starts) + [self.T]
        self.n_segs = len(starts)
        self.pos = np.zeros(self.n_rows * L, np.int64)
        if self.T:
            first = np.asarray(self.seg[:-1], np.int64)
            t = np.arange(self.T, dtype=np.int64)
            self.pos[:self.T] = t - first[np.searchsorted(first, t, side="right") - 1]
        assert self.n_segs <= self.n_rows + len(ids_per_doc) and (self.T == 0 or (0 <= self.pos.min() and self.pos.max() < L))


class Ctx(SP.Ctx):
    """spans_cases.Ctx with the transport of the packed entry."""

    def oracle_ids(self, docs, allowed=()):
        if self.specials and allowed:
            return [self.oenc.encode(d.decode("utf-8"), list(allowed)) for d in docs]
        return [self.oenc.encode_bytes(d) for d in docs]

    def packed_device(self, b, L, index=(), bos=-1, eos=-1, pad=0, want_pos=True, want_segs=True, cap=None, scap=None):
        """the device entry with guard words behind every buffer; a dict of the results cut to the figures the call returned"""
        f = (bos >= 0) + (eos >= 0)
        if cap is None or scap is None:
            bound, sbound = N.Encoder.packed_bounds(b["n"], b["total"], L, f)
            cap, scap = bound if cap is None else cap, sbound if scap is None else scap
        ids = self.upload(np.full(cap + GUARD, -7, np.int32))
        pos = self.upload(np.full(cap + GUARD, -7, np.int32)) if want_pos else (None, 0)
        seg = self.upload(np.full(scap + 1 + GUARD, -7, np.int64)) if want_segs else (None, 0)
        out = self.upload(np.full(b["n"] + 1 + GUARD, -5, np.int64))
        try:
            T, rows, segs = self.enc.encode_batch_packed_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], list(index), bos, eos, L, pad, ids[1], cap, out[1],
                                                                pos[1], seg[1], scap)
        finally:                                              # (whatever the call returned: nothing behind the capacities it was told)
            assert (self.back(ids[0])[cap:] == -7).all() and (self.back(out[0])[b["n"] + 1:] == -5).all(), "guard words behind ids / offsets"
            assert not want_pos or (self.back(pos[0])[cap:] == -7).all(), "guard words behind pos"
            assert not want_segs or (self.back(seg[0])[scap + 1:] == -7).all(), "guard words behind seg_starts"
        n = rows * L
        assert (self.back(ids[0])[n:] == -7).all() and (not want_pos or (self.back(pos[0])[n:] == -7).all()), "written at or behind n_rows * L"
        assert not want_segs or (self.back(seg[0])[segs + 1:] == -7).all(), "written behind seg_starts[n_segs]"
        return dict(T=T, n_rows=rows, n_segs=segs, ids=self.back(ids[0])[:n].astype(np.int64), offs=self.back(out[0])[:b["n"] + 1].tolist(),
                    pos=self.back(pos[0])[:n].astype(np.int64) if want_pos else None, seg=self.back(seg[0])[:segs + 1].tolist() if want_segs else None)


def assert_packed(what, got, m):
    assert (got["T"], got["n_rows"], got["n_segs"]) == (m.T, m.n_rows, m.n_segs), (what, (got["T"], got["n_rows"], got["n_segs"]), (m.T, m.n_rows, m.n_segs))
    SP._same(what, "offs", [int(x) for x in got["offs"]], m.offs)
    SP._same(what, "ids", got["ids"].tolist(), m.ids.tolist())
    if got["pos"] is not None:
        SP._same(what, "pos", got["pos"].tolist(), m.pos.tolist())
    if got["seg"] is not None:
        SP._same(what, "seg_starts", [int(x) for x in got["seg"]], m.seg)


def check_device(ctx, docs, L, what, bos=-1, eos=-1, pad=-3, allowed=(), forms=((True, True),), ids_per_doc=None, b=None):
    ids_per_doc = ids_per_doc if ids_per_doc is not None else ctx.oracle_ids(docs, allowed)
    m = Model(ids_per_doc, L, bos, eos, pad)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = b or ctx.device_buffers(docs)
    for wp, ws in forms:
        assert_packed("%s, L %d, bos %d, eos %d (pos %d, segs %d)" % (what, L, bos, eos, wp, ws), ctx.packed_device(b, L, index, bos, eos, pad, wp, ws), m)
    return m


ALL_FORMS = ((True, True), (True, False), (False, True), (False, False))


# ---- 1. framing forms ----

def check_framing(ctx):
    rng = random.Random(3)
    docs = [b"", words(rng, 3), b"", words(rng, 5), b"", b"", words(rng, 2)] + [b""] * 70 + [words(rng, 4), b"x", b""]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    for bos, eos in FORMS:
        for L in (4, 7):
            m = check_device(ctx, docs, L, "framing", bos, eos, ids_per_doc=ids, b=b, forms=ALL_FORMS if L == 4 else ((True, True),))
            f = (bos >= 0) + (eos >= 0)
            assert m.T == 15 + f * len(docs) and m.offs[9] - m.offs[8] == f            # an empty document is its framing alone
    # every document empty: with framing the stream is the framing ids, without it there is nothing
    empties = [b""] * 5
    for bos, eos in FORMS:
        m = check_device(ctx, empties, 3, "all empty", bos, eos, forms=ALL_FORMS)
        f = (bos >= 0) + (eos >= 0)
        assert (m.T, m.n_rows) == (5 * f, -(-5 * f // 3)) and (f > 0 or (m.n_segs, m.seg) == (0, [0]))
    m = check_device(ctx, empties, 1, "all empty, L 1", 7, 9)
    assert m.n_segs == 10


# ---- 2. row lengths ----

def check_row_lengths(ctx):
    rng = random.Random(5)
    docs = [words(rng, n) for n in (700, 0, 1, 2300, 64, 0, 0, 1500, 431)]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    T = sum(map(len, ids)) + len(docs)
    assert T > 2 * K
    for L in (1, 2, 7, 64, 1000, K, 2 * K, T - 1, T, T + 1, 10 * T):
        m = check_device(ctx, docs, L, "row lengths", eos=9, ids_per_doc=ids, b=b)
        assert m.T == T
        if L == 1:
            assert m.n_segs == T and not m.pos.any()
        if L > T:
            assert m.n_rows == 1 and (m.ids[T:] == -3).all() and len(m.ids) == L
    for L in (1, 7, K, T - len(docs) + 1):                    # without framing the ids stand where the encode kernels wrote them
        check_device(ctx, docs, L, "row lengths, no framing", ids_per_doc=ids, b=b, forms=((True, True), (False, False)))


# ---- 3. tile edges ----

def check_tile_edges(ctx):
    rng = random.Random(7)
    for T in (K - 1, K, K + 1, 4 * K, 4 * K + 1):              # (4K: one workgroup's four wavefronts)
        docs = [words(rng, 100), words(rng, T - 100 - 7 - 3), words(rng, 7)]
        ids = ctx.oracle_ids(docs)
        b = ctx.device_buffers(docs)
        assert check_device(ctx, docs, 512, "T = %d" % T, eos=9, ids_per_doc=ids, b=b).T == T
        plain = [words(rng, 100), words(rng, T - 107), words(rng, 7)]
        assert check_device(ctx, plain, 512, "T = %d, no framing" % T).T == T
    # a document start exactly at K and at K - 1
    for first, bos, eos in ((K - 1, -1, 9), (K, -1, -1), (K - 1, -1, -1), (K - 2, 7, 9)):
        m = check_device(ctx, [words(rng, first), words(rng, 10)], 3 * K, "a start at a tile edge", bos, eos)
        assert m.offs[1] in (K - 1, K) and m.offs[1] in m.seg
    # a document that covers three whole tiles (the straight copy), between two short ones
    m = check_device(ctx, [words(rng, 10), words(rng, 4 * K), words(rng, 10)], 1000, "three whole tiles", 7, 9)
    assert m.offs[1] < K and m.offs[2] > 4 * K
    # more than 64 document starts in one tile; with no framing, 300 empty documents between two tokens of one tile
    for bos, eos in ((-1, -1), (7, 9)):
        m = check_device(ctx, [words(rng, 1) for _ in range(300)], 50, "300 documents of one token", bos, eos)
        assert m.n_segs == (300 if bos < 0 else 300 + len([t for t in range(0, 900, 50) if t % 3])) and all(x in m.seg for x in m.offs)
    m = check_device(ctx, [words(rng, 5)] + [b""] * 300 + [words(rng, 5)], 4, "300 empty documents inside a tile")
    assert m.seg == [0, 4, 5, 8, 10] and m.offs[1:302] == [5] * 301


def check_grid_stride(ctx, lib):
    """more tiles than the capped grid has wavefronts: a pad tail that long (the stream itself is a few tokens)"""
    rng = random.Random(9)
    docs = [words(rng, 3), b"", words(rng, 2)]
    L = (GRID * 4 + 3) * K + 5
    m = check_device(ctx, docs, L, "grid stride", eos=9, forms=((False, True),))
    assert m.n_rows == 1 and len(m.ids) > GRID * 4 * K


# ---- 4. coincidence ----

def check_coincidence(ctx):
    rng = random.Random(11)
    docs = [words(rng, 3), b"", words(rng, 2)]                 # the worked example of tkz.h
    m = check_device(ctx, docs, 4, "example, L 4", eos=9, forms=ALL_FORMS)
    assert (m.offs, m.T, m.seg, m.n_segs, m.pos.tolist()) == ([0, 4, 5, 8], 8, [0, 4, 5, 8], 3, [0, 1, 2, 3, 0, 0, 1, 2])
    assert m.ids.reshape(2, 4)[:, 3].tolist() == [9, 9] and m.ids[4] == 9
    m = check_device(ctx, docs, 3, "example, L 3", eos=9, forms=ALL_FORMS)
    assert (m.seg, m.n_segs, m.pos.tolist(), m.ids[8]) == ([0, 3, 4, 5, 6, 8], 5, [0, 1, 2, 0, 0, 0, 0, 1, 0], -3)
    # a document start one position in front of a row boundary, on it, and one behind it
    for n, segs in ((3, [0, 3, 4, 8]), (4, [0, 4, 8, 9]), (5, [0, 4, 5, 8, 10])):
        m = check_device(ctx, [words(rng, n), words(rng, 5)], 4, "a start beside a row boundary")
        assert m.seg == segs


# ---- 5. special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    docs = [("the of" + EOT + " and to").encode(), EOT.encode(), b"", b" in is that"]
    on = check_device(ctx, docs, 5, "special: allowed", eos=eot, allowed=[EOT], forms=ALL_FORMS)
    assert on.ids.tolist().count(eot) == 2 + len(docs)
    s0 = ctx.enc.special_stats()
    off = check_device(ctx, docs, 5, "special: registered, not allowed", eos=eot, allowed=[])
    assert off.ids.tolist().count(eot) == len(docs) and off.T > on.T and ctx.enc.special_stats() == s0      # (split as plain text)


# ---- 6. capacity and arguments ----

def check_capacity(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, L = ctx.enc, ctx.enc.lib.L
    rng = random.Random(13)
    docs = [words(rng, 9), b"", words(rng, 30), (" the" + EOT + " of").encode()]
    RL = 8
    m = Model(ctx.oracle_ids(docs, [EOT]), RL, 7, eot, 0)
    b = ctx.device_buffers(docs)
    need, nseg = m.n_rows * RL, m.n_segs
    c0 = enc.packed_calls()
    for cap, scap in ((need - 1, nseg), (need, nseg - 1), (need - 1, nseg - 1), (0, 0)):
        with pytest.raises(N.TkzError) as ei:
            ctx.packed_device(b, RL, [0], 7, eot, 0, cap=cap, scap=scap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_rows, ei.value.needed_segs) == (m.T, m.n_rows, nseg), (cap, scap)
    with pytest.raises(N.TkzError) as ei:                      # (without seg_starts their capacity is not looked at, and n_segs is still reported)
        ctx.packed_device(b, RL, [0], 7, eot, 0, want_segs=False, cap=need - 1, scap=0)
    assert (ei.value.needed_rows, ei.value.needed_segs) == (m.n_rows, nseg) and enc.packed_calls() == c0      # failed calls are not counted
    for wp, ws in ALL_FORMS:                                   # exact capacities, sized from the figures above; either array or both absent
        assert_packed("exact capacity", ctx.packed_device(b, RL, [0], 7, eot, 0, wp, ws, cap=need, scap=nseg if ws else 0), m)
    assert enc.packed_calls() == c0 + 4
    data, offs = parity.pack(docs)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_packed(data, offs, RL, [0], 7, eot, seg_cap=nseg - 1)
    assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_ids, ei.value.needed_segs) == (m.T, need, nseg)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_packed(data, offs, RL, [0], 7, eot, out_cap=need - 1)
    assert ei.value.code == N.E_CAPACITY and (ei.value.needed_ids, ei.value.needed_segs) == (need, nseg)
    r = enc.encode_batch_packed(data, offs, RL, [0], 7, eot, out_cap=need, seg_cap=nseg)
    assert r[0].reshape(-1).tolist() == m.ids.tolist() and r[3].tolist() == m.seg and r[4] == m.T
    # arguments
    for kw in (dict(bos=-2), dict(eos=-2), dict(eos=-(1 << 31)), dict(L=0), dict(L=-4), dict(L=1 << 31), dict(index=[1]), dict(index=[0, 0]), dict(index=[-1])):
        a = dict(L=RL, index=[0], bos=7, eos=eot)
        a.update(kw)
        with pytest.raises(N.TkzError) as ei:
            ctx.packed_device(b, a["L"], a["index"], a["bos"], a["eos"], cap=need, scap=nseg)
        assert ei.value.code == N.E_ARG, kw
        if "index" not in kw:
            for call in (lambda: enc.encode_batch_packed(data, offs, a["L"], [0], a["bos"], a["eos"], out_cap=need, seg_cap=nseg),
                         lambda: enc.encode_batch_packed_utf16(np.asarray([65, 66], np.uint16), np.asarray([0, 2], np.int64), a["L"], [0], a["bos"], a["eos"], out_cap=8, seg_cap=8)):
                with pytest.raises(N.TkzError) as ei:
                    call()
                assert ei.value.code == N.E_ARG, kw
    ids, ooff, pos, seg = ctx.upload(np.zeros(need, np.int32)), ctx.upload(np.zeros(len(docs) + 1, np.int64)), ctx.upload(np.zeros(need, np.int32)), ctx.upload(np.zeros(nseg + 1, np.int64))
    t, r, s = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ok = (enc._h, b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], None, 0, 7, eot, RL, 0, ids[1], need, ooff[1], pos[1], seg[1], nseg + 2, None, C.byref(t), C.byref(r), C.byref(s))
    assert L.tkz_encode_batch_packed_device(*ok) == N.OK and t.value == Model(ctx.oracle_ids(docs), RL, 7, eot).T
    for k in (0, 1, 2, 11, 13, 18, 19, 20):                    # the encoder, the bytes, the offsets, d_out_ids, d_out_offsets, total_tokens, n_rows, n_segs
        assert L.tkz_encode_batch_packed_device(*(ok[:k] + (None,) + ok[k + 1:])) == N.E_ARG, k
    assert L.tkz_encode_batch_packed_device(*(ok[:16] + (-1,) + ok[17:])) == N.E_ARG and L.tkz_encode_batch_packed_device(*(ok[:12] + (-1,) + ok[13:])) == N.E_ARG
    hid, hoo = np.zeros(need, np.int32), np.zeros(len(docs) + 1, np.int64)
    hok = (enc._h, data.ctypes.data, offs.ctypes.data, len(docs), None, 0, 7, eot, RL, 0, hid.ctypes.data, need, hoo.ctypes.data, None, None, 0, None, C.byref(r), C.byref(s))
    assert L.tkz_encode_batch_packed_utf8(*hok) == N.OK and r.value == need and hoo.tolist() == Model(ctx.oracle_ids(docs), RL, 7, eot).offs
    for k in (0, 2, 10, 12, 17, 18):                           # the encoder, the offsets, out_ids, out_offsets, needed_ids, needed_segs
        assert L.tkz_encode_batch_packed_utf8(*(hok[:k] + (None,) + hok[k + 1:])) == N.E_ARG, k
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        ctx.packed_device(ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]), RL, eos=9)
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_packed(data, np.asarray([0, 12, 11, 40, len(data)], np.int64), RL)
    assert ei.value.code == N.E_ARG
    # no documents: TKZ_OK, seg_starts[0] = 0, all three counts 0 -- framed or not; documents without bytes through the host entries
    none = ctx.device_buffers([])
    for bos, eos in FORMS:
        got = ctx.packed_device(none, RL, (), bos, eos, cap=0, scap=0)
        assert (got["T"], got["n_rows"], got["n_segs"], got["offs"], got["seg"]) == (0, 0, 0, [0], [0])
        r = enc.encode_batch_packed(np.zeros(0, np.uint8), np.zeros(4, np.int64), 2, (), bos, eos)
        m3 = Model([[], [], []], 2, bos, eos)
        assert (r[0].reshape(-1).tolist(), r[1].tolist(), r[2].reshape(-1).tolist(), r[3].tolist(), r[4]) == (m3.ids.tolist(), m3.offs, m3.pos.tolist(), m3.seg, m3.T)
        r16 = enc.encode_batch_packed_utf16(np.zeros(0, np.uint16), np.zeros(4, np.int64), 2, (), bos, eos)
        assert (r16[0].reshape(-1).tolist(), r16[1].tolist(), r16[3].tolist(), r16[4]) == (m3.ids.tolist(), m3.offs, m3.seg, m3.T)
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    d1, o1 = parity.pack([b"a<|s7|>b"])
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_batch_packed(d1, o1, 4, [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_batch_packed(d1, o1, 4)[4] == len(many.oenc.encode_bytes(b"a<|s7|>b"))          # (nothing allowed: the plain call)


# ---- 7. agreement of the entries ----

def check_agreement(make_ctx, lib, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc = ctx.enc
    rng, gib, mixed, crowded = CC.generators(7)
    w = lambda n: CC.fill(rng, n).decode()
    lone = "lone \ud800 high"
    texts = [w(300) + EOT + w(40), gib(600, 2, 9), "", w(2 * K + 9), "café " + EMOJI + " 漢字 " + w(20), lone, mixed(1500, 3, 3, 30), EOT, w(5)]
    unit_docs = [U16S.units(t) for t in texts]
    docs = [U16.get_bytes(u) for u in unit_docs]                 # (Encoding.UTF8.GetBytes: the lone surrogate becomes EF BF BD)
    data, offs = parity.pack(docs)
    flat, uoffs = U16S.pack(unit_docs)
    b = ctx.device_buffers(docs)
    for index, allowed in (([0], [EOT]), ([], [])):
        want = ctx.oracle_ids(docs, allowed)
        for bos, eos, RL in ((-1, -1, 64), (7, eot, 64), (-1, eot, 1000)):
            m = Model(want, RL, bos, eos, 0)
            c0 = enc.packed_calls()
            dev = ctx.packed_device(b, RL, index, bos, eos, 0)
            assert_packed("agreement: device", dev, m)
            assert parity.read_device_i64(lib, enc.counts_device, 3).tolist() == [len(docs), len(data), m.T]      # the counts block receives T
            for name, r in (("utf8", enc.encode_batch_packed(data, offs, RL, index, bos, eos, 0)), ("utf16", enc.encode_batch_packed_utf16(flat, uoffs, RL, index, bos, eos, 0))):
                host = dict(T=r[4], n_rows=r[0].shape[0], n_segs=len(r[3]) - 1, ids=r[0].reshape(-1).astype(np.int64), offs=r[1].tolist(), pos=r[2].reshape(-1).astype(np.int64), seg=r[3].tolist())
                assert_packed("agreement: " + name, host, m)
                assert r[0].shape == r[2].shape == (m.n_rows, RL)
            assert enc.packed_calls() == c0 + 3
            if bos < 0 and eos < 0:                             # no framing: the first T ids and the offsets are the encode entry's, exactly
                eids, eoff = enc.encode_batch_special(data, offs, index)
                assert dev["ids"][:m.T].tolist() == eids.tolist() and dev["offs"] == eoff.tolist()
                if not index:
                    ids = ctx.upload(np.zeros(max(1, b["total"]), np.int32))
                    out = ctx.upload(np.zeros(b["n"] + 1, np.int64))
                    tot = enc.encode_batch_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], ids[1], b["total"], out[1])
                    assert tot == m.T and ctx.back(ids[0])[:tot].tolist() == dev["ids"][:m.T].tolist() and ctx.back(out[0]).tolist() == dev["offs"]


# ---- 8. retry ----

def check_retry(make_ctx):
    """the first call of a fresh encoder is a packed call whose miss lists overflow (CJK text under gpt2, consonant strings): the attempt is run again inside the call"""
    ctx = make_ctx()
    rng, gib, mixed, crowded = CC.generators(47)
    cjk = "漢字かな交じり文、한국어 " + EMOJI + " naïve café "
    docs = [(cjk * 80).encode("utf-8")] + CC.cut(gib(30000, 2, 2).encode(), [700, 9000]) + [b"", CC.fill(rng, 300)]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    w0 = ctx.enc.workspace_bytes
    first = check_device(ctx, docs, 512, "retry: first call", 7, 9, ids_per_doc=ids, b=b)
    assert ctx.enc.workspace_bytes > w0
    again = check_device(ctx, docs, 512, "retry: again", 7, 9, ids_per_doc=ids, b=b)
    assert first.T == again.T
    check_device(ctx, docs, 512, "retry: no framing", ids_per_doc=ids, b=b)


# ---- 9. the Python mirror ----

def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    oenc = O.Encoder(O.Vocab(raw_gpt2), N.P1, specials=specials)
    lines = lib_rs_text.split("\n")
    L = 512
    ids, pos, seg, offs = tok.EncodeBatchPacked(lines, L, eos=EOT)
    m = Model([oenc.encode(t, [EOT]) for t in lines], L, -1, 50256, 0)
    assert ids.shape == pos.shape == (m.n_rows, L) and ids.dtype == np.int32 and m.n_rows >= 3
    assert (ids.reshape(-1).tolist(), pos.reshape(-1).tolist(), seg.tolist(), offs.tolist()) == (m.ids.tolist(), m.pos.tolist(), m.seg, m.offs)
    flat, T = ids.reshape(-1), int(offs[-1])
    assert T == m.T and not flat[T:].any()
    for d, line in enumerate(lines):                           # every document range minus its framing decodes back to the line
        lo, hi = int(offs[d]), int(offs[d + 1])
        assert flat[hi - 1] == 50256 and tok.Decode(flat[lo:hi - 1].tolist()) == line, d
    # bos as an int, eos as a literal, another pad; the literal in the text allowed and not
    text = ["a" + EOT + "b", "", "Hi " + EMOJI + " café"]
    for apply in (True, False):
        ids, pos, seg, offs = tok.EncodeBatchPacked(text, 4, apply, bos=11, eos=EOT, pad=-1)
        m = Model([oenc.encode(t, [EOT] if apply else []) for t in text], 4, 11, 50256, -1)
        assert (ids.reshape(-1).tolist(), pos.reshape(-1).tolist(), seg.tolist(), offs.tolist()) == (m.ids.tolist(), m.pos.tolist(), m.seg, m.offs)
    ids, pos, seg, offs = tok.EncodeBatchPacked([], 4, eos=EOT)
    assert ids.shape == (0, 4) and seg.tolist() == [0] and offs.tolist() == [0]
    for bad in (dict(row_len=0), dict(row_len=4, bos="<|nope|>"), dict(row_len=4, eos=-5)):
        with pytest.raises(ValueError):
            tok.EncodeBatchPacked(text, **bad)
    # a literal that holds U+FFFD beside a lone surrogate: through the UTF-16 entry
    fffd = {k: v + 200000 for k, v in U16S.FFFD_SPECIALS.items()}
    tok3 = TokenizerBuilder.CreateTokenizer(raw_gpt2, fffd, REGEX_PATTERN_1, lib=lib)
    lone = ["ab x\ud83d b x� c it's", "plain"]
    ids, pos, seg, offs = tok3.EncodeBatchPacked(lone, 8, list(fffd), eos=3)
    exp = U16S.Expect(O, O.Vocab(raw_gpt2), N.P1, fffd)
    m = Model([exp.encode(U16S.units(t), list(fffd)) for t in lone], 8, -1, 3, 0)
    assert (ids.reshape(-1).tolist(), seg.tolist(), offs.tolist()) == (m.ids.tolist(), m.seg, m.offs)
