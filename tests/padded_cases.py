"""Padded rows (tkz_encode_batch_padded_device / _utf8 / _utf16; k_pad_lens, k_pad_write): the cases and comparisons the emulated (CPU) and the GPU test modules
share.  Every comparison is exact.

No expected value comes from the code under test.  The model (`Model`) is numpy over the ORACLE's ids -- oracle.Encoder, the special-token form where literals are
allowed; TrimOracle's literal search for UTF-16 text with lone surrogates (u16_special_cases.Expect) -- and applies the rule of tkz.h: the cut, the framing, the
width, the rows, the mask, pos and lens.  It never reads the library's own encode output.

The kernel cases go through tkz_encode_batch_padded_device.  `upload(np_array) -> (owner, pointer)` as in count_cases: identity for the emulated build, a device
tensor on the hardware.  Every output buffer carries GUARD words behind the capacity the call is told, and they must be intact afterwards -- and so must everything
at or behind n_docs * W.

Geometry (tkz_kernels.h): k_pad_lens a lane a document, k_pad_write a wavefront per tile of K = kPadTile output positions, four wavefronts a workgroup, at most
GRID workgroups each.  Documents are short words of one token each (" the", " of" ...: keys of the tables the tests use), so a case is a few tens of KB.
"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import count_cases as CC
import packed_cases as PK
import parity
import spans_cases as SP
import special_cases as SC
import u16_cases as U16
import u16_special_cases as U16S
from conftest import ROOT
from tokenizer_amd import _native as N

_HEAD = open(os.path.join(ROOT, "tokenizer_amd", "csrc", "tkz_kernels.h")).read()
K = int(re.search(r"\bkPadTile = (\d+)\b", _HEAD).group(1))
GRID = int(re.search(r"\bkPadGridMax = (\d+)\b", _HEAD).group(1))
EOT = SC.EOT
EOT_ID = SP.EOT_ID
EMOJI = PK.EMOJI
GUARD = 8
FORMS = PK.FORMS                                       # none, bos only, eos only, both
SUFFIX, PREFIX, RIGHT, LEFT = N.TRIM_SUFFIX, N.TRIM_PREFIX, N.PAD_RIGHT, N.PAD_LEFT
SIDES = ((SUFFIX, RIGHT), (SUFFIX, LEFT), (PREFIX, RIGHT), (PREFIX, LEFT))
# mask, pos and offsets present and NULL: all, none, and the two that tell the three apart
ARRAYS = ((True, True, True), (False, False, False), (True, False, True), (False, True, False))
words = PK.words


class Model:
    """the rule of tkz.h over the oracle's ids of every document"""

    def __init__(self, ids_per_doc, L, bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1):
        fb, fe = int(bos >= 0), int(eos >= 0)
        f, n = fb + fe, len(ids_per_doc)
        assert max(1, f) <= L
        content = []
        for di in ids_per_doc:
            di = list(di)
            k = min(len(di), L - f)
            kept = di[:k] if cut == SUFFIX else di[len(di) - k:]
            content.append([bos] * fb + kept + [eos] * fe)
        self.offs = np.concatenate([[0], np.cumsum([len(di) for di in ids_per_doc], dtype=np.int64)]).astype(np.int64).tolist()
        self.total = self.offs[-1]
        self.lens = [len(c) for c in content]
        self.n_cut = sum(len(di) > L - f for di in ids_per_doc)
        longest = max(self.lens, default=0)
        self.W = W = 0 if longest == 0 else (L if M == 0 else min(L, -(-longest // M) * M))
        self.ids = np.full((n, W), pad, np.int64)
        self.mask = np.zeros((n, W), np.int64)
        self.pos = np.zeros((n, W), np.int64)
        for d, c in enumerate(content):
            s = W - len(c) if side == LEFT else 0
            self.ids[d, s:s + len(c)] = c
            self.mask[d, s:s + len(c)] = 1
            self.pos[d, s:s + len(c)] = np.arange(len(c))
        assert W <= L and (M == 0 or W % M == 0 or W == L)


class Ctx(PK.Ctx):
    """packed_cases.Ctx (the oracle's ids of every document) with the transport of the padded entry."""

    def padded_device(self, b, L, index=(), bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1, arrays=(True, True, True), cap=None):
        """the device entry with guard words behind every buffer; a dict of the results cut to the figures the call returned"""
        wm, wp, wo = arrays
        n = b["n"]
        cap = N.Encoder.padded_bounds(n, L) if cap is None else cap
        ids = self.upload(np.full(cap + GUARD, -7, np.int32))
        mask = self.upload(np.full(cap + GUARD, 0xA5, np.uint8)) if wm else (None, 0)
        pos = self.upload(np.full(cap + GUARD, -7, np.int32)) if wp else (None, 0)
        lens = self.upload(np.full(n + GUARD, -7, np.int32))
        out = self.upload(np.full(n + 1 + GUARD, -5, np.int64)) if wo else (None, 0)
        W = None
        try:
            total, W, n_cut = self.enc.encode_batch_padded_device(b["d_bytes"][1], b["d_offs"][1], n, b["total"], list(index), bos, eos, L, cut, side, pad, M, ids[1], cap,
                                                                  mask[1], pos[1], lens[1], out[1])
        finally:                                              # (whatever the call returned: nothing behind the capacities it was told)
            assert (self.back(ids[0])[cap:] == -7).all() and (self.back(lens[0])[n:] == -7).all(), "guard words behind ids / lens"
            assert not wm or (self.back(mask[0])[cap:] == 0xA5).all(), "guard words behind the mask"
            assert not wp or (self.back(pos[0])[cap:] == -7).all(), "guard words behind pos"
            assert not wo or (self.back(out[0])[n + 1:] == -5).all(), "guard words behind the offsets"
        k = n * W
        assert (self.back(ids[0])[k:] == -7).all() and (not wm or (self.back(mask[0])[k:] == 0xA5).all()) and (not wp or (self.back(pos[0])[k:] == -7).all()), \
            "written at or behind n_docs * W"
        return dict(total=total, W=W, n_cut=n_cut, ids=self.back(ids[0])[:k].astype(np.int64), lens=self.back(lens[0])[:n].tolist(),
                    mask=self.back(mask[0])[:k].astype(np.int64) if wm else None, pos=self.back(pos[0])[:k].astype(np.int64) if wp else None,
                    offs=self.back(out[0])[:n + 1].tolist() if wo else None)


def assert_padded(what, got, m):
    assert (got["total"], got["W"], got["n_cut"]) == (m.total, m.W, m.n_cut), (what, (got["total"], got["W"], got["n_cut"]), (m.total, m.W, m.n_cut))
    SP._same(what, "lens", [int(x) for x in got["lens"]], m.lens)
    SP._same(what, "ids", got["ids"].tolist(), m.ids.reshape(-1).tolist())
    if got["mask"] is not None:
        SP._same(what, "mask", got["mask"].tolist(), m.mask.reshape(-1).tolist())
    if got["pos"] is not None:
        SP._same(what, "pos", got["pos"].tolist(), m.pos.reshape(-1).tolist())
    if got["offs"] is not None:
        SP._same(what, "offsets", [int(x) for x in got["offs"]], m.offs)


def check_device(ctx, docs, L, what, bos=-1, eos=-1, pad=-3, cut=SUFFIX, side=RIGHT, M=1, allowed=(), arrays=((True, True, True),), ids_per_doc=None, b=None, exact=False):
    """the device entry against the model, with the capacity that always suffices (n_docs * L) or -- exact -- with n_docs * W, not an entry more"""
    ids_per_doc = ids_per_doc if ids_per_doc is not None else ctx.oracle_ids(docs, allowed)
    m = Model(ids_per_doc, L, bos, eos, pad, cut, side, M)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = b or ctx.device_buffers(docs)
    for a in arrays:
        label = "%s, L %d, M %d, bos %d, eos %d, cut %d, pad side %d (mask %d, pos %d, offsets %d)" % ((what, L, M, bos, eos, cut, side) + tuple(a))
        assert_padded(label, ctx.padded_device(b, L, index, bos, eos, pad, cut, side, M, a, cap=len(docs) * m.W if exact else None), m)
    return m


# ---- 1. cut edges ----

def check_cut_edges(ctx):
    rng = random.Random(3)
    L = 9
    for bos, eos in FORMS:
        f = (bos >= 0) + (eos >= 0)
        sizes = [0, 1, L - f - 1, L - f, L - f + 1, 3 * L]
        docs = [words(rng, n) for n in sizes]
        ids = ctx.oracle_ids(docs)
        assert [len(x) for x in ids] == sizes
        b = ctx.device_buffers(docs)
        for cut, side in SIDES:
            m = check_device(ctx, docs, L, "cut edges", bos, eos, cut=cut, side=side, ids_per_doc=ids, b=b)
            assert (m.W, m.n_cut, m.lens) == (L, 2, [f, 1 + f, L - 1, L, L, L])
            assert m.lens[0] == f                             # an empty document is its framing alone
            kept = ids[5][:L - f] if cut == SUFFIX else ids[5][-(L - f):] if L > f else []
            row = m.ids[5].tolist()
            assert row[(1 if bos >= 0 else 0):L - (1 if eos >= 0 else 0)] == kept
        if f:                                                 # L == f: nothing is kept, every row is the framing
            for cut, side in SIDES:
                m = check_device(ctx, docs, f, "L == f", bos, eos, cut=cut, side=side, ids_per_doc=ids, b=b)
                assert (m.W, m.n_cut, m.lens) == (f, 5, [f] * 6) and m.mask.all()
    for cut, side in SIDES:                                   # L == 1 without framing: the first or the last id of every document
        docs = [words(rng, n) for n in (3, 0, 1, 5)]
        m = check_device(ctx, docs, 1, "L == 1", cut=cut, side=side)
        assert (m.W, m.n_cut, m.lens) == (1, 2, [1, 0, 1, 1])
    # 75 empty documents: with framing every row is the framing, without it W is 0 and nothing is written
    empties = [b""] * 75
    for bos, eos in FORMS:
        f = (bos >= 0) + (eos >= 0)
        for M in (0, 1, 8):
            for side in (RIGHT, LEFT):
                m = check_device(ctx, empties, 6, "75 empty documents", bos, eos, side=side, M=M, arrays=ARRAYS)
                assert (m.total, m.n_cut, m.lens) == (0, 0, [f] * 75) and m.W == (0 if f == 0 else 6 if M == 0 else min(6, M) if M > 1 else f)


# ---- 2. width ----

def check_width(ctx):
    rng = random.Random(5)
    L = 200
    for M in (0, 1, 8, 64):
        base = max(M, 1) * (24 // max(M, 1) + 1)              # (above the other documents' 18)
        for longest in (base - 1, base, base + 1):            # the longest len a multiple of M, one below it and one above it (eos included)
            docs = [words(rng, n) for n in (3, longest - 1, 0, 17, longest - 2)]
            for side in (RIGHT, LEFT):
                m = check_device(ctx, docs, L, "width", eos=9, side=side, M=M, exact=True)
                assert m.n_cut == 0 and max(m.lens) == longest
                assert m.W == (L if M == 0 else -(-longest // M) * M)
    # the round-up exceeds L: clamped
    docs = [words(rng, n) for n in (70, 5, 300)]
    for M, L in ((64, 100), (8, 21), (64, 63), (1000, 7)):
        for cut, side in SIDES:
            m = check_device(ctx, docs, L, "width clamped", 7, 9, cut=cut, side=side, M=M, exact=True)
            assert m.W == L and m.n_cut == (1 if L == 100 else 2)
    m = check_device(ctx, docs, 100, "width below L", 7, 9, M=8)          # (cut documents, and still a round-up below L: not with these -- the longest is L)
    assert m.W == 100 and m.n_cut == 1
    m = check_device(ctx, docs[:2], 100, "width from the longest", 7, 9, M=8)
    assert (m.W, m.n_cut, m.lens) == (72, 0, [72, 7])


# ---- 3. tile and row geometry ----

def _factor(target):
    """(n_docs, W) with n_docs * W == target and as many rows as a small factor gives"""
    n = next((k for k in range(2, 200) if target % k == 0), 1)
    return n, target // n


def check_geometry(ctx):
    rng = random.Random(7)
    # many rows in a group of 64 positions: 150 documents of 0 .. W + 2 tokens, fixed width
    for W in (1, 3, 7, 63, 64, 65):
        sizes = [(5 * d) % (W + 3) for d in range(150)]
        docs = [words(rng, n) for n in sizes]
        ids = ctx.oracle_ids(docs)
        b = ctx.device_buffers(docs)
        for side in (RIGHT, LEFT):
            m = check_device(ctx, docs, W, "W = %d" % W, eos=9, pad=-3, cut=PREFIX if side == LEFT else SUFFIX, side=side, M=0, arrays=ARRAYS, ids_per_doc=ids, b=b, exact=True)
            assert m.W == W
    # a row across tiles
    for W in (K - 1, K, K + 1, 2 * K + 5):
        docs = [words(rng, W), words(rng, 5), words(rng, W + 7)]
        ids = ctx.oracle_ids(docs)
        b = ctx.device_buffers(docs)
        for side in (RIGHT, LEFT):
            m = check_device(ctx, docs, W, "W = %d" % W, 7, -1, cut=PREFIX if side == LEFT else SUFFIX, side=side, arrays=ARRAYS, ids_per_doc=ids, b=b, exact=True)
            assert (m.W, m.n_cut, m.lens) == (W, 2, [W, 6, W])
    # n_docs * W one below, at and one above a tile multiple
    for target in (2 * K - 1, 2 * K, 2 * K + 1):
        n, W = _factor(target)
        docs = [words(rng, (7 * d) % (W + 2)) for d in range(n)]
        docs[-1] = words(rng, W)                              # (the longest row is W)
        for side in (RIGHT, LEFT):
            m = check_device(ctx, docs, W, "n_docs * W = %d" % target, -1, 9, side=side, arrays=ARRAYS, exact=True)
            assert n * m.W == target


# ---- 4. grid stride ----

def check_grid_stride(ctx, lib):
    """more tiles than the capped grid has wavefronts: one fixed-width row that long, nearly all of it padding (the text is a few tokens); and more documents
    than k_pad_lens has lanes: empty ones, a row of one framing id each"""
    rng = random.Random(9)
    L = (GRID * 4 + 3) * K + 5
    for side in (RIGHT, LEFT):
        m = check_device(ctx, [words(rng, 5)], L, "grid stride: tiles", eos=9, side=side, M=0, arrays=((False, False, False),), exact=True)
        assert m.W == L > GRID * 4 * K and m.lens == [6]
    n = GRID * 256 + 300
    docs = [b""] * n
    docs[7], docs[n - 2] = words(rng, 3), words(rng, 2)
    ids = [[]] * n
    ids[7], ids[n - 2] = ctx.oracle_ids([docs[7]])[0], ctx.oracle_ids([docs[n - 2]])[0]
    m = check_device(ctx, docs, 2, "grid stride: documents", 7, -1, arrays=((True, False, True),), ids_per_doc=ids, exact=True)
    assert (m.W, m.n_cut, m.total) == (2, 2, 5) and m.lens.count(1) == n - 2


# ---- 5. special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    docs = [(" the of" + EOT + " and to in").encode(), (" is that for" + EOT).encode(), b"", EOT.encode()]
    ids = ctx.oracle_ids(docs, [EOT])
    assert [len(x) for x in ids] == [6, 4, 0, 1] and ids[0][2] == ids[1][3] == ids[3][0] == eot
    b = ctx.device_buffers(docs)
    for L in (3, 4, 5, 6, 7, 8):
        for cut, side in SIDES:
            m = check_device(ctx, docs, L, "special: allowed", eos=eot, cut=cut, side=side, allowed=[EOT], ids_per_doc=ids, b=b)
            row0 = m.ids[0][m.mask[0] == 1].tolist()
            if L == 3 and cut == SUFFIX:
                assert row0 == ids[0][:2] + [eot] and row0.count(eot) == 1            # the cut removes the literal: the one eot left is the framing
            if L == 4 and cut == SUFFIX:
                assert row0 == ids[0][:3] + [eot] and row0[-2:] == [eot, eot]         # the literal at the last kept position, the eos behind it
            if L == 4 and cut == PREFIX:
                assert m.ids[1][m.mask[1] == 1].tolist() == ids[1][1:] + [eot]        # ... and of the prefix cut: the document's last id
            if L == 5 and cut == PREFIX:
                assert row0 == ids[0][2:] + [eot] and row0[0] == eot                  # the literal is the first id the prefix cut keeps
    s0 = ctx.enc.special_stats()
    off = check_device(ctx, docs, 6, "special: registered, not allowed", eos=eot, allowed=[])
    assert off.total > sum(map(len, ids)) and ctx.enc.special_stats() == s0              # (split as plain text)


# ---- 6. capacity and arguments ----

def check_capacity(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, lib = ctx.enc, ctx.enc.lib.L
    rng = random.Random(13)
    docs = [words(rng, 9), b"", words(rng, 30), (" the" + EOT + " of").encode()]
    n, ML = len(docs), 16
    m = Model(ctx.oracle_ids(docs, [EOT]), ML, 7, eot, 0, M=8)
    assert (m.W, m.n_cut) == (16, 1)
    b = ctx.device_buffers(docs)
    need = n * m.W
    c0 = enc.padded_calls()
    for cap in (need - 1, m.W, 0):
        with pytest.raises(N.TkzError) as ei:
            ctx.padded_device(b, ML, [0], 7, eot, 0, M=8, cap=cap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_width, ei.value.n_cut) == (m.total, m.W, m.n_cut), cap
    assert enc.padded_calls() == c0                              # failed calls are not counted
    for a in ARRAYS:                                             # the exact capacity, sized from the figures above
        assert_padded("exact capacity", ctx.padded_device(b, ML, [0], 7, eot, 0, M=8, arrays=a, cap=need), m)
    assert enc.padded_calls() == c0 + 4
    data, offs = parity.pack(docs)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_padded(data, offs, ML, [0], 7, eot, pad_multiple=8, out_cap=need - 1)
    assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_width, ei.value.n_cut) == (m.total, m.W, m.n_cut)
    r = enc.encode_batch_padded(data, offs, ML, [0], 7, eot, pad_multiple=8, out_cap=need)
    assert r[0].tolist() == m.ids.tolist() and r[1].tolist() == m.mask.tolist() and r[2].tolist() == m.pos.tolist() and r[3].tolist() == m.lens
    assert r[4].tolist() == m.offs and r[5:] == (m.total, m.n_cut)
    # every TKZ_E_ARG of the rule
    bad = (dict(bos=-2), dict(eos=-2), dict(eos=-(1 << 31)), dict(L=0), dict(L=-4), dict(L=1 << 31), dict(L=1), dict(cut=2), dict(cut=-1), dict(side=2), dict(side=-1),
           dict(M=-1), dict(M=1 << 31), dict(index=[1]), dict(index=[0, 0]), dict(index=[-1]))
    for kw in bad:
        a = dict(L=ML, index=[0], bos=7, eos=eot, cut=SUFFIX, side=RIGHT, M=8)
        a.update(kw)
        with pytest.raises(N.TkzError) as ei:
            ctx.padded_device(b, a["L"], a["index"], a["bos"], a["eos"], 0, a["cut"], a["side"], a["M"], cap=need)
        assert ei.value.code == N.E_ARG, kw
        if "index" not in kw:
            for call in (lambda: enc.encode_batch_padded(data, offs, a["L"], [0], a["bos"], a["eos"], 0, a["cut"], a["side"], a["M"], out_cap=need),
                         lambda: enc.encode_batch_padded_utf16(np.asarray([65, 66], np.uint16), np.asarray([0, 2], np.int64), a["L"], [0], a["bos"], a["eos"], 0, a["cut"],
                                                               a["side"], a["M"], out_cap=64)):
                with pytest.raises(N.TkzError) as ei:
                    call()
                assert ei.value.code == N.E_ARG, kw
    assert Model(ctx.oracle_ids(docs), 1, 7, -1).W == 1 and Model(ctx.oracle_ids(docs), 2, 7, 9).W == 2          # (L == f is in range; L == 1 with two framing ids is not)
    # NULL for a required pointer; for one that may be NULL
    ids, msk, pos = ctx.upload(np.zeros(need, np.int32)), ctx.upload(np.zeros(need, np.uint8)), ctx.upload(np.zeros(need, np.int32))
    lens, ooff = ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n + 1, np.int64))
    t, w, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ok = (enc._h, b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], None, 0, 7, eot, ML, SUFFIX, RIGHT, 0, 8, ids[1], need, msk[1], pos[1], lens[1], ooff[1], None,
          C.byref(t), C.byref(w), C.byref(c))
    plain = Model(ctx.oracle_ids(docs), ML, 7, eot, 0, M=8)
    assert lib.tkz_encode_batch_padded_device(*ok) == N.OK and (t.value, w.value, c.value) == (plain.total, plain.W, plain.n_cut)
    for k in (0, 1, 2, 14, 18, 21, 22, 23):                      # the encoder, the bytes, the offsets, d_out_ids, d_lens, total_tokens, width, n_cut
        assert lib.tkz_encode_batch_padded_device(*(ok[:k] + (None,) + ok[k + 1:])) == N.E_ARG, k
    for k in (16, 17, 19):                                       # d_mask, d_pos, d_out_offsets
        assert lib.tkz_encode_batch_padded_device(*(ok[:k] + (None,) + ok[k + 1:])) == N.OK, k
    assert lib.tkz_encode_batch_padded_device(*(ok[:15] + (-1,) + ok[16:])) == N.E_ARG
    hid, hl = np.zeros(need, np.int32), np.zeros(n, np.int32)
    hok = (enc._h, data.ctypes.data, offs.ctypes.data, n, None, 0, 7, eot, ML, SUFFIX, RIGHT, 0, 8, hid.ctypes.data, need, None, None, hl.ctypes.data, None,
           C.byref(t), C.byref(w), C.byref(c))
    assert lib.tkz_encode_batch_padded_utf8(*hok) == N.OK and w.value == plain.W and hl.tolist() == plain.lens and hid.tolist() == plain.ids.reshape(-1).tolist()
    for k in (0, 2, 13, 17, 19, 20, 21):                         # the encoder, the offsets, out_ids, lens, total_tokens, width, n_cut
        assert lib.tkz_encode_batch_padded_utf8(*(hok[:k] + (None,) + hok[k + 1:])) == N.E_ARG, k
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        ctx.padded_device(ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]), ML, eos=9)
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_padded(data, np.asarray([0, 12, 11, 40, len(data)], np.int64), ML)
    assert ei.value.code == N.E_ARG
    # no documents: TKZ_OK, W 0, the offset cleared; documents without bytes through the host entries
    none = ctx.device_buffers([])
    for bos, eos in FORMS:
        got = ctx.padded_device(none, ML, (), bos, eos, cap=0)
        assert (got["total"], got["W"], got["n_cut"], got["offs"], got["lens"]) == (0, 0, 0, [0], [])
        m3 = Model([[], [], []], 4, bos, eos, 5, side=LEFT, M=2)
        for r in (enc.encode_batch_padded(np.zeros(0, np.uint8), np.zeros(4, np.int64), 4, (), bos, eos, 5, pad_side=LEFT, pad_multiple=2),
                  enc.encode_batch_padded_utf16(np.zeros(0, np.uint16), np.zeros(4, np.int64), 4, (), bos, eos, 5, pad_side=LEFT, pad_multiple=2)):
            assert r[0].shape == (3, m3.W) and (r[0].tolist(), r[1].tolist(), r[2].tolist(), r[3].tolist(), r[4].tolist(), r[5], r[6]) == \
                (m3.ids.tolist(), m3.mask.tolist(), m3.pos.tolist(), m3.lens, [0, 0, 0, 0], 0, 0)
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    d1, o1 = parity.pack([b"a<|s7|>b"])
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_batch_padded(d1, o1, 4, [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_batch_padded(d1, o1, 64)[5] == len(many.oenc.encode_bytes(b"a<|s7|>b"))          # (nothing allowed: the plain call)


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
        for bos, eos, ML, cut, side, M in ((-1, -1, 64, SUFFIX, RIGHT, 1), (7, eot, 64, PREFIX, LEFT, 8), (-1, eot, 1000, SUFFIX, LEFT, 0), (-1, eot, 5000, PREFIX, RIGHT, 64)):
            m = Model(want, ML, bos, eos, 0, cut, side, M)
            c0 = enc.padded_calls()
            assert_padded("agreement: device", ctx.padded_device(b, ML, index, bos, eos, 0, cut, side, M), m)
            assert parity.read_device_i64(lib, enc.counts_device, 3).tolist() == [len(docs), len(data), m.total]      # the counts block receives the uncut total
            for name, r in (("utf8", enc.encode_batch_padded(data, offs, ML, index, bos, eos, 0, cut, side, M)),
                            ("utf16", enc.encode_batch_padded_utf16(flat, uoffs, ML, index, bos, eos, 0, cut, side, M))):
                host = dict(total=r[5], W=r[0].shape[1], n_cut=r[6], ids=r[0].reshape(-1).astype(np.int64), mask=r[1].reshape(-1).astype(np.int64),
                            pos=r[2].reshape(-1).astype(np.int64), lens=r[3].tolist(), offs=r[4].tolist())
                assert_padded("agreement: " + name, host, m)
                assert r[0].shape == r[1].shape == r[2].shape == (len(docs), m.W) and r[1].dtype == np.uint8
            assert enc.padded_calls() == c0 + 3


# ---- 8. retry ----

def check_retry(make_ctx):
    """the first call of a fresh encoder is a padded call whose miss lists overflow (CJK text under gpt2, consonant strings): the attempt is run again inside the
    call, and the caller's buffers hold the final attempt's rows only"""
    ctx = make_ctx()
    rng, gib, mixed, crowded = CC.generators(47)
    cjk = "漢字かな交じり文、한국어 " + EMOJI + " naïve café "
    docs = [(cjk * 80).encode("utf-8")] + CC.cut(gib(30000, 2, 2).encode(), [700, 9000]) + [b"", CC.fill(rng, 300)]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    w0 = ctx.enc.workspace_bytes
    first = check_device(ctx, docs, 512, "retry: first call", 7, 9, M=64, ids_per_doc=ids, b=b, exact=True)
    assert ctx.enc.workspace_bytes > w0
    again = check_device(ctx, docs, 512, "retry: again", 7, 9, M=64, ids_per_doc=ids, b=b, exact=True)
    assert (first.total, first.W) == (again.total, again.W) and first.n_cut >= 2
    check_device(ctx, docs, 512, "retry: the tails", cut=PREFIX, side=LEFT, ids_per_doc=ids, b=b)


# ---- 9. the Python mirror ----

def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    oenc = O.Encoder(O.Vocab(raw_gpt2), N.P1, specials=specials)
    lines = lib_rs_text.split("\n")
    want = [oenc.encode(t, [EOT]) for t in lines]
    L = 24
    ids, mask, lens, pos = tok.EncodeBatchPadded(lines, L, eos=EOT, pad_to_multiple_of=8, return_pos=True)
    m = Model(want, L, -1, 50256, 0, M=8)
    assert ids.shape == mask.shape == pos.shape == (len(lines), m.W) and ids.dtype == np.int32 and mask.dtype == np.uint8 and m.n_cut >= 3
    assert (ids.tolist(), mask.tolist(), pos.tolist(), lens.tolist()) == (m.ids.tolist(), m.mask.tolist(), m.pos.tolist(), m.lens)
    # ... and against EncodeBatch plus the host loop this call replaces
    loop = np.zeros((len(lines), m.W), np.int64)
    for d, di in enumerate(tok.EncodeBatch(lines, [EOT])):
        row = di[:L - 1] + [50256]
        loop[d, :len(row)] = row
    assert ids.tolist() == loop.tolist()
    # the tails, padded on the left to the fixed width; bos as an int, eos as a literal, another pad; the literal in the text allowed and not
    text = ["a" + EOT + "b", "", "Hi " + EMOJI + " café", " the of and to in is that for it with"]
    for apply in (True, False):
        ids, mask, lens = tok.EncodeBatchPadded(text, 6, apply, bos=11, eos=EOT, pad=-1, truncation_side="left", padding_side="left", fixed_width=True)
        m = Model([oenc.encode(t, [EOT] if apply else []) for t in text], 6, 11, 50256, -1, PREFIX, LEFT, 0)
        assert (ids.tolist(), mask.tolist(), lens.tolist()) == (m.ids.tolist(), m.mask.tolist(), m.lens) and ids.shape == (4, 6)
    ids, mask, lens = tok.EncodeBatchPadded([], 4, eos=EOT)
    assert ids.shape == mask.shape == (0, 0) and lens.tolist() == []
    for bad in (dict(max_length=0), dict(max_length=1, bos=11, eos=EOT), dict(max_length=4, bos="<|nope|>"), dict(max_length=4, eos=-5), dict(max_length=4, pad_to_multiple_of=0),
                dict(max_length=4, truncation_side="up"), dict(max_length=4, padding_side="down")):
        with pytest.raises(ValueError):
            tok.EncodeBatchPadded(text, **bad)
    # a literal that holds U+FFFD beside a lone surrogate: through the UTF-16 entry
    fffd = {k: v + 200000 for k, v in U16S.FFFD_SPECIALS.items()}
    tok3 = TokenizerBuilder.CreateTokenizer(raw_gpt2, fffd, REGEX_PATTERN_1, lib=lib)
    lone = ["ab x\ud83d b x� c it's", "plain"]
    ids, mask, lens = tok3.EncodeBatchPadded(lone, 8, list(fffd), eos=3)
    exp = U16S.Expect(O, O.Vocab(raw_gpt2), N.P1, fffd)
    m = Model([exp.encode(U16S.units(t), list(fffd)) for t in lone], 8, -1, 3, 0)
    assert (ids.tolist(), mask.tolist(), lens.tolist()) == (m.ids.tolist(), m.mask.tolist(), m.lens)
