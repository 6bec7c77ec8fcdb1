"""Length-bucketed padded rows (tkz_encode_batch_bucketed_device / _utf8 / _utf16; k_bkt_hist, k_bkt_scatter, k_bkt_table, k_bkt_write): the cases and comparisons
the emulated (CPU) and the GPU test modules share.  Every comparison is exact.

No expected value comes from the code under test or from the padded entry.  The model (`Model`) is numpy over the ORACLE's ids (padded_cases.Ctx.oracle_ids) and
restates the rule of tkz.h: the cut and the framing, the stable order by len (numpy.argsort, kind="stable", of len or of -len), the buckets of B sorted rows, a
width per bucket, the offsets, the rows, the mask and pos.  BESIDE it, `assert_property` holds every bucket against what tkz_encode_batch_padded_device writes for
the bucket's documents with the same parameters.

The kernel cases go through tkz_encode_batch_bucketed_device with GUARD words behind every output array, which must be intact afterwards -- and so must
everything at or behind P, n_docs, n_docs + 1, n_buckets and n_buckets + 1.

Geometry (tkz_kernels.h): the sort takes a workgroup per tile of T = kBktSortTile keys, k_bkt_write a wavefront per tile of K = kBktTile output positions, four
wavefronts a workgroup, at most GRID workgroups (k_pad_lens likewise).  Documents are short words of one token each, so a case is a few tens of KB.
"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import count_cases as CC
import padded_cases as PD
import parity
import spans_cases as SP
import special_cases as SC
import u16_cases as U16
import u16_special_cases as U16S
from conftest import ROOT
from tokenizer_amd import _native as N

_HEAD = open(os.path.join(ROOT, "tokenizer_amd", "csrc", "tkz_kernels.h")).read()
T = int(re.search(r"\bkBktSortTile = (\d+)\b", _HEAD).group(1))
K = int(re.search(r"\bkBktTile = (\d+)\b", _HEAD).group(1))
GRID = PD.GRID
EOT, EOT_ID, EMOJI, GUARD, FORMS = PD.EOT, PD.EOT_ID, PD.EMOJI, PD.GUARD, PD.FORMS
SUFFIX, PREFIX, RIGHT, LEFT, SIDES = PD.SUFFIX, PD.PREFIX, PD.RIGHT, PD.LEFT, PD.SIDES
ASC, DESC = N.BUCKET_ASCENDING, N.BUCKET_DESCENDING
BMAX = (1 << 31) - 1
# mask, pos, offsets and rank present and NULL: all, none, and two that tell the four apart
ARRAYS = ((True, True, True, True), (False, False, False, False), (True, False, True, False), (False, True, False, True))
words = PD.words


class Model:
    """the rule of tkz.h over the oracle's ids of every document"""

    def __init__(self, ids_per_doc, L, B, order=ASC, bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1):
        fb, fe = int(bos >= 0), int(eos >= 0)
        f, n = fb + fe, len(ids_per_doc)
        assert max(1, f) <= L and 1 <= B <= BMAX and order in (ASC, DESC)
        content = []
        for di in ids_per_doc:
            di = list(di)
            k = min(len(di), L - f)
            content.append([bos] * fb + (di[:k] if cut == SUFFIX else di[len(di) - k:]) + [eos] * fe)
        self.offs = [0] + np.cumsum([len(di) for di in ids_per_doc], dtype=np.int64).tolist()
        self.total = self.offs[-1]
        self.lens = [len(c) for c in content]
        self.n_cut = sum(len(di) > L - f for di in ids_per_doc)
        lens = np.asarray(self.lens, np.int64)
        self.order = np.argsort(lens if order == ASC else -lens, kind="stable").tolist()
        self.rank = [0] * n
        for r, d in enumerate(self.order):
            self.rank[d] = r
        self.nb = nb = -(-n // B)
        self.widths, self.boffs, self.blocks = [], [0], []
        for b in range(nb):
            docs = self.order[b * B:(b + 1) * B]
            longest = max(self.lens[d] for d in docs)
            W = 0 if longest == 0 else (L if M == 0 else min(L, -(-longest // M) * M))
            ids, mask, pos = np.full((len(docs), W), pad, np.int64), np.zeros((len(docs), W), np.int64), np.zeros((len(docs), W), np.int64)
            for i, d in enumerate(docs):
                c = content[d]
                s = W - len(c) if side == LEFT else 0
                ids[i, s:s + len(c)] = c
                mask[i, s:s + len(c)] = 1
                pos[i, s:s + len(c)] = np.arange(len(c))
            self.widths.append(W)
            self.boffs.append(self.boffs[-1] + len(docs) * W)
            self.blocks.append((ids, mask, pos))
        self.P = self.boffs[-1]
        flat = lambda k: np.concatenate([blk[k].reshape(-1) for blk in self.blocks]).tolist() if self.blocks else []
        self.ids, self.mask, self.pos = flat(0), flat(1), flat(2)
        assert self.P <= n * L and len(self.ids) == self.P


class Ctx(PD.Ctx):
    """padded_cases.Ctx (the oracle's ids of every document, the padded entry's transport) with the transport of the bucketed entry."""

    def bucketed_device(self, b, L, B, order=ASC, index=(), bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1, arrays=(True, True, True, True), cap=None):
        """the device entry with guard words behind every buffer; a dict of the results cut to the figures the call returned"""
        wm, wp, wo, wr = arrays
        n = b["n"]
        nb = N.Encoder.bucket_count(n, B)
        cap = N.Encoder.padded_bounds(n, L) if cap is None else cap
        ids = self.upload(np.full(cap + GUARD, -7, np.int32))
        mask = self.upload(np.full(cap + GUARD, 0xA5, np.uint8)) if wm else (None, 0)
        pos = self.upload(np.full(cap + GUARD, -7, np.int32)) if wp else (None, 0)
        lens = self.upload(np.full(n + GUARD, -7, np.int32))
        out = self.upload(np.full(n + 1 + GUARD, -5, np.int64)) if wo else (None, 0)
        perm = self.upload(np.full(n + GUARD, -5, np.int64))
        rank = self.upload(np.full(n + GUARD, -5, np.int64)) if wr else (None, 0)
        boffs = self.upload(np.full(nb + 1 + GUARD, -5, np.int64))
        widths = self.upload(np.full(nb + GUARD, -7, np.int32))
        P = None
        try:
            total, P, n_cut = self.enc.encode_batch_bucketed_device(b["d_bytes"][1], b["d_offs"][1], n, b["total"], list(index), bos, eos, L, cut, side, pad, M, B, order,
                                                                    ids[1], cap, mask[1], pos[1], lens[1], out[1], perm[1], rank[1], boffs[1], widths[1])
        finally:                                              # (whatever the call returned: nothing behind the capacities it was told)
            assert (self.back(ids[0])[cap:] == -7).all() and (self.back(lens[0])[n:] == -7).all(), "guard words behind ids / lens"
            assert not wm or (self.back(mask[0])[cap:] == 0xA5).all(), "guard words behind the mask"
            assert not wp or (self.back(pos[0])[cap:] == -7).all(), "guard words behind pos"
            assert not wo or (self.back(out[0])[n + 1:] == -5).all(), "guard words behind the offsets"
            assert (self.back(perm[0])[n:] == -5).all() and (not wr or (self.back(rank[0])[n:] == -5).all()), "guard words behind order / rank"
            assert (self.back(boffs[0])[nb + 1:] == -5).all() and (self.back(widths[0])[nb:] == -7).all(), "guard words behind the bucket arrays"
        assert (self.back(ids[0])[P:] == -7).all() and (not wm or (self.back(mask[0])[P:] == 0xA5).all()) and (not wp or (self.back(pos[0])[P:] == -7).all()), \
            "written at or behind P"
        return dict(total=total, P=P, n_cut=n_cut, ids=self.back(ids[0])[:P].astype(np.int64), lens=self.back(lens[0])[:n].tolist(),
                    mask=self.back(mask[0])[:P].astype(np.int64) if wm else None, pos=self.back(pos[0])[:P].astype(np.int64) if wp else None,
                    offs=self.back(out[0])[:n + 1].tolist() if wo else None, order=self.back(perm[0])[:n].tolist(), rank=self.back(rank[0])[:n].tolist() if wr else None,
                    boffs=self.back(boffs[0])[:nb + 1].tolist(), widths=self.back(widths[0])[:nb].tolist())


def assert_bucketed(what, got, m):
    assert (got["total"], got["P"], got["n_cut"]) == (m.total, m.P, m.n_cut), (what, (got["total"], got["P"], got["n_cut"]), (m.total, m.P, m.n_cut))
    SP._same(what, "lens", [int(x) for x in got["lens"]], m.lens)
    SP._same(what, "order", [int(x) for x in got["order"]], m.order)
    SP._same(what, "widths", [int(x) for x in got["widths"]], m.widths)
    SP._same(what, "bucket offsets", [int(x) for x in got["boffs"]], m.boffs)
    SP._same(what, "ids", got["ids"].tolist(), m.ids)
    for name, want in (("mask", m.mask), ("pos", m.pos)):
        if got[name] is not None:
            SP._same(what, name, got[name].tolist(), want)
    for name, want in (("offs", m.offs), ("rank", m.rank)):
        if got[name] is not None:
            SP._same(what, name, [int(x) for x in got[name]], want)


def assert_property(ctx, what, docs, got, L, B, index=(), bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1, buckets=None):
    """bucket b equals what the PADDED entry writes for the documents order[b * B ..] with the same parameters"""
    nb = len(got["widths"])
    for b in (range(nb) if buckets is None else buckets):
        sub = [docs[d] for d in got["order"][b * B:(b + 1) * B]]
        p = ctx.padded_device(ctx.device_buffers(sub), L, index, bos, eos, pad, cut, side, M)
        assert p["W"] == got["widths"][b], (what, b, p["W"], got["widths"][b])
        lo, hi = got["boffs"][b], got["boffs"][b + 1]
        assert hi - lo == len(sub) * p["W"], (what, b)
        SP._same(what, "bucket %d against the padded entry: ids" % b, got["ids"][lo:hi].tolist(), p["ids"].tolist())
        SP._same(what, "bucket %d against the padded entry: mask" % b, got["mask"][lo:hi].tolist(), p["mask"].tolist())
        SP._same(what, "bucket %d against the padded entry: pos" % b, got["pos"][lo:hi].tolist(), p["pos"].tolist())
        assert p["lens"] == [got["lens"][d] for d in got["order"][b * B:(b + 1) * B]], (what, b)


def check_device(ctx, docs, L, B, what, order=ASC, bos=-1, eos=-1, pad=-3, cut=SUFFIX, side=RIGHT, M=1, allowed=(), arrays=((True, True, True, True),), ids_per_doc=None, b=None,
                 exact=False, prop=None):
    """the device entry against the model, with the capacity that always suffices (n_docs * L) or -- exact -- with P, not an entry more; prop: the buckets held
    against the padded entry as well (an iterable, or True for all of them)"""
    ids_per_doc = ids_per_doc if ids_per_doc is not None else ctx.oracle_ids(docs, allowed)
    m = Model(ids_per_doc, L, B, order, bos, eos, pad, cut, side, M)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = b or ctx.device_buffers(docs)
    for a in arrays:
        label = "%s, L %d, M %d, B %d, order %d, bos %d, eos %d, cut %d, pad side %d (mask %d, pos %d, offsets %d, rank %d)" % ((what, L, M, B, order, bos, eos, cut, side) + tuple(a))
        got = ctx.bucketed_device(b, L, B, order, index, bos, eos, pad, cut, side, M, a, cap=m.P if exact else None)
        assert_bucketed(label, got, m)
        if prop and a[0] and a[1]:
            assert_property(ctx, label, docs, got, L, B, index, bos, eos, pad, cut, side, M, None if prop is True else prop)
    return m


# ---- 1. the worked example of tkz.h ----

def check_worked_example(ctx):
    rng = random.Random(2)
    docs = [words(rng, n) for n in (5, 0, 2, 3, 2)]
    (a, _, c, d, e) = ids = ctx.oracle_ids(docs)
    assert [len(x) for x in ids] == [5, 0, 2, 3, 2]
    X, P = 9, 77
    b = ctx.device_buffers(docs)
    got = ctx.bucketed_device(b, 4, 2, ASC, (), -1, X, P, SUFFIX, RIGHT, 1)
    assert (got["total"], got["P"], got["n_cut"], got["lens"]) == (12, 18, 1, [4, 1, 3, 4, 3])
    assert (got["order"], got["rank"], got["widths"], got["boffs"]) == ([1, 2, 4, 0, 3], [3, 0, 1, 4, 2], [3, 4, 4], [0, 6, 14, 18])
    assert got["ids"].tolist() == [X, P, P, c[0], c[1], X, e[0], e[1], X, P, a[0], a[1], a[2], X, d[0], d[1], d[2], X]
    assert got["mask"].tolist() == [1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1] and got["pos"].tolist() == [0, 0, 0, 0, 1, 2, 0, 1, 2, 0, 0, 1, 2, 3, 0, 1, 2, 3]
    assert got["offs"] == [0, 5, 5, 7, 10, 12]
    assert_bucketed("the worked example, ascending", got, Model(ids, 4, 2, ASC, -1, X, P))
    got = ctx.bucketed_device(b, 4, 2, DESC, (), -1, X, P, SUFFIX, RIGHT, 1)
    assert (got["total"], got["P"], got["n_cut"], got["lens"]) == (12, 15, 1, [4, 1, 3, 4, 3])
    assert (got["order"], got["rank"], got["widths"], got["boffs"]) == ([0, 3, 2, 4, 1], [0, 4, 2, 1, 3], [4, 3, 1], [0, 8, 14, 15])
    assert got["ids"].tolist() == [a[0], a[1], a[2], X, d[0], d[1], d[2], X, c[0], c[1], X, e[0], e[1], X, X]
    assert got["mask"].tolist() == [1] * 15 and got["pos"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 0, 1, 2, 0]
    assert_bucketed("the worked example, descending", got, Model(ids, 4, 2, DESC, -1, X, P))
    assert ctx.padded_device(b, 4, (), -1, X, P)["W"] * 5 == 20      # (the padded entry writes 20 positions for the same batch)


# ---- 2. stability and ties ----

def check_ties(ctx):
    rng = random.Random(3)
    W = 7
    sizes = [(5 * d) % (W + 3) for d in range(150)]          # few distinct lengths, many ties
    docs = [words(rng, n) for n in sizes]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    for order in (ASC, DESC):
        m = check_device(ctx, docs, W, 64, "ties", order, eos=9, ids_per_doc=ids, b=b, arrays=ARRAYS, exact=True, prop=True)
        assert len(set(m.lens)) <= W and m.nb == 3 and len(m.blocks[2][0]) == 22
        for r in range(149):                                  # (ties keep ascending document index in BOTH directions)
            d0, d1 = m.order[r], m.order[r + 1]
            assert m.lens[d0] != m.lens[d1] or d0 < d1
    # all documents equal: the identity in both directions
    same = [words(rng, 3) for _ in range(70)]
    for order in (ASC, DESC):
        m = check_device(ctx, same, 8, 16, "all equal", order, bos=7, exact=True)
        assert m.order == list(range(70)) and m.rank == list(range(70)) and m.widths == [4] * 5


def check_sort_tiles(ctx):
    """n_docs one below, at and one above the sort's tile, and twice the tile"""
    rng = random.Random(5)
    lex = [words(rng, n) for n in range(6)]
    ids6 = ctx.oracle_ids(lex)
    for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        pick = [(7 * d + d // 5) % 6 for d in range(n)]
        docs, ids = [lex[k] for k in pick], [ids6[k] for k in pick]
        for order in (ASC, DESC):
            m = check_device(ctx, docs, 5, 300, "n_docs = %d" % n, order, eos=9, ids_per_doc=ids, exact=True, arrays=((True, False, True, True),))
            assert sorted(m.order) == list(range(n))


# ---- 3. digits ----

def check_digits(ctx, long_documents=False):
    rng = random.Random(7)
    sizes = [3, 257, 255, 0, 256, 256, 1, 255, 257, 40]       # the second pass decides
    docs = [words(rng, n) for n in sizes]
    ids = ctx.oracle_ids(docs)
    assert [len(x) for x in ids] == sizes
    b = ctx.device_buffers(docs)
    for order in (ASC, DESC):
        m = check_device(ctx, docs, 1000, 3, "255 / 256 / 257", order, ids_per_doc=ids, b=b, exact=True, prop=(0, 3))
        assert m.order == ([3, 6, 0, 9, 2, 7, 4, 5, 1, 8] if order == ASC else [1, 8, 4, 5, 2, 7, 9, 0, 6, 3])
        m = check_device(ctx, docs, 256, 3, "cut at 256", order, ids_per_doc=ids, b=b, exact=True)      # (the longest four tie at L: document order)
        assert m.n_cut == 2 and (m.order[-4:] == [1, 4, 5, 8] if order == ASC else m.order[:4] == [1, 4, 5, 8])
    # L = 2^31 - 1 on tiny documents: every pass the host schedules runs
    tiny = [words(rng, n) for n in (4, 0, 9, 2, 2, 7, 1)]
    for order in (ASC, DESC):
        for bos, eos in ((-1, -1), (7, 9)):
            m = check_device(ctx, tiny, BMAX, 2, "L = 2^31 - 1", order, bos, eos, exact=True, arrays=ARRAYS)
            assert m.n_cut == 0 and max(m.widths) == 9 + (bos >= 0) + (eos >= 0)
    if long_documents:                                        # three passes
        sizes = [5, 65537, 65535, 0, 65536, 12]
        docs = [words(rng, n) for n in sizes]
        ids = ctx.oracle_ids(docs)
        assert [len(x) for x in ids] == sizes
        b = ctx.device_buffers(docs)
        for order in (ASC, DESC):
            m = check_device(ctx, docs, 1 << 20, 2, "65,535 / 65,536 / 65,537", order, ids_per_doc=ids, b=b, exact=True, arrays=((True, True, False, True),))
            assert m.order == ([3, 0, 5, 2, 4, 1] if order == ASC else [1, 4, 2, 5, 0, 3])


# ---- 4. more than the grids hold ----

def check_grid_stride(ctx, lib):
    """more documents than k_pad_lens has lanes -- empty ones, a row of one framing id each, all tie; two that are not -- and ONE fixed-width bucket of more tiles
    than the writer's capped grid has wavefronts, nearly all of it padding"""
    rng = random.Random(9)
    n = GRID * 256 + 300
    docs = [b""] * n
    docs[7], docs[n - 2] = words(rng, 3), words(rng, 2)
    ids = [[]] * n
    ids[7], ids[n - 2] = ctx.oracle_ids([docs[7]])[0], ctx.oracle_ids([docs[n - 2]])[0]
    b = ctx.device_buffers(docs)
    m = check_device(ctx, docs, 2, 100000, "grid stride: documents", ASC, 7, -1, arrays=((True, False, True, True),), ids_per_doc=ids, b=b, exact=True)
    assert (m.n_cut, m.total, m.nb) == (2, 5, 6) and m.lens.count(1) == n - 2
    assert m.order == [d for d in range(n) if d not in (7, n - 2)] + [7, n - 2] and m.widths == [1] * 5 + [2]
    L = (GRID * 4 + 3) * K + 5
    for side in (RIGHT, LEFT):
        m = check_device(ctx, [words(rng, 5)], L, 1, "grid stride: tiles", DESC, eos=9, side=side, M=0, arrays=((False, False, False, False),), exact=True)
        assert m.widths == [L] and m.P == L > GRID * 4 * K and m.lens == [6]


# ---- 5. buckets ----

def check_buckets(ctx):
    rng = random.Random(11)
    n = 150
    sizes = [(11 * d + d // 7) % 40 for d in range(n)]
    docs = [words(rng, k) for k in sizes]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    for B in (1, 64, n - 1, n, n + 1, BMAX):
        for order in (ASC, DESC):
            m = check_device(ctx, docs, 30, B, "B = %d" % B, order, 7, 9, ids_per_doc=ids, b=b, exact=True, M=8, prop=(0, -(-n // B) - 1))
            assert m.nb == -(-n // B) and m.n_cut == sum(k > 28 for k in sizes)
            if B == 64:                                       # a last bucket of 22 rows; M rounds every bucket by itself, the longest is clipped at L
                assert len(m.blocks[2][0]) == 22 and all(w % 8 == 0 or w == 30 for w in m.widths) and 30 in m.widths and len(set(m.widths)) >= 2
                assert m.widths == sorted(m.widths, reverse=order == DESC) and m.P < n * 30
    # M == 0: every bucket is L wide; M rounding below L; a round-up beyond L clipped
    for order in (ASC, DESC):
        m = check_device(ctx, docs, 64, 32, "M = 0", order, eos=9, ids_per_doc=ids, b=b, exact=True, M=0)
        assert m.widths == [64] * 5 and m.P == n * 64
        m = check_device(ctx, docs, 37, 32, "M = 16 clipped", order, eos=9, ids_per_doc=ids, b=b, exact=True, M=16, cut=PREFIX, side=LEFT, prop=(4,))
        assert set(m.widths) <= {16, 32, 37} and 37 in m.widths
    # buckets of width 0: empty documents, no framing, ascending -- their offsets equal their neighbour's and nothing is written for them
    docs0 = [words(rng, 2), b"", b"", words(rng, 1), b"", b"", b"", words(rng, 4)]
    m = check_device(ctx, docs0, 8, 2, "width 0", ASC, arrays=ARRAYS, exact=True, prop=True)
    assert m.widths == [0, 0, 1, 4] and m.boffs == [0, 0, 0, 2, 10] and m.order == [1, 2, 4, 5, 6, 3, 0, 7]
    m = check_device(ctx, docs0, 8, 2, "width 0, descending", DESC, arrays=ARRAYS, exact=True)
    assert m.widths == [4, 1, 0, 0] and m.boffs == [0, 8, 10, 10, 10]
    m = check_device(ctx, [b""] * 5, 8, 2, "nothing but width 0", ASC, arrays=ARRAYS, exact=True)
    assert (m.P, m.widths, m.boffs) == (0, [0, 0, 0], [0, 0, 0, 0])


# ---- 6. the writer's geometry ----

def check_geometry(ctx):
    rng = random.Random(13)
    # B = 1 with widths 0 .. 5: one tile spans hundreds of buckets
    sizes = [(7 * d + d // 6) % 6 for d in range(900)]
    lex = [words(rng, k) for k in range(6)]
    ids6 = ctx.oracle_ids(lex)
    docs, ids = [lex[k] for k in sizes], [ids6[k] for k in sizes]
    b = ctx.device_buffers(docs)
    for order, (cut, side) in zip((ASC, DESC, ASC, DESC), SIDES):
        m = check_device(ctx, docs, 5, 1, "B = 1", order, cut=cut, side=side, ids_per_doc=ids, b=b, exact=True, arrays=ARRAYS)
        assert m.nb == 900 and m.P == sum(sizes) > 2 * K
        m = check_device(ctx, docs, 6, 3, "B = 3", order, eos=9, cut=cut, side=side, ids_per_doc=ids, b=b, exact=True, M=4)
    # a bucket base one below, at and one above a tile multiple; a row across two and three tiles
    for first in (K - 1, K, K + 1, 2 * K + 5):
        docs = [words(rng, 5), words(rng, first - 1), words(rng, 70), b"", words(rng, 64)]
        ids = ctx.oracle_ids(docs)
        b = ctx.device_buffers(docs)
        for cut, side in SIDES:
            m = check_device(ctx, docs, 3 * K, 1, "first bucket of %d" % first, DESC, eos=9, cut=cut, side=side, ids_per_doc=ids, b=b, exact=True, arrays=ARRAYS[:2])
            assert m.boffs[:3] == [0, first, first + 71]
            m = check_device(ctx, docs, first - 7, 2, "rows across tiles", ASC, 7, 9, cut=cut, side=side, ids_per_doc=ids, b=b, exact=True, M=0, prop=(0, 2))
            assert m.n_cut == 1 and m.widths == [first - 7] * 3


# ---- 7. special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    docs = [(" the of" + EOT + " and to in").encode(), (" is that for" + EOT).encode(), b"", EOT.encode()]
    ids = ctx.oracle_ids(docs, [EOT])
    assert [len(x) for x in ids] == [6, 4, 0, 1] and ids[0][2] == ids[1][3] == ids[3][0] == eot
    b = ctx.device_buffers(docs)
    for L in (3, 4, 5, 8):
        for order, (cut, side) in zip((ASC, DESC, DESC, ASC), SIDES):
            m = check_device(ctx, docs, L, 2, "special: allowed", order, eos=eot, cut=cut, side=side, allowed=[EOT], ids_per_doc=ids, b=b, prop=True)
            assert m.lens == [min(6, L - 1) + 1, min(4, L - 1) + 1, 1, 2]
    s0 = ctx.enc.special_stats()
    off = check_device(ctx, docs, 6, 2, "special: registered, not allowed", eos=eot, allowed=[])
    assert off.total > sum(map(len, ids)) and ctx.enc.special_stats() == s0              # (split as plain text)


# ---- 8. capacity and arguments ----

def check_capacity(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, lib = ctx.enc, ctx.enc.lib.L
    rng = random.Random(17)
    docs = [words(rng, 9), b"", words(rng, 30), (" the" + EOT + " of").encode(), words(rng, 2)]
    n, ML, B = len(docs), 16, 2
    m = Model(ctx.oracle_ids(docs, [EOT]), ML, B, DESC, 7, eot, 0, M=8)
    assert (m.widths, m.P, m.n_cut) == ([16, 8, 8], 56, 1)
    b = ctx.device_buffers(docs)
    c0 = enc.bucketed_calls()
    for cap in (m.P - 1, 16, 0):
        with pytest.raises(N.TkzError) as ei:
            ctx.bucketed_device(b, ML, B, DESC, [0], 7, eot, 0, M=8, cap=cap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_positions, ei.value.n_cut) == (m.total, m.P, m.n_cut), cap
    assert enc.bucketed_calls() == c0                            # failed calls are not counted
    for a in ARRAYS:                                             # the exact capacity, sized from the figures above
        assert_bucketed("exact capacity", ctx.bucketed_device(b, ML, B, DESC, [0], 7, eot, 0, M=8, arrays=a, cap=m.P), m)
    assert enc.bucketed_calls() == c0 + 4
    data, offs = parity.pack(docs)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_bucketed(data, offs, ML, B, DESC, [0], 7, eot, pad_multiple=8, out_cap=m.P - 1)
    assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_positions, ei.value.n_cut) == (m.total, m.P, m.n_cut)
    r = enc.encode_batch_bucketed(data, offs, ML, B, DESC, [0], 7, eot, pad_multiple=8, out_cap=m.P)
    assert (r[0].tolist(), r[1].tolist(), r[2].tolist(), r[3].tolist(), r[4].tolist()) == (m.ids, m.mask, m.pos, m.lens, m.offs)
    assert (r[5].tolist(), r[6].tolist(), r[7].tolist(), r[8].tolist(), r[9], r[10]) == (m.order, m.rank, m.boffs, m.widths, m.total, m.n_cut)
    # every TKZ_E_ARG of the rule: the padded entry's rows, B < 1, B > 2^31 - 1, an order that is neither
    bad = (dict(bos=-2), dict(eos=-2), dict(eos=-(1 << 31)), dict(L=0), dict(L=-4), dict(L=1 << 31), dict(L=1), dict(cut=2), dict(cut=-1), dict(side=2), dict(side=-1),
           dict(M=-1), dict(M=1 << 31), dict(index=[1]), dict(index=[0, 0]), dict(index=[-1]), dict(B=0), dict(B=-1), dict(B=1 << 31), dict(order=2), dict(order=-1))
    for kw in bad:
        a = dict(L=ML, index=[0], bos=7, eos=eot, cut=SUFFIX, side=RIGHT, M=8, B=B, order=ASC)
        a.update(kw)
        cap = n * ML
        with pytest.raises(N.TkzError) as ei:
            pd = ctx.upload(np.zeros(cap, np.int32)), ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n, np.int64)), ctx.upload(np.zeros(n + 1, np.int64)), \
                ctx.upload(np.zeros(n, np.int32))
            enc.encode_batch_bucketed_device(b["d_bytes"][1], b["d_offs"][1], n, b["total"], a["index"], a["bos"], a["eos"], a["L"], a["cut"], a["side"], 0, a["M"], a["B"],
                                             a["order"], pd[0][1], cap, 0, 0, pd[1][1], 0, pd[2][1], 0, pd[3][1], pd[4][1])
        assert ei.value.code == N.E_ARG, kw
        if "index" not in kw:
            for call in (lambda: enc.encode_batch_bucketed(data, offs, a["L"], a["B"], a["order"], [0], a["bos"], a["eos"], 0, a["cut"], a["side"], a["M"], out_cap=cap),
                         lambda: enc.encode_batch_bucketed_utf16(np.asarray([65, 66], np.uint16), np.asarray([0, 2], np.int64), a["L"], a["B"], a["order"], [0], a["bos"],
                                                                 a["eos"], 0, a["cut"], a["side"], a["M"], out_cap=64)):
                with pytest.raises(N.TkzError) as ei:
                    call()
                assert ei.value.code == N.E_ARG, kw
    # NULL for a required pointer; for one that may be NULL
    nb = m.nb
    plain = Model(ctx.oracle_ids(docs), ML, B, DESC, 7, eot, 0, M=8)          # (nothing allowed below: the literal is plain text)
    ids, msk, pos = ctx.upload(np.zeros(plain.P, np.int32)), ctx.upload(np.zeros(plain.P, np.uint8)), ctx.upload(np.zeros(plain.P, np.int32))
    lens, ooff, perm, rank = ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n + 1, np.int64)), ctx.upload(np.zeros(n, np.int64)), ctx.upload(np.zeros(n, np.int64))
    boffs, wid = ctx.upload(np.zeros(nb + 1, np.int64)), ctx.upload(np.zeros(nb, np.int32))
    t, p, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ok = (enc._h, b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], None, 0, 7, eot, ML, SUFFIX, RIGHT, 0, 8, B, DESC, ids[1], plain.P, msk[1], pos[1], lens[1], ooff[1],
          perm[1], rank[1], boffs[1], wid[1], None, C.byref(t), C.byref(p), C.byref(c))
    assert lib.tkz_encode_batch_bucketed_device(*ok) == N.OK and (t.value, p.value, c.value) == (plain.total, plain.P, plain.n_cut)
    assert ctx.back(perm[0]).tolist() == plain.order and ctx.back(boffs[0]).tolist() == plain.boffs and ctx.back(wid[0]).tolist() == plain.widths
    for k in (0, 1, 2, 16, 20, 22, 24, 25, 27, 28, 29):          # the encoder, the bytes, the offsets, d_out_ids, d_lens, d_order, the bucket arrays, the three scalars
        assert lib.tkz_encode_batch_bucketed_device(*(ok[:k] + (None,) + ok[k + 1:])) == N.E_ARG, k
    for k in (18, 19, 21, 23):                                   # d_mask, d_pos, d_out_offsets, d_rank
        assert lib.tkz_encode_batch_bucketed_device(*(ok[:k] + (None,) + ok[k + 1:])) == N.OK, k
    assert lib.tkz_encode_batch_bucketed_device(*(ok[:17] + (-1,) + ok[18:])) == N.E_ARG
    hid, hl, hp, hb, hw = np.zeros(plain.P, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(nb + 1, np.int64), np.zeros(nb, np.int32)
    hok = (enc._h, data.ctypes.data, offs.ctypes.data, n, None, 0, 7, eot, ML, SUFFIX, RIGHT, 0, 8, B, DESC, hid.ctypes.data, plain.P, None, None, hl.ctypes.data, None,
           hp.ctypes.data, None, hb.ctypes.data, hw.ctypes.data, C.byref(t), C.byref(p), C.byref(c))
    assert lib.tkz_encode_batch_bucketed_utf8(*hok) == N.OK and p.value == plain.P
    assert (hl.tolist(), hid.tolist(), hp.tolist(), hb.tolist(), hw.tolist()) == (plain.lens, plain.ids, plain.order, plain.boffs, plain.widths)
    for k in (0, 2, 15, 19, 21, 23, 24, 25, 26, 27):             # the encoder, the offsets, out_ids, lens, order, the bucket arrays, the three scalars
        assert lib.tkz_encode_batch_bucketed_utf8(*(hok[:k] + (None,) + hok[k + 1:])) == N.E_ARG, k
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        ctx.bucketed_device(ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]), ML, B, eos=9)
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_bucketed(data, np.asarray([0, 12, 11, 40, 50, len(data)], np.int64), ML, B)
    assert ei.value.code == N.E_ARG
    # no documents: TKZ_OK, bucket_offsets[0] and out_offsets[0] cleared, all scalars 0; documents without bytes through the host entries
    none = ctx.device_buffers([])
    for bos, eos in FORMS:
        got = ctx.bucketed_device(none, ML, B, ASC, (), bos, eos, cap=0)
        assert (got["total"], got["P"], got["n_cut"], got["offs"], got["lens"], got["order"], got["boffs"], got["widths"]) == (0, 0, 0, [0], [], [], [0], [])
        m3 = Model([[], [], []], 4, 2, DESC, bos, eos, 5, side=LEFT, M=2)
        for r in (enc.encode_batch_bucketed(np.zeros(0, np.uint8), np.zeros(4, np.int64), 4, 2, DESC, (), bos, eos, 5, pad_side=LEFT, pad_multiple=2),
                  enc.encode_batch_bucketed_utf16(np.zeros(0, np.uint16), np.zeros(4, np.int64), 4, 2, DESC, (), bos, eos, 5, pad_side=LEFT, pad_multiple=2)):
            assert (r[0].tolist(), r[1].tolist(), r[2].tolist(), r[3].tolist(), r[4].tolist(), r[5].tolist(), r[6].tolist(), r[7].tolist(), r[8].tolist(), r[9], r[10]) == \
                (m3.ids, m3.mask, m3.pos, m3.lens, [0, 0, 0, 0], [0, 1, 2], [0, 1, 2], m3.boffs, m3.widths, 0, 0)
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    d1, o1 = parity.pack([b"a<|s7|>b"])
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_batch_bucketed(d1, o1, 4, 1, ASC, [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_batch_bucketed(d1, o1, 64, 1)[9] == len(many.oenc.encode_bytes(b"a<|s7|>b"))          # (nothing allowed: the plain call)


# ---- 9. agreement of the entries ----

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
        for bos, eos, ML, B, order, cut, side, M in ((-1, -1, 64, 4, ASC, SUFFIX, RIGHT, 1), (7, eot, 64, 2, DESC, PREFIX, LEFT, 8), (-1, eot, 1000, 9, ASC, SUFFIX, LEFT, 0),
                                                    (-1, eot, 5000, 3, DESC, PREFIX, RIGHT, 64)):
            m = Model(want, ML, B, order, bos, eos, 0, cut, side, M)
            c0 = enc.bucketed_calls()
            assert_bucketed("agreement: device", ctx.bucketed_device(b, ML, B, order, index, bos, eos, 0, cut, side, M), m)
            assert parity.read_device_i64(lib, enc.counts_device, 3).tolist() == [len(docs), len(data), m.total]      # the counts block receives the uncut total
            for name, r in (("utf8", enc.encode_batch_bucketed(data, offs, ML, B, order, index, bos, eos, 0, cut, side, M)),
                            ("utf16", enc.encode_batch_bucketed_utf16(flat, uoffs, ML, B, order, index, bos, eos, 0, cut, side, M))):
                host = dict(total=r[9], P=len(r[0]), n_cut=r[10], ids=r[0].astype(np.int64), mask=r[1].astype(np.int64), pos=r[2].astype(np.int64), lens=r[3].tolist(),
                            offs=r[4].tolist(), order=r[5].tolist(), rank=r[6].tolist(), boffs=r[7].tolist(), widths=r[8].tolist())
                assert_bucketed("agreement: " + name, host, m)
                assert r[1].dtype == np.uint8 and r[5].dtype == np.int64 and r[8].dtype == np.int32
            assert enc.bucketed_calls() == c0 + 3


# ---- 10. retry ----

def check_retry(make_ctx):
    """the first call of a fresh encoder is a bucketed call whose miss lists overflow (CJK text under gpt2, consonant strings): the attempt is run again inside
    the call, and the caller's buffers hold the final attempt's results only"""
    ctx = make_ctx()
    rng, gib, mixed, crowded = CC.generators(47)
    cjk = "漢字かな交じり文、한국어 " + EMOJI + " naïve café "
    docs = [(cjk * 80).encode("utf-8")] + CC.cut(gib(30000, 2, 2).encode(), [700, 9000]) + [b"", CC.fill(rng, 300)]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    w0 = ctx.enc.workspace_bytes
    first = check_device(ctx, docs, 512, 2, "retry: first call", DESC, 7, 9, M=64, ids_per_doc=ids, b=b, exact=True, arrays=ARRAYS[:1])
    assert ctx.enc.workspace_bytes > w0
    again = check_device(ctx, docs, 512, 2, "retry: again", DESC, 7, 9, M=64, ids_per_doc=ids, b=b, exact=True)
    assert (first.total, first.P) == (again.total, again.P) and first.n_cut >= 2
    check_device(ctx, docs, 512, 3, "retry: the tails", ASC, cut=PREFIX, side=LEFT, ids_per_doc=ids, b=b)


# ---- 11. the Python mirror ----

def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    oenc = O.Encoder(O.Vocab(raw_gpt2), N.P1, specials=specials)
    lines = lib_rs_text.split("\n")
    want = [oenc.encode(t, [EOT]) for t in lines]
    L, B = 24, 16
    for desc in (False, True):
        buckets, order, rank, lens = tok.EncodeBatchBucketed(lines, L, B, eos=EOT, pad_to_multiple_of=8, descending=desc, return_pos=True)
        m = Model(want, L, B, DESC if desc else ASC, -1, 50256, 0, M=8)
        assert len(buckets) == m.nb and (order.tolist(), rank.tolist(), lens.tolist()) == (m.order, m.rank, m.lens) and m.n_cut >= 3 and len(set(m.widths)) >= 2
        for (ids, mask, pos), (wi, wm, wp) in zip(buckets, m.blocks):
            assert ids.shape == mask.shape == pos.shape == wi.shape and ids.dtype == np.int32 and mask.dtype == np.uint8
            assert (ids.tolist(), mask.tolist(), pos.tolist()) == (wi.tolist(), wm.tolist(), wp.tolist())
        assert buckets[0][0].base is not None and all(x[0].base is buckets[0][0].base for x in buckets if x[0].size)      # (views of the one buffer)
    # the tails, padded on the left to the fixed width; bos as an int, eos as a literal, another pad; the literal in the text allowed and not
    text = ["a" + EOT + "b", "", "Hi " + EMOJI + " café", " the of and to in is that for it with"]
    for apply in (True, False):
        buckets, order, rank, lens = tok.EncodeBatchBucketed(text, 6, 3, apply, bos=11, eos=EOT, pad=-1, truncation_side="left", padding_side="left", fixed_width=True)
        m = Model([oenc.encode(t, [EOT] if apply else []) for t in text], 6, 3, ASC, 11, 50256, -1, PREFIX, LEFT, 0)
        assert [(i.tolist(), k.tolist()) for i, k in buckets] == [(x[0].tolist(), x[1].tolist()) for x in m.blocks] and (order.tolist(), lens.tolist()) == (m.order, m.lens)
    buckets, order, rank, lens = tok.EncodeBatchBucketed([], 4, 2, eos=EOT)
    assert buckets == [] and order.tolist() == rank.tolist() == lens.tolist() == []
    for bad in (dict(max_length=0, bucket_rows=2), dict(max_length=1, bucket_rows=2, bos=11, eos=EOT), dict(max_length=4, bucket_rows=0), dict(max_length=4, bucket_rows=1 << 31),
                dict(max_length=4, bucket_rows=2, pad_to_multiple_of=0), dict(max_length=4, bucket_rows=2, truncation_side="up"), dict(max_length=4, bucket_rows=2, padding_side="down")):
        with pytest.raises(ValueError):
            tok.EncodeBatchBucketed(text, **bad)
    # a literal that holds U+FFFD beside a lone surrogate: through the UTF-16 entry
    fffd = {k: v + 200000 for k, v in U16S.FFFD_SPECIALS.items()}
    tok3 = TokenizerBuilder.CreateTokenizer(raw_gpt2, fffd, REGEX_PATTERN_1, lib=lib)
    lone = ["ab x\ud83d b x� c it's", "plain"]
    buckets, order, rank, lens = tok3.EncodeBatchBucketed(lone, 8, 1, list(fffd), eos=3, descending=True)
    exp = U16S.Expect(O, O.Vocab(raw_gpt2), N.P1, fffd)
    m = Model([exp.encode(U16S.units(t), list(fffd)) for t in lone], 8, 1, DESC, -1, 3, 0)
    assert [(i.tolist(), k.tolist()) for i, k in buckets] == [(x[0].tolist(), x[1].tolist()) for x in m.blocks] and (order.tolist(), lens.tolist()) == (m.order, m.lens)
