"""Token-budget buckets (tkz_encode_batch_budgeted_device / _utf8 / _utf16; k_tbk_mark, k_tbk_chain, k_tbk_table, k_tbk_write): the cases and comparisons the
emulated (CPU) and the GPU test modules share.  Every comparison is exact.

No expected value comes from the code under test.  The model (`Model`) is numpy over the ORACLE's ids (padded_cases.Ctx.oracle_ids) and restates the rule of tkz.h
as the SEQUENTIAL greedy loop: the cut and the framing, the stable order by len, then bucket after bucket -- a bucket takes the next sorted row while it has fewer
than B rows and (rows + 1) * w(longest len) <= T.  The device walks the runs of equal width instead; that the two agree is what is tested.  BESIDE the model,
`assert_property` holds every bucket against what tkz_encode_batch_padded_device writes for the bucket's documents, and `check_row_cap_only` every array against
the bucketed entry's where only B binds.

The kernel cases go through tkz_encode_batch_budgeted_device with GUARD words behind every output array, which must be intact afterwards -- and so must
everything at or behind P, n_docs, n_docs + 1, n_buckets and n_buckets + 1, in bucket arrays that are larger than that.

Geometry (tkz_kernels.h): the sort takes a workgroup per tile of T_SORT = kBktSortTile keys, k_tbk_mark one per tile of T_MARK = kTbkMarkTile sorted rows, the chain
looks at LOOK = kTbkLook runs at once, k_tbk_write takes a wavefront per tile of kBktTile positions.  Documents are short words of one token each.
"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import bucketed_cases as BK
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
T_SORT = BK.T
T_MARK = int(re.search(r"\bkTbkMarkTile = (\d+)\b", _HEAD).group(1))
LOOK = int(re.search(r"\bkTbkLook = (\d+)\b", _HEAD).group(1))
GRID = PD.GRID
EOT, EOT_ID, EMOJI, GUARD, FORMS = PD.EOT, PD.EOT_ID, PD.EMOJI, PD.GUARD, PD.FORMS
SUFFIX, PREFIX, RIGHT, LEFT, SIDES = PD.SUFFIX, PD.PREFIX, PD.RIGHT, PD.LEFT, PD.SIDES
ASC, DESC = N.BUCKET_ASCENDING, N.BUCKET_DESCENDING
NONE = N.NO_ROW_CAP                                        # B = 2^31 - 1: no cap on the rows of a bucket
TMAX = 1 << 62
ARRAYS = BK.ARRAYS
words = PD.words


def width(l, L, M):
    """w(l) of tkz.h"""
    return 0 if l == 0 else (L if M == 0 else min(L, -(-l // M) * M))


class Model:
    """the rule of tkz.h over the oracle's ids of every document: the sequential greedy loop"""

    def __init__(self, ids_per_doc, L, T, B=NONE, order=ASC, bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1):
        fb, fe = int(bos >= 0), int(eos >= 0)
        f, n = fb + fe, len(ids_per_doc)
        assert max(1, f) <= L <= T <= TMAX and 1 <= B <= NONE and order in (ASC, DESC)
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
        self.sorted_w = sw = [width(self.lens[d], L, M) for d in self.order]
        self.rows = [0] if n else [0]
        s = 0
        while s < n:                                       # bucket after bucket, row after row
            e = s + 1
            while e < n and e + 1 - s <= B and (e + 1 - s) * (sw[e] if order == ASC else sw[s]) <= T:
                e += 1
            self.rows.append(e)
            s = e
        self.nb = len(self.rows) - 1
        self.widths, self.boffs, self.blocks = [], [0], []
        for b in range(self.nb):
            docs = self.order[self.rows[b]:self.rows[b + 1]]
            W = max(width(self.lens[d], L, M) for d in docs)
            assert W == (sw[self.rows[b + 1] - 1] if order == ASC else sw[self.rows[b]]) and len(docs) * W <= T and len(docs) <= B
            ids, mask, pos = np.full((len(docs), W), pad, np.int64), np.zeros((len(docs), W), np.int64), np.zeros((len(docs), W), np.int64)
            for i, d in enumerate(docs):
                c = content[d]
                s0 = W - len(c) if side == LEFT else 0
                ids[i, s0:s0 + len(c)] = c
                mask[i, s0:s0 + len(c)] = 1
                pos[i, s0:s0 + len(c)] = np.arange(len(c))
            self.widths.append(W)
            self.boffs.append(self.boffs[-1] + len(docs) * W)
            self.blocks.append((ids, mask, pos))
        self.P = self.boffs[-1]
        flat = lambda k: np.concatenate([blk[k].reshape(-1) for blk in self.blocks]).tolist() if self.blocks else []
        self.ids, self.mask, self.pos = flat(0), flat(1), flat(2)
        assert self.P <= n * L and len(self.ids) == self.P and self.nb <= n
        # the runs of equal width and, for every bucket, the run its first row and the run its last row lie in
        self.run_first = [r for r in range(n) if r == 0 or sw[r] != sw[r - 1]]
        run_of = np.searchsorted(self.run_first, np.arange(n), side="right") - 1 if n else []
        self.first_run = [int(run_of[self.rows[b]]) for b in range(self.nb)]
        self.last_run = [int(run_of[self.rows[b + 1] - 1]) for b in range(self.nb)]
        self.ends_at_run_end = [self.rows[b + 1] == n or self.rows[b + 1] in self.run_first for b in range(self.nb)]


class Ctx(BK.Ctx):
    """bucketed_cases.Ctx (the oracle's ids, the padded and the bucketed entries' transport) with the transport of the budgeted entry."""

    def budgeted_device(self, b, L, T, B=NONE, order=ASC, index=(), bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1, arrays=(True, True, True, True), cap=None, bcap=None):
        """the device entry with guard words behind every buffer; a dict of the results cut to the figures the call returned"""
        wm, wp, wo, wr = arrays
        n = b["n"]
        cap = N.Encoder.padded_bounds(n, L) if cap is None else cap
        bcap = n if bcap is None else bcap
        ids = self.upload(np.full(cap + GUARD, -7, np.int32))
        mask = self.upload(np.full(cap + GUARD, 0xA5, np.uint8)) if wm else (None, 0)
        pos = self.upload(np.full(cap + GUARD, -7, np.int32)) if wp else (None, 0)
        lens = self.upload(np.full(n + GUARD, -7, np.int32))
        out = self.upload(np.full(n + 1 + GUARD, -5, np.int64)) if wo else (None, 0)
        perm = self.upload(np.full(n + GUARD, -5, np.int64))
        rank = self.upload(np.full(n + GUARD, -5, np.int64)) if wr else (None, 0)
        boffs = self.upload(np.full(bcap + 1 + GUARD, -5, np.int64))
        brows = self.upload(np.full(bcap + 1 + GUARD, -5, np.int64))
        widths = self.upload(np.full(bcap + GUARD, -7, np.int32))
        P = nb = None
        try:
            total, P, n_cut, nb = self.enc.encode_batch_budgeted_device(b["d_bytes"][1], b["d_offs"][1], n, b["total"], list(index), bos, eos, L, cut, side, pad, M, T, B, order,
                                                                        ids[1], cap, mask[1], pos[1], lens[1], out[1], perm[1], rank[1], boffs[1], brows[1], widths[1], bcap)
        finally:                                              # (whatever the call returned: nothing behind the capacities it was told)
            assert (self.back(ids[0])[cap:] == -7).all() and (self.back(lens[0])[n:] == -7).all(), "guard words behind ids / lens"
            assert not wm or (self.back(mask[0])[cap:] == 0xA5).all(), "guard words behind the mask"
            assert not wp or (self.back(pos[0])[cap:] == -7).all(), "guard words behind pos"
            assert not wo or (self.back(out[0])[n + 1:] == -5).all(), "guard words behind the offsets"
            assert (self.back(perm[0])[n:] == -5).all() and (not wr or (self.back(rank[0])[n:] == -5).all()), "guard words behind order / rank"
            assert (self.back(boffs[0])[bcap + 1:] == -5).all() and (self.back(brows[0])[bcap + 1:] == -5).all() and (self.back(widths[0])[bcap:] == -7).all(), \
                "guard words behind the bucket arrays"
        assert (self.back(ids[0])[P:] == -7).all() and (not wm or (self.back(mask[0])[P:] == 0xA5).all()) and (not wp or (self.back(pos[0])[P:] == -7).all()), \
            "written at or behind P"
        assert (self.back(boffs[0])[nb + 1:] == -5).all() and (self.back(brows[0])[nb + 1:] == -5).all() and (self.back(widths[0])[nb:] == -7).all(), \
            "written at or behind n_buckets (+ 1)"
        return dict(total=total, P=P, n_cut=n_cut, nb=nb, ids=self.back(ids[0])[:P].astype(np.int64), lens=self.back(lens[0])[:n].tolist(),
                    mask=self.back(mask[0])[:P].astype(np.int64) if wm else None, pos=self.back(pos[0])[:P].astype(np.int64) if wp else None,
                    offs=self.back(out[0])[:n + 1].tolist() if wo else None, order=self.back(perm[0])[:n].tolist(), rank=self.back(rank[0])[:n].tolist() if wr else None,
                    boffs=self.back(boffs[0])[:nb + 1].tolist(), rows=self.back(brows[0])[:nb + 1].tolist(), widths=self.back(widths[0])[:nb].tolist())


def assert_budgeted(what, got, m):
    assert (got["total"], got["P"], got["n_cut"], got["nb"]) == (m.total, m.P, m.n_cut, m.nb), (what, (got["total"], got["P"], got["n_cut"], got["nb"]), (m.total, m.P, m.n_cut, m.nb))
    SP._same(what, "lens", [int(x) for x in got["lens"]], m.lens)
    SP._same(what, "order", [int(x) for x in got["order"]], m.order)
    SP._same(what, "bucket rows", [int(x) for x in got["rows"]], m.rows)
    SP._same(what, "widths", [int(x) for x in got["widths"]], m.widths)
    SP._same(what, "bucket offsets", [int(x) for x in got["boffs"]], m.boffs)
    SP._same(what, "ids", got["ids"].tolist(), m.ids)
    for name, want in (("mask", m.mask), ("pos", m.pos)):
        if got[name] is not None:
            SP._same(what, name, got[name].tolist(), want)
    for name, want in (("offs", m.offs), ("rank", m.rank)):
        if got[name] is not None:
            SP._same(what, name, [int(x) for x in got[name]], want)


def assert_property(ctx, what, docs, got, L, index=(), bos=-1, eos=-1, pad=0, cut=SUFFIX, side=RIGHT, M=1, buckets=None):
    """bucket b equals what the PADDED entry writes for the documents order[rows[b] : rows[b + 1]] with the same parameters"""
    for b in (range(got["nb"]) if buckets is None else buckets):
        picked = got["order"][got["rows"][b]:got["rows"][b + 1]]
        sub = [docs[d] for d in picked]
        p = ctx.padded_device(ctx.device_buffers(sub), L, index, bos, eos, pad, cut, side, M)
        assert p["W"] == got["widths"][b], (what, b, p["W"], got["widths"][b])
        lo, hi = got["boffs"][b], got["boffs"][b + 1]
        assert hi - lo == len(sub) * p["W"], (what, b)
        SP._same(what, "bucket %d against the padded entry: ids" % b, got["ids"][lo:hi].tolist(), p["ids"].tolist())
        SP._same(what, "bucket %d against the padded entry: mask" % b, got["mask"][lo:hi].tolist(), p["mask"].tolist())
        SP._same(what, "bucket %d against the padded entry: pos" % b, got["pos"][lo:hi].tolist(), p["pos"].tolist())
        assert p["lens"] == [got["lens"][d] for d in picked], (what, b)


def check_device(ctx, docs, L, T, B, what, order=ASC, bos=-1, eos=-1, pad=-3, cut=SUFFIX, side=RIGHT, M=1, allowed=(), arrays=((True, True, True, True),), ids_per_doc=None,
                 b=None, exact=False, prop=None):
    """the device entry against the model, with the capacities that always suffice (n_docs * L, n_docs) or -- exact -- with P and n_buckets, not an entry more; prop:
    the buckets held against the padded entry as well (an iterable, or True for all of them)"""
    ids_per_doc = ids_per_doc if ids_per_doc is not None else ctx.oracle_ids(docs, allowed)
    m = Model(ids_per_doc, L, T, B, order, bos, eos, pad, cut, side, M)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = b or ctx.device_buffers(docs)
    for a in arrays:
        label = "%s, L %d, M %d, T %d, B %d, order %d, bos %d, eos %d, cut %d, pad side %d (mask %d, pos %d, offsets %d, rank %d)" % ((what, L, M, T, B, order, bos, eos, cut, side) + tuple(a))
        got = ctx.budgeted_device(b, L, T, B, order, index, bos, eos, pad, cut, side, M, a, cap=m.P if exact else None, bcap=m.nb if exact else None)
        assert_budgeted(label, got, m)
        if prop and a[0] and a[1]:
            assert_property(ctx, label, docs, got, L, index, bos, eos, pad, cut, side, M, None if prop is True else prop)
    return m


class Lexicon:
    """documents of 0 .. top one-token words with the oracle's ids, encoded once: a batch is a list of sizes"""

    def __init__(self, ctx, top, seed):
        rng = random.Random(seed)
        self.docs = [words(rng, k) for k in range(top + 1)]
        self.ids = ctx.oracle_ids(self.docs)
        assert [len(x) for x in self.ids] == list(range(top + 1))

    def batch(self, sizes):
        return [self.docs[k] for k in sizes], [self.ids[k] for k in sizes]


# ---- 1. the worked examples of tkz.h ----

def check_worked_examples(ctx):
    rng = random.Random(2)
    docs = [words(rng, n) for n in (5, 0, 2, 3, 2)]
    (a, _, c, d, e) = ids = ctx.oracle_ids(docs)
    assert [len(x) for x in ids] == [5, 0, 2, 3, 2]
    X, P = 9, 77
    b = ctx.device_buffers(docs)
    got = ctx.budgeted_device(b, 4, 9, NONE, ASC, (), -1, X, P, SUFFIX, RIGHT, 1)
    assert (got["total"], got["P"], got["n_cut"], got["nb"], got["lens"]) == (12, 17, 1, 2, [4, 1, 3, 4, 3])
    assert (got["order"], got["rank"], got["rows"], got["widths"], got["boffs"]) == ([1, 2, 4, 0, 3], [3, 0, 1, 4, 2], [0, 3, 5], [3, 4], [0, 9, 17])
    assert got["ids"].tolist() == [X, P, P, c[0], c[1], X, e[0], e[1], X, a[0], a[1], a[2], X, d[0], d[1], d[2], X]
    assert got["mask"].tolist() == [1, 0, 0] + [1] * 14 and got["pos"].tolist() == [0, 0, 0, 0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3]
    assert got["offs"] == [0, 5, 5, 7, 10, 12]
    assert_budgeted("the worked example, ascending", got, Model(ids, 4, 9, NONE, ASC, -1, X, P))
    got = ctx.budgeted_device(b, 4, 9, NONE, DESC, (), -1, X, P, SUFFIX, RIGHT, 1)
    assert (got["total"], got["P"], got["n_cut"], got["nb"], got["lens"]) == (12, 17, 1, 2, [4, 1, 3, 4, 3])
    assert (got["order"], got["rank"], got["rows"], got["widths"], got["boffs"]) == ([0, 3, 2, 4, 1], [0, 4, 2, 1, 3], [0, 2, 5], [4, 3], [0, 8, 17])
    assert got["ids"].tolist() == [a[0], a[1], a[2], X, d[0], d[1], d[2], X, c[0], c[1], X, e[0], e[1], X, X, P, P]
    assert got["mask"].tolist() == [1] * 15 + [0, 0] and got["pos"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 0, 1, 2, 0, 0, 0]
    assert_budgeted("the worked example, descending", got, Model(ids, 4, 9, NONE, DESC, -1, X, P))
    got = ctx.budgeted_device(b, 4, 9, 2, ASC, (), -1, X, P, SUFFIX, RIGHT, 1)
    assert (got["P"], got["nb"], got["rows"], got["widths"], got["boffs"]) == (18, 3, [0, 2, 4, 5], [3, 4, 4], [0, 6, 14, 18])
    same = ctx.bucketed_device(b, 4, 2, ASC, (), -1, X, P, SUFFIX, RIGHT, 1)      # (these are the bucketed entry's buckets)
    assert same["ids"].tolist() == got["ids"].tolist() and same["boffs"] == got["boffs"] and same["widths"] == got["widths"]
    assert_budgeted("the worked example, B = 2", got, Model(ids, 4, 9, 2, ASC, -1, X, P))


# ---- 2. one run, many buckets ----

def check_one_run(ctx):
    rng = random.Random(3)
    n = 2 * T_SORT + 1
    doc = words(rng, 3)
    docs, ids = [doc] * n, [ctx.oracle_ids([doc])[0]] * n
    b = ctx.device_buffers(docs)
    for order in (ASC, DESC):
        m = check_device(ctx, docs, 4, 4, NONE, "one run, T = L", order, eos=9, ids_per_doc=ids, b=b, exact=True, arrays=((True, False, True, True),))
        assert m.nb == n and m.widths == [4] * n and m.rows == list(range(n + 1)) and len(m.run_first) == 1      # one row a bucket
        m = check_device(ctx, docs, 5, 15, NONE, "one run, M = 0", order, eos=9, ids_per_doc=ids, b=b, exact=True, M=0, arrays=((False, True, False, False),))
        assert m.nb == -(-n // 3) and m.widths == [5] * m.nb and len(m.blocks[-1][0]) == (n - 1) % 3 + 1 and len(m.run_first) == 1


# ---- 3. / 4. runs ----

RUN_SIZES = [1] * 2 + [2] * 2 + [3] * 2 + [4] * 6 + [5] * 9 + [6] * 3 + [7] * 2 + [8] * 10 + [9] * 4 + [10] * 5


def check_runs(ctx, order):
    """ascending: a bucket that swallows three whole runs and ends inside a fourth, one that ends exactly at a run's end, the T bound and the B bound binding in
    the same batch; descending: the same batch, with an entry that jumps over two whole runs"""
    lex = Lexicon(ctx, 10, 5)
    sizes = list(RUN_SIZES)
    random.Random(7).shuffle(sizes)
    docs, ids = lex.batch(sizes)
    b = ctx.device_buffers(docs)
    m = check_device(ctx, docs, 10, 40, 7, "runs", order, ids_per_doc=ids, b=b, exact=True, arrays=ARRAYS, prop=True)
    n, whole = len(sizes), [m.last_run[k] - m.first_run[k] - (0 if m.ends_at_run_end[k] else 1) + (1 if m.rows[k] in m.run_first else 0) for k in range(m.nb)]
    rows = [m.rows[k + 1] - m.rows[k] for k in range(m.nb)]
    assert len(m.run_first) == 10
    assert any(r == 7 for r in rows) and any(r < 7 and (r + 1) * w > 40 for r, w in zip(rows[:-1], m.widths[:-1])), "the B bound and the T bound both bind"
    if order == ASC:
        assert m.rows[:3] == [0, 7, 14] and whole[0] == 3 and not m.ends_at_run_end[0], "rows 0 .. 7: the runs of width 1, 2 and 3 and one row of the fourth"
        assert any(m.ends_at_run_end[k] and m.first_run[k] != m.last_run[k] for k in range(m.nb - 1)), "a crossing bucket that ends exactly at a run's end"
    m = check_device(ctx, docs, 10, 60, NONE, "runs, no row cap", order, 7, ids_per_doc=ids, b=b, exact=True, M=1, cut=PREFIX, side=LEFT)
    if order == DESC:                                         # short runs at a large R: the next entry lies three runs on
        short = [10] * 2 + [9] + [8] + [7] * 30 + [3] * 4 + [0] * 3
        docs2, ids2 = lex.batch(short)
        m = check_device(ctx, docs2, 10, 40, NONE, "runs, an entry that jumps", DESC, ids_per_doc=ids2, exact=True, arrays=ARRAYS[:2], prop=(0, 1))
        assert m.rows[:3] == [0, 4, 9] and m.first_run[0] == 0 and m.first_run[1] == 3, "bucket 0 starts in the run of width 10, bucket 1 in the run of width 7"
    else:                                                     # every bucket swallows runs: widths 1 .. 10, a row each
        docs2, ids2 = lex.batch(list(range(1, 11)) * 1)
        m = check_device(ctx, docs2, 10, 12, NONE, "a row a run", ASC, ids_per_doc=ids2, exact=True)
        assert m.rows == [0, 3, 5, 6, 7, 8, 9, 10]


# ---- 5. width 0 ----

def check_width_zero(ctx):
    lex = Lexicon(ctx, 4, 11)
    sizes = [2, 0, 0, 1, 0, 0, 0, 4, 0]
    docs, ids = lex.batch(sizes)
    b = ctx.device_buffers(docs)
    # rows of width 0 cost nothing against T: only B stops them -- and a bucket that starts with them goes on into the rows that cost
    m = check_device(ctx, docs, 8, 8, 4, "width 0 leading", ASC, ids_per_doc=ids, b=b, arrays=ARRAYS, exact=True, prop=True)
    assert (m.rows, m.widths, m.boffs) == ([0, 4, 8, 9], [0, 2, 4], [0, 0, 8, 12])
    m = check_device(ctx, docs, 8, 8, NONE, "width 0 leading, no cap", ASC, ids_per_doc=ids, b=b, arrays=ARRAYS, exact=True)
    assert (m.rows, m.widths) == ([0, 7, 9], [1, 4])
    m = check_device(ctx, docs, 8, 8, 4, "width 0 trailing", DESC, ids_per_doc=ids, b=b, arrays=ARRAYS, exact=True, prop=True)
    assert (m.rows, m.widths, m.boffs) == ([0, 2, 6, 9], [4, 1, 0], [0, 8, 12, 12])
    m = check_device(ctx, docs, 8, 8, NONE, "width 0 trailing, no cap", DESC, ids_per_doc=ids, b=b, arrays=ARRAYS, exact=True)
    assert (m.rows, m.widths) == ([0, 2, 9], [4, 1])
    for order in (ASC, DESC):
        m = check_device(ctx, [b""] * 5, 8, 8, 2, "nothing but width 0", order, arrays=ARRAYS, exact=True)
        assert (m.P, m.rows, m.widths, m.boffs) == (0, [0, 2, 4, 5], [0, 0, 0], [0, 0, 0, 0])
        m = check_device(ctx, [b""] * 5, 8, 8, NONE, "nothing but width 0, no cap", order, exact=True, M=0)
        assert (m.P, m.rows, m.widths) == (0, [0, 5], [0])


# ---- 6. run counts at the chain's geometry ----

def check_run_counts(ctx):
    top = 2 * LOOK + 1
    lex = Lexicon(ctx, top, 13)
    for nruns in (1, LOOK - 1, LOOK, LOOK + 1, 2 * LOOK + 1):
        sizes = list(range(1, nruns + 1)) + [nruns, 1]           # every length 1 .. nruns, M = 1: nruns runs
        random.Random(nruns).shuffle(sizes)
        docs, ids = lex.batch(sizes)
        b = ctx.device_buffers(docs)
        L = top + 1
        for order in (ASC, DESC):
            for T, B in ((L, NONE), (3 * L, 5), (len(sizes) * L, NONE)):      # a row or two a bucket; a few; ONE bucket over all the runs
                m = check_device(ctx, docs, L, T, B, "%d runs" % nruns, order, eos=9, ids_per_doc=ids, b=b, exact=True, arrays=((True, True, False, True),))
                assert len(m.run_first) == nruns
            assert m.nb == 1


# ---- 7. n_docs at the tiles ----

def check_tiles(ctx):
    """n_docs one below, at and one above the sort's tile and the run-marking tile"""
    lex = Lexicon(ctx, 5, 17)
    for n in sorted({T_MARK - 1, T_MARK, T_MARK + 1, T_SORT - 1, T_SORT, T_SORT + 1, 63, 64, 65}):
        docs, ids = lex.batch([(7 * d + d // 5) % 6 for d in range(n)])
        for order in (ASC, DESC):
            m = check_device(ctx, docs, 6, 50, 11, "n_docs = %d" % n, order, eos=9, ids_per_doc=ids, exact=True, arrays=((True, False, True, True),))
            assert len(m.run_first) == len(set(m.lens)) >= 5 and m.nb >= n // 11


# ---- 8. more than the grids hold ----

def check_grid_stride(ctx, lib):
    """more documents than k_pad_lens has lanes -- empty ones, a row of one framing id each; two that are not"""
    rng = random.Random(9)
    n = GRID * 256 + 300
    docs = [b""] * n
    docs[7], docs[n - 2] = words(rng, 3), words(rng, 2)
    ids = [[]] * n
    ids[7], ids[n - 2] = ctx.oracle_ids([docs[7]])[0], ctx.oracle_ids([docs[n - 2]])[0]
    b = ctx.device_buffers(docs)
    m = check_device(ctx, docs, 2, 150000, 100000, "grid stride: documents", ASC, 7, -1, arrays=((True, False, True, True),), ids_per_doc=ids, b=b, exact=True)
    assert (m.n_cut, m.total) == (2, 5) and m.lens.count(1) == n - 2 and m.widths[-1] == 2 and m.widths[0] == 1 and m.rows[1] == 100000


# ---- 9. only B binds: the bucketed entry's buckets ----

def check_row_cap_only(ctx):
    lex = Lexicon(ctx, 40, 19)
    n = 150
    sizes = [(11 * d + d // 7) % 40 for d in range(n)]
    docs, ids = lex.batch(sizes)
    b = ctx.device_buffers(docs)
    L = 30
    for B in (1, 64, n - 1, n, n + 1):
        for order in (ASC, DESC):
            args = (order, (), 7, 9, -3, SUFFIX, RIGHT, 8)
            got = ctx.budgeted_device(b, L, n * L, B, *args)
            want = ctx.bucketed_device(b, L, B, *args)
            assert got["nb"] == len(want["widths"]) == -(-n // B) and got["rows"] == [min(k * B, n) for k in range(got["nb"] + 1)]
            for name in ("total", "P", "n_cut", "lens", "offs", "order", "rank", "boffs", "widths"):
                assert got[name] == want[name], (name, B, order)
            for name in ("ids", "mask", "pos"):
                assert got[name].tobytes() == want[name].tobytes(), (name, B, order)
            assert_budgeted("only B binds, B = %d" % B, got, Model(ids, L, n * L, B, order, 7, 9, -3, M=8))
            assert_property(ctx, "only B binds, B = %d" % B, docs, got, L, (), 7, 9, -3, SUFFIX, RIGHT, 8, (0, got["nb"] - 1))


# ---- 10. random small batches ----

def check_random(ctx, rounds=60):
    rng = random.Random(20261021)
    lex = Lexicon(ctx, 24, 23)
    for i in range(rounds):
        L = rng.choice((1, 2, 5, 8, 16, 21))
        n = rng.randint(1, 60)
        top = rng.choice((2, L, L + 3, 24))
        sizes = [rng.choice((0, rng.randint(0, min(top, 24)))) if rng.random() < 0.2 else rng.randint(0, min(top, 24)) for _ in range(n)]
        docs, ids = lex.batch(sizes)
        bos, eos = rng.choice(FORMS) if L >= 2 else rng.choice(FORMS[:3])
        M = (0, 1, 8)[i % 3]
        T = rng.randint(L, 10 * L)
        B = rng.choice((NONE, NONE, 1, 2, 3, 7, n))
        cut, side = rng.choice(SIDES)
        b = ctx.device_buffers(docs)
        for order in (ASC, DESC):
            check_device(ctx, docs, L, T, B, "random %d" % i, order, bos, eos, cut=cut, side=side, M=M, ids_per_doc=ids, b=b, exact=bool(i & 1))


# ---- special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    docs = [(" the of" + EOT + " and to in").encode(), (" is that for" + EOT).encode(), b"", EOT.encode()]
    ids = ctx.oracle_ids(docs, [EOT])
    assert [len(x) for x in ids] == [6, 4, 0, 1] and ids[0][2] == ids[1][3] == ids[3][0] == eot
    b = ctx.device_buffers(docs)
    for L in (3, 4, 5, 8):
        for order, (cut, side) in zip((ASC, DESC, DESC, ASC), SIDES):
            m = check_device(ctx, docs, L, 2 * L, NONE, "special: allowed", order, eos=eot, cut=cut, side=side, allowed=[EOT], ids_per_doc=ids, b=b, prop=True)
            assert m.lens == [min(6, L - 1) + 1, min(4, L - 1) + 1, 1, 2]
    s0 = ctx.enc.special_stats()
    off = check_device(ctx, docs, 6, 12, 3, "special: registered, not allowed", eos=eot, allowed=[])
    assert off.total > sum(map(len, ids)) and ctx.enc.special_stats() == s0              # (split as plain text)


# ---- 11. / 12. capacity and arguments ----

def check_capacity(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, lib = ctx.enc, ctx.enc.lib.L
    rng = random.Random(17)
    docs = [words(rng, 9), b"", words(rng, 30), (" the" + EOT + " of").encode(), words(rng, 2)]
    n, ML, T, B = len(docs), 16, 24, NONE
    m = Model(ctx.oracle_ids(docs, [EOT]), ML, T, B, DESC, 7, eot, 0, M=8)
    assert (m.rows, m.widths, m.P, m.nb, m.n_cut) == ([0, 1, 2, 5], [16, 16, 8], 56, 3, 1)
    b = ctx.device_buffers(docs)
    c0 = enc.budgeted_calls()
    need = (m.total, m.P, m.n_cut, m.nb)
    for cap, bcap in ((m.P - 1, n), (n * ML, m.nb - 1), (m.P - 1, m.nb - 1), (0, n), (n * ML, 0), (0, 0)):
        with pytest.raises(N.TkzError) as ei:
            ctx.budgeted_device(b, ML, T, B, DESC, [0], 7, eot, 0, M=8, cap=cap, bcap=bcap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_positions, ei.value.n_cut, ei.value.needed_buckets) == need, (cap, bcap)
    assert enc.budgeted_calls() == c0                            # failed calls are not counted
    for a in ARRAYS:                                             # the exact capacities, sized from the figures above
        assert_budgeted("exact capacity", ctx.budgeted_device(b, ML, T, B, DESC, [0], 7, eot, 0, M=8, arrays=a, cap=m.P, bcap=m.nb), m)
    assert enc.budgeted_calls() == c0 + 4
    data, offs = parity.pack(docs)
    for cap, bcap in ((m.P - 1, None), (None, m.nb - 1), (0, 0)):
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_budgeted(data, offs, ML, T, None, DESC, [0], 7, eot, pad_multiple=8, out_cap=cap, bucket_cap=bcap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_positions, ei.value.n_cut, ei.value.needed_buckets) == need
    r = enc.encode_batch_budgeted(data, offs, ML, T, None, DESC, [0], 7, eot, pad_multiple=8, out_cap=m.P, bucket_cap=m.nb)
    assert (r[0].tolist(), r[1].tolist(), r[2].tolist(), r[3].tolist(), r[4].tolist()) == (m.ids, m.mask, m.pos, m.lens, m.offs)
    assert (r[5].tolist(), r[6].tolist(), r[7].tolist(), r[8].tolist(), r[9].tolist(), r[10], r[11]) == (m.order, m.rank, m.boffs, m.rows, m.widths, m.total, m.n_cut)
    # every TKZ_E_ARG of the rule: T < L, T > 2^62, the B range, bucket_cap < 0, and the bucketed entry's own
    bad = (dict(T=ML - 1), dict(T=0), dict(T=-1), dict(T=TMAX + 1), dict(B=0), dict(B=-1), dict(B=1 << 31), dict(bcap=-1), dict(order=2), dict(order=-1),
           dict(bos=-2), dict(eos=-2), dict(eos=-(1 << 31)), dict(L=0), dict(L=-4), dict(L=1 << 31), dict(L=1), dict(cut=2), dict(cut=-1), dict(side=2), dict(side=-1),
           dict(M=-1), dict(M=1 << 31), dict(index=[1]), dict(index=[0, 0]), dict(index=[-1]))
    for kw in bad:
        a = dict(L=ML, index=[0], bos=7, eos=eot, cut=SUFFIX, side=RIGHT, M=8, T=T, B=B, order=ASC, bcap=n)
        a.update(kw)
        if "L" in kw:
            a["T"] = max(T, a["L"])                              # (the length alone is what is wrong)
        cap = n * ML
        with pytest.raises(N.TkzError) as ei:
            pd = ctx.upload(np.zeros(cap, np.int32)), ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n, np.int64)), ctx.upload(np.zeros(n + 1, np.int64)), \
                ctx.upload(np.zeros(n + 1, np.int64)), ctx.upload(np.zeros(n, np.int32))
            enc.encode_batch_budgeted_device(b["d_bytes"][1], b["d_offs"][1], n, b["total"], a["index"], a["bos"], a["eos"], a["L"], a["cut"], a["side"], 0, a["M"], a["T"],
                                             a["B"], a["order"], pd[0][1], cap, 0, 0, pd[1][1], 0, pd[2][1], 0, pd[3][1], pd[4][1], pd[5][1], a["bcap"])
        assert ei.value.code == N.E_ARG, kw
        if "index" not in kw:
            for call in (lambda: enc.encode_batch_budgeted(data, offs, a["L"], a["T"], a["B"], a["order"], [0], a["bos"], a["eos"], 0, a["cut"], a["side"], a["M"], out_cap=cap,
                                                           bucket_cap=a["bcap"]),
                         lambda: enc.encode_batch_budgeted_utf16(np.asarray([65, 66], np.uint16), np.asarray([0, 2], np.int64), a["L"], a["T"], a["B"], a["order"], [0],
                                                                 a["bos"], a["eos"], 0, a["cut"], a["side"], a["M"], out_cap=64, bucket_cap=a["bcap"])):
                with pytest.raises(N.TkzError) as ei:
                    call()
                assert ei.value.code == N.E_ARG, kw
    # the ends of the ranges are arguments like any other
    for T2, B2 in ((TMAX, NONE), (ML, 1)):
        assert_budgeted("the ends of the ranges", ctx.budgeted_device(b, ML, T2, B2, DESC, [0], 7, eot, 0, M=8), Model(ctx.oracle_ids(docs, [EOT]), ML, T2, B2, DESC, 7, eot, 0, M=8))
    # NULL for a required pointer; for one that may be NULL
    plain = Model(ctx.oracle_ids(docs), ML, T, B, DESC, 7, eot, 0, M=8)          # (nothing allowed below: the literal is plain text)
    nb = plain.nb
    ids, msk, pos = ctx.upload(np.zeros(plain.P, np.int32)), ctx.upload(np.zeros(plain.P, np.uint8)), ctx.upload(np.zeros(plain.P, np.int32))
    lens, ooff, perm, rank = ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n + 1, np.int64)), ctx.upload(np.zeros(n, np.int64)), ctx.upload(np.zeros(n, np.int64))
    boffs, brows, wid = ctx.upload(np.zeros(nb + 1, np.int64)), ctx.upload(np.zeros(nb + 1, np.int64)), ctx.upload(np.zeros(nb, np.int32))
    t, p, c, k = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ok = (enc._h, b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], None, 0, 7, eot, ML, SUFFIX, RIGHT, 0, 8, T, B, DESC, ids[1], plain.P, msk[1], pos[1], lens[1], ooff[1],
          perm[1], rank[1], boffs[1], brows[1], wid[1], nb, None, C.byref(t), C.byref(p), C.byref(c), C.byref(k))
    assert lib.tkz_encode_batch_budgeted_device(*ok) == N.OK and (t.value, p.value, c.value, k.value) == (plain.total, plain.P, plain.n_cut, plain.nb)
    assert ctx.back(perm[0]).tolist() == plain.order and ctx.back(boffs[0]).tolist() == plain.boffs and ctx.back(wid[0]).tolist() == plain.widths
    assert ctx.back(brows[0]).tolist() == plain.rows
    for j in (0, 1, 2, 17, 21, 23, 25, 26, 27, 30, 31, 32, 33):   # the encoder, the bytes, the offsets, d_out_ids, d_lens, d_order, the bucket arrays, the four scalars
        assert lib.tkz_encode_batch_budgeted_device(*(ok[:j] + (None,) + ok[j + 1:])) == N.E_ARG, j
    for j in (19, 20, 22, 24):                                   # d_mask, d_pos, d_out_offsets, d_rank
        assert lib.tkz_encode_batch_budgeted_device(*(ok[:j] + (None,) + ok[j + 1:])) == N.OK, j
    assert lib.tkz_encode_batch_budgeted_device(*(ok[:18] + (-1,) + ok[19:])) == N.E_ARG
    hid, hl, hp, hb, hr, hw = np.zeros(plain.P, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(nb + 1, np.int64), np.zeros(nb + 1, np.int64), np.zeros(nb, np.int32)
    hok = (enc._h, data.ctypes.data, offs.ctypes.data, n, None, 0, 7, eot, ML, SUFFIX, RIGHT, 0, 8, T, B, DESC, hid.ctypes.data, plain.P, None, None, hl.ctypes.data, None,
           hp.ctypes.data, None, hb.ctypes.data, hr.ctypes.data, hw.ctypes.data, nb, C.byref(t), C.byref(p), C.byref(c), C.byref(k))
    assert lib.tkz_encode_batch_budgeted_utf8(*hok) == N.OK and (p.value, k.value) == (plain.P, plain.nb)
    assert (hl.tolist(), hid.tolist(), hp.tolist(), hb.tolist(), hr.tolist(), hw.tolist()) == (plain.lens, plain.ids, plain.order, plain.boffs, plain.rows, plain.widths)
    for j in (0, 2, 16, 20, 22, 24, 25, 26, 28, 29, 30, 31):     # the encoder, the offsets, out_ids, lens, order, the bucket arrays, the four scalars
        assert lib.tkz_encode_batch_budgeted_utf8(*(hok[:j] + (None,) + hok[j + 1:])) == N.E_ARG, j
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        ctx.budgeted_device(ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]), ML, T, B, eos=9)
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_budgeted(data, np.asarray([0, 12, 11, 40, 50, len(data)], np.int64), ML, T)
    assert ei.value.code == N.E_ARG
    # no documents: TKZ_OK, bucket_offsets[0], bucket_rows_out[0] and out_offsets[0] cleared, all scalars 0; documents without bytes through the host entries
    none = ctx.device_buffers([])
    for bos, eos in FORMS:
        got = ctx.budgeted_device(none, ML, T, B, ASC, (), bos, eos, cap=0, bcap=0)
        assert (got["total"], got["P"], got["n_cut"], got["nb"], got["offs"], got["lens"], got["order"], got["boffs"], got["rows"], got["widths"]) == (0, 0, 0, 0, [0], [], [], [0], [0], [])
        m3 = Model([[], [], []], 4, 4, 2, DESC, bos, eos, 5, side=LEFT, M=2)
        for r in (enc.encode_batch_budgeted(np.zeros(0, np.uint8), np.zeros(4, np.int64), 4, 4, 2, DESC, (), bos, eos, 5, pad_side=LEFT, pad_multiple=2),
                  enc.encode_batch_budgeted_utf16(np.zeros(0, np.uint16), np.zeros(4, np.int64), 4, 4, 2, DESC, (), bos, eos, 5, pad_side=LEFT, pad_multiple=2)):
            assert (r[0].tolist(), r[1].tolist(), r[2].tolist(), r[3].tolist(), r[4].tolist(), r[5].tolist(), r[6].tolist(), r[7].tolist(), r[8].tolist(), r[9].tolist(), r[10], r[11]) == \
                (m3.ids, m3.mask, m3.pos, m3.lens, [0, 0, 0, 0], [0, 1, 2], [0, 1, 2], m3.boffs, m3.rows, m3.widths, 0, 0)
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    d1, o1 = parity.pack([b"a<|s7|>b"])
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_batch_budgeted(d1, o1, 4, 4, None, ASC, [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_batch_budgeted(d1, o1, 64, 64)[10] == len(many.oenc.encode_bytes(b"a<|s7|>b"))          # (nothing allowed: the plain call)


# ---- 13. agreement of the entries ----

def check_agreement(make_ctx, lib, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc = ctx.enc
    rng, gib, mixed, crowded = CC.generators(7)
    w = lambda n: CC.fill(rng, n).decode()
    lone = "lone \ud800 high"
    texts = [w(300) + EOT + w(40), gib(600, 2, 9), "", w(2 * BK.K + 9), "café " + EMOJI + " 漢字 " + w(20), lone, mixed(1500, 3, 3, 30), EOT, w(5)]
    unit_docs = [U16S.units(t) for t in texts]
    docs = [U16.get_bytes(u) for u in unit_docs]                 # (Encoding.UTF8.GetBytes: the lone surrogate becomes EF BF BD)
    data, offs = parity.pack(docs)
    flat, uoffs = U16S.pack(unit_docs)
    b = ctx.device_buffers(docs)
    for index, allowed in (([0], [EOT]), ([], [])):
        want = ctx.oracle_ids(docs, allowed)
        for bos, eos, ML, T, B, order, cut, side, M in ((-1, -1, 64, 200, NONE, ASC, SUFFIX, RIGHT, 1), (7, eot, 64, 128, 3, DESC, PREFIX, LEFT, 8),
                                                       (-1, eot, 1000, 2500, NONE, ASC, SUFFIX, LEFT, 0), (-1, eot, 5000, 6000, 4, DESC, PREFIX, RIGHT, 64)):
            m = Model(want, ML, T, B, order, bos, eos, 0, cut, side, M)
            c0 = enc.budgeted_calls()
            assert_budgeted("agreement: device", ctx.budgeted_device(b, ML, T, B, order, index, bos, eos, 0, cut, side, M), m)
            assert parity.read_device_i64(lib, enc.counts_device, 3).tolist() == [len(docs), len(data), m.total]      # the counts block receives the uncut total
            for name, r in (("utf8", enc.encode_batch_budgeted(data, offs, ML, T, B, order, index, bos, eos, 0, cut, side, M)),
                            ("utf16", enc.encode_batch_budgeted_utf16(flat, uoffs, ML, T, B, order, index, bos, eos, 0, cut, side, M))):
                host = dict(total=r[10], P=len(r[0]), n_cut=r[11], nb=len(r[9]), ids=r[0].astype(np.int64), mask=r[1].astype(np.int64), pos=r[2].astype(np.int64), lens=r[3].tolist(),
                            offs=r[4].tolist(), order=r[5].tolist(), rank=r[6].tolist(), boffs=r[7].tolist(), rows=r[8].tolist(), widths=r[9].tolist())
                assert_budgeted("agreement: " + name, host, m)
                assert r[1].dtype == np.uint8 and r[5].dtype == np.int64 and r[8].dtype == np.int64 and r[9].dtype == np.int32
            assert enc.budgeted_calls() == c0 + 3


def check_retry(make_ctx):
    """the first call of a fresh encoder is a budgeted call whose miss lists overflow (CJK text under gpt2, consonant strings): the attempt is run again inside
    the call, and the caller's buffers hold the final attempt's results only"""
    ctx = make_ctx()
    rng, gib, mixed, crowded = CC.generators(47)
    cjk = "漢字かな交じり文、한국어 " + EMOJI + " naïve café "
    docs = [(cjk * 80).encode("utf-8")] + CC.cut(gib(30000, 2, 2).encode(), [700, 9000]) + [b"", CC.fill(rng, 300)]
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    w0 = ctx.enc.workspace_bytes
    first = check_device(ctx, docs, 512, 1024, NONE, "retry: first call", DESC, 7, 9, M=64, ids_per_doc=ids, b=b, exact=True, arrays=ARRAYS[:1])
    assert ctx.enc.workspace_bytes > w0
    again = check_device(ctx, docs, 512, 1024, NONE, "retry: again", DESC, 7, 9, M=64, ids_per_doc=ids, b=b, exact=True)
    assert (first.total, first.P, first.nb) == (again.total, again.P, again.nb) and first.n_cut >= 2
    check_device(ctx, docs, 512, 900, 3, "retry: the tails", ASC, cut=PREFIX, side=LEFT, ids_per_doc=ids, b=b)


def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    oenc = O.Encoder(O.Vocab(raw_gpt2), N.P1, specials=specials)
    lines = lib_rs_text.split("\n")
    want = [oenc.encode(t, [EOT]) for t in lines]
    L, T = 24, 200
    for desc, rows in ((False, None), (True, None), (False, 10)):
        buckets, order, rank, lens = tok.EncodeBatchBudgeted(lines, L, T, rows, eos=EOT, pad_to_multiple_of=8, descending=desc, return_pos=True)
        m = Model(want, L, T, NONE if rows is None else rows, DESC if desc else ASC, -1, 50256, 0, M=8)
        assert len(buckets) == m.nb and (order.tolist(), rank.tolist(), lens.tolist()) == (m.order, m.rank, m.lens) and m.n_cut >= 3 and len(set(m.widths)) >= 2
        for (ids, mask, pos), (wi, wm, wp) in zip(buckets, m.blocks):
            assert ids.shape == mask.shape == pos.shape == wi.shape and ids.dtype == np.int32 and mask.dtype == np.uint8 and ids.size <= T
            assert (ids.tolist(), mask.tolist(), pos.tolist()) == (wi.tolist(), wm.tolist(), wp.tolist())
        assert buckets[0][0].base is not None and all(x[0].base is buckets[0][0].base for x in buckets if x[0].size)      # (views of the one buffer)
    # the tails, padded on the left to the fixed width; bos as an int, eos as a literal, another pad; the literal in the text allowed and not
    text = ["a" + EOT + "b", "", "Hi " + EMOJI + " café", " the of and to in is that for it with"]
    for apply in (True, False):
        buckets, order, rank, lens = tok.EncodeBatchBudgeted(text, 6, 12, None, apply, bos=11, eos=EOT, pad=-1, truncation_side="left", padding_side="left", fixed_width=True)
        m = Model([oenc.encode(t, [EOT] if apply else []) for t in text], 6, 12, NONE, ASC, 11, 50256, -1, PREFIX, LEFT, 0)
        assert [(i.tolist(), k.tolist()) for i, k in buckets] == [(x[0].tolist(), x[1].tolist()) for x in m.blocks] and (order.tolist(), lens.tolist()) == (m.order, m.lens)
    buckets, order, rank, lens = tok.EncodeBatchBudgeted([], 4, 8, eos=EOT)
    assert buckets == [] and order.tolist() == rank.tolist() == lens.tolist() == []
    for bad in (dict(max_length=0, max_tokens=2), dict(max_length=1, max_tokens=2, bos=11, eos=EOT), dict(max_length=4, max_tokens=3), dict(max_length=4, max_tokens=(1 << 62) + 1),
                dict(max_length=4, max_tokens=8, max_rows=0), dict(max_length=4, max_tokens=8, max_rows=1 << 31), dict(max_length=4, max_tokens=8, pad_to_multiple_of=0),
                dict(max_length=4, max_tokens=8, truncation_side="up"), dict(max_length=4, max_tokens=8, padding_side="down")):
        with pytest.raises(ValueError):
            tok.EncodeBatchBudgeted(text, **bad)
    # a literal that holds U+FFFD beside a lone surrogate: through the UTF-16 entry
    fffd = {k: v + 200000 for k, v in U16S.FFFD_SPECIALS.items()}
    tok3 = TokenizerBuilder.CreateTokenizer(raw_gpt2, fffd, REGEX_PATTERN_1, lib=lib)
    lone = ["ab x\ud83d b x� c it's", "plain"]
    buckets, order, rank, lens = tok3.EncodeBatchBudgeted(lone, 8, 8, None, list(fffd), eos=3, descending=True)
    exp = U16S.Expect(O, O.Vocab(raw_gpt2), N.P1, fffd)
    m = Model([exp.encode(U16S.units(t), list(fffd)) for t in lone], 8, 8, NONE, DESC, -1, 3, 0)
    assert [(i.tolist(), k.tolist()) for i, k in buckets] == [(x[0].tolist(), x[1].tolist()) for x in m.blocks] and (order.tolist(), lens.tolist()) == (m.order, m.lens)
