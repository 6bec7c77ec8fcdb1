"""Pair rows (tkz_encode_batch_pairs_device / _utf8 / _utf16; k_pair_lens, k_pair_write): the cases and comparisons the emulated (CPU) and the GPU test modules
share.  Every comparison is exact.

No expected value comes from the code under test.  The model (`Model`) is numpy over the ORACLE's ids -- packed_cases.Ctx.oracle_ids; TrimOracle's literal search
for UTF-16 text with lone surrogates (u16_special_cases.Expect) -- and applies the rule of tkz.h: the cut of the two texts by the strategy, the framing and the
separators, the width, the rows, the mask, the types, pos, lens and kept.  LONGEST_FIRST is computed by the LOOP of the rule (an id at a time from the longer
text, from the second on a tie), not by the closed form the kernel uses.  It never reads the library's own encode output.

The kernel cases go through tkz_encode_batch_pairs_device.  `upload(np_array) -> (owner, pointer)` as in count_cases.  Every output buffer carries GUARD words
behind the capacity the call is told, and they must be intact afterwards -- and so must everything at or behind n_pairs * W.

Geometry (tkz_kernels.h): k_pair_lens a lane a pair, k_pair_write a wavefront per tile of K = kPairTile output positions, four wavefronts a workgroup, at most
GRID workgroups each.  Documents are runs of one-token words (packed_cases.words), so a case is a few tens of KB.
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
K = int(re.search(r"\bkPairTile = (\d+)\b", _HEAD).group(1))
GRID = int(re.search(r"\bkPairGridMax = (\d+)\b", _HEAD).group(1))
EOT = SC.EOT
EOT_ID = SP.EOT_ID
EMOJI = PK.EMOJI
GUARD = 8
FORMS = PK.FORMS                                       # none, bos only, eos only, both
SEP = 5
SUFFIX, PREFIX, RIGHT, LEFT = N.TRIM_SUFFIX, N.TRIM_PREFIX, N.PAD_RIGHT, N.PAD_LEFT
LONGEST, ONLY_FIRST, ONLY_SECOND = N.TRUNC_LONGEST_FIRST, N.TRUNC_ONLY_FIRST, N.TRUNC_ONLY_SECOND
STRATEGIES = (LONGEST, ONLY_FIRST, ONLY_SECOND)
SIDES = ((SUFFIX, RIGHT), (SUFFIX, LEFT), (PREFIX, RIGHT), (PREFIX, LEFT))
# mask, types, pos, kept and offsets present and NULL: all, none, and four that tell every two of the five apart
ALL = (True, True, True, True, True)
ARRAYS = (ALL, (False,) * 5, (True, False, True, False, True), (False, True, False, True, False), (True, True, False, False, False), (False, False, True, True, False))
words = PK.words


def kept_counts(a, b, R, strategy):
    """the rule's cut, an id at a time"""
    ka, kb = a, b
    while ka + kb > R:
        if strategy == LONGEST:
            if ka > kb:
                ka -= 1
            else:
                kb -= 1                                # the second text on a tie
        elif strategy == ONLY_FIRST:
            if ka > 0:
                ka -= 1
            else:
                kb -= 1
        else:
            if kb > 0:
                kb -= 1
            else:
                ka -= 1
    return ka, kb


class Model:
    """the rule of tkz.h over the oracle's ids of every document: documents 2p and 2p + 1 are the two texts of pair p"""

    def __init__(self, ids_per_doc, L, bos=-1, sep=-1, s=0, eos=-1, pad=0, strategy=LONGEST, cut=SUFFIX, side=RIGHT, M=1):
        fb, fe = int(bos >= 0), int(eos >= 0)
        f, nd = fb + s + fe, len(ids_per_doc)
        assert max(1, f) <= L and nd % 2 == 0 and (s == 0 or sep >= 0)
        n, R = nd // 2, L - f
        content, types, self.kept, self.n_cut = [], [], [], 0
        for p in range(n):
            A, B = list(ids_per_doc[2 * p]), list(ids_per_doc[2 * p + 1])
            ka, kb = kept_counts(len(A), len(B), R, strategy)
            keepA = A[:ka] if cut == SUFFIX else A[len(A) - ka:]
            keepB = B[:kb] if cut == SUFFIX else B[len(B) - kb:]
            content.append([bos] * fb + keepA + [sep] * s + keepB + [eos] * fe)
            types.append([0] * (fb + ka + s) + [1] * (kb + fe))
            self.kept += [ka, kb]
            self.n_cut += len(A) + len(B) > R
        self.offs = np.concatenate([[0], np.cumsum([len(di) for di in ids_per_doc], dtype=np.int64)]).astype(np.int64).tolist()
        self.total = self.offs[-1]
        self.lens = [len(c) for c in content]
        longest = max(self.lens, default=0)
        self.W = W = 0 if longest == 0 else (L if M == 0 else min(L, -(-longest // M) * M))
        self.ids = np.full((n, W), pad, np.int64)
        self.mask = np.zeros((n, W), np.int64)
        self.types = np.zeros((n, W), np.int64)
        self.pos = np.zeros((n, W), np.int64)
        for p, c in enumerate(content):
            at = W - len(c) if side == LEFT else 0
            self.ids[p, at:at + len(c)] = c
            self.mask[p, at:at + len(c)] = 1
            self.types[p, at:at + len(c)] = types[p]
            self.pos[p, at:at + len(c)] = np.arange(len(c))
        assert W <= L and (M == 0 or W % M == 0 or W == L)


class Ctx(PK.Ctx):
    """packed_cases.Ctx (the oracle's ids of every document) with the transport of the pair entry."""

    def pairs_device(self, b, L, index=(), bos=-1, sep=-1, s=0, eos=-1, pad=0, strategy=LONGEST, cut=SUFFIX, side=RIGHT, M=1, arrays=ALL, cap=None):
        """the device entry with guard words behind every buffer; a dict of the results cut to the figures the call returned"""
        wm, wt, wp, wk, wo = arrays
        nd = b["n"]
        n = nd // 2
        cap = N.Encoder.pairs_bounds(n, L) if cap is None else cap
        ids = self.upload(np.full(cap + GUARD, -7, np.int32))
        mask = self.upload(np.full(cap + GUARD, 0xA5, np.uint8)) if wm else (None, 0)
        types = self.upload(np.full(cap + GUARD, 0xA5, np.uint8)) if wt else (None, 0)
        pos = self.upload(np.full(cap + GUARD, -7, np.int32)) if wp else (None, 0)
        lens = self.upload(np.full(n + GUARD, -7, np.int32))
        kept = self.upload(np.full(nd + GUARD, -7, np.int32)) if wk else (None, 0)
        out = self.upload(np.full(nd + 1 + GUARD, -5, np.int64)) if wo else (None, 0)
        W = None
        try:
            total, W, n_cut = self.enc.encode_batch_pairs_device(b["d_bytes"][1], b["d_offs"][1], nd, b["total"], list(index), bos, sep, s, eos, L, strategy, cut, side, pad, M,
                                                                 ids[1], cap, mask[1], types[1], pos[1], lens[1], kept[1], out[1])
        finally:                                              # (whatever the call returned: nothing behind the capacities it was told)
            assert (self.back(ids[0])[cap:] == -7).all() and (self.back(lens[0])[n:] == -7).all(), "guard words behind ids / lens"
            assert not wm or (self.back(mask[0])[cap:] == 0xA5).all(), "guard words behind the mask"
            assert not wt or (self.back(types[0])[cap:] == 0xA5).all(), "guard words behind the types"
            assert not wp or (self.back(pos[0])[cap:] == -7).all(), "guard words behind pos"
            assert not wk or (self.back(kept[0])[nd:] == -7).all(), "guard words behind kept"
            assert not wo or (self.back(out[0])[nd + 1:] == -5).all(), "guard words behind the offsets"
        k = n * W
        assert (self.back(ids[0])[k:] == -7).all() and (not wm or (self.back(mask[0])[k:] == 0xA5).all()) and (not wt or (self.back(types[0])[k:] == 0xA5).all()) \
            and (not wp or (self.back(pos[0])[k:] == -7).all()), "written at or behind n_pairs * W"
        return dict(total=total, W=W, n_cut=n_cut, ids=self.back(ids[0])[:k].astype(np.int64), lens=self.back(lens[0])[:n].tolist(),
                    mask=self.back(mask[0])[:k].astype(np.int64) if wm else None, types=self.back(types[0])[:k].astype(np.int64) if wt else None,
                    pos=self.back(pos[0])[:k].astype(np.int64) if wp else None, kept=self.back(kept[0])[:nd].tolist() if wk else None,
                    offs=self.back(out[0])[:nd + 1].tolist() if wo else None)


def _same_array(what, name, got, want):
    """exact, without two Python lists of a long row"""
    want = want.reshape(-1)
    if got.shape != want.shape or not np.array_equal(got, want):
        at = int(np.flatnonzero(got[:len(want)] != want[:len(got)])[0]) if got.shape == want.shape else -1
        raise AssertionError("%s: %s differ at %d: %r / %r" % (what, name, at, got[max(at - 3, 0):at + 4].tolist(), want[max(at - 3, 0):at + 4].tolist()))


def assert_pairs(what, got, m):
    assert (got["total"], got["W"], got["n_cut"]) == (m.total, m.W, m.n_cut), (what, (got["total"], got["W"], got["n_cut"]), (m.total, m.W, m.n_cut))
    SP._same(what, "lens", [int(x) for x in got["lens"]], m.lens)
    _same_array(what, "ids", got["ids"], m.ids)
    for name, want in (("mask", m.mask), ("types", m.types), ("pos", m.pos)):
        if got[name] is not None:
            _same_array(what, name, got[name], want)
    if got["kept"] is not None:
        SP._same(what, "kept", [int(x) for x in got["kept"]], m.kept)
    if got["offs"] is not None:
        SP._same(what, "offsets", [int(x) for x in got["offs"]], m.offs)


def check_device(ctx, docs, L, what, bos=-1, sep=-1, s=0, eos=-1, pad=-3, strategy=LONGEST, cut=SUFFIX, side=RIGHT, M=1, allowed=(), arrays=(ALL,), ids_per_doc=None, b=None,
                 exact=False):
    """the device entry against the model, with the capacity that always suffices (n_pairs * L) or -- exact -- with n_pairs * W, not an entry more"""
    ids_per_doc = ids_per_doc if ids_per_doc is not None else ctx.oracle_ids(docs, allowed)
    m = Model(ids_per_doc, L, bos, sep, s, eos, pad, strategy, cut, side, M)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = b or ctx.device_buffers(docs)
    for a in arrays:
        label = "%s, L %d, M %d, bos %d, sep %d x %d, eos %d, strategy %d, cut %d, pad side %d (mask %d, types %d, pos %d, kept %d, offsets %d)" \
            % ((what, L, M, bos, sep, s, eos, strategy, cut, side) + tuple(a))
        assert_pairs(label, ctx.pairs_device(b, L, index, bos, sep, s, eos, pad, strategy, cut, side, M, a, cap=(len(docs) // 2) * m.W if exact else None), m)
    return m


def interleave(first, second):
    return [d for pair in zip(first, second) for d in pair]


# ---- 1. strategy edges ----

def check_closed_form():
    """the loop of the rule and the closed forms tkz.h states beside it (the model uses the loop)"""
    for R in range(0, 40):
        h = R // 2
        H = R - h
        for a in range(0, 60):
            for b in range(0, 60):
                assert kept_counts(a, b, R, LONGEST) == (min(a, max(H, R - b)), min(b, max(h, R - a))), (a, b, R)
                kb = min(b, R)
                assert kept_counts(a, b, R, ONLY_FIRST) == (min(a, R - kb), kb), (a, b, R)
                ka = min(a, R)
                assert kept_counts(a, b, R, ONLY_SECOND) == (ka, min(b, R - ka)), (a, b, R)


def check_strategy_edges(ctx):
    rng = random.Random(3)
    pool = {n: words(rng, n) for n in range(0, 40)}
    pool_ids = dict(zip(pool, ctx.oracle_ids(list(pool.values()))))
    assert all(len(pool_ids[n]) == n for n in pool)
    for L in (11, 12):                                        # R odd and even
        for bos, eos in FORMS:
            for s in (0, 1, 2):
                f = (bos >= 0) + s + (eos >= 0)
                R = L - f
                h = R // 2
                H = R - h
                sizes = sorted({0, 1, h - 1, h, H, H + 1, R - 1, R, R + 1, 3 * L})
                assert sizes[0] == 0 and (L + f) % 2 == R % 2
                pairs = [(a, b) for a in sizes for b in sizes]
                docs = interleave([pool[a] for a, _ in pairs], [pool[b] for _, b in pairs])
                ids = interleave([pool_ids[a] for a, _ in pairs], [pool_ids[b] for _, b in pairs])
                bufs = ctx.device_buffers(docs)
                for strategy in STRATEGIES:
                    for cut, side in SIDES:
                        m = check_device(ctx, docs, L, "strategy edges", bos, SEP if s else -1, s, eos, strategy=strategy, cut=cut, side=side, ids_per_doc=ids, b=bufs)
                        assert m.W == L and m.n_cut == sum(a + b > R for a, b in pairs)
                        for p, (a, b) in enumerate(pairs):
                            ka, kb = m.kept[2 * p:2 * p + 2]
                            assert ka + kb == min(a + b, R) and m.lens[p] == ka + kb + f
                            if strategy == LONGEST and a + b > R:
                                assert abs(ka - kb) <= 1 and ka >= kb or ka == a or kb == b      # both cut: A gets the odd id; else the shorter one is whole
                if f:                                         # L == f: every row is the framing, nothing is kept
                    for strategy in STRATEGIES:
                        for cut, side in SIDES:
                            m = check_device(ctx, docs, f, "L == f", bos, SEP if s else -1, s, eos, strategy=strategy, cut=cut, side=side, ids_per_doc=ids, b=bufs)
                            assert (m.W, m.lens, m.kept) == (f, [f] * len(pairs), [0] * len(docs)) and m.mask.all() and m.n_cut == len(pairs) - 1
    sizes = ((3, 2), (0, 0), (1, 0), (0, 4), (2, 2))          # L == 1 without framing: one id of the pair, or none
    docs = interleave([pool[a] for a, _ in sizes], [pool[b] for _, b in sizes])
    for strategy in STRATEGIES:
        for cut, side in SIDES:
            m = check_device(ctx, docs, 1, "L == 1", strategy=strategy, cut=cut, side=side)
            assert (m.W, m.n_cut, m.lens) == (1, 3, [1, 0, 1, 1, 1])
            assert m.kept == ([1, 0, 0, 0, 1, 0, 0, 1] + [1, 0] if strategy != ONLY_FIRST else [0, 1, 0, 0, 1, 0, 0, 1, 0, 1])


# ---- 2. type ids and NULL arrays ----

def check_types_and_nulls(ctx):
    rng = random.Random(4)
    docs = [b"", words(rng, 3), words(rng, 4), b"", b"", b"", words(rng, 2), words(rng, 5), words(rng, 9), words(rng, 9)]
    ids = ctx.oracle_ids(docs)
    bufs = ctx.device_buffers(docs)
    for bos, eos in FORMS:
        for s in (0, 1, 2):
            for side in (RIGHT, LEFT):
                m = check_device(ctx, docs, 12, "types", bos, SEP if s else -1, s, eos, side=side, arrays=ARRAYS, ids_per_doc=ids, b=bufs)
                fe = int(eos >= 0)
                assert m.types.sum(axis=1).tolist() == [kb + fe for kb in m.kept[1::2]]          # the second text's kept ids and the eos, nothing else
                assert m.types[2].sum() == fe and m.types[1].sum() == fe                           # an empty B, both empty: the eos alone
                assert ((m.types == 1) <= (m.mask == 1)).all()
    # 75 pairs of empty texts: with framing every row is the framing, without it W is 0 and nothing is written
    empties = [b""] * 150
    for bos, eos in FORMS:
        for s in (0, 2):
            f = (bos >= 0) + s + (eos >= 0)
            for M in (0, 1, 8):
                m = check_device(ctx, empties, 6, "75 empty pairs", bos, SEP if s else -1, s, eos, side=LEFT, M=M, arrays=ARRAYS)
                assert (m.total, m.n_cut, m.lens) == (0, 0, [f] * 75) and m.W == (0 if f == 0 else 6 if M == 0 else min(6, M) if M > 1 else f)


# ---- 3. width ----

def check_width(ctx):
    rng = random.Random(5)
    L = 200
    for M in (0, 1, 8, 64):
        base = max(M, 1) * (24 // max(M, 1) + 1)              # (above the other pairs' rows)
        for longest in (base - 1, base, base + 1):            # the longest len a multiple of M, one below it and one above it (separator and eos included)
            a = (longest - 2) // 2
            docs = [words(rng, 3), words(rng, 4), words(rng, a), words(rng, longest - 2 - a), b"", b"", words(rng, 9), words(rng, 8)]
            for side in (RIGHT, LEFT):
                m = check_device(ctx, docs, L, "width", -1, SEP, 1, 9, side=side, M=M, exact=True)
                assert m.n_cut == 0 and max(m.lens) == longest
                assert m.W == (L if M == 0 else -(-longest // M) * M)
    # the round-up exceeds L: clamped
    docs = [words(rng, 40), words(rng, 30), words(rng, 2), words(rng, 3), words(rng, 100), words(rng, 200)]
    for M, L in ((64, 100), (8, 21), (64, 63), (1000, 7)):
        for strategy in STRATEGIES:
            for cut, side in SIDES:
                m = check_device(ctx, docs, L, "width clamped", 7, SEP, 2, 9, strategy=strategy, cut=cut, side=side, M=M, exact=True)
                assert m.W == L and m.n_cut == (1 if L == 100 else 3 if L == 7 else 2)
    m = check_device(ctx, docs[:4], 100, "width from the longest", 7, SEP, 2, 9, M=8)
    assert (m.W, m.n_cut, m.lens) == (80, 0, [74, 9])


# ---- 4. tile, row and seam geometry ----

def _factor(target):
    """(n_pairs, W) with n_pairs * W == target and as many rows as a small factor gives"""
    n = next((k for k in range(2, 200) if target % k == 0), 1)
    return n, target // n


def check_geometry(ctx):
    rng = random.Random(7)
    # many rows in a group of 64 positions: 150 pairs, fixed width
    for W in (1, 3, 7, 63, 64, 65):
        first = [words(rng, (5 * p) % (W + 3)) for p in range(150)]
        second = [words(rng, (3 * p) % (W + 2)) for p in range(150)]
        docs = interleave(first, second)
        ids = ctx.oracle_ids(docs)
        bufs = ctx.device_buffers(docs)
        s, eos = (0, -1) if W == 1 else (1, 9)
        for side in (RIGHT, LEFT):
            m = check_device(ctx, docs, W, "W = %d" % W, -1, SEP if s else -1, s, eos, cut=PREFIX if side == LEFT else SUFFIX, side=side, M=0, arrays=ARRAYS, ids_per_doc=ids,
                             b=bufs, exact=True)
            assert m.W == W
    # a row across tiles
    for W in (K - 1, K, K + 1, 2 * K + 5):
        docs = [words(rng, W // 2), words(rng, W), words(rng, 5), words(rng, 2), words(rng, W + 7), b""]
        ids = ctx.oracle_ids(docs)
        bufs = ctx.device_buffers(docs)
        for side in (RIGHT, LEFT):
            m = check_device(ctx, docs, W, "W = %d" % W, 7, SEP, 1, -1, cut=PREFIX if side == LEFT else SUFFIX, side=side, arrays=ARRAYS, ids_per_doc=ids, b=bufs, exact=True)
            assert (m.W, m.n_cut, m.lens) == (W, 2, [W, 9, W])
    # the seam between the two texts, its two separators astride an edge of a group of 64 and of a tile
    for seam in (63, 64, 65, K - 1, K, K + 1):
        W = seam + 40
        docs = [words(rng, seam - 1), words(rng, 10), words(rng, 2), words(rng, 1), words(rng, seam - 1), words(rng, 90)]
        ids = ctx.oracle_ids(docs)
        bufs = ctx.device_buffers(docs)
        for strategy, side in ((ONLY_SECOND, RIGHT), (LONGEST, RIGHT), (ONLY_SECOND, LEFT)):
            m = check_device(ctx, docs, W, "seam at %d" % seam, 7, SEP, 2, 9, strategy=strategy, side=side, M=0, arrays=ARRAYS, ids_per_doc=ids, b=bufs, exact=True)
            assert m.W == W
            if strategy == ONLY_SECOND:
                assert m.kept[0] == m.kept[4] == seam - 1 and m.lens[2] == W
                if side == RIGHT:
                    assert m.ids[0, seam:seam + 2].tolist() == [SEP, SEP] and m.types[0, seam + 1] == 0 and m.types[0, seam + 2] == 1
    # n_pairs * W one below, at and one above a tile multiple
    for target in (2 * K - 1, 2 * K, 2 * K + 1):
        n, W = _factor(target)
        docs = interleave([words(rng, (7 * p) % (W + 2)) for p in range(n)], [words(rng, (3 * p) % 5) for p in range(n)])
        docs[-2] = words(rng, W)                              # (the longest row is W)
        for side in (RIGHT, LEFT):
            m = check_device(ctx, docs, W, "n_pairs * W = %d" % target, -1, SEP, 1, 9, side=side, arrays=ARRAYS, exact=True)
            assert n * m.W == target


# ---- 5. grid stride ----

def check_grid_stride(ctx, lib):
    """more tiles than the capped grid has wavefronts: one fixed-width row that long, nearly all of it padding (the texts are a few tokens); and more pairs than
    k_pair_lens has lanes: empty texts, a row of one framing id each"""
    rng = random.Random(9)
    L = (GRID * 4 + 3) * K + 5
    docs = [words(rng, 3), words(rng, 2)]
    for side, arrays in ((RIGHT, (False, True, False, False, False)), (LEFT, (False,) * 5)):
        m = check_device(ctx, docs, L, "grid stride: tiles", -1, SEP, 1, 9, side=side, M=0, arrays=(arrays,), exact=True)
        assert m.W == L > GRID * 4 * K and m.lens == [7] and m.types.sum() == 3
    n = GRID * 256 + 300
    docs = [b""] * (2 * n)
    docs[2 * 7], docs[2 * (n - 2) + 1] = words(rng, 3), words(rng, 2)
    ids = [[]] * (2 * n)
    ids[2 * 7], ids[2 * (n - 2) + 1] = ctx.oracle_ids([docs[2 * 7]])[0], ctx.oracle_ids([docs[2 * (n - 2) + 1]])[0]
    m = check_device(ctx, docs, 2, "grid stride: pairs", 7, arrays=((True, True, False, True, True),), ids_per_doc=ids, exact=True)
    assert (m.W, m.n_cut, m.total) == (2, 2, 5) and m.lens.count(1) == n - 2 and m.types.sum() == 1


# ---- 6. special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    A = (" the of" + EOT + " and to in").encode()            # 6 ids, the literal the third
    B = (EOT + " is that for" + EOT).encode()                 # 5 ids, the literal the first and the last
    docs = [A, B, B, A, b"", EOT.encode(), (" it" + EOT).encode(), (EOT + " was").encode()]
    ids = ctx.oracle_ids(docs, [EOT])
    assert [len(x) for x in ids] == [6, 5, 5, 6, 0, 1, 2, 2] and ids[0][2] == ids[1][0] == ids[1][4] == ids[5][0] == ids[6][1] == ids[7][0] == eot
    bufs = ctx.device_buffers(docs)
    for strategy in STRATEGIES:
        for L in (4, 6, 7, 8, 10, 14):
            for cut, side in SIDES:
                m = check_device(ctx, docs, L, "special: allowed", -1, SEP, 1, eot, strategy=strategy, cut=cut, side=side, allowed=[EOT], ids_per_doc=ids, b=bufs)
                row3 = m.ids[3][m.mask[3] == 1].tolist()
                assert row3[-1] == eot and m.types[3][m.mask[3] == 1].tolist()[-1] == 1              # eos equal to the literal's id: the framing is the last one
                if L == 14:                                   # nothing cut: the literal the last id of A and the first of B (pair 3), either side of the separator
                    assert row3 == [ids[6][0], eot, SEP, eot, ids[7][1], eot] and m.n_cut == 0
        # the literal the last kept id of A and the first kept id of B
        m = check_device(ctx, docs[:2], 8, "special: at the seam", -1, SEP, 1, -1, strategy=strategy, allowed=[EOT], ids_per_doc=ids[:2], b=None)
        ka, kb = {LONGEST: (4, 3), ONLY_FIRST: (2, 5), ONLY_SECOND: (6, 1)}[strategy]
        assert m.kept == [ka, kb] and m.ids[0].tolist() == ids[0][:ka] + [SEP] + ids[1][:kb]
        assert m.ids[0, ka] == SEP and m.ids[0, ka + 1] == eot and m.types[0, ka:ka + 2].tolist() == [0, 1]      # the literal is the first kept id of B
        L3 = {LONGEST: 7, ONLY_FIRST: 9, ONLY_SECOND: 4}[strategy]          # (three ids of A survive: the literal is the last of them)
        m = check_device(ctx, docs[:2], L3, "special: the last kept id of A", -1, SEP, 1, -1, strategy=strategy, allowed=[EOT], ids_per_doc=ids[:2], b=None)
        assert m.kept[0] == 3 and m.ids[0, :4].tolist() == ids[0][:3] + [SEP] and m.ids[0, 2] == eot
        m = check_device(ctx, docs[:2], L3, "special: the first kept id of A", -1, SEP, 1, -1, strategy=strategy, cut=PREFIX, allowed=[EOT], ids_per_doc=ids[:2], b=None)
        assert m.kept[0] == 3 and m.ids[0, 2] != eot
    s0 = ctx.enc.special_stats()
    off = check_device(ctx, docs, 12, "special: registered, not allowed", -1, SEP, 1, eot, allowed=[])
    assert off.total > sum(map(len, ids)) and ctx.enc.special_stats() == s0              # (split as plain text)


# ---- 7. capacity and arguments ----

def check_capacity(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, lib = ctx.enc, ctx.enc.lib.L
    rng = random.Random(13)
    docs = [words(rng, 9), b"", words(rng, 30), (" the" + EOT + " of").encode(), words(rng, 2), words(rng, 3)]
    nd, n, ML = len(docs), len(docs) // 2, 16
    m = Model(ctx.oracle_ids(docs, [EOT]), ML, 7, SEP, 1, eot, 0, M=8)
    assert (m.W, m.n_cut) == (16, 1)
    b = ctx.device_buffers(docs)
    need = n * m.W
    c0 = enc.pairs_calls()
    for cap in (need - 1, m.W, 0):
        with pytest.raises(N.TkzError) as ei:
            ctx.pairs_device(b, ML, [0], 7, SEP, 1, eot, 0, M=8, cap=cap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_width, ei.value.n_cut) == (m.total, m.W, m.n_cut), cap
    assert enc.pairs_calls() == c0                               # failed calls are not counted
    for a in ARRAYS:                                             # the exact capacity, sized from the figures above
        assert_pairs("exact capacity", ctx.pairs_device(b, ML, [0], 7, SEP, 1, eot, 0, M=8, arrays=a, cap=need), m)
    assert enc.pairs_calls() == c0 + len(ARRAYS)
    data, offs = parity.pack(docs)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_pairs(data, offs, ML, [0], 7, SEP, 1, eot, pad_multiple=8, out_cap=need - 1)
    assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_width, ei.value.n_cut) == (m.total, m.W, m.n_cut)
    r = enc.encode_batch_pairs(data, offs, ML, [0], 7, SEP, 1, eot, pad_multiple=8, out_cap=need)
    assert r[0].tolist() == m.ids.tolist() and r[1].tolist() == m.mask.tolist() and r[2].tolist() == m.types.tolist() and r[3].tolist() == m.pos.tolist()
    assert r[4].tolist() == m.lens and r[5].reshape(-1).tolist() == m.kept and r[6].tolist() == m.offs and r[7:] == (m.total, m.n_cut)
    # every TKZ_E_ARG of the rule, through all three entries
    bad = (dict(odd=True), dict(strategy=-1), dict(strategy=3), dict(s=-1), dict(s=3), dict(sep=-1), dict(sep=-2), dict(bos=-2), dict(eos=-2), dict(eos=-(1 << 31)),
           dict(L=0), dict(L=-4), dict(L=1 << 31), dict(L=2), dict(cut=2), dict(cut=-1), dict(side=2), dict(side=-1), dict(M=-1), dict(M=1 << 31),
           dict(index=[1]), dict(index=[0, 0]), dict(index=[-1]))
    u16 = np.asarray([65, 66, 67], np.uint16)
    for kw in bad:
        a = dict(L=ML, index=[0], bos=7, sep=SEP, s=1, eos=eot, strategy=LONGEST, cut=SUFFIX, side=RIGHT, M=8, odd=False)
        a.update(kw)
        bb = dict(b, n=nd - 1) if a["odd"] else b
        tail = (a["bos"], a["sep"], a["s"], a["eos"], 0, a["strategy"], a["cut"], a["side"], a["M"])
        with pytest.raises(N.TkzError) as ei:
            ctx.pairs_device(bb, a["L"], a["index"], a["bos"], a["sep"], a["s"], a["eos"], 0, a["strategy"], a["cut"], a["side"], a["M"], cap=need)
        assert ei.value.code == N.E_ARG, kw
        ho = offs[:-1] if a["odd"] else offs
        uo = np.asarray([0, 2] if a["odd"] else [0, 2, 3], np.int64)
        for call in (lambda: enc.encode_batch_pairs(data[:ho[-1]], ho, a["L"], a["index"], *tail, out_cap=need),
                     lambda: enc.encode_batch_pairs_utf16(u16[:uo[-1]], uo, a["L"], a["index"], *tail, out_cap=64)):
            with pytest.raises(N.TkzError) as ei:
                call()
            assert ei.value.code == N.E_ARG, kw
    assert enc.pairs_calls() == c0 + len(ARRAYS) + 1
    plain_ids = ctx.oracle_ids(docs)
    assert Model(plain_ids, 1, 7).W == 1 and Model(plain_ids, 4, 7, SEP, 2, 9).W == 4          # (L == f is in range)
    r = enc.encode_batch_pairs(data, offs, 3, (), 7, -5, 0, -1)                                  # sep_id is not read when sep_count == 0
    assert r[0].tolist() == Model(plain_ids, 3, 7).ids.tolist()
    # NULL for a required pointer; for one that may be NULL
    ids, msk, typ, pos = ctx.upload(np.zeros(need, np.int32)), ctx.upload(np.zeros(need, np.uint8)), ctx.upload(np.zeros(need, np.uint8)), ctx.upload(np.zeros(need, np.int32))
    lens, kept, ooff = ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(nd, np.int32)), ctx.upload(np.zeros(nd + 1, np.int64))
    t, w, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    ok = (enc._h, b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], None, 0, 7, SEP, 1, eot, ML, LONGEST, SUFFIX, RIGHT, 0, 8, ids[1], need, msk[1], typ[1], pos[1], lens[1],
          kept[1], ooff[1], None, C.byref(t), C.byref(w), C.byref(c))
    plain = Model(plain_ids, ML, 7, SEP, 1, eot, 0, M=8)
    assert lib.tkz_encode_batch_pairs_device(*ok) == N.OK and (t.value, w.value, c.value) == (plain.total, plain.W, plain.n_cut)
    for k in (0, 1, 2, 17, 22, 26, 27, 28):                      # the encoder, the bytes, the offsets, d_out_ids, d_lens, total_tokens, width, n_cut
        assert lib.tkz_encode_batch_pairs_device(*(ok[:k] + (None,) + ok[k + 1:])) == N.E_ARG, k
    for k in (19, 20, 21, 23, 24):                               # d_mask, d_type_ids, d_pos, d_kept, d_out_offsets
        assert lib.tkz_encode_batch_pairs_device(*(ok[:k] + (None,) + ok[k + 1:])) == N.OK, k
    assert lib.tkz_encode_batch_pairs_device(*(ok[:18] + (-1,) + ok[19:])) == N.E_ARG
    hid, hl = np.zeros(need, np.int32), np.zeros(n, np.int32)
    hok = (enc._h, data.ctypes.data, offs.ctypes.data, nd, None, 0, 7, SEP, 1, eot, ML, LONGEST, SUFFIX, RIGHT, 0, 8, hid.ctypes.data, need, None, None, None, hl.ctypes.data,
           None, None, C.byref(t), C.byref(w), C.byref(c))
    uflat, uoffs = U16S.pack([U16S.units(d.decode()) for d in docs])
    for fn, src in ((lib.tkz_encode_batch_pairs_utf8, hok), (lib.tkz_encode_batch_pairs_utf16, (enc._h, uflat.ctypes.data, uoffs.ctypes.data) + hok[3:])):
        hid[:] = 0
        assert fn(*src) == N.OK and w.value == plain.W and hl.tolist() == plain.lens and hid.tolist() == plain.ids.reshape(-1).tolist()
        for k in (0, 2, 16, 21, 24, 25, 26):                     # the encoder, the offsets, out_ids, lens, total_tokens, width, n_cut
            assert fn(*(src[:k] + (None,) + src[k + 1:])) == N.E_ARG, k
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        ctx.pairs_device(ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]), ML, eos=9)
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_pairs(data, np.asarray([0, 12, 11, 40, 41, 42, len(data)], np.int64), ML)
    assert ei.value.code == N.E_ARG
    # no documents: TKZ_OK, W 0, the offset cleared; documents without bytes through the host entries
    none = ctx.device_buffers([])
    for bos, eos in FORMS:
        got = ctx.pairs_device(none, ML, (), bos, SEP, 1, eos, cap=0)
        assert (got["total"], got["W"], got["n_cut"], got["offs"], got["lens"], got["kept"]) == (0, 0, 0, [0], [], [])
        m3 = Model([[]] * 6, 4, bos, SEP, 1, eos, 5, side=LEFT, M=2)
        for r in (enc.encode_batch_pairs(np.zeros(0, np.uint8), np.zeros(7, np.int64), 4, (), bos, SEP, 1, eos, 5, pad_side=LEFT, pad_multiple=2),
                  enc.encode_batch_pairs_utf16(np.zeros(0, np.uint16), np.zeros(7, np.int64), 4, (), bos, SEP, 1, eos, 5, pad_side=LEFT, pad_multiple=2)):
            assert r[0].shape == (3, m3.W) and (r[0].tolist(), r[1].tolist(), r[2].tolist(), r[3].tolist(), r[4].tolist(), r[5].tolist(), r[6].tolist(), r[7], r[8]) == \
                (m3.ids.tolist(), m3.mask.tolist(), m3.types.tolist(), m3.pos.tolist(), m3.lens, [[0, 0]] * 3, [0] * 7, 0, 0)
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    d1, o1 = parity.pack([b"a<|s7|>b", b"c"])
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_batch_pairs(d1, o1, 4, [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_batch_pairs(d1, o1, 64)[7] == len(many.oenc.encode_bytes(b"a<|s7|>b")) + 1          # (nothing allowed: the plain call)


# ---- 8. agreement of the entries ----

def check_agreement(make_ctx, lib, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc = ctx.enc
    rng, gib, mixed, crowded = CC.generators(7)
    w = lambda n: CC.fill(rng, n).decode()
    lone = "lone \ud800 high"
    texts = [w(300) + EOT + w(40), gib(600, 2, 9), "", words(rng, 2 * K + 9).decode(), "café " + EMOJI + " 漢字 " + w(20), lone, mixed(1500, 3, 3, 30), EOT, w(5), ""]
    unit_docs = [U16S.units(t) for t in texts]
    docs = [U16.get_bytes(u) for u in unit_docs]                 # (Encoding.UTF8.GetBytes: the lone surrogate becomes EF BF BD)
    data, offs = parity.pack(docs)
    flat, uoffs = U16S.pack(unit_docs)
    b = ctx.device_buffers(docs)
    for index, allowed in (([0], [EOT]), ([], [])):
        want = ctx.oracle_ids(docs, allowed)
        assert len(want[3]) == 2 * K + 9
        for bos, s, eos, ML, strategy, cut, side, M in ((-1, 0, -1, 64, LONGEST, SUFFIX, RIGHT, 1), (7, 2, eot, 64, ONLY_FIRST, PREFIX, LEFT, 8),
                                                        (-1, 1, eot, 1000, ONLY_SECOND, SUFFIX, LEFT, 0), (7, 1, eot, 5000, LONGEST, PREFIX, RIGHT, 64)):
            sep = SEP if s else -1
            m = Model(want, ML, bos, sep, s, eos, 0, strategy, cut, side, M)
            c0 = enc.pairs_calls()
            assert_pairs("agreement: device", ctx.pairs_device(b, ML, index, bos, sep, s, eos, 0, strategy, cut, side, M), m)
            assert parity.read_device_i64(lib, enc.counts_device, 3).tolist() == [len(docs), len(data), m.total]      # the counts block receives the uncut total
            for name, r in (("utf8", enc.encode_batch_pairs(data, offs, ML, index, bos, sep, s, eos, 0, strategy, cut, side, M)),
                            ("utf16", enc.encode_batch_pairs_utf16(flat, uoffs, ML, index, bos, sep, s, eos, 0, strategy, cut, side, M))):
                host = dict(total=r[7], W=r[0].shape[1], n_cut=r[8], ids=r[0].reshape(-1).astype(np.int64), mask=r[1].reshape(-1).astype(np.int64),
                            types=r[2].reshape(-1).astype(np.int64), pos=r[3].reshape(-1).astype(np.int64), lens=r[4].tolist(), kept=r[5].reshape(-1).tolist(), offs=r[6].tolist())
                assert_pairs("agreement: " + name, host, m)
                assert r[0].shape == r[1].shape == r[2].shape == r[3].shape == (len(docs) // 2, m.W) and r[1].dtype == r[2].dtype == np.uint8
            assert enc.pairs_calls() == c0 + 3


# ---- 9. retry ----

def check_retry(make_ctx):
    """the first call of a fresh encoder is a pair call whose miss lists overflow (the padded retry text, read as pairs): the attempt is run again inside the
    call, and the caller's buffers hold the final attempt's rows only"""
    ctx = make_ctx()
    rng, gib, mixed, crowded = CC.generators(47)
    cjk = "漢字かな交じり文、한국어 " + EMOJI + " naïve café "
    docs = [(cjk * 80).encode("utf-8")] + CC.cut(gib(30000, 2, 2).encode(), [700, 9000]) + [b"", CC.fill(rng, 300)]
    docs += [b""] * (len(docs) % 2)
    ids = ctx.oracle_ids(docs)
    b = ctx.device_buffers(docs)
    w0 = ctx.enc.workspace_bytes
    first = check_device(ctx, docs, 512, "retry: first call", 7, SEP, 1, 9, M=64, ids_per_doc=ids, b=b, exact=True)
    assert ctx.enc.workspace_bytes > w0
    again = check_device(ctx, docs, 512, "retry: again", 7, SEP, 1, 9, M=64, ids_per_doc=ids, b=b, exact=True)
    assert (first.total, first.W) == (again.total, again.W) and first.n_cut >= 1
    check_device(ctx, docs, 512, "retry: the tails", strategy=ONLY_FIRST, cut=PREFIX, side=LEFT, ids_per_doc=ids, b=b)


# ---- 10. the Python mirror ----

def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256, "<s>": 50300, "</s>": 50301}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    oenc = O.Encoder(O.Vocab(raw_gpt2), N.P1, specials=specials)
    lines = lib_rs_text.split("\n")
    first, second = lines[:-1], lines[1:]                        # line i beside line i + 1
    want = [oenc.encode(t, [EOT]) for t in interleave(first, second)]
    L = 40
    ids, mask, types, lens, kept, pos = tok.EncodeBatchPairs(first, second, L, [EOT], sep=EOT, eos=EOT, pad_to_multiple_of=8, return_pos=True)
    m = Model(want, L, -1, 50256, 1, 50256, 0, M=8)
    assert ids.shape == mask.shape == types.shape == pos.shape == (len(first), m.W) and ids.dtype == np.int32 and mask.dtype == types.dtype == np.uint8 and m.n_cut >= 3
    assert (ids.tolist(), mask.tolist(), types.tolist(), pos.tolist(), lens.tolist(), kept.reshape(-1).tolist()) == \
        (m.ids.tolist(), m.mask.tolist(), m.types.tolist(), m.pos.tolist(), m.lens, m.kept)
    # ... and against EncodeBatch plus the host loop this call replaces
    loop = np.zeros((len(first), m.W), np.int64)
    enc_a, enc_b = tok.EncodeBatch(first, [EOT]), tok.EncodeBatch(second, [EOT])
    for p, (A, B) in enumerate(zip(enc_a, enc_b)):
        A, B = list(A), list(B)
        while len(A) + len(B) > L - 2:
            (A if len(A) > len(B) else B).pop()
        row = A + [50256] + B + [50256]
        loop[p, :len(row)] = row
    assert ids.tolist() == loop.tolist()
    # <s> A </s></s> B </s>: two separators, the tails, padded on the left to the fixed width; the literal in the text allowed and not
    a_texts = ["a" + EOT + "b", "", "Hi " + EMOJI + " café", " the of and to in is that for it with"]
    b_texts = [" of and", "x", "", " was on are as with his they at be this from"]
    for apply in (True, False):
        for truncation, code in (("longest_first", LONGEST), ("only_first", ONLY_FIRST), ("only_second", ONLY_SECOND)):
            ids, mask, types, lens, kept = tok.EncodeBatchPairs(a_texts, b_texts, 12, apply, bos="<s>", sep="</s>", sep_count=2, eos="</s>", pad=-1, truncation=truncation,
                                                                truncation_side="left", padding_side="left", fixed_width=True)
            m = Model([oenc.encode(t, list(specials) if apply else []) for t in interleave(a_texts, b_texts)], 12, 50300, 50301, 2, 50301, -1, code, PREFIX, LEFT, 0)
            assert (ids.tolist(), mask.tolist(), types.tolist(), lens.tolist(), kept.tolist()) == (m.ids.tolist(), m.mask.tolist(), m.types.tolist(), m.lens,
                                                                                               np.asarray(m.kept).reshape(-1, 2).tolist())
            assert ids.shape == (4, 12) and m.n_cut >= 1
    r = tok.EncodeBatchPairs(["a b"], ["c"], 8, sep=None)          # no separator
    assert r[0].tolist() == [oenc.encode("a b", []) + oenc.encode("c", [])] and r[2].tolist() == [[0, 0, 1]]
    ids, mask, types, lens, kept = tok.EncodeBatchPairs([], [], 4, eos=EOT)
    assert ids.shape == mask.shape == types.shape == (0, 0) and lens.tolist() == [] and kept.shape == (0, 2)
    for bad in (dict(max_length=0), dict(max_length=2, bos=11, sep=EOT, eos=EOT), dict(max_length=4, bos="<|nope|>"), dict(max_length=4, sep=-5), dict(max_length=4, pad_to_multiple_of=0),
                dict(max_length=4, truncation_side="up"), dict(max_length=4, padding_side="down"), dict(max_length=4, truncation="do_not_truncate"),
                dict(max_length=8, sep=EOT, sep_count=3)):
        with pytest.raises(ValueError):
            tok.EncodeBatchPairs(a_texts, b_texts, **bad)
    with pytest.raises(ValueError):
        tok.EncodeBatchPairs(a_texts, b_texts[:3], 8)
    # a literal that holds U+FFFD beside a lone surrogate: through the UTF-16 entry
    fffd = {k: v + 200000 for k, v in U16S.FFFD_SPECIALS.items()}
    tok3 = TokenizerBuilder.CreateTokenizer(raw_gpt2, fffd, REGEX_PATTERN_1, lib=lib)
    lone_a, lone_b = ["ab x\ud83d b x� c it's", "plain"], ["x� c", "b \ud83d x� it's"]
    ids, mask, types, lens, kept = tok3.EncodeBatchPairs(lone_a, lone_b, 12, list(fffd), sep=4, eos=3)
    exp = U16S.Expect(O, O.Vocab(raw_gpt2), N.P1, fffd)
    m = Model([exp.encode(U16S.units(t), list(fffd)) for t in interleave(lone_a, lone_b)], 12, -1, 4, 1, 3, 0)
    assert (ids.tolist(), mask.tolist(), types.tolist(), lens.tolist(), kept.reshape(-1).tolist()) == (m.ids.tolist(), m.mask.tolist(), m.types.tolist(), m.lens, m.kept)
