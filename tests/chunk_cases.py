"""Token-budget chunks (tkz_encode_batch_chunks_device / _utf8 / _utf16, tkz_encode_chunks_utf8 / _utf16; k_chunk_walk, k_chunk_walk_long, k_chunk_unitcount,
k_chunk_units): the cases and comparisons the emulated (CPU) and the GPU test modules share.  Every comparison is exact.

No expected value comes from the code under test:
  ids, offsets   the oracle's (oracle.Encoder; TrimOracle's literal search for UTF-16 text with lone surrogates: u16_special_cases.Expect);
  chunks (a)     the caller's loop itself: TrimOracle.encode_trim_suffix on the rest of the string, again and again.  When it returns no ids the budget is raised
                 by one until it returns some: that result is the oversize item alone, which split_oversize cuts by the rule of tkz.h;
  chunks (b)     the rule of tkz.h over the items -- oracle.split_utf8's pieces with Vocab.rank / bpe token counts, an allowed literal one item of one token;
                 small cases run (a) and (b) and both must agree with each other and with the device, large ones (b) only: (a) is quadratic pure Python;
  byte starts    the running sum of the key lengths of the oracle's ids (spans_cases.Ctx.expected_spans);
  unit starts    spans_cases.units_begun over the document's bytes.

The kernel cases go through tkz_encode_batch_chunks_device.  `upload(np_array) -> (owner, pointer)` as in count_cases: identity for the emulated build, a device
tensor on the hardware.

Geometry (tkz_kernels.h / .hip): a document of more than LONG = 1024 items is walked by a wavefront (64 items a load), a shorter one by a lane; the unit counts are
per sub-tile of SUB = 1024 bytes of the batch; the piece-granular path strides 256 KiB; a workgroup is 256 lanes.
"""
import ctypes as C
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
from tokenizer_amd import _native as N

SUB = CC.SUB
LONG = 1024
EOT = SC.EOT
fill = CC.fill
EOT_ID = SP.EOT_ID
units_begun = SP.units_begun
EMOJI = "\U0001F600"


class Ctx(SP.Ctx):
    """spans_cases.Ctx with the trim oracle and the transport of the chunk entry."""

    def __init__(self, lib, O, raw, pattern=N.CL100K, specials=None, upload=None, options=()):
        super().__init__(lib, O, raw, pattern, specials, upload, options)
        self.trim = O.TrimOracle(self.ovocab, pattern, specials)
        self._sized = {}

    def chunks_device(self, b, mx, index=(), want_bytes=True, want_units=True, cap=None, ccap=None):
        cap = b["total"] if cap is None else cap
        ccap = N.Encoder.chunk_bound(b["n"], b["total"], mx) if ccap is None else ccap
        ids = self.upload(np.full(max(1, cap), -7, np.int32))
        out = self.upload(np.full(b["n"] + 1, -5, np.int64))
        dco = self.upload(np.full(b["n"] + 1, -5, np.int64))
        ct = self.upload(np.full(max(1, ccap) + 1, -7, np.int64))
        cb = self.upload(np.full(max(1, ccap), -7, np.int64)) if want_bytes else (None, 0)
        cu = self.upload(np.full(max(1, ccap), -7, np.int64)) if want_units else (None, 0)
        tot, nch = self.enc.encode_batch_chunks_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], mx, list(index), ids[1], cap, out[1], dco[1], ct[1],
                                                       cb[1], cu[1], ccap)
        offs, dcos = self.back(out[0]).tolist(), self.back(dco[0]).tolist()
        assert tot == offs[-1] and nch == dcos[-1]
        return dict(ids=self.back(ids[0])[:tot].tolist(), offs=offs, dco=dcos, ct=self.back(ct[0])[:nch + 1].tolist(),
                    cb=self.back(cb[0])[:nch].tolist() if want_bytes else None, cu=self.back(cu[0])[:nch].tolist() if want_units else None)

    def piece_of_tokens(self, n, rng=None):
        """a piece (a space and consonants: one regex piece under every pattern) that the table cuts into exactly n tokens"""
        if n not in self._sized:
            rng = rng or random.Random(1000 + n)
            for _ in range(20000):
                p = (" " + "".join(rng.choice(CC.CONS) for _ in range(rng.randint(max(1, n), 3 * n + 2)))).encode()
                k = 1 if self.ovocab.rank(p) >= 0 else len(self.ovocab.bpe(p))
                self._sized.setdefault(k, p)
                if n in self._sized:
                    break
        return self._sized[n]


# ---- the two models ----

def items_of(ctx, doc, allowed=()):
    """model (b)'s items: (byte start, byte length, tokens) -- the regex pieces of the plain stretches and one item of one token per allowed literal, found as
    FindNextSpecialToken finds them (the first match of the alternation of ALL registered literals; one that is not allowed is passed by one character)"""
    if not (ctx.specials and allowed):
        return SP.pieces_of(ctx, doc)
    alt = re.compile(b"|".join(re.escape(k.encode()) for k in ctx.specials))
    names = {a.encode() for a in allowed}
    out, start, find = [], 0, 0
    while True:
        m = alt.search(doc, find)
        if m is not None and m.group(0) not in names:
            find = m.start() + 1
            continue
        end = m.start() if m else len(doc)
        out += [(start + a, n, t) for a, n, t in SP.pieces_of(ctx, doc[start:end])]
        if m is None:
            return out
        out.append((m.start(), m.end() - m.start(), 1))
        start = find = m.end()


def rule(counts, mx):
    """the rule of tkz.h over the items' token counts: the first token of every chunk"""
    bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total, s, starts = int(bounds[-1]), 0, []
    while s < total:
        starts.append(s)
        if total - s <= mx:
            break
        b = int(bounds[np.searchsorted(bounds, s + mx, side="right") - 1])        # the largest boundary at or below s + max
        s = b if b > s else s + mx
    return starts


def split_oversize(n, mx):
    """an item of n > mx tokens at a chunk's start: the runs of mx tokens, and the tokens of the last partial run (0: the item ends with a full run)"""
    return [mx] * ((n - 1) // mx), n - mx * ((n - 1) // mx)


def model_a(ctx, text, allowed, mx):
    """the caller's loop: [(ids, text or None)] -- the text where the loop itself yields it (a chunk made of whole items)"""
    chunks, rest = [], text
    while rest:
        ids, part = ctx.trim.encode_trim_suffix(rest, list(allowed), mx)
        if ids:
            chunks.append((ids, part))
            rest = rest[len(part):]
            continue
        up = mx
        while not ids:                                                            # (the next item alone holds more than mx tokens: this is where the loop spins)
            up += 1
            ids, part = ctx.trim.encode_trim_suffix(rest, list(allowed), up)
        assert len(ids) == up > mx
        rest = rest[len(part):]
        full, last = split_oversize(len(ids), mx)
        pos = 0
        for n in full:
            chunks.append((ids[pos:pos + n], None))
            pos += n
        more, part = ctx.trim.encode_trim_suffix(rest, list(allowed), mx - last) if rest else ([], "")     # the partial run goes on taking the items that follow
        chunks.append((ids[pos:] + more, None))
        rest = rest[len(part):]
    return chunks


class Expected:
    """what the entry must return for `docs` (bytes) at budget mx, by model (b); with small=True model (a) is run as well and must agree"""

    def __init__(self, ctx, docs, mx, allowed=(), small=True, ids_per_doc=None, items=None):
        self.ids, self.offs, tb, tu = ctx.expected_spans(docs, allowed, ids_per_doc)
        self.items = items if items is not None else [items_of(ctx, d, allowed) for d in docs]
        self.dco, self.ct, self.cb, self.cu, self.starts = [0], [], [], [], []
        for d, doc in enumerate(docs):
            lo, hi = self.offs[d], self.offs[d + 1]
            assert sum(t for _, _, t in self.items[d]) == hi - lo, "model (b)'s items do not hold the oracle's tokens"
            starts = rule([t for _, _, t in self.items[d]], mx)
            self.starts.append(starts)
            self.ct += [lo + s for s in starts]
            self.cb += [tb[lo + s] for s in starts]
            self.cu += [tu[lo + s] for s in starts]
            self.dco.append(len(self.ct))
            if small and ids_per_doc is None:
                a = model_a(ctx, doc.decode("utf-8"), allowed, mx)
                assert [len(i) for i, _ in a] == [e - s for s, e in zip(starts, starts[1:] + [hi - lo])], ("models (a) and (b) disagree", d, mx)
                assert [x for i, _ in a for x in i] == self.ids[lo:hi]
                u16 = doc.decode("utf-8").encode("utf-16-le")
                cuts = [tu[lo + s] for s in starts] + [len(u16) // 2]
                for c, (_, part) in enumerate(a):
                    assert part is None or part == u16[2 * cuts[c]:2 * cuts[c + 1]].decode("utf-16-le"), ("model (a)'s text", d, c)
        self.ct.append(len(self.ids))

    def sizes(self, d):
        """the token counts of document d's chunks"""
        s = self.starts[d]
        return [e - b for b, e in zip(s, s[1:] + [self.offs[d + 1] - self.offs[d]])]

    def inside(self, d):
        """the chunks of document d that start inside an item"""
        bounds = set(np.cumsum([0] + [t for _, _, t in self.items[d]]).tolist())
        return [c for c, s in enumerate(self.starts[d]) if s not in bounds]


def assert_chunks(what, got, exp, mx):
    for name in ("offs", "ids", "dco", "ct", "cb", "cu"):
        if got[name] is not None:
            SP._same(what, name, [int(x) for x in got[name]], getattr(exp, name))
    sizes = [b - a for a, b in zip(got["ct"], got["ct"][1:])]
    assert all(1 <= n <= mx for n in sizes), what                                 # no chunk is empty and none exceeds the budget


FORMS = ((True, True),)
ALL_FORMS = ((True, True), (True, False), (False, True), (False, False))


def check_device(ctx, docs, mx, what, allowed=(), forms=FORMS, small=True):
    exp = Expected(ctx, docs, mx, allowed, small)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = ctx.device_buffers(docs)
    for wb, wu in forms:
        assert_chunks("%s, max %d (bytes %d, units %d)" % (what, mx, wb, wu), ctx.chunks_device(b, mx, index, wb, wu), exp, mx)
    return exp


def words(rng, n):
    """a document of exactly n items of one token each: every word with the blank in front of it (a key of the tables the tests use)"""
    return "".join(" " + rng.choice(CC.WORDS) for _ in range(n)).encode()


# ---- 1. document sizes and small budgets ----

def check_sizes(ctx):
    rng = random.Random(5)
    for mx in (1, 2, 7):
        docs = [b"", words(rng, mx), words(rng, mx + 1), b"", words(rng, 3 * mx), words(rng, 3 * mx + 1), b"x", b""]
        exp = check_device(ctx, docs, mx, "sizes", forms=ALL_FORMS)
        assert exp.sizes(0) == [] and exp.sizes(1) == [mx] and exp.sizes(2) == [mx, 1]      # 0 tokens, exactly max, max + 1; an empty document between two others
        assert exp.sizes(4) == [mx] * 3 and exp.dco[3] == exp.dco[4]                         # a chunk end that coincides with the document end
        assert len(exp.sizes(5)) >= 3
    # max = 1: every token a chunk, pieces of several tokens split; max = 2
    gib = b"it's zqxjkvbwpm and wvkqzzj the\n\nqqxz"
    for mx in (1, 2):
        exp = check_device(ctx, [gib, b"a", gib[:9]], mx, "small budgets")
        assert exp.inside(0) and (mx > 1 or exp.sizes(0) == [1] * len(exp.sizes(0)))
    # no documents; no bytes
    for n in (0, 3):
        b0 = ctx.device_buffers([b""] * n)
        got = ctx.chunks_device(b0, 4, cap=0, ccap=0)
        assert (got["ids"], got["offs"], got["dco"], got["ct"], got["cb"], got["cu"]) == ([], [0] * (n + 1), [0] * (n + 1), [0], [], [])
        r = ctx.enc.encode_batch_chunks(np.zeros(0, np.uint8), np.zeros(n + 1, np.int64), 4)
        assert (len(r[0]), r[1].tolist(), r[2].tolist(), r[3].tolist(), len(r[4]), len(r[5])) == (0, [0] * (n + 1), [0] * (n + 1), [0], 0, 0)
    r = ctx.enc.encode_batch_chunks_utf16(np.zeros(0, np.uint16), np.zeros(3, np.int64), 4)
    assert r[1].tolist() == [0, 0, 0] and r[2].tolist() == [0, 0, 0] and r[3].tolist() == [0]
    assert ctx.enc.encode_chunks(b"", 4) == ([], [0], [], []) and ctx.enc.encode_chunks_utf16([], 4) == ([], [0], [])


# ---- 2. oversize items ----

def check_oversize(ctx):
    rng = random.Random(11)
    for mx in (3, 4):
        for n in (mx + 1, 2 * mx, 2 * mx + 1):
            big = ctx.piece_of_tokens(n)
            half = words(rng, mx // 2 + 1)                                        # items that half-fill a chunk
            docs = [big + words(rng, 2 * mx),                                      # at the document's start, followed by items that fill the tail chunk
                    words(rng, 2 * mx) + big,                                     # at its end
                    half + big + words(rng, mx),                                  # after items that half-fill a chunk: the chunk closes in front of the item
                    big + big + big]
            exp = check_device(ctx, docs, mx, "oversize item of %d tokens" % n, forms=((True, True), (False, True)))
            for d in range(len(docs)):
                assert n in [t for _, _, t in exp.items[d]] and exp.inside(d), (mx, n, d)
            full, last = split_oversize(n, mx)
            assert exp.sizes(0)[:len(full)] == full and (last == mx or exp.sizes(0)[len(full)] > last)      # the partial run takes the items that follow
            k = len(exp.items[2]) - 1 - mx                                          # (the oversize item of docs[2])
            assert exp.items[2][k][2] == n and sum(t for _, _, t in exp.items[2][:k]) in exp.starts[2] and exp.sizes(2)[0] < mx
            assert exp.sizes(1)[-1] == (last if last < mx else mx)


# ---- 3. special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot, "<|other|>": eot + 1})
    rng = random.Random(17)
    w = lambda n: words(rng, n).decode()
    # an allowed literal as an item at a chunk boundary: it is token 4 (the last of chunk 0), token 5 (the first of chunk 1) ...
    docs = [w(3) + EOT + w(9), w(4) + EOT + w(9), w(3) + EOT + EOT + w(3), EOT, w(2) + "<|other|>" + w(2) + EOT, "", EOT + w(8)]
    bdocs = [d.encode() for d in docs]
    for mx in (1, 4):
        s0 = ctx.enc.special_stats()
        on = check_device(ctx, bdocs, mx, "special: allowed", allowed=[EOT])
        s1 = ctx.enc.special_stats()
        assert s1[0] - s0[0] == 1 and s1[1] - s0[1] == on.ids.count(eot) == 7
        off = check_device(ctx, bdocs, mx, "special: n_allowed == 0", allowed=[])      # the same text with nothing allowed
        assert ctx.enc.special_stats() == s1 and eot not in off.ids and len(off.ids) > len(on.ids)
        assert eot + 1 not in on.ids                                                  # a literal that is not allowed is plain text
    assert on.ids[on.ct[on.dco[1] + 1]] == eot and on.ids[on.ct[on.dco[0] + 1] - 1] == eot and on.cb[on.dco[1] + 1] == len(w(0)) + len(docs[1].split(EOT)[0])


# ---- 4. units at sub-tile edges ----

def check_units(ctx, gpt2=True):
    # a token and an item at every byte: at max = 1 a chunk starts at batch bytes 1023, 1024 and 1025
    every = b"a\nb\nc\nd\n" * 140
    exp = check_device(ctx, [b"xy", every], 1, "units: a chunk at every byte", forms=((True, True), (False, True)))
    starts = {2 + b for b in exp.cb[exp.dco[1]:exp.dco[2]]}
    assert {SUB - 1, SUB, SUB + 1} <= starts
    # a 4-byte character across the sub-tile edge in front of a chunk start, and an emoji split across chunks at max = 1
    n = len(ctx.oenc.encode_bytes(EMOJI.encode()))
    doc = b"a\n" * 511 + EMOJI.encode() + b"a\nb\n" * 8
    assert len(b"a\n" * 511) == SUB - 2
    exp = check_device(ctx, [doc], 1, "units: a character across the sub-tile edge", forms=((True, True), (False, True)))
    k = exp.cb.index(SUB + 2)
    assert exp.cu[k] == SUB - 2 + 2 and exp.cu[k + 1] == exp.cu[k] + 1
    if gpt2:
        assert n > 1
    if n > 1:                                                                        # the first chunk carries both units, the others start behind them
        ids, ct, cb, cu = ctx.enc.encode_chunks(EMOJI.encode(), 1)
        assert ct == list(range(n + 1)) and cu == [0] + [2] * (n - 1) and cb[0] == 0 and sorted(set(cb)) == cb
    texts = [EMOJI, "a" + EMOJI + "b", "café naïve 漢字 " + EMOJI * 3 + " \U0001F44D\U0001F3FD end", "", "漢字かな交じり文、한국어 " * 30]
    for mx in (1, 3):
        check_device(ctx, [t.encode("utf-8") for t in texts], mx, "units", forms=((True, True), (False, True)))
    # the UTF-16 entry: a lone surrogate, a pair cut by a document boundary
    docs = [U16S.units("cut " + EMOJI)[:-1], U16S.units(EMOJI)[1:] + U16S.units(" here"), U16S.units("lone ") + [0xD800] + U16S.units(" high it's zqxjk"), [],
            U16S.units(EMOJI + " end")]
    flat, uoffs = U16S.pack(docs)
    bdocs = [U16.get_bytes(d) for d in docs]
    for mx in (1, 2):
        want = Expected(ctx, bdocs, mx, small=False)
        ids, ooff, dco, ct, cu = ctx.enc.encode_batch_chunks_utf16(flat, uoffs, mx)
        assert_chunks("units: utf16", dict(ids=ids.tolist(), offs=ooff.tolist(), dco=dco.tolist(), ct=ct.tolist(), cb=None, cu=cu.tolist()), want, mx)
        for d, doc in enumerate(docs):                                              # the lone surrogate is the one unit it is: the last chunk ends at the length in units
            if want.dco[d + 1] > want.dco[d]:
                c = want.dco[d + 1] - 1
                assert cu[c] + int(units_begun(bdocs[d][want.cb[c]:])[-1]) == len(doc)
            i1, c1, u1 = ctx.enc.encode_chunks_utf16(doc, mx)
            lo = want.offs[d]
            assert i1 == want.ids[lo:want.offs[d + 1]] and c1 == [x - lo for x in want.ct[want.dco[d]:want.dco[d + 1]]] + [len(i1)] and u1 == want.cu[want.dco[d]:want.dco[d + 1]]


# ---- 5. search widths, workgroup edges, the long-document form ----

def check_widths(ctx):
    rng = random.Random(23)
    short, long = words(rng, 900), words(rng, 1500)
    for mx in (63, 64, 65, 200):
        exp = check_device(ctx, [short, long], mx, "widths", small=False)
        assert len(exp.items[0]) == 900 <= LONG < len(exp.items[1]) == 1500
        assert exp.sizes(0)[:3] == [mx] * 3 and exp.sizes(1)[:3] == [mx] * 3         # chunks of mx items: under, at and over a window of 64
    check_device(ctx, [short[:3000]], 64, "widths: models", small=True)


def check_workgroup_edges(ctx):
    rng = random.Random(29)
    for n in (255, 256, 257):
        docs = [words(rng, rng.choice([0, 1, 3, 4, 5, 9])) for _ in range(n)]
        docs[-1] = words(rng, 9)
        exp = check_device(ctx, docs, 4, "%d documents" % n, small=False)
        assert exp.sizes(n - 1) == [4, 4, 1] and exp.dco[-1] > n


def check_long_form(ctx):
    rng = random.Random(31)
    gib = ctx.piece_of_tokens(9)
    for mx in (4, 50):
        docs = [words(rng, LONG), words(rng, LONG + 1), words(rng, 40), words(rng, LONG - 1) + gib, words(rng, 700) + gib + words(rng, 700), words(rng, 2 * LONG + 70)]
        exp = check_device(ctx, docs, mx, "long documents", forms=((True, True), (False, False)), small=False)
        assert [len(i) for i in exp.items] == [LONG, LONG + 1, 40, LONG, 1401, 2 * LONG + 70]      # just under and just over the threshold
        assert (mx > 9) == (not exp.inside(4)) and (mx > 9) == (not exp.inside(3))
    check_device(ctx, [words(rng, LONG + 1)[:2500]], 4, "long documents: models", small=True)


# ---- 6. the piece-granular path's stride ----

def check_stride(ctx, total=300 << 10):
    rng = random.Random(37)
    doc = fill(rng, total)
    exp = check_device(ctx, [doc], 8, "one document of 300 KiB", small=False)
    assert len(doc) > 256 << 10 and exp.dco[-1] > 3000 and len(exp.items[0]) > LONG


# ---- 7. capacity, argument errors ----

def check_errors(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, L = ctx.enc, ctx.enc.lib.L
    docs = [b"hello world it's a fine day", b"", b"zqxjk " + EOT.encode() + b" and more words here"]
    mx = 3
    exp = Expected(ctx, docs, mx, [EOT])
    b = ctx.device_buffers(docs)
    need, nch = len(exp.ids), exp.dco[-1]
    assert nch >= 4
    c0 = enc.chunks_calls()
    for cap, ccap in ((need - 1, nch), (need, nch - 1), (need - 1, nch - 1), (0, 0)):
        with pytest.raises(N.TkzError) as ei:
            ctx.chunks_device(b, mx, [0], cap=cap, ccap=ccap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_chunks) == (need, nch), (cap, ccap)
    data, offs = parity.pack(docs)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_chunks(data, offs, mx, [0], chunk_cap=nch - 1)
    assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_chunks) == (need, nch)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_chunks(docs[0], mx, chunk_cap=exp.dco[1] - 1)
    assert ei.value.code == N.E_CAPACITY and ei.value.needed_chunks == exp.dco[1]
    assert enc.chunks_calls() == c0                                                  # failed calls are not counted
    assert_chunks("exact capacity", ctx.chunks_device(b, mx, [0], cap=need, ccap=nch), exp, mx)
    assert enc.chunks_calls() == c0 + 1
    # max_tokens 0 and negative, a bad or repeated allowed index
    for bad in (0, -1, -(1 << 40)):
        with pytest.raises(N.TkzError) as ei:
            ctx.chunks_device(b, bad, [0])
        assert ei.value.code == N.E_ARG
        for call in (lambda: enc.encode_batch_chunks(data, offs, bad), lambda: enc.encode_chunks(docs[0], bad), lambda: enc.encode_chunks_utf16([65, 66], bad),
                     lambda: enc.encode_batch_chunks_utf16(np.asarray([65, 66], np.uint16), np.asarray([0, 2], np.int64), bad)):
            with pytest.raises(N.TkzError) as ei:
                call()
            assert ei.value.code == N.E_ARG
    for index in ([1], [0, 0], [-1]):
        with pytest.raises(N.TkzError) as ei:
            ctx.chunks_device(b, mx, index)
        assert ei.value.code == N.E_ARG
    # null buffers
    ids, ooff, dco, ct, n, c = np.zeros(64, np.int32), np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(65, np.int64), C.c_int64(-1), C.c_int64(-1)
    p = lambda a: a.ctypes.data
    ok = (enc._h, p(data), p(offs), 3, None, 0, 3, p(ids), 64, p(ooff), p(dco), p(ct), None, None, 64, C.byref(n), C.byref(c))
    assert L.tkz_encode_batch_chunks_utf8(*ok) == N.OK and c.value == Expected(ctx, docs, mx, []).dco[-1]
    for k in (0, 2, 9, 10, 11):                                                      # the encoder, the offsets, out_offsets, doc_chunk_offsets, chunk_tokens
        assert L.tkz_encode_batch_chunks_utf8(*(ok[:k] + (None,) + ok[k + 1:])) == N.E_ARG, k
    assert L.tkz_encode_batch_chunks_utf8(*(ok[:14] + (-1,) + ok[15:])) == N.E_ARG
    assert L.tkz_encode_chunks_utf8(enc._h, p(data), 5, None, 0, 3, p(ids), 64, p(ct), None, None, 64, None, C.byref(c)) == N.E_ARG
    assert L.tkz_encode_chunks_utf8(enc._h, p(data), 5, None, 0, 3, p(ids), 64, p(ct), None, None, 64, C.byref(n), None) == N.E_ARG
    assert L.tkz_encode_chunks_utf8(enc._h, p(data), -1, None, 0, 3, p(ids), 64, p(ct), None, None, 64, C.byref(n), C.byref(c)) == N.E_ARG
    assert L.tkz_encode_chunks_utf16(enc._h, p(data), 2, None, 0, 3, p(ids), 64, None, None, 64, C.byref(n), C.byref(c)) == N.E_ARG
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_chunks_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], mx, [], 0, 64, 0, 0, 0, 0, 0, 64)
    assert ei.value.code == N.E_ARG
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        ctx.chunks_device(ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]), mx)
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_chunks(data, np.asarray([0, 12, 11, len(data)], np.int64), mx)
    assert ei.value.code == N.E_ARG
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_chunks(b"a<|s7|>b", mx, [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_chunks(b"a<|s7|>b", mx)[0] == many.oenc.encode_bytes(b"a<|s7|>b")          # (nothing allowed: the plain call)


# ---- 8. agreement of the entries ----

def check_agreement(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc = ctx.enc
    rng, gib, mixed, crowded = CC.generators(7)
    w = lambda n: fill(rng, n).decode()
    texts = [w(300) + EOT + w(40), gib(600, 2, 9), "", w(2 * SUB + 9), "café " + EMOJI + " 漢字 " + w(20), mixed(1500, 3, 3, 30), EOT, w(5)]
    docs = [t.encode("utf-8") for t in texts]
    data, offs = parity.pack(docs)
    flat, uoffs = U16S.pack([U16S.units(t) for t in texts])
    b = ctx.device_buffers(docs)
    for index in ([0], []):
        for mx in (1, 5, 64):
            dev = ctx.chunks_device(b, mx, index)
            ids, ooff, dco, ct, cb, cu = enc.encode_batch_chunks(data, offs, mx, index)
            host = dict(ids=ids.tolist(), offs=ooff.tolist(), dco=dco.tolist(), ct=ct.tolist(), cb=cb.tolist(), cu=cu.tolist())
            assert host == dev, (index, mx)
            eids, eoff = enc.encode_batch_special(data, offs, index)
            assert host["ids"] == eids.tolist() and host["offs"] == eoff.tolist()
            ids, ooff, dco, ct, cu = enc.encode_batch_chunks_utf16(flat, uoffs, mx, index)
            assert (ids.tolist(), ooff.tolist(), dco.tolist(), ct.tolist(), cu.tolist()) == (dev["ids"], dev["offs"], dev["dco"], dev["ct"], dev["cu"]), (index, mx)
            for d, doc in enumerate(docs):                                          # the single-text entries
                lo, c0, c1 = dev["offs"][d], dev["dco"][d], dev["dco"][d + 1]
                want = (dev["ids"][lo:dev["offs"][d + 1]], [x - lo for x in dev["ct"][c0:c1]] + [dev["offs"][d + 1] - lo], dev["cb"][c0:c1], dev["cu"][c0:c1])
                assert enc.encode_chunks(doc, mx, index) == want, (index, mx, d)
                assert enc.encode_chunks_utf16(U16S.units(texts[d]), mx, index) == (want[0], want[1], want[3]), (index, mx, d)
            # a suffix trim at the same maximum keeps every document's first chunk, wherever that chunk ends at an item boundary
            kids, koff, kb, ku = enc.encode_batch_trim(data, offs, index, N.TRIM_SUFFIX, mx)
            for d in range(len(docs)):
                kept = int(koff[d + 1] - koff[d])
                if kept:
                    c0 = dev["dco"][d]
                    assert dev["ct"][c0 + 1] - dev["ct"][c0] == kept, (index, mx, d)


# ---- 9. the Python mirror ----

def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    ctx = Ctx(lib, O, raw_gpt2, N.P1, specials)
    odd = "Hi " + EMOJI + "\U0001F44D\U0001F3FD café " + EOT + " 漢字 zqxjkvbwpmzq end"

    def compare(t, text, allowed, mx, model=None):
        a = model_a(model or ctx, text, allowed, mx)
        got = t.EncodeChunks(text, allowed, mx)
        assert [i for i, _ in got] == [i for i, _ in a], (mx, allowed)
        assert "".join(p for _, p in got) == text and all(p is None or p == g for (_, p), (_, g) in zip(a, got))
        return got
    for text, allowed, mx in ((lib_rs_text, [EOT], 64), (lib_rs_text[:6000], [], 7), (odd, [EOT], 1), (odd, [EOT], 3), (odd, [], 2), (EOT, [EOT], 5)):
        got = compare(tok, text, allowed, mx)
        assert len(got) >= (3 if len(text) > 20 else 1) and [i for g in got for i in g[0]] == tok.Encode(text, allowed)
    assert tok.EncodeChunks("", 5) == [] and tok.EncodeChunksBatch([], 5) == []
    assert tok.EncodeChunks(odd, 3) == tok.EncodeChunks(odd, [EOT], 3) and tok.EncodeChunks(odd, 3, False) == tok.EncodeChunks(odd, [], 3)      # the two overload shapes
    batch = [odd, "", lib_rs_text[:3000], EOT + "x"]
    assert tok.EncodeChunksBatch(batch, [EOT], 6) == [tok.EncodeChunks(t, [EOT], 6) for t in batch]
    for bad in (0, -3):
        with pytest.raises(ValueError):
            tok.EncodeChunks(odd, bad)
    # the host fallback: a set of literals the device's special entries refuse, and a lone surrogate beside a literal that holds U+FFFD
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TokenizerBuilder.CreateTokenizer(raw_gpt2, many, REGEX_PATTERN_1, lib=lib)
    ctx2 = Ctx(lib, O, raw_gpt2, N.P1, many)
    c0 = tok2._encoder.chunks_calls()
    text = "alpha<|s7|> zqxjkvbwpmzq beta gamma<|s8|>" + EMOJI + " delta"
    for mx in (1, 2, 5):
        got = compare(tok2, text, ["<|s7|>"], mx, ctx2)
        assert 200007 in [i for g in got for i in g[0]] and 200008 not in [i for g in got for i in g[0]]
    mixed = lib_rs_text[:9000] + "<|s7|>" + lib_rs_text[9000:] + "<|s8|>"
    got = compare(tok2, mixed, ["<|s7|>"], 64, ctx2)
    assert len(got) > 50 and [i for g in got for i in g[0]].count(200007) == 1
    assert tok2._special_on_host and tok2._encoder.chunks_calls() == c0
    fffd = {k: v + 200000 for k, v in U16S.FFFD_SPECIALS.items()}
    tok3 = TokenizerBuilder.CreateTokenizer(raw_gpt2, fffd, REGEX_PATTERN_1, lib=lib)
    lone = "ab x\ud83d b x� c it's zqxjkvb"
    c0 = tok3._encoder.chunks_calls()
    got = tok3.EncodeChunks(lone, list(fffd), 2)
    assert tok3._encoder.chunks_calls() == c0 and "".join(p for _, p in got) == lone and all(1 <= len(i) <= 2 for i, _ in got)
    assert [i for g in got for i in g[0]] == tok3.Encode(lone, list(fffd))
