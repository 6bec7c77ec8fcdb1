"""Overlapping token-budget chunks (tkz_encode_batch_chunks_overlap_device / _utf8 / _utf16, tkz_encode_chunks_overlap_utf8 / _utf16; k_chunkov_walk,
k_chunkov_walk_long, k_chunkov_units): the cases and comparisons the emulated (CPU) and the GPU test modules share.  Every comparison is exact.

No expected value comes from the code under test:
  ids, offsets, positions   the oracle's, as chunk_cases.Expected takes them (spans_cases.Ctx.expected_spans, units_begun);
  table (b)                 the rule of tkz.h over the oracle's items (`rule`, the brute-force script of the issue, kept here as a property test);
  table (a)                 on small cases the caller's own loop: TrimOracle.encode_trim_suffix for a chunk, TrimOracle.encode_trim_prefix(chunk text, overlap) for
                            the text the next chunk starts with (the whole chunk kept: its first item is dropped), a trial encode_trim_suffix for the chunk that
                            adds nothing, and split_oversize-style arithmetic inside an item over the budget.  (a) applies to a chunk only where the chunk's text
                            alone splits into the items it has inside the document; `left_out` counts the others, and is 0 for words() / piece_of_tokens().
"""
import bisect
import ctypes as C
import random

import numpy as np
import pytest

import chunk_cases as CK
import parity
import special_cases as SC
import u16_cases as U16
import u16_special_cases as U16S
from tokenizer_amd import _native as N

SUB, LONG, EOT, EMOJI = CK.SUB, CK.LONG, CK.EOT, CK.EMOJI
words, fill = CK.words, CK.fill
ALL = (True, True, True, True)


# ---- the rule (tkz.h) and its brute-force check ----

def end_of(bounds, T, s, N_):
    if T - s <= N_:
        return T
    b = bounds[bisect.bisect_right(bounds, s + N_) - 1]
    return b if b > s else s + N_


def rule0(bounds, T, N_):
    s, out = 0, []
    while s < T:
        out.append(s)
        e = end_of(bounds, T, s, N_)
        if e == T:
            break
        s = e
    return out


def rule(counts, N_, O_):
    """[(s, e)] of every chunk, the items' boundaries, T, and how often the adds-nothing rule fired"""
    bounds = [0]
    for c in counts:
        bounds.append(bounds[-1] + c)
    T, s, out, fb = bounds[-1], 0, [], 0
    while s < T:
        e = end_of(bounds, T, s, N_)
        out.append((s, e))
        if e == T:
            break
        x = max(e - O_, s + 1)
        i = bisect.bisect_left(bounds, x)
        n = bounds[i] if bounds[i] <= e else x
        if end_of(bounds, T, n, N_) == e:
            n = e
            fb += 1
        s = n
    return out, bounds, T, fb


def check_rule_properties(lists=200000):
    rng = random.Random(1)
    fbs, worst = 0, 0.0
    for _ in range(lists):
        k = rng.randint(0, 30)
        counts = [rng.choice([1, 1, 1, 2, 3, rng.randint(1, 25)]) for _ in range(k)]
        N_ = rng.randint(1, 12)
        O_ = rng.randint(0, N_ - 1)
        ch, b, T, fb = rule(counts, N_, O_)
        fbs += fb
        if O_ == 0:
            assert [s for s, _ in ch] == rule0(b, T, N_)
        assert (not ch) == (T == 0)
        if ch:
            assert ch[0][0] == 0 and ch[-1][1] == T
            for s, e in ch:
                assert 1 <= e - s <= N_
            for (s, e), (s2, e2) in zip(ch, ch[1:]):
                assert s < s2 <= e < e2 and e - s2 <= O_
                assert s2 in b or (e not in b and s2 == e - O_), (counts, N_, O_, ch)
            for (s, e), (s3, e3) in zip(ch, ch[2:]):
                assert e3 - e > N_ - O_
            assert len(ch) <= 2 * T // (N_ - O_) + 1
            worst = max(worst, len(ch) / (2 * T / (N_ - O_) + 1))
    assert lists < 200000 or (fbs, worst) == (209911, 0.8709677419354839)
    return fbs, worst


# ---- model (a): the caller's loop over the two trim functions ----

def model_a(ctx, doc, allowed, N_, O_, items):
    """([(s, e, text or None)], left_out) for the document `doc` (bytes); items: the document's (byte start, length, tokens) -- used only to tell whether a
    chunk's text alone splits as it does inside the document, and to go on behind a chunk where it does not"""
    text, al = doc.decode("utf-8"), list(allowed)
    bounds = [0]
    for _, _, t in items:
        bounds.append(bounds[-1] + t)
    at = {b: len(doc[:a].decode("utf-8")) for b, (a, _, _) in zip(bounds, items)}      # token boundary -> str index
    at[bounds[-1]] = len(text)
    T = bounds[-1]
    suffix = lambda t, n: ctx.trim.encode_trim_suffix(t, al, n)
    left = [0]

    def step(sb, p, e, part, lo):
        """the start behind a chunk that ends at e and whose items from the boundary sb (str index p) on are the text `part`; lo: the earliest start"""
        if not part:
            return e, p
        alone = [0]
        for _, _, t in CK.items_of(ctx, part.encode("utf-8"), al):
            alone.append(alone[-1] + t)
        if alone != [b - sb for b in bounds if sb <= b <= e]:                        # (a) does not apply: go on from the rule's start
            left[0] += 1
            x = max(e - O_, lo)
            n = bounds[bisect.bisect_left(bounds, x)]
            if end_of(bounds, T, n, N_) == e:
                n = e
            return n, at[n]
        kept, ktext = ctx.trim.encode_trim_prefix(part, al, O_) if O_ else ([], "")
        n, pn = e - len(kept), p + len(part) - len(ktext)
        if n < lo:                                                                    # the whole chunk kept: its first item is dropped
            first, k = [], 0
            while not first:
                k += 1
                first, ftext = suffix(part, k)
            n, pn = sb + len(first), p + len(ftext)
        if n < e and n + len(suffix(text[pn:], N_)[0]) == e:                          # a chunk begun there would end at e again
            n, pn = e, p + len(part)
        return n, pn

    out, s, p = [], 0, 0
    while p < len(text):
        rest = text[p:]
        ids, part = suffix(rest, N_)
        if ids:
            e = s + len(ids)
            out.append((s, e, part))
            if len(part) == len(rest):
                break
            s, p = step(s, p, e, part, s + 1)
            continue
        up = N_
        while not ids:                                                                # the item at p alone holds more than N_ tokens
            up += 1
            ids, ipart = suffix(rest, up)
        assert len(ids) == up
        iend, pend, cur = s + up, p + len(ipart), s
        while iend - cur > N_:                                                        # runs of N_ tokens, each starting O_ behind the end of the one before
            out.append((cur, cur + N_, None))
            cur = max(cur + N_ - O_, cur + 1)
        after, room = text[pend:], N_ - (iend - cur)
        more, mpart = suffix(after, room) if after and room > 0 else ([], "")          # the partial run goes on taking the items that follow
        e = iend + len(more)
        out.append((cur, e, None))
        if len(mpart) == len(after):
            break
        s, p = step(iend, pend, e, mpart, cur + 1)
    return out, left[0]


# ---- expected values and the transport ----

class Expected:
    """what the entry must return for `docs` (bytes) at (N_, O_), by model (b); with small=True model (a) runs as well and must agree"""

    def __init__(self, ctx, docs, N_, O_, allowed=(), small=True, ids_per_doc=None):
        self.ids, self.offs, tb, tu = ctx.expected_spans(docs, allowed, ids_per_doc)
        self.items = [CK.items_of(ctx, d, allowed) for d in docs]
        self.dco, self.ct, self.ce, self.cb, self.cu, self.ceb, self.ceu = [0], [], [], [], [], [], []
        self.chunks, self.bounds, self.fb, self.left_out = [], [], 0, 0
        for d, doc in enumerate(docs):
            lo, hi = self.offs[d], self.offs[d + 1]
            ch, bounds, T, fb = rule([t for _, _, t in self.items[d]], N_, O_)
            assert T == hi - lo, "model (b)'s items do not hold the oracle's tokens"
            self.chunks.append(ch)
            self.bounds.append(bounds)
            self.fb += fb
            n_units = int(CK.units_begun(doc)[-1])
            for s, e in ch:
                self.ct.append(lo + s)
                self.ce.append(lo + e)
                self.cb.append(tb[lo + s])
                self.cu.append(tu[lo + s])
                self.ceb.append(tb[lo + e] if e < T else len(doc))
                self.ceu.append(tu[lo + e] if e < T else n_units)
            self.dco.append(len(self.ct))
            if small and ids_per_doc is None:
                a, left = model_a(ctx, doc, allowed, N_, O_, self.items[d])
                self.left_out += left
                assert [(s, e) for s, e, _ in a] == ch, ("models (a) and (b) disagree", d, N_, O_)
                u16 = doc.decode("utf-8").encode("utf-16-le")
                for c, (_, _, part) in enumerate(a):
                    c0 = self.dco[d] + c
                    assert part is None or part == u16[2 * self.cu[c0]:2 * self.ceu[c0]].decode("utf-16-le"), ("model (a)'s text", d, c)

    def shared(self, d):
        """the tokens every chunk of document d shares with the next"""
        return [e - s2 for (_, e), (s2, _) in zip(self.chunks[d], self.chunks[d][1:])]

    def inside(self, d):
        """(starts, ends) of document d that lie inside an item"""
        b = set(self.bounds[d])
        return [s for s, _ in self.chunks[d] if s not in b], [e for _, e in self.chunks[d] if e not in b]


NAMES = ("offs", "ids", "dco", "ct", "ce", "cb", "cu", "ceb", "ceu")


def chunks_device(ctx, b, N_, O_, index=(), want=ALL, cap=None, ccap=None):
    cap = b["total"] if cap is None else cap
    ccap = N.Encoder.chunk_bound_overlap(b["n"], b["total"], N_, O_) if ccap is None else ccap
    up = ctx.upload
    ids, out, dco = up(np.full(max(1, cap), -7, np.int32)), up(np.full(b["n"] + 1, -5, np.int64)), up(np.full(b["n"] + 1, -5, np.int64))
    ct, ce = up(np.full(max(1, ccap), -7, np.int64)), up(np.full(max(1, ccap), -7, np.int64))
    pos = [up(np.full(max(1, ccap), -7, np.int64)) if w else (None, 0) for w in want]
    tot, nch = ctx.enc.encode_batch_chunks_overlap_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], N_, O_, list(index), ids[1], cap, out[1], dco[1], ct[1],
                                                          ce[1], pos[0][1], pos[1][1], pos[2][1], pos[3][1], ccap)
    offs, dcos = ctx.back(out[0]).tolist(), ctx.back(dco[0]).tolist()
    assert tot == offs[-1] and nch == dcos[-1]
    got = dict(ids=ctx.back(ids[0])[:tot].tolist(), offs=offs, dco=dcos, ct=ctx.back(ct[0])[:nch].tolist(), ce=ctx.back(ce[0])[:nch].tolist())
    for name, w, a in zip(("cb", "cu", "ceb", "ceu"), want, pos):
        got[name] = ctx.back(a[0])[:nch].tolist() if w else None
    for a in [ct, ce] + [a for a, w in zip(pos, want) if w]:                           # nothing is written behind the last chunk
        assert (ctx.back(a[0])[nch:] == -7).all()
    return got


def assert_table(what, got, exp, N_, O_):
    for name in NAMES:
        if got.get(name) is not None:
            CK.SP._same(what, name, [int(x) for x in got[name]], getattr(exp, name))
    assert all(1 <= e - s <= N_ for s, e in zip(got["ct"], got["ce"])), what


def check_device(ctx, docs, N_, O_, what, allowed=(), forms=(ALL,), small=True):
    exp = Expected(ctx, docs, N_, O_, allowed, small)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = ctx.device_buffers(docs)
    for want in forms:
        assert_table("%s, (%d, %d) %s" % (what, N_, O_, want), chunks_device(ctx, b, N_, O_, index, want), exp, N_, O_)
    assert exp.dco[-1] <= N.Encoder.chunk_bound_overlap(len(docs), b["total"], N_, O_)
    return exp


# ---- 1. sizes ----

SIZES = ((1, 0), (2, 1), (7, 1), (7, 3), (7, 6))


def check_sizes(ctx):
    rng = random.Random(5)
    for N_, O_ in SIZES:
        docs = [b"", words(rng, N_), words(rng, N_ + 1), b"", words(rng, 3 * N_), words(rng, 3 * N_ + 1), b"x", b""]
        exp = check_device(ctx, docs, N_, O_, "sizes", forms=(ALL, (False, False, False, False)))
        assert exp.chunks[0] == [] and exp.chunks[1] == [(0, N_)] and exp.chunks[2][0] == (0, N_) and exp.chunks[2][-1][1] == N_ + 1 and exp.left_out == 0
        assert exp.dco[3] == exp.dco[4] and len(exp.chunks[5]) >= 3 and all(x <= O_ for d in range(len(docs)) for x in exp.shared(d))
        if O_ == 0:                                                                   # exactly the chunks of the existing entry
            b = ctx.device_buffers(docs)
            old, new = ctx.chunks_device(b, N_), chunks_device(ctx, b, N_, 0)
            assert new["ct"] == old["ct"][:-1] and new["cb"] == old["cb"] and new["cu"] == old["cu"] and new["dco"] == old["dco"]
            for d in range(len(docs)):
                c0, c1 = new["dco"][d], new["dco"][d + 1]
                assert c0 == c1 or (new["ce"][c0:c1 - 1] == new["ct"][c0 + 1:c1] and new["ce"][c1 - 1] == new["offs"][d + 1])
    gib = b"it's zqxjkvbwpm and wvkqzzj the\n\nqqxz"
    for N_, O_ in ((2, 1), (3, 2)):
        exp = check_device(ctx, [gib, b"a", gib[:9]], N_, O_, "small budgets")
        assert exp.inside(0)[0]
    # no documents; no bytes
    enc = ctx.enc
    for n in (0, 3):
        b0 = ctx.device_buffers([b""] * n)
        got = chunks_device(ctx, b0, 4, 1, cap=0, ccap=0)
        assert [got[k] for k in NAMES] == [[0] * (n + 1), [], [0] * (n + 1), [], [], [], [], [], []]
        r = enc.encode_batch_chunks_overlap(np.zeros(0, np.uint8), np.zeros(n + 1, np.int64), 4, 1)
        assert [len(x) for x in r] == [0, n + 1, n + 1, 0, 0, 0, 0, 0, 0] and not r[1].any() and not r[2].any()
    r = enc.encode_batch_chunks_overlap_utf16(np.zeros(0, np.uint16), np.zeros(3, np.int64), 4, 1)
    assert r[1].tolist() == [0, 0, 0] and r[2].tolist() == [0, 0, 0] and [len(x) for x in r[3:]] == [0, 0, 0, 0]
    assert enc.encode_chunks_overlap(b"", 4, 1) == ([], [], [], [], [], [], []) and enc.encode_chunks_overlap_utf16([], 4, 1) == ([], [], [], [], [])


# ---- 2. the clamp and the adds-nothing rule ----

def check_fallback(ctx):
    rng = random.Random(7)
    exp = check_device(ctx, [words(rng, 2) + ctx.piece_of_tokens(5)], 6, 5, "items 1, 1, 5")
    assert [t for _, _, t in exp.items[0]] == [1, 1, 5] and exp.fb == 0 and exp.chunks[0] == [(0, 2), (1, 7)] and exp.left_out == 0      # (the clamp: x = s + 1)
    for N_, O_ in ((7, 3), (6, 5)):
        for k in range(N_ - O_ + 1, N_ + 1):
            exp = check_device(ctx, [words(rng, N_) + ctx.piece_of_tokens(k) + words(rng, N_)], N_, O_, "an item of %d tokens" % k)
            assert exp.fb >= 1 and min(exp.shared(0)) < O_ and exp.left_out == 0, (N_, O_, k)
    exp = check_device(ctx, [words(rng, 9)], 4, 3, "the clamp")                      # (x = s + 1 where e - O would not move on)
    assert exp.chunks[0][:2] == [(0, 4), (1, 5)]


# ---- 3. oversize items ----

def check_oversize(ctx):
    rng = random.Random(11)
    for N_ in (3, 4):
        for O_ in (1, N_ - 1):
            for n in (N_ + 1, 2 * N_, 2 * N_ + 1):
                big = ctx.piece_of_tokens(n)
                half = words(rng, N_ // 2 + 1)
                docs = [big + words(rng, 2 * N_), words(rng, 2 * N_) + big, half + big + words(rng, N_), big + big + big]
                exp = check_device(ctx, docs, N_, O_, "oversize item of %d tokens" % n, forms=(ALL, (False, True, False, True), (True, False, False, False)))
                assert exp.left_out == 0
                for d in range(len(docs)):
                    starts, ends = exp.inside(d)
                    assert starts and ends, (N_, O_, n, d)
                    # starts inside an item lie behind the end before them: the two sequences interleave
                    assert any(s2 < e for (_, e), (s2, _) in zip(exp.chunks[d], exp.chunks[d][1:]) if s2 in starts and e in ends), (N_, O_, n, d)


# ---- 4. special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot, "<|other|>": eot + 1})
    rng = random.Random(17)
    w = lambda n: words(rng, n).decode()
    # chunk 0 of documents 0..2 at (4, 2) is [0, 4): the literal is token 2 = e - O, token 1 = s + 1 (at (4, 3)), token 4 = e
    docs = [w(2) + EOT + w(9), w(1) + EOT + w(9), w(4) + EOT + w(9), w(3) + EOT + EOT + w(3), EOT, w(2) + "<|other|>" + w(2) + EOT, "", EOT + w(8)]
    bdocs = [d.encode() for d in docs]
    for N_, O_ in ((4, 2), (4, 3), (2, 1)):
        s0 = ctx.enc.special_stats()
        on = check_device(ctx, bdocs, N_, O_, "special: allowed", allowed=[EOT])
        s1 = ctx.enc.special_stats()
        assert s1[0] - s0[0] == 1 and s1[1] - s0[1] == on.ids.count(eot) == 8
        off = check_device(ctx, bdocs, N_, O_, "special: n_allowed == 0", allowed=[])
        assert ctx.enc.special_stats() == s1 and eot not in off.ids and len(off.ids) > len(on.ids) and eot + 1 not in on.ids
        if (N_, O_) == (4, 2):
            assert on.ids[on.ct[on.dco[0] + 1]] == eot and on.ids[on.ce[on.dco[2]]] == eot
        if (N_, O_) == (4, 3):
            assert on.ids[on.ct[on.dco[1] + 1]] == eot and on.ct[on.dco[1] + 1] == on.ct[on.dco[1]] + 1


# ---- 5. units and ends ----

def check_units(ctx):
    every = b"a\nb\nc\nd\n" * 300
    for N_, O_ in ((1, 0), (2, 1)):
        exp = check_device(ctx, [b"xy", every[:1120]], N_, O_, "units: an end at every byte", forms=(ALL, (False, False, False, True), (False, True, False, True)))
        assert {SUB - 1, SUB, SUB + 1} <= {2 + x for x in exp.ceb[exp.dco[1]:exp.dco[2]]}
    # the last document's end is `total`: a multiple of 1024, of 128 only, and an empty document behind it
    for docs in ([b"xy", every[:2 * SUB - 2]], [every[:384]], [every[:384], b""], [b"xy", every[:SUB - 2], b"", b""]):
        total = sum(len(d) for d in docs)
        assert total % 128 == 0
        exp = check_device(ctx, docs, 3, 1, "units: the last end is the batch's", forms=(ALL, (False, False, False, True)))
        assert exp.ceb[-1] == len([d for d in docs if d][-1]) and exp.ceu[-1] == exp.ceb[-1]
    # every combination of the optional arrays
    for k in range(16):
        want = tuple(bool(k >> j & 1) for j in range(4))
        check_device(ctx, [every[:300], "café 漢字 ".encode() * 9, b""], 5, 2, "units: optional arrays", forms=(want,), small=False)
    # a 4-byte character across the sub-tile edge in front of an end
    doc = b"a\n" * 511 + EMOJI.encode() + b"a\nb\n" * 8
    for N_, O_ in ((1, 0), (3, 2)):
        exp = check_device(ctx, [doc], N_, O_, "units: a character across the sub-tile edge", forms=(ALL, (False, True, False, True)))
        k = min(i for i, x in enumerate(exp.ceb) if x >= SUB + 2)                    # the first end behind the character: 4 bytes, 2 units
        assert exp.ceu[k] == exp.ceb[k] - 2 and exp.ceb[k] <= SUB + 4 and (N_ > 1 or exp.ceb[k] == SUB + 2)
    texts = [EMOJI, "a" + EMOJI + "b", "café naïve 漢字 " + EMOJI * 3 + " \U0001F44D\U0001F3FD end", "", "漢字かな交じり文、한국어 " * 30]
    for N_, O_ in ((1, 0), (3, 1), (5, 4)):
        check_device(ctx, [t.encode("utf-8") for t in texts], N_, O_, "units", forms=(ALL, (False, True, False, True)))
    # the UTF-16 entry: a lone surrogate, a pair cut by a document boundary
    docs = [U16S.units("cut " + EMOJI)[:-1], U16S.units(EMOJI)[1:] + U16S.units(" here"), U16S.units("lone ") + [0xD800] + U16S.units(" high it's zqxjk"), [],
            U16S.units(EMOJI + " end")]
    flat, uoffs = U16S.pack(docs)
    bdocs = [U16.get_bytes(d) for d in docs]
    for N_, O_ in ((1, 0), (2, 1), (4, 2)):
        want = Expected(ctx, bdocs, N_, O_, small=False)
        ids, ooff, dco, ct, ce, cu, ceu = ctx.enc.encode_batch_chunks_overlap_utf16(flat, uoffs, N_, O_)
        got = dict(ids=ids.tolist(), offs=ooff.tolist(), dco=dco.tolist(), ct=ct.tolist(), ce=ce.tolist(), cu=cu.tolist(), ceu=ceu.tolist())
        assert_table("units: utf16", got, want, N_, O_)
        for d, doc in enumerate(docs):                                                # a document's last chunk ends at its length in units
            c0, c1, lo = want.dco[d], want.dco[d + 1], want.offs[d]
            assert c1 == c0 or int(ceu[c1 - 1]) == len(doc)
            one = ctx.enc.encode_chunks_overlap_utf16(doc, N_, O_)
            assert one == (want.ids[lo:want.offs[d + 1]], [x - lo for x in want.ct[c0:c1]], [x - lo for x in want.ce[c0:c1]], want.cu[c0:c1], want.ceu[c0:c1])


# ---- 6. search widths and the long form ----

def check_widths(ctx):
    rng = random.Random(23)
    short, long = words(rng, 900), words(rng, 1500)
    for N_ in (63, 64, 65, 200):
        for O_ in sorted({o for o in (1, 63, 64, N_ - 1) if o < N_}):
            exp = check_device(ctx, [short, long], N_, O_, "widths", small=False)
            assert len(exp.items[0]) == 900 <= LONG < len(exp.items[1]) == 1500
            assert exp.chunks[0][:2] == [(0, N_), (N_ - O_, 2 * N_ - O_)] and exp.chunks[1][:2] == exp.chunks[0][:2]
    check_device(ctx, [short[:3000]], 64, 8, "widths: models", small=True)


def check_long_form(ctx):
    rng = random.Random(31)
    gib = ctx.piece_of_tokens(9)
    for N_, O_ in ((4, 1), (50, 7), (50, 49)):
        docs = [words(rng, LONG), words(rng, LONG + 1), words(rng, 40), words(rng, LONG - 1) + gib, words(rng, 700) + gib + words(rng, 700),
                words(rng, 2 * LONG + 70), gib + words(rng, LONG + 5), words(rng, LONG - 1)]
        exp = check_device(ctx, docs, N_, O_, "long documents", forms=(ALL, (False, False, False, False)), small=False)
        assert [len(i) for i in exp.items] == [LONG, LONG + 1, 40, LONG, 1401, 2 * LONG + 70, LONG + 6, LONG - 1]
        assert (N_ > 9) == (not exp.inside(4)[0]) and (N_ > 9) == (not exp.inside(3)[1]) and (exp.fb > 0 or O_ != 49)
    check_device(ctx, [words(rng, LONG + 1)[:2500]], 4, 2, "long documents: models", small=True)


# ---- 7. workgroup edges, 8. the piece-granular path's stride ----

def check_workgroup_edges(ctx):
    rng = random.Random(29)
    for n in (255, 256, 257):
        docs = [words(rng, rng.choice([0, 1, 3, 4, 5, 9])) for _ in range(n)]
        docs[-1] = words(rng, 9)
        exp = check_device(ctx, docs, 4, 2, "%d documents" % n, small=False)
        assert exp.chunks[n - 1] == [(0, 4), (2, 6), (4, 8), (6, 9)] and exp.dco[-1] > n


def check_stride(ctx, total=300 << 10):
    rng = random.Random(37)
    doc = fill(rng, total)
    exp = check_device(ctx, [doc], 8, 3, "one document of 300 KiB", small=False)
    assert len(doc) > 256 << 10 and exp.dco[-1] > 3000 and len(exp.items[0]) > LONG


# ---- 9. capacity, argument errors ----

def check_errors(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, L = ctx.enc, ctx.enc.lib.L
    docs = [b"hello world it's a fine day", b"", b"zqxjk " + EOT.encode() + b" and more words here"]
    N_, O_ = 3, 1
    exp = Expected(ctx, docs, N_, O_, [EOT])
    b = ctx.device_buffers(docs)
    need, nch = len(exp.ids), exp.dco[-1]
    assert nch >= 6
    c0, k0 = enc.chunks_overlap_calls(), enc.chunks_calls()
    for cap, ccap in ((need - 1, nch), (need, nch - 1), (need - 1, nch - 1), (0, 0)):
        with pytest.raises(N.TkzError) as ei:
            chunks_device(ctx, b, N_, O_, [0], cap=cap, ccap=ccap)
        assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_chunks) == (need, nch), (cap, ccap)
    data, offs = parity.pack(docs)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_chunks_overlap(data, offs, N_, O_, [0], chunk_cap=nch - 1)
    assert ei.value.code == N.E_CAPACITY and (ei.value.needed, ei.value.needed_chunks) == (need, nch)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_chunks_overlap(docs[0], N_, O_, chunk_cap=exp.dco[1] - 1)
    assert ei.value.code == N.E_CAPACITY and ei.value.needed_chunks == exp.dco[1]
    assert enc.chunks_overlap_calls() == c0                                          # failed calls are not counted
    assert_table("exact capacity", chunks_device(ctx, b, N_, O_, [0], cap=need, ccap=nch), exp, N_, O_)
    assert enc.chunks_overlap_calls() == c0 + 1 and enc.chunks_calls() == k0
    # overlap of -1, N and N + 1; max_tokens < 1: in all five entries
    u2, o2 = np.asarray([65, 66], np.uint16), np.asarray([0, 2], np.int64)
    for mx, ov in ((N_, -1), (N_, N_), (N_, N_ + 1), (0, 0), (-1, 0), (-(1 << 40), 0), (1, 1)):
        for call in (lambda: chunks_device(ctx, b, mx, ov, [0]), lambda: enc.encode_batch_chunks_overlap(data, offs, mx, ov), lambda: enc.encode_chunks_overlap(docs[0], mx, ov),
                     lambda: enc.encode_chunks_overlap_utf16([65, 66], mx, ov), lambda: enc.encode_batch_chunks_overlap_utf16(u2, o2, mx, ov)):
            with pytest.raises(N.TkzError) as ei:
                call()
            assert ei.value.code == N.E_ARG, (mx, ov)
    for index in ([1], [0, 0], [-1]):
        with pytest.raises(N.TkzError) as ei:
            chunks_device(ctx, b, N_, O_, index)
        assert ei.value.code == N.E_ARG
    # null buffers
    ids, ooff, dco, ct, ce, n, c = np.zeros(64, np.int32), np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(64, np.int64), np.zeros(64, np.int64), C.c_int64(-1), C.c_int64(-1)
    p = lambda a: a.ctypes.data
    ok = (enc._h, p(data), p(offs), 3, None, 0, N_, O_, p(ids), 64, p(ooff), p(dco), p(ct), p(ce), None, None, None, None, 64, C.byref(n), C.byref(c))
    plain = Expected(ctx, docs, N_, O_, [])
    assert L.tkz_encode_batch_chunks_overlap_utf8(*ok) == N.OK and c.value == plain.dco[-1] and ce[:c.value].tolist() == plain.ce
    for k in (0, 2, 10, 11, 12, 13):                                                 # the encoder, the offsets, out_offsets, doc_chunk_offsets, chunk_tokens, chunk_ends
        assert L.tkz_encode_batch_chunks_overlap_utf8(*(ok[:k] + (None,) + ok[k + 1:])) == N.E_ARG, k
    assert L.tkz_encode_batch_chunks_overlap_utf8(*(ok[:18] + (-1,) + ok[19:])) == N.E_ARG
    one = (enc._h, p(data), 5, None, 0, N_, O_, p(ids), 64, p(ct), p(ce), None, None, None, None, 64, C.byref(n), C.byref(c))
    assert L.tkz_encode_chunks_overlap_utf8(*one) == N.OK
    for k, v in ((16, None), (17, None), (2, -1), (10, None)):
        assert L.tkz_encode_chunks_overlap_utf8(*(one[:k] + (v,) + one[k + 1:])) == N.E_ARG, k
    assert L.tkz_encode_chunks_overlap_utf16(enc._h, p(data), 2, None, 0, N_, O_, p(ids), 64, p(ct), None, None, None, 64, C.byref(n), C.byref(c)) == N.E_ARG
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_chunks_overlap_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], N_, O_, [], 0, 64, 0, 0, 0, 0, 0, 0, 0, 0, 64)
    assert ei.value.code == N.E_ARG
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        chunks_device(ctx, ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]), N_, O_)
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_chunks_overlap(data, np.asarray([0, 12, 11, len(data)], np.int64), N_, O_)
    assert ei.value.code == N.E_ARG
    assert enc.chunks_overlap_calls() == c0 + 3
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_chunks_overlap(b"a<|s7|>b", N_, O_, [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_chunks_overlap(b"a<|s7|>b", N_, O_)[0] == many.oenc.encode_bytes(b"a<|s7|>b")


# ---- 10. agreement of the entries ----

def check_agreement(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc = ctx.enc
    rng, gib, mixed, crowded = CK.CC.generators(7)
    w = lambda n: fill(rng, n).decode()
    texts = [w(300) + EOT + w(40), gib(600, 2, 9), "", w(2 * SUB + 9), "café " + EMOJI + " 漢字 " + w(20), mixed(1500, 3, 3, 30), EOT, w(5)]
    docs = [t.encode("utf-8") for t in texts]
    data, offs = parity.pack(docs)
    flat, uoffs = U16S.pack([U16S.units(t) for t in texts])
    b = ctx.device_buffers(docs)
    for index in ([0], []):
        for N_, O_ in ((1, 0), (5, 2), (64, 8)):
            dev = chunks_device(ctx, b, N_, O_, index)
            r = enc.encode_batch_chunks_overlap(data, offs, N_, O_, index)
            host = dict(zip(("ids", "offs", "dco", "ct", "ce", "cb", "cu", "ceb", "ceu"), [x.tolist() for x in r]))
            assert host == dev, (index, N_, O_)
            eids, eoff = enc.encode_batch_special(data, offs, index)
            assert host["ids"] == eids.tolist() and host["offs"] == eoff.tolist()
            r = enc.encode_batch_chunks_overlap_utf16(flat, uoffs, N_, O_, index)
            assert [x.tolist() for x in r] == [dev[k] for k in ("ids", "offs", "dco", "ct", "ce", "cu", "ceu")], (index, N_, O_)
            assert len(dev["ct"]) <= N.Encoder.chunk_bound_overlap(len(docs), len(data), N_, O_)
            for d, doc in enumerate(docs):                                          # the single-text entries
                lo, c0, c1 = dev["offs"][d], dev["dco"][d], dev["dco"][d + 1]
                want = (dev["ids"][lo:dev["offs"][d + 1]], [x - lo for x in dev["ct"][c0:c1]], [x - lo for x in dev["ce"][c0:c1]], dev["cb"][c0:c1], dev["cu"][c0:c1],
                        dev["ceb"][c0:c1], dev["ceu"][c0:c1])
                assert enc.encode_chunks_overlap(doc, N_, O_, index) == want, (index, N_, O_, d)
                assert enc.encode_chunks_overlap_utf16(U16S.units(texts[d]), N_, O_, index) == (want[0], want[1], want[2], want[4], want[6]), (index, N_, O_, d)


# ---- 11. the Python mirror ----

def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    ctx = CK.Ctx(lib, O, raw_gpt2, N.P1, specials)
    odd = "Hi " + EMOJI + "\U0001F44D\U0001F3FD café " + EOT + " 漢字 zqxjkvbwpmzq end"

    def compare(t, text, allowed, N_, O_, model=None):
        m = model or ctx
        doc = text.encode("utf-8")
        exp = Expected(m, [doc], N_, O_, allowed, small=True)                       # (model (a) runs inside, against (b))
        got = t.EncodeChunksOverlap(text, allowed, N_, O_)
        u16 = text.encode("utf-16-le")
        assert [i for i, _ in got] == [exp.ids[s:e] for s, e in zip(exp.ct, exp.ce)], (N_, O_, allowed)
        assert [p for _, p in got] == [u16[2 * a:2 * z].decode("utf-16-le", "replace") for a, z in zip(exp.cu, exp.ceu)]
        return got, exp
    total = left = 0
    for text, allowed, N_, O_ in ((lib_rs_text, [EOT], 64, 8), (odd, [EOT], 3, 1), (odd, [EOT], 2, 1), (odd, [], 3, 1), (EOT, [EOT], 5, 2)):
        got, exp = compare(tok, text, allowed, N_, O_)
        total, left = total + len(got), left + exp.left_out
        assert len(got) >= (3 if len(text) > 20 else 1) and got[0][1] == text[:len(got[0][1])] and text.endswith(got[-1][1])
    assert left * 20 <= total, "model (a) leaves out %d of %d chunks" % (left, total)
    assert tok.EncodeChunksOverlap("", 5, 2) == [] and tok.EncodeChunksOverlapBatch([], 5, 2) == []
    assert tok.EncodeChunksOverlap(odd, 3, 1) == tok.EncodeChunksOverlap(odd, [EOT], 3, 1) and tok.EncodeChunksOverlap(odd, 3, 1, False) == tok.EncodeChunksOverlap(odd, [], 3, 1)
    assert [i for i, _ in tok.EncodeChunksOverlap(odd, [EOT], 3, 0)] == [i for i, _ in tok.EncodeChunks(odd, [EOT], 3)]
    batch = [odd, "", lib_rs_text[:3000], EOT + "x"]
    assert tok.EncodeChunksOverlapBatch(batch, [EOT], 6, 2) == [tok.EncodeChunksOverlap(t, [EOT], 6, 2) for t in batch]
    for bad in ((0, 0), (-3, 0), (3, 3), (3, -1), (3, 4)):
        with pytest.raises(ValueError):
            tok.EncodeChunksOverlap(odd, *bad)
    # the host fallback: a set of literals the device's special entries refuse
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TokenizerBuilder.CreateTokenizer(raw_gpt2, many, REGEX_PATTERN_1, lib=lib)
    ctx2 = CK.Ctx(lib, O, raw_gpt2, N.P1, many)
    c0 = tok2._encoder.chunks_overlap_calls()
    text = "alpha<|s7|> zqxjkvbwpmzq beta gamma<|s8|>" + EMOJI + " delta"
    for N_, O_ in ((1, 0), (2, 1), (5, 2), (5, 4)):
        got, _ = compare(tok2, text, ["<|s7|>"], N_, O_, ctx2)
        assert 200007 in [i for g in got for i in g[0]] and 200008 not in [i for g in got for i in g[0]]
    mixed = lib_rs_text[:9000] + "<|s7|>" + lib_rs_text[9000:12000] + "<|s8|>"
    got, _ = compare(tok2, mixed, ["<|s7|>"], 64, 8, ctx2)
    assert len(got) > 50 and tok2._special_on_host and tok2._encoder.chunks_overlap_calls() == c0
