"""Token spans (tkz_encode_batch_spans_device / _utf8 / _utf16, tkz_encode_spans_utf8 / _utf16; k_tokspan_mark, k_tokspan_count, k_tokspan_write): the cases and
comparisons the emulated (CPU) and the GPU test modules share.  Every comparison is exact.

No expected value comes from the code under test:
  ids, offsets   the oracle's (oracle.Encoder; TrimOracle's literal search for UTF-16 text with lone surrogates: u16_special_cases.Expect);
  byte starts    the running sum of len(key(id)) from the rank file (oracle.Vocab.entries()), the literal's length for an allowed special token -- and the slice
                 property bytes[start_t : start_t+1] == key(id_t) is asserted directly;
  unit starts    from the document's bytes by the rule of tkz.h, written out here (units_begun): one per non-continuation byte and one more per byte >= 0xF0 in
                 front of the token's first byte;
  UTF-16 input   transcoded here (u16_cases.get_bytes), lone surrogates to EF BF BD.

The kernel cases go through tkz_encode_batch_spans_device.  `upload(np_array) -> (owner, pointer)` as in count_cases: identity for the emulated build, a device
tensor on the hardware.

Geometry (tkz_kernels.h / .hip): a sub-tile is SUB = 1024 bytes of the batch, a wavefront of k_tokspan_count / _write takes one, a lane 16 bytes of it; the bitmaps are
64-bit words; the piece-granular path strides 256 KiB.
"""
import ctypes as C
import random

import numpy as np
import pytest

import count_cases as CC
import parity
import special_cases as SC
import u16_cases as U16
import u16_special_cases as U16S
from tokenizer_amd import _native as N

SUB = CC.SUB
EOT = SC.EOT
fill, cut = CC.fill, CC.cut
EOT_ID = {"gpt2": 50256, "synth100k": 100257}          # an id outside the table's ranks


def units_begun(data):
    """prefix[p] = UTF-16 units begun in data[0:p]"""
    b = np.frombuffer(bytes(data), np.uint8)
    per = ((b & 0xC0) != 0x80).astype(np.int64) + (b >= 0xF0)
    return np.concatenate([[0], np.cumsum(per)])


class Ctx(CC.Ctx):
    """count_cases.Ctx with the rank file's key of every id."""

    def __init__(self, lib, O, raw, pattern=N.CL100K, specials=None, upload=None, options=()):
        super().__init__(lib, O, raw, pattern, specials, upload, options)
        self.key = {r: k for k, r in self.ovocab.entries()}
        self.lit = {i: s.encode("utf-8") for s, i in (specials or {}).items()}

    def token_text(self, i, allowed_ids):
        return self.lit[i] if i in allowed_ids else self.key[i]

    def expected_spans(self, docs, allowed=(), ids_per_doc=None):
        """docs: bytes.  (ids, offsets, tok_bytes, tok_units); ids_per_doc: the oracle's ids when the caller has them (UTF-16 text with lone surrogates)"""
        allowed_ids = {self.specials[a] for a in allowed} if self.specials else set()
        ids, offs, tb, tu = [], [0], [], []
        for k, d in enumerate(docs):
            if ids_per_doc is not None:
                di = ids_per_doc[k]
            elif self.specials and allowed:
                di = self.oenc.encode(d.decode("utf-8"), list(allowed))
            else:
                di = self.oenc.encode_bytes(d)
            pre = units_begun(d)
            pos = 0
            for i in di:
                t = self.token_text(i, allowed_ids)
                assert d[pos:pos + len(t)] == t, "the oracle's ids do not spell the document"
                tb.append(pos); tu.append(int(pre[pos]))
                pos += len(t)
            assert pos == len(d)
            ids += di
            offs.append(len(ids))
        return ids, offs, tb, tu

    def spans_device(self, b, index=(), want_bytes=True, want_units=True, cap=None):
        cap = b["total"] if cap is None else cap
        ids = self.upload(np.full(max(1, cap), -7, np.int32))
        tb = self.upload(np.full(max(1, cap), -7, np.int32)) if want_bytes else (None, 0)
        tu = self.upload(np.full(max(1, cap), -7, np.int32)) if want_units else (None, 0)
        out = self.upload(np.full(b["n"] + 1, -5, np.int64))
        tot = self.enc.encode_batch_spans_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], list(index), ids[1], cap, out[1], tb[1], tu[1])
        offs = self.back(out[0]).tolist()
        assert tot == offs[-1]
        return (self.back(ids[0])[:tot].tolist(), offs, self.back(tb[0])[:tot].tolist() if want_bytes else None,
                self.back(tu[0])[:tot].tolist() if want_units else None)


def _same(what, name, got, want):
    if got != want:
        k = SC.first_diff(got, want)
        raise AssertionError("%s: %s differ at %d of %d/%d: got %s, expected %s" % (what, name, k, len(got), len(want), got[max(0, k - 3):k + 5], want[max(0, k - 3):k + 5]))


def assert_spans(ctx, what, got, exp, docs, allowed=()):
    for name, g, w in zip(("offsets", "ids", "tok_bytes", "tok_units"), (got[1], got[0], got[2], got[3]), (exp[1], exp[0], exp[2], exp[3])):
        if g is not None:
            _same(what, name, [int(x) for x in g], w)
    # the slice property on what the entry returned, and the last token's implied end in units
    allowed_ids = {ctx.specials[a] for a in allowed} if ctx.specials else set()
    ids, offs, tb, tu = got
    for d, doc in enumerate(docs):
        lo, hi = offs[d], offs[d + 1]
        if tb is not None:
            ends = tb[lo + 1:hi] + [len(doc)]
            for t in range(lo, hi):
                assert doc[tb[t]:ends[t - lo]] == ctx.token_text(ids[t], allowed_ids), (what, d, t)
            assert hi == lo or tb[lo] == 0
        if tu is not None and tb is not None and hi > lo:
            try:
                n_units = len(doc.decode("utf-8").encode("utf-16-le")) // 2
            except UnicodeDecodeError:
                continue
            assert tu[hi - 1] + int(units_begun(doc[tb[hi - 1]:])[-1]) == n_units, (what, d)


def check_device(ctx, docs, what, allowed=(), forms=((True, True),)):
    """tkz_encode_batch_spans_device on `docs` (bytes).  Returns the expected (ids, offsets, tok_bytes, tok_units)."""
    exp = ctx.expected_spans(docs, allowed)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = ctx.device_buffers(docs)
    for wb, wu in forms:
        assert_spans(ctx, "%s (bytes %d, units %d)" % (what, wb, wu), ctx.spans_device(b, index, wb, wu), exp, docs, allowed)
    return exp


def global_starts(exp, docs):
    base = np.cumsum([0] + [len(d) for d in docs])
    offs = exp[1]
    return {int(base[d]) + exp[2][t] for d in range(len(docs)) for t in range(offs[d], offs[d + 1])}


def pieces_of(ctx, doc):
    """(start, length, tokens) of every regex piece of a plain document"""
    out = []
    for a, n in ctx.O.split_utf8(ctx.pattern, doc):
        p = doc[a:a + n]
        out.append((a, n, 1 if ctx.ovocab.rank(p) >= 0 else len(ctx.ovocab.bpe(p))))
    return out


# ---- 1. placement at edges ----

def check_edges(ctx):
    rng = random.Random(3)
    every = b"a\nb\nc\nd\n" * 140                                            # a token at every byte: starts at 63, 64, 1023 and 1024 of the batch
    exp = check_device(ctx, [every], "edges: a token at every byte", forms=((True, True), (True, False), (False, True)))
    assert {63, 64, 1023, 1024} <= global_starts(exp, [every])
    # a piece of several tokens across the sub-tile edge at 1024, and one across the word edge at 64
    gib = b" zqxjkvbwpmzqxj"
    for edge in (SUB, 64):
        doc = fill(rng, edge - 6)[:edge - 6] + gib + b" " + fill(rng, 300)
        hit = [p for p in pieces_of(ctx, doc) if p[0] < edge < p[0] + p[1]]
        assert hit and hit[0][2] > 1, hit
        exp = check_device(ctx, [doc], "edges: a piece of several tokens across byte %d" % edge)
        assert any(hit[0][0] < s < hit[0][0] + hit[0][1] for s in exp[2])      # an interior token start
    # two documents that start in one sub-tile; empty documents in front, at the back and three in a row; a document start on a sub-tile's first and last byte
    a, b = fill(rng, 2 * SUB), fill(rng, SUB + SUB - 1)
    docs = [b"", b"", fill(rng, 100), fill(rng, 200), b"", b"", b"", a, b, fill(rng, 3 * SUB + 5), fill(rng, 7), b"", b""]
    check_device(ctx, docs, "edges: documents", forms=((True, True), (False, True)))
    check_device(ctx, [fill(rng, 5 * SUB + 17)], "edges: one document over several sub-tiles")
    check_device(ctx, [b"x"], "edges: one byte")
    check_device(ctx, [rng.choice(CC.TINY) for _ in range(2000)], "edges: tiny documents")
    # no documents; no bytes
    for n in (0, 3):
        b0 = ctx.device_buffers([b""] * n)
        assert ctx.spans_device(b0, cap=0) == ([], [0] * (n + 1), [], [])
        ids, ooff, tb, tu = ctx.enc.encode_batch_spans(np.zeros(0, np.uint8), np.zeros(n + 1, np.int64))
        assert (len(ids), ooff.tolist(), len(tb), len(tu)) == (0, [0] * (n + 1), 0, 0)
    assert ctx.enc.encode_batch_spans_utf16(np.zeros(0, np.uint16), np.zeros(3, np.int64))[1].tolist() == [0, 0, 0]
    assert ctx.enc.encode_spans(b"") == ([], [], []) and ctx.enc.encode_spans_utf16([]) == ([], [])


# ---- 2. every source of a piece of several tokens ----

def check_sources(make_ctx, seed=41):
    ctx = make_ctx()
    rng, gib, mixed, crowded = CC.generators(seed)
    tail = lambda: b" " + fill(rng, 40)
    cons = lambda n: "".join(rng.choice(CC.CONS) for _ in range(n)).encode()
    batches = {
        "short misses": cut(gib(4000, 2, 2).encode(), [1030, 2000]) + [tail()],                        # ~340 list entries a sub-tile
        "short and long misses": cut(mixed(5000, 3, 3, 30).encode(), [2100, 900]) + [tail()],
        "more than 64 list entries": cut(crowded(6000, 2).encode(), [1500, 1500, 1500]) + [tail()],
        "long misses of 17..128 bytes": [fill(rng, 300) + b" " + cons(17) + b" " + cons(60) + b" " + cons(128) + tail()],
        "long misses of 129..1024 bytes": [fill(rng, 900) + b" " + cons(129) + b" " + cons(600) + b" x " + cons(1024) + tail(), fill(rng, 50)],
        "giant pieces": [gib(700, 2, 3).encode() + b"x" * 1500, fill(rng, 300), fill(rng, 500) + b" " + cons(3000), b"=" * 1100 + b" tail"],
    }
    for name, docs in batches.items():
        first = check_device(ctx, docs, "sources: " + name)
        assert len(first[0]) > sum(len(pieces_of(ctx, d)) for d in docs), name            # (pieces of several tokens)
        check_device(ctx, docs, "sources: %s, the memo's second call" % name)


def check_promoted(ctx, seed=61):
    """count_cases.check_promoted's text and option sequence"""
    r1 = random.Random(seed + 1)
    lex = ["".join(r1.choice(CC.CONS) + r1.choice("aeiou") for _ in range(r1.randint(2, 6))) + r1.choice(["", "s", "ed", "ing"]) for _ in range(150)]

    def words(n, r):
        out = []
        while sum(map(len, out)) < n:
            out.append(r.choice([" ", " ", "\n", " the ", ", ", " 12 "]) + r.choice(lex))
        return "".join(out).encode()
    docs = [words(n, random.Random(seed + 10 + i)) for i, n in enumerate([400, 3000, 9000, 3000, 500, 40])]
    enc = ctx.enc
    enc.set_option(N.OPT_PROMOTE, 0)
    check_device(ctx, docs, "promotion: before")
    check_device(ctx, docs, "promotion: memo filled")
    enc.set_option(N.OPT_PIECE_STATS, 1)
    enc.set_option(N.OPT_PROMOTE, 2)
    enc.piece_stats(reset=True)
    check_device(ctx, docs, "promotion: promoted")
    assert enc.piece_stats(reset=True)["promoted_pieces_in_tables"] > 20
    enc.set_option(N.OPT_PROMOTE, 3)
    check_device(ctx, docs, "promotion: dropped")
    enc.set_option(N.OPT_PIECE_STATS, 0)


# ---- 3. the key-length lookup ----

def check_sparse_table(lib, O, upload=None):
    """the decode table's sorted, binary-searched form (ranks up to ~2^26)"""
    ctx = Ctx(lib, O, U16.sparse_vocab_bytes(), upload=upload)
    rng = random.Random(9)
    docs = ["".join(rng.choice("abc") for _ in range(n)).encode() for n in (5, 40, 700, 1500, 0, 3)]
    exp = check_device(ctx, docs, "sparse decode table")
    assert max(exp[0]) >= 1 << 22 and len(exp[0]) > len(docs)


def check_key_lengths(ctx):
    """keys of 1 byte and of max_key_len inside pieces of several tokens"""
    rng = random.Random(13)
    top = ctx.ovocab.max_key_len
    for longest in sorted(k for k in ctx.key.values() if len(k) == top):
        last = longest.decode("utf-8")[-1].encode("utf-8")                     # (the longest keys of the three tables are whole characters)
        docs = [fill(rng, 200) + b" zq" + longest + last * 3 + b"j " + fill(rng, 100), longest + longest + last, b"zq" + longest + b"j"]
        ids = [i for d in docs for i in ctx.oenc.encode_bytes(d)]
        if top in {len(ctx.key[i]) for i in ids}:                            # (the merges of this text reach the longest key)
            break
    exp = check_device(ctx, docs, "key lengths")
    lens = {len(ctx.key[i]) for i in exp[0]}
    assert 1 in lens and top in lens, sorted(lens)
    assert len(exp[0]) > sum(len(pieces_of(ctx, d)) for d in docs)


def check_rank_band(lib, O, upload=None, top=1 << 22):
    """ranks of 2^21 and more (the merge kernels keep an ids[] array then, tkz_bpe.h): rank_band_cases' table whose largest rank is `top`"""
    import rank_band_cases as RB
    ctx = Ctx(lib, O, RB.band_table(top), upload=upload)
    assert max(ctx.key) == top and min(ctx.key) >= 1 << 21
    rng = random.Random(top)
    word = lambda: "".join(rng.choice("abc") for _ in range(rng.choice([1, 3, 7, 12, 20, 40, 200])))
    docs = [" ".join(word() for _ in range(n)).encode() for n in (3, 40, 0, 150, 1)]
    exp = check_device(ctx, docs, "ranks up to %d" % top)
    assert len(exp[0]) > sum(len(pieces_of(ctx, d)) for d in docs)


# ---- 4. special tokens ----

def check_special(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    rng = random.Random(17)
    w = lambda n: fill(rng, n).decode()
    docs = [EOT + w(30), w(40) + EOT, w(25) + EOT + w(25), w(10) + EOT + EOT + w(10), EOT, EOT + EOT, w(SUB - 5) + EOT + w(50),
            w(30) + EOT[:6], EOT[6:] + w(30),                                # the literal cut by a document boundary
            "", w(20)]
    bdocs = [d.encode() for d in docs]
    s0 = ctx.enc.special_stats()
    on = check_device(ctx, bdocs, "special: allowed", allowed=[EOT])
    s1 = ctx.enc.special_stats()
    assert s1[0] - s0[0] == 1 and s1[1] - s0[1] == on[0].count(eot) == 9
    off = check_device(ctx, bdocs, "special: not allowed", allowed=[])
    assert ctx.enc.special_stats() == s1 and len(off[0]) > len(on[0]) and eot not in off[0]
    # the literal allowed is ONE token whose span is the literal's length
    k = on[0].index(eot, on[1][2])
    assert on[2][k + 1] - on[2][k] == len(EOT) and on[3][k + 1] - on[3][k] == len(EOT)


def check_special_utf16(lib, O, raw, pattern=N.CL100K):
    """a registered literal that holds U+FFFD next to a lone surrogate: the literals are searched as .NET searches the string"""
    specials = {k: v + 200000 for k, v in U16S.FFFD_SPECIALS.items()}       # (ids outside every table's ranks)
    ctx = Ctx(lib, O, raw, pattern, specials)
    exp = U16S.Expect(O, ctx.ovocab, pattern, specials)
    names = list(specials)
    docs = [U16S.units("ab x") + [U16S.HI] + U16S.units(" b x� c"), U16S.units("<") + [U16S.LO] + U16S.units("> <�> x"), U16S.units("x�"), [],
            [U16S.HI], U16S.units("plain text it's"), U16S.units("cut \U0001F600")[:-1], U16S.units("\U0001F600")[1:] + U16S.units(" here")]
    flat, uoffs = U16S.pack(docs)
    for allowed in (names, names[1:], []):
        ids_per_doc = [exp.encode(d, allowed) for d in docs]
        bdocs = [U16.get_bytes(d) for d in docs]
        want = ctx.expected_spans(bdocs, allowed, ids_per_doc)
        ids, ooff, tu = ctx.enc.encode_batch_spans_utf16(flat, uoffs, SC.indices(specials, allowed))
        assert_spans(ctx, "utf16 special %s" % (allowed,), (ids.tolist(), ooff.tolist(), None, tu.tolist()), want, bdocs, allowed)
        eids, eoff = ctx.enc.encode_batch_special_utf16(flat, uoffs, SC.indices(specials, allowed))
        assert ids.tolist() == eids.tolist() and ooff.tolist() == eoff.tolist()
        for d, doc in enumerate(docs):                                      # the single-text entry
            i1, u1 = ctx.enc.encode_spans_utf16(doc, SC.indices(specials, allowed))
            assert i1 == ids_per_doc[d] and u1 == want[3][want[1][d]:want[1][d + 1]], (allowed, d)


# ---- 5. units ----

def split_char(ctx, candidates):
    """the first candidate character that the table splits into several tokens"""
    for ch in candidates:
        if len(ctx.oenc.encode_bytes(ch.encode("utf-8"))) > 1:
            return ch
    raise AssertionError("no candidate is split: %r" % (candidates,))


def check_units(ctx):
    emoji = "\U0001F600"
    c2, c3 = split_char(ctx, "ʘʬԠԮ߷"), split_char(ctx, "ꙮⴰ꧁ᲀ⳿")
    n = len(ctx.oenc.encode_bytes(emoji.encode("utf-8")))
    assert n > 1
    ids, tb, tu = ctx.enc.encode_spans(emoji.encode("utf-8"))
    assert tu == [0] + [2] * (n - 1) and tb[0] == 0 and len(tb) == n        # the first token carries both units, the others have empty unit spans
    texts = [emoji, "a" + emoji + "b", c2, c3, "x" + c2 + c3 + "y", c3 * 5, "café naïve 漢字 " + emoji * 3 + " \U0001F44D\U0001F3FD end", ""]
    exp = check_device(ctx, [t.encode("utf-8") for t in texts], "units", forms=((True, True), (False, True)))
    for ch in (c2, c3):                                                      # a token starts inside the character
        k = texts.index(ch)
        assert exp[1][k + 1] - exp[1][k] > 1 and exp[3][exp[1][k] + 1] == 1
    # UTF-16: lone surrogates, a surrogate pair cut by a document boundary
    docs = [U16S.units("cut " + emoji)[:-1], U16S.units(emoji)[1:] + U16S.units(" here"), U16S.units("lone ") + [0xD800] + U16S.units(" high"), U16S.units(emoji + c3),
            [], U16S.units("end")]
    flat, uoffs = U16S.pack(docs)
    bdocs = [U16.get_bytes(d) for d in docs]
    want = ctx.expected_spans(bdocs)
    ids, ooff, tu = ctx.enc.encode_batch_spans_utf16(flat, uoffs)
    assert_spans(ctx, "units: utf16", (ids.tolist(), ooff.tolist(), None, tu.tolist()), want, bdocs)
    for d, doc in enumerate(docs):                                          # ... the last token ends at the document's length in units
        lo, hi = want[1][d], want[1][d + 1]
        if hi > lo:
            last = bdocs[d][want[2][hi - 1]:]
            assert tu[hi - 1] + int(units_begun(last)[-1]) == len(doc)


# ---- 6. size ----

def check_size(ctx, total=300 << 10):
    """one batch beyond the piece path's 256 KiB stride, ASCII and CJK, every token checked"""
    rng = random.Random(29)
    cjk = "漢字かな交じり文、한국어 \U0001F600 naïve café "
    docs = []
    while sum(map(len, docs)) < total:
        n = rng.choice([0, 30, 700, 5000, 20000])
        docs.append((cjk * (n // 60)).encode("utf-8") if rng.random() < 0.4 else fill(rng, n))
    assert sum(map(len, docs)) > 256 << 10
    check_device(ctx, docs, "size")


# ---- 7. errors ----

def check_errors(make_ctx, lib, O, raw, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc, L = ctx.enc, ctx.enc.lib.L
    docs = [b"hello world it's", b"", b"zqxjk " + EOT.encode()]
    exp = ctx.expected_spans(docs, [EOT])
    b = ctx.device_buffers(docs)
    need = len(exp[0])
    c0 = enc.spans_calls()
    with pytest.raises(N.TkzError) as ei:
        ctx.spans_device(b, [0], cap=need - 1)
    assert ei.value.code == N.E_CAPACITY and ei.value.needed == need
    data, offs = parity.pack(docs)
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_spans(data, offs, [0], out_cap=need - 1)
    assert ei.value.code == N.E_CAPACITY and ei.value.needed == need
    with pytest.raises(N.TkzError) as ei:
        enc.encode_spans(docs[2], [0], out_cap=len(exp[0]) - exp[1][2] - 1)
    assert ei.value.code == N.E_CAPACITY and ei.value.needed == len(exp[0]) - exp[1][2]
    assert enc.spans_calls() == c0                                           # failed calls are not counted
    assert_spans(ctx, "exact capacity", ctx.spans_device(b, [0], cap=need), exp, docs, [EOT])
    assert enc.spans_calls() == c0 + 1
    # both span arrays NULL
    ids, ooff, n = np.zeros(64, np.int32), np.zeros(4, np.int64), C.c_int64(-1)
    tb = np.zeros(64, np.int32)
    assert L.tkz_encode_batch_spans_utf8(enc._h, data.ctypes.data, offs.ctypes.data, 3, None, 0, ids.ctypes.data, 64, ooff.ctypes.data, None, None, C.byref(n)) == N.E_ARG
    assert L.tkz_encode_batch_spans_utf16(enc._h, data.ctypes.data, offs.ctypes.data, 3, None, 0, ids.ctypes.data, 64, ooff.ctypes.data, None, C.byref(n)) == N.E_ARG
    assert L.tkz_encode_spans_utf8(enc._h, data.ctypes.data, 5, None, 0, ids.ctypes.data, 64, None, None, C.byref(n)) == N.E_ARG
    assert L.tkz_encode_spans_utf16(enc._h, data.ctypes.data, 2, None, 0, ids.ctypes.data, 64, None, C.byref(n)) == N.E_ARG
    with pytest.raises(N.TkzError) as ei:
        ctx.spans_device(b, [0], want_bytes=False, want_units=False)
    assert ei.value.code == N.E_ARG
    # a bad or repeated allowed index, a null n_out
    for index in ([1], [0, 0], [-1]):
        with pytest.raises(N.TkzError) as ei:
            ctx.spans_device(b, index)
        assert ei.value.code == N.E_ARG
        with pytest.raises(N.TkzError) as ei:
            enc.encode_spans(docs[0], index)
        assert ei.value.code == N.E_ARG
    assert L.tkz_encode_spans_utf8(enc._h, data.ctypes.data, 5, None, 0, ids.ctypes.data, 64, tb.ctypes.data, None, None) == N.E_ARG
    assert L.tkz_encode_spans_utf16(enc._h, data.ctypes.data, 2, None, 0, ids.ctypes.data, 64, tb.ctypes.data, None) == N.E_ARG
    assert L.tkz_encode_spans_utf8(enc._h, data.ctypes.data, -1, None, 0, ids.ctypes.data, 64, tb.ctypes.data, None, C.byref(n)) == N.E_ARG
    assert L.tkz_encode_batch_spans_utf8(None, data.ctypes.data, offs.ctypes.data, 3, None, 0, ids.ctypes.data, 64, ooff.ctypes.data, tb.ctypes.data, None, C.byref(n)) == N.E_ARG
    assert L.tkz_encode_batch_spans_utf8(enc._h, data.ctypes.data, offs.ctypes.data, 3, None, 0, ids.ctypes.data, 64, None, tb.ctypes.data, None, C.byref(n)) == N.E_ARG
    # invalid UTF-8 and bad offsets, as the encode entries
    with pytest.raises(N.TkzError) as ei:
        ctx.spans_device(ctx.device_buffers([b"ok text " * 30, b"broken \xff here"]))
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_spans(data, np.asarray([0, 12, 11, len(data)], np.int64))
    assert ei.value.code == N.E_ARG
    # more than 256 registered literals
    many = make_ctx({"<|s%d|>" % i: 200000 + i for i in range(300)})
    with pytest.raises(N.TkzError) as ei:
        many.enc.encode_spans(b"a<|s7|>b", [7])
    assert ei.value.code == N.E_UNSUPPORTED
    assert many.enc.encode_spans(b"a<|s7|>b")[0] == many.oenc.encode_bytes(b"a<|s7|>b")        # (nothing allowed: the plain call)


# ---- 8. agreement with the entries there were ----

def check_agreement(make_ctx, eot=50256):
    ctx = make_ctx({EOT: eot})
    enc = ctx.enc
    rng, gib, mixed, crowded = CC.generators(7)
    w = lambda n: fill(rng, n).decode()
    texts = [w(300) + EOT + w(40), gib(600, 2, 9), "", w(2 * SUB + 9), "café \U0001F600 漢字 " + w(20), mixed(1500, 3, 3, 30), EOT, w(5)]
    docs = [t.encode("utf-8") for t in texts]
    data, offs = parity.pack(docs)
    for index in ([0], []):
        ids, ooff, tb, tu = enc.encode_batch_spans(data, offs, index)
        eids, eoff = enc.encode_batch_special(data, offs, index)
        assert ids.tolist() == eids.tolist() and ooff.tolist() == eoff.tolist()
        # with the kept token count as the index: a suffix trim's cut is the position of the first token that goes, the document's length when none goes
        for mx in (0, 1, 7, 60, 1 << 40):
            kids, koff, cb, cu = enc.encode_batch_trim(data, offs, index, N.TRIM_SUFFIX, mx)
            for d, doc in enumerate(docs):
                kept, t = int(koff[d + 1] - koff[d]), int(ooff[d]) + int(koff[d + 1] - koff[d])
                whole = kept == ooff[d + 1] - ooff[d]
                assert cb[d] == (len(doc) if whole else tb[t]) and cu[d] == (int(units_begun(doc)[-1]) if whole else tu[t]), (index, mx, d)
    # the spans at the piece starts are the piece entry's byte offsets
    ids, ooff, tb, tu = enc.encode_batch_spans(data, offs)
    pids, dpo, pbo, pto = enc.encode_batch_pieces(data, offs)
    assert pids.tolist() == ids.tolist()
    doc_of = np.searchsorted(ooff, pto[:-1], side="right") - 1
    assert [int(tb[t]) + int(offs[doc_of[k]]) for k, t in enumerate(pto[:-1].tolist())] == pbo[:-1].tolist()


# ---- 9. the Python mirror ----

def check_python_mirror(lib, O, raw_gpt2, lib_rs_text):
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, {EOT: 50256}, REGEX_PATTERN_1, lib=lib)
    key = {r: k for k, r in O.Vocab(raw_gpt2).entries()}
    key[50256] = EOT.encode()
    for text, apply in ((lib_rs_text, False), ("Hi \U0001F600\U0001F44D\U0001F3FD café " + EOT + " 漢字 end", True), ("", True), (EOT, True)):
        ids = tok.Encode(text, apply)
        data = text.encode("utf-8")
        pos, want_b = 0, []
        for i in ids:
            want_b.append(pos)
            pos += len(key[i])
        pre = units_begun(data)
        got = tok.EncodeWithOffsets(text, apply, bytes=True)
        assert got == (ids, want_b)
        got = tok.EncodeWithOffsets(text, apply)
        assert got == (ids, [int(pre[p]) for p in want_b])
        u16 = text.encode("utf-16-le")
        for t, (a, b) in enumerate(zip(got[1], got[1][1:] + [len(u16) // 2])):      # a token whose span holds whole characters spells them
            piece = key[ids[t]]
            try:
                assert u16[2 * a:2 * b].decode("utf-16-le") == piece.decode("utf-8")
            except UnicodeDecodeError:
                pass
    texts = ["Hello World", "", lib_rs_text[:2000], EOT + "x"]
    bi, bs = tok.EncodeWithOffsetsBatch(texts)
    assert bi == tok.EncodeBatch(texts) and bs == [tok.EncodeWithOffsets(t)[1] for t in texts] and tok.EncodeWithOffsetsBatch([]) == ([], [])
