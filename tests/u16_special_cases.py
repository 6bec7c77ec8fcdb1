"""Special tokens and trimming for UTF-16 batches on the device (tkz_encode_batch_special_utf16 / tkz_encode_batch_trim_utf16): the case builders and the
comparisons the emulated (CPU) and the GPU test modules share.  A document is a list of UTF-16 code units -- lone surrogates included --; the reference is
oracle.TrimOracle on the string those units are (TrimOracle._str), which searches the literals on the string as the reference does: a lone surrogate is not
U+FFFD there, although it is EF BF BD after the transcode.  Plain Encode with specials = encode_trim_suffix(text, allowed, 2**40)[0].  Every comparison is
exact: ids, offsets, cut_units."""
import numpy as np

import special_cases as SC
from tokenizer_amd import _native as N

HI, LO = 0xD83D, 0xDE00                       # the halves of U+1F600
A, B, C = "x�", "x", "<�>"          # on bytes alone A wins over B at `x` + a lone surrogate; on the string it does not match there
D = "yyy�"                               # three bytes in front of its U+FFFD: a start in the last 3 bytes of a k_lit_scan block, the replacement in the next
E = "<|" + "q" * 60 + "�" + "q" * 61 + "|>"      # 128 bytes with U+FFFD in the middle: three bitmap words when it starts late in one
FFFD_SPECIALS = {A: 60001, B: 60002, C: 60003}
EDGE_SPECIALS = {A: 60001, B: 60002, C: 60003, D: 60004, E: 60005}
assert len(E.encode("utf-8")) == 128
SIDES = (N.TRIM_SUFFIX, N.TRIM_PREFIX)
TILE, GROUP, BLOCK = 1024, 16, 4096           # units per transcoder tile / lane group, bytes per k_lit_scan block


def units(s):
    return [int(u) for u in np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16)]


def text(us):
    return np.asarray(us, dtype=np.uint16).tobytes().decode("utf-16-le", "surrogatepass")      # (= TrimOracle._str)


def pack(docs):
    flat = np.asarray([u for d in docs for u in d], dtype=np.uint16)
    return flat, np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)


def as_units(strs):
    return [units(s) for s in strs]


def utf8_len(us):
    return len(text(us).encode("utf-16-le", "surrogatepass").decode("utf-16-le", "replace").encode("utf-8"))


class Expect:
    """TrimOracle per document, remembered."""

    def __init__(self, O, ovocab, pattern, specials):
        self.oracle = O.TrimOracle(ovocab, pattern, specials)
        self.c_oracle = O.Encoder(ovocab, pattern, specials=specials)
        self._memo = {}

    def encode(self, us, allowed):
        """well-formed text: the C oracle's Encoder.encode (an equal and faster reference, and -- unlike TrimOracle, which counts a literal's length in code
        points -- right for a literal beyond the BMP); text with a lone surrogate: TrimOracle"""
        key = (tuple(us), tuple(allowed))
        if key not in self._memo:
            try:
                utf8 = text(us).encode("utf-8")
            except UnicodeEncodeError:
                return self.trim(us, allowed, N.TRIM_SUFFIX, 2 ** 40)[0]
            self._memo[key] = self.c_oracle.encode(utf8.decode("utf-8"), list(allowed))
        return self._memo[key]

    def trim(self, us, allowed, side, mx):
        key = (tuple(us), tuple(allowed), side, mx)
        if key not in self._memo:
            t = text(us)
            if side == N.TRIM_SUFFIX:
                ids, kept = self.oracle.encode_trim_suffix(t, list(allowed) or None, mx)
                cut = len(units(kept))                     # the kept text
            else:
                ids, kept = self.oracle.encode_trim_prefix(t, list(allowed) or None, mx)
                cut = len(us) - len(units(kept))           # the dropped text
            self._memo[key] = ([int(i) for i in ids], cut)
        return self._memo[key]


def _diff(what, name, got, want):
    got, want = [int(x) for x in got], [int(x) for x in want]
    if got != want:
        k = SC.first_diff(got, want)
        raise AssertionError("%s: %s differ at %d: got %s, expected %s" % (what, name, k, got[max(0, k - 2):k + 8], want[max(0, k - 2):k + 8]))


def compare_special(enc, exp, specials, allowed, docs, what="", call=None):
    """docs: lists of code units.  call(flat, offs, index) -> (ids, offsets): the entry under test (default: tkz_encode_batch_special_utf16)."""
    flat, offs = pack(docs)
    ids, ooff = (call or enc.encode_batch_special_utf16)(flat, offs, SC.indices(specials, allowed))
    want, woff = [], [0]
    for d in docs:
        want += exp.encode(d, allowed)
        woff.append(len(want))
    _diff(what, "offsets", ooff, woff)
    _diff(what, "ids", ids, want)
    return want


def compare_trim(enc, exp, specials, allowed, docs, side, mx, what="", per_doc=None):
    flat, offs = pack(docs)
    ids, ooff, cu = enc.encode_batch_trim_utf16(flat, offs, SC.indices(specials, allowed), side, mx, per_doc)
    maxima = [max(int(m), 0) for m in per_doc] if per_doc is not None else [mx] * len(docs)
    want, woff, wcu = [], [0], []
    for d, m in zip(docs, maxima):
        i, c = exp.trim(d, allowed, side, m)
        want += i
        woff.append(len(want))
        wcu.append(c)
    what = "%s side %d max %s" % (what, side, mx if per_doc is None else "per document")
    _diff(what, "offsets", ooff, woff)
    _diff(what, "cut_units", cu, wcu)
    _diff(what, "ids", ids, want)
    return want


def check_both(enc, exp, specials, allowed, docs, what="", maxima=(0, 1, 2, 3, 4, 6)):
    """the special entry, and the trim entry on both sides at maxima around the literal's item (the literal is the 2nd..4th item of the lone-surrogate documents)"""
    want = compare_special(enc, exp, specials, allowed, docs, what)
    for side in SIDES:
        for mx in maxima:
            compare_trim(enc, exp, specials, allowed, docs, side, mx, what)
    return want


# ---- lone surrogates against a U+FFFD literal -----------------------------------------------------------------------------------------------------------------

def lone_docs():
    """One batch.  The documents in order: `x` + a lone high half; `x` + a real U+FFFD; `<` + a lone low half + `>`; a pair split by the document boundary
    in front of and behind `<...>` (documents 3|4 and 5|6); a well-formed pair in a literal-free stretch; the real literal C; a lone low half after `x`; a
    high half that ends the batch."""
    u = units
    return [u("a x") + [HI] + u(" b"), u("a x� b"), u("a <") + [LO] + u("> b"),
            u("a <") + [HI], [LO] + u("> b"),
            u("a <") + [HI], [LO] + u(">") + [HI], [LO] + u(" b"),
            u("a \U0001F600 b \U0001F600\U0001F600 c"), u("a <�> b"), u("x") + [LO], u("x <") + [HI]]


def lone_expectations(exp):
    """what the bitmap is there for, stated without the oracle: (document index, allowed) -> the ids of A / B / C the result must (not) hold"""
    ida, idb, idc = (FFFD_SPECIALS[k] for k in (A, B, C))
    docs = lone_docs()
    got = lambda d, allowed: [i for i in exp.encode(docs[d], allowed) if i >= 60000]
    assert got(0, [A, B, C]) == [idb] and got(0, [A]) == [] and got(0, [A, C]) == []        # `x` + lone high: B when allowed, else plain text
    assert got(1, [A, B, C]) == [ida] and got(1, [B]) == []                                  # `x` + real U+FFFD: A (B allowed alone: A still matches first, plain)
    assert got(2, [A, B, C]) == [] and got(9, [C]) == [idc]                                  # `<` + lone low + `>`: plain; the real one: C
    for d in (3, 4, 5, 6, 7, 8):
        assert got(d, [A, B, C]) == [], d
    return docs


# ---- the positions at which the new code can go wrong ---------------------------------------------------------------------------------------------------------

_WORDS = "ab cd the fox 12 it's "


def ascii_fill(n):
    return (_WORDS * (n // len(_WORDS) + 1))[:n]


def fill(n_units, n_bytes=None):
    """n_units code units of filler that starts with 2- and 3-byte chars (so that byte and unit positions differ): n_bytes of UTF-8 when given (else whatever comes)"""
    head = "é中 "                                   # 3 units, 6 bytes
    if n_bytes is None:
        assert n_units >= 3
        return units(head + ascii_fill(n_units - 3))
    extra = n_bytes - n_units                                # every `é` adds one byte over its unit, every `中` two
    assert 0 <= extra <= 2 * n_units
    s = "中" * (extra // 2) + "é" * (extra % 2)
    s += ascii_fill(n_units - len(s))
    assert len(s) == n_units and len(s.encode("utf-8")) == n_bytes
    return units(s)


# (pattern, index of its surrogate / U+FFFD unit): what stands at the position under test
P_XHI = (units("x") + [HI] + units(" b"), 1)                 # A on bytes; B or plain on the string
P_XLO = (units("x") + [LO] + units(" b"), 1)
P_XREAL = (units("x� b"), 1)                            # A
P_CLO = (units("<") + [LO] + units("> b"), 1)                # C on bytes; plain on the string
P_CREAL = (units("<�> b"), 1)                           # C
P_DHI = (units("yyy") + [HI] + units(" b"), 3)               # D on bytes; plain on the string
P_DREAL = (units("yyy� b"), 3)


def at_unit(pat, pos):
    """a one-document batch with the pattern's surrogate at code unit `pos` of the batch"""
    p, k = pat
    return [fill(pos - k) + p + units(" tail")]


def at_byte(pat, start_byte):
    """... with the pattern's FIRST byte at byte `start_byte` of the transcoded batch (its units in front: fewer, the filler holds 3-byte chars)"""
    p, _ = pat
    return [fill(start_byte - 40, start_byte) + p + units(" tail")]


def e_docs(start_byte):
    """the 128-byte literal E with its first byte at start_byte: as it is, and with a lone surrogate in the place of its U+FFFD -- in one batch, each in its own
    document, then both in one document"""
    real = units(E)
    k = real.index(0xFFFD)
    lone_hi = real[:k] + [HI] + real[k + 1:]
    lone_lo = real[:k] + [LO] + real[k + 1:]
    f = fill(start_byte - 40, start_byte)
    return [f + real + units(" t"), f + lone_hi + units(" t"), f[:-1] + units(" ") + lone_lo + real + lone_hi]


def edge_batches():
    """(what, allowed sets, one-batch document list).  Unit positions: the replacement at the last unit of a 1024-unit tile and the first of the next, of a
    16-unit lane group; byte positions: its EF at bit 63 / bit 0 of a bitmap word with the literal's start in the word before; the literal starting within the
    last 3 bytes of a 4096-byte k_lit_scan block with the replacement in the next; E across three bitmap words."""
    out = []
    three = [[A, B, C, D, E], [A, C, D], [B]]
    for pos in (TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, GROUP - 1, GROUP, TILE + GROUP - 1, TILE + GROUP, 3 * TILE + 5 * GROUP - 1):
        for name, pat in (("x+high", P_XHI), ("x+low", P_XLO), ("x+real", P_XREAL), ("<low>", P_CLO), ("<real>", P_CREAL)):
            out.append(("%s, surrogate at unit %d" % (name, pos), three, at_unit(pat, pos)))
        # (a pair cut by a document boundary exactly there: the high half ends a document at the tile's / group's last unit)
        out.append(("pair cut by a boundary at unit %d" % pos, three, [fill(pos - 1) + units("x") + [HI], [LO] + units("> x") + [HI] + units(" <") + [HI], [LO] + units(">")]))
    for word in (1, 17, 64, 65):                             # (word 64: the first of the second k_lit_scan block)
        for start in (64 * word - 2, 64 * word - 1):         # `x` at bit 62 -> EF at bit 63; `x` at bit 63 -> EF at bit 0 of the next word
            for name, pat in (("x+high", P_XHI), ("x+real", P_XREAL), ("<low>", P_CLO), ("<real>", P_CREAL)):
                out.append(("%s, first byte at %d" % (name, start), three, at_byte(pat, start)))
    for blk in (1, 2):
        for start in (BLOCK * blk - 3, BLOCK * blk - 2, BLOCK * blk - 1):
            for name, pat in (("yyy+high", P_DHI), ("yyy+real", P_DREAL), ("x+high", P_XHI), ("<low>", P_CLO)):
                out.append(("%s, first byte at %d" % (name, start), three, at_byte(pat, start)))
    for start in (64 * 3 + 60, 64 * 5 + 63, BLOCK - 100, BLOCK - 64, 2 * BLOCK - 1):
        out.append(("128-byte literal, first byte at %d" % start, [[E], [A, B, C, D, E]], e_docs(start)))
    return out


def edge_smoke(batches):
    """the builders put things where they say: checked on the transcoded bytes"""
    for what, _, docs in batches:
        if "first byte at" in what and "128-byte" not in what:
            start = int(what.rsplit(" ", 1)[1])
            b = text(docs[0]).encode("utf-16-le", "surrogatepass").decode("utf-16-le", "replace").encode("utf-8")
            assert b[start:start + 1] in (b"x", b"<", b"y"), what


# ---- the existing UTF-8 documents, as units ----------------------------------------------------------------------------------------------------------------------

def agree_with_utf8(enc, specials, allowed, strs, what=""):
    """well-formed texts: the UTF-16 entries give what the UTF-8 entries give on the same texts"""
    import parity
    index = SC.indices(specials, allowed)
    data, offs = parity.pack([s.encode("utf-8") for s in strs])
    flat, uoffs = pack(as_units(strs))
    a = enc.encode_batch_special(data, offs, index)
    b = enc.encode_batch_special_utf16(flat, uoffs, index)
    _diff(what, "offsets (UTF-16 vs UTF-8 entry)", b[1], a[1])
    _diff(what, "ids (UTF-16 vs UTF-8 entry)", b[0], a[0])
    for side in SIDES:
        for mx in (2, 40):
            ta = enc.encode_batch_trim(data, offs, index, side, mx)
            tb = enc.encode_batch_trim_utf16(flat, uoffs, index, side, mx)
            _diff(what, "trim offsets (UTF-16 vs UTF-8 entry)", tb[1], ta[1])
            _diff(what, "trim cut_units (UTF-16 vs UTF-8 entry)", tb[2], ta[3])
            _diff(what, "trim ids (UTF-16 vs UTF-8 entry)", tb[0], ta[0])


# ---- the chunk pipeline, in a child process with a small TKZ_HOST_CHUNK_BYTES ------------------------------------------------------------------------------------

def chunk_docs():
    """~30 KiB of units: several 4 KiB chunks.  Documents of a few hundred units, one that ends in a lone high half in front of every cut candidate (and its low
    half opening the next), the lone-surrogate documents in between, runs of empty documents, and ONE document of 9,000 units: longer than two chunks, so two
    cuts fall on the same document and the chunk between them is empty."""
    docs = []
    lone = lone_docs()
    for k in range(20):
        docs.append(fill(250 + 7 * k) + units(" x") + [HI])          # ends in a lone high half: whichever document ends a chunk, many do
        docs.append([LO] + units("> after <") + [HI])                 # starts with the low half
        docs.append(lone[k % len(lone)])
        if k % 9 == 4:
            docs += [[], [], []]
        if k == 10:
            docs.append(fill(9000) + units(" x") + [HI])
    return docs


def check_chunks(enc, exp, specials):
    docs = chunk_docs()
    b0 = enc.special_stats()
    for allowed in ([A, B, C], [A]):
        compare_special(enc, exp, specials, allowed, docs, "chunk pipeline, allowed %s" % allowed)
    assert enc.special_stats()[0] == b0[0] + 2
    # a batch whose documents are all empty but the last: the first chunks hold no unit at all
    tail = [[]] * 50 + [fill(7000) + units(" x") + [HI], units("x") + [LO] + units(" <�>")]
    compare_special(enc, exp, specials, [A, B, C], tail, "chunks without units")
    return sum(len(d) for d in docs)
