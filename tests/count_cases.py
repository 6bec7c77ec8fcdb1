"""Count calls (tkz_count_batch_device / _utf8 / _utf16, tkz_count_utf8 / _utf16: k_tokcount where k_place stands): the cases and comparisons the emulated (CPU)
and the GPU test modules share.  Every comparison is exact.

Every expected value is the oracle's: the length of each document's ids (parity.oracle_encode_docs; special_cases.oracle_docs with literals).  The offsets a count
call returns must also equal, entry for entry, the offsets the existing encode entry returns for the same call.

The kernel cases go through tkz_count_batch_device, which always takes the batch path.  `upload(np_array) -> (owner, pointer)` as in
special_cases.check_special_beside_plain: identity for the emulated build, a device tensor on the hardware.

Geometry the cases are built on (tkz_kernels.h / .hip): a sub-tile is SUB = 1024 bytes of the batch; k_tokcount reads a sub-tile's records -- one per piece that
starts in it -- 256 at a time, four consecutive ones a lane, and keeps the counts of SLOTS = 128 miss-list entries in LDS.
"""
import ctypes as C
import os
import random
import threading
import types

import numpy as np
import pytest

import parity
import special_cases as SC
from tokenizer_amd import _native as N

SUB, SLOTS = 1024, 128
EOT = SC.EOT
WORDS = "the of and to in is that for it with as was on be at by this had not are but from or have an they which one you were her all".split()
CONS = "bcdfghjklmnpqrstvwxz"
TINY = [b"a", b" b", b"\n", b"c d", b"qz", b" the", b"x\n\n", b" zqxj"]          # parity.check_miss_lists' `tiny` documents: 1..5 bytes each


def nested(outer, name, **cells):
    """The function `name` that `outer` defines inside its body, bound to the given values of the variables it closes over: parity.check_miss_lists' generators
    (crowded, mixed, gib) are such closures -- this runs THEIR code, it does not copy it."""
    code = next(c for c in outer.__code__.co_consts if isinstance(c, types.CodeType) and c.co_name == name)
    return types.FunctionType(code, outer.__globals__, name, None, tuple(types.CellType(cells[v]) for v in code.co_freevars))


def generators(seed):
    rng = random.Random(seed)
    g = {n: nested(parity.check_miss_lists, n, rng=rng, cons=CONS, words=WORDS) for n in ("gib", "mixed", "crowded")}
    return rng, g["gib"], g["mixed"], g["crowded"]


def fill(rng, n):
    """n bytes of plain words (every piece a key of the tables the tests use)"""
    s = ""
    while len(s) < n:
        s += rng.choice(WORDS) + " "
    return s[:n].encode()


def cut(blob, sizes):
    """blob as consecutive documents of the given sizes, the rest as the last one"""
    docs, pos = [], 0
    for n in sizes:
        docs.append(blob[pos:pos + n])
        pos += n
    docs.append(blob[pos:])
    return docs


class Ctx:
    """An encoder, its oracle and the transport of the device entry."""

    def __init__(self, lib, O, raw, pattern=N.CL100K, specials=None, upload=None, options=()):
        self.O, self.pattern, self.specials = O, pattern, specials
        self.vocab, self.ovocab = N.Vocab(raw, lib), O.Vocab(raw)
        self.enc = N.Encoder(self.vocab, pattern)
        for opt, val in options:
            self.enc.set_option(opt, val)
        if specials:
            self.enc.set_special_tokens(specials)
        self.oenc = O.Encoder(self.ovocab, pattern, specials=specials) if specials else O.Encoder(self.ovocab, pattern)
        self.upload = upload or (lambda arr: (arr, arr.ctypes.data))

    @staticmethod
    def back(o):
        return o.cpu().numpy() if hasattr(o, "cpu") else o

    def expected(self, docs, allowed=()):
        if self.specials:
            return SC.oracle_docs(self.oenc, [d.decode("utf-8") for d in docs], list(allowed))[1]
        return parity.oracle_encode_docs(self.oenc, docs)[1]

    def device_buffers(self, docs):
        data, offs = parity.pack(docs)
        padded = np.zeros(len(data) + 64, np.uint8); padded[:len(data)] = data
        return dict(n=len(docs), total=len(data), d_bytes=self.upload(padded), d_offs=self.upload(offs.astype(np.int64)))

    def count_device(self, b, index=()):
        out = self.upload(np.full(b["n"] + 1, -5, np.int64))
        tot = self.enc.count_batch_device(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], list(index), out[1])
        got = self.back(out[0]).tolist()
        assert tot == got[-1]
        return got

    def encode_device(self, b, index=()):
        ids, out = self.upload(np.zeros(max(1, b["total"]), np.int32)), self.upload(np.full(b["n"] + 1, -5, np.int64))
        args = (b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"])
        if index:
            self.enc.encode_batch_special_device(*args, list(index), ids[1], b["total"], out[1])
        else:
            self.enc.encode_batch_device(*args, ids[1], b["total"], out[1])
        return self.back(out[0]).tolist()


def check_device(ctx, docs, what, allowed=(), expect=None, beside=True):
    """tkz_count_batch_device on `docs`: the oracle's offsets, and -- entry for entry -- the encode entry's for the same call.  Returns the expected offsets."""
    exp = expect if expect is not None else ctx.expected(docs, allowed)
    index = SC.indices(ctx.specials, allowed) if ctx.specials else ()
    b = ctx.device_buffers(docs)
    got = ctx.count_device(b, index)
    if got != exp:
        d = SC.first_diff(got, exp)
        raise AssertionError("%s: count offsets differ at entry %d of %d: got %s, expected %s" % (what, d, len(exp), got[max(0, d - 2):d + 2], exp[max(0, d - 2):d + 2]))
    if beside:
        assert ctx.encode_device(b, index) == got, what + ": not the encode entry's offsets"
    return exp


# ---- 1. marks and skipping ----

def mark_batches(seed=5):
    rng = random.Random(seed)
    small = lambda: fill(rng, 100)
    out = {}
    # sub-tiles with no mark between sub-tiles with marks
    out["long_between_short"] = [small() for _ in range(7)] + [fill(rng, 5 * SUB)] + [small() for _ in range(9)] + [fill(rng, 3 * SUB + 17)] + [small()]
    # a document that starts on byte 0 of a sub-tile, on its last byte, and as the last record of a sub-tile (a word that runs across the edge)
    a = fill(rng, 2 * SUB)                                                  # -> the next one starts at byte 0 of sub-tile 2
    b = fill(rng, SUB + SUB - 1)                                            # -> the next one starts at the last byte of sub-tile 3
    c = fill(rng, 1 + 2 * SUB + SUB - 5)                                    # -> the next one starts 5 bytes before the end of sub-tile 6 ...
    d = b"abcdefghijkl" + fill(rng, 300)                                    # ... with one piece across the edge: that sub-tile's last record
    out["edges"] = [a, b, c, d, fill(rng, SUB)]
    assert [sum(map(len, out["edges"][:k])) % SUB for k in (1, 2, 3)] == [0, SUB - 1, SUB - 5]
    out["empties"] = [b"", b"", b""] + [small(), b"", small(), b"", b"", b"", b"", fill(rng, 2 * SUB + 3), b"", b"", small()] + [b"", b"", b"", b""]
    out["ends_at_total"] = [small(), b"", fill(rng, 3 * SUB)]
    out["one_document"] = [fill(rng, 4 * SUB + 100)]
    out["one_short_document"] = [b"hello world"]
    out["tiny"] = [rng.choice(TINY) for _ in range(3000)]                   # up to four marks in the four records a lane holds
    return out


def check_marks(ctx):
    for name, docs in mark_batches().items():
        check_device(ctx, docs, "marks: " + name)


# ---- 2. more than 256 records a sub-tile ----

def many_record_batches():
    text = b"a\nb\nc\nd\n" * (SUB * 5 // 8)                                   # two pieces per two bytes: 1,024 records a sub-tile
    out = {}
    # a document start behind record 256 and behind record 768 of a sub-tile (byte b of this text is record b of its sub-tile)
    out["behind_256_and_768"] = cut(text, [SUB + 258, 512, 2 * SUB + 1])
    # the only mark of a sub-tile at record 3: the walk stops after the first chunk
    out["only_mark_at_3"] = cut(text, [2 * SUB + 3])
    out["marks_in_every_chunk"] = cut(text, [SUB + 2, 255, 2, 253, 259, 255, 1])
    return out


def check_many_records(ctx):
    for name, docs in many_record_batches().items():
        check_device(ctx, docs, "many records: " + name)


# ---- 3. answers in and beyond LDS ----

def list_batches(seed=41):
    rng, gib, mixed, crowded = generators(seed)
    tail = lambda: b" " + fill(rng, 40)
    out = {}
    # 65 .. 128 list entries a sub-tile (crowded_5, _3), around 128 (_2, _1) and well beyond (_0: 136 short and 34 long), a fifth of them long (from the top of the list down); the mixed ones
    # add sub-tiles of fewer than 64 entries, of short ones only and of long ones only
    for h in (5, 3, 2, 1, 0):
        blob = crowded(6000, h).encode()
        out["crowded_%d" % h] = cut(blob, [1500, 1500, 1500]) + [tail()]
    # short and long misses from both ends
    for k, (e, lo, hi) in enumerate(((3, 3, 9), (3, 3, 30), (2, 4, 24), (2, 2, 40), (3, 17, 22), (2, 2, 4), (7, 17, 30))):
        blob = mixed(5000, e, lo, hi).encode()
        out["mixed_%d" % k] = cut(blob, [2100, 900]) + [tail()]
    out["all_short_misses"] = cut(gib(4000, 2, 2).encode(), [1030, 2000]) + [tail()]      # ~340 entries a sub-tile
    return out


def check_lists(ctx):
    batches = list_batches()
    for name, docs in batches.items():
        check_device(ctx, docs, "lists: " + name)
    # ... and once more on the lists as they have grown
    check_device(ctx, batches["crowded_2"], "lists: crowded_2 again")


# ---- 4. long token runs (a table of nothing but the 256 single bytes) ----

def byte_table(lib, O, upload=None):
    return Ctx(lib, O, parity.random_vocab_bytes(random.Random(1), n_keys=0), upload=upload)


def check_token_runs(ctx):
    docs = [(("x" * 30 + "1") * 24 + "a1" * 140).encode() * 3,               # 24 x 30-token pieces in a chunk: 952 tokens
            (("y" * 32 + "2") * 10 + "b2" * 300).encode(), (("y" * 33 + "2") * 10 + "b2" * 300).encode(),
            ("q7" * 500 + ("z" * 17 + "3") * 30 + "c3" * 100).encode(),
            ("w" * 700 + " " + "v" * 900 + "4").encode(),
            ("ab1 " * 40 + "w" * 20000).encode(), b"u" * 17000]              # 20,000 tokens in one lane's records, beyond what the packed scan takes: 64 records at a time
    # ... with document starts behind multi-token pieces in the chunk that holds the long run (one sub-tile, fewer than 256 records)
    beside = [b"ab1 " * 30, b"cd2 " * 10, b"ef3 " * 10, b"w" * 20000, b"tail x"]
    for k, dd in enumerate((docs, docs[::-1], [b"".join(docs), b"a1"], [p for d in docs for p in (d, b"c3 ")], beside)):
        check_device(ctx, dd, "token runs %d" % k)


# ---- 5. giant pieces ----

def check_giant(ctx, seed=43):
    rng, gib, mixed, crowded = generators(seed)
    first = gib(700, 2, 3).encode() + b"x" * 1500                             # the giant piece ends its document: the next one starts right behind it
    docs = [first, gib(2 * SUB, 2, 16).encode(), fill(rng, 300), gib(700, 2, 16).encode(), fill(rng, 500) + b" " + b"y" * 3000, fill(rng, 200),
            b"=" * 1100 + b" tail", fill(rng, 100)]
    check_device(ctx, docs, "giant pieces")
    check_device(ctx, [b"x" * 5000], "one giant document")


# ---- 6. promoted pieces ----

def check_promoted(ctx, seed=61):
    r1 = random.Random(seed + 1)
    vow = "aeiou"
    lex = ["".join(r1.choice(CONS) + r1.choice(vow) for _ in range(r1.randint(2, 6))) + r1.choice(["", "s", "ed", "ing"]) for _ in range(150)]

    def words(n, r):
        out = []
        while sum(map(len, out)) < n:
            out.append(r.choice([" ", " ", "\n", " the ", ", ", " 12 "]) + r.choice(lex))
        return "".join(out).encode()
    docs = [words(n, random.Random(seed + 10 + i)) for i, n in enumerate([400, 3000, 9000, 20000, 3000, 500, 40, 2500])]
    enc = ctx.enc
    enc.set_option(N.OPT_PROMOTE, 0)
    exp = check_device(ctx, docs, "promotion: before")
    check_device(ctx, docs, "promotion: memo filled", expect=exp)
    enc.set_option(N.OPT_PIECE_STATS, 1)
    enc.set_option(N.OPT_PROMOTE, 2)
    enc.piece_stats(reset=True)
    check_device(ctx, docs, "promotion: promoted", expect=exp)
    assert enc.piece_stats(reset=True)["promoted_pieces_in_tables"] > 20
    enc.set_option(N.OPT_PROMOTE, 3)
    check_device(ctx, docs, "promotion: dropped", expect=exp)
    assert enc.piece_stats(reset=True)["promoted_pieces_in_tables"] == 0
    enc.set_option(N.OPT_PIECE_STATS, 0)


# ---- 7. retry ----

def check_retry(make_ctx, seed=47):
    """the first call of a fresh encoder is a count call whose lists overflow: the attempt is redone"""
    ctx = make_ctx()
    rng, gib, mixed, crowded = generators(seed)
    crowd = cut(gib(50000, 2, 2).encode(), [700, 20000, 9000])
    plain = [fill(rng, n) for n in (300, 5000, 120, 2000)]
    w0 = ctx.enc.workspace_bytes
    exp = check_device(ctx, crowd, "retry: first call, crowded", beside=False)
    assert ctx.enc.workspace_bytes > w0
    check_device(ctx, plain, "retry: plain")
    check_device(ctx, crowd, "retry: crowded again", expect=exp)


# ---- 8. special tokens ----

def check_special(make_ctx):
    ctx = make_ctx({EOT: 50256})
    _, b = SC.side_by_side_inputs()
    docs = [d.encode() for d in b]
    s0 = ctx.enc.special_stats()
    on = check_device(ctx, docs, "special: allowed", allowed=[EOT], beside=False)
    s1 = ctx.enc.special_stats()
    assert s1[0] - s0[0] == 1 and s1[1] - s0[1] == "".join(b).count(EOT)
    off = check_device(ctx, docs, "special: not allowed", allowed=[], beside=False)
    assert ctx.enc.special_stats() == s1 and off[-1] > on[-1]
    buf = ctx.device_buffers(docs)
    assert ctx.encode_device(buf, [0]) == on and ctx.encode_device(buf, []) == off
    s2 = ctx.enc.special_stats()
    assert (s2[0] - s1[0], s2[1] - s1[1]) == (s1[0] - s0[0], s1[1] - s0[1])          # the encode entry moves the counters by as much
    with pytest.raises(N.TkzError) as ei:
        ctx.count_device(buf, [1])
    assert ei.value.code == N.E_ARG and "not a registered special token" in str(ei.value)
    with pytest.raises(N.TkzError) as ei:
        ctx.enc.count_batch(*parity.pack(docs), allowed=[0, 0])
    assert ei.value.code == N.E_ARG
    assert ctx.enc.count_batch(*parity.pack(docs), allowed=[0]).tolist() == on
    # one text with the literal in it
    t = b[0].encode()
    assert ctx.enc.count(t, [0]) == len(ctx.oenc.encode(b[0], [EOT])) < ctx.enc.count(t) == len(ctx.oenc.encode(b[0], []))


# ---- 9. patterns ----

def check_patterns(ctx):
    m = mark_batches()
    for name in ("tiny", "long_between_short", "edges", "empties"):
        check_device(ctx, m[name], "pattern %d: %s" % (ctx.pattern, name))


# ---- 10. host entries ----

def host_batch(seed=160):
    rng = random.Random(seed)
    docs = [fill(rng, 2560) for _ in range(64)]
    assert sum(map(len, docs)) == 160 << 10
    return docs


def check_host(make_ctx):
    ctx = make_ctx()
    enc = ctx.enc
    big = host_batch()
    exp = ctx.expected(big)
    data, offs = parity.pack(big)
    c0, s0 = enc.count_calls(), enc.small_path_calls()
    assert enc.count_batch(data, offs).tolist() == exp
    assert enc.count_calls() == (c0[0] + 1, c0[1]) and enc.small_path_calls() == s0           # the batch path
    assert enc.encode_batch(data, offs)[1].tolist() == exp
    small = big[:1][0][:2000]
    small = cut(small, [300, 0, 700])
    sdata, soffs = parity.pack(small)
    sexp = ctx.expected(small)
    c1, s1 = enc.count_calls(), enc.small_path_calls()
    assert enc.count_batch(sdata, soffs).tolist() == sexp
    assert enc.count_calls() == (c1[0] + 1, c1[1] + 1) and enc.small_path_calls()[0] == s1[0] + 1      # the single launch
    # total_tokens may be NULL
    ooff = np.zeros(len(small) + 1, np.int64)
    enc.lib.check(enc.lib.L.tkz_count_batch_utf8(enc._h, sdata.ctypes.data, soffs.ctypes.data, len(small), None, 0, ooff.ctypes.data, None))
    assert ooff.tolist() == sexp
    # empty batches: zero offsets
    assert enc.count_batch(np.zeros(0, np.uint8), np.zeros(4, np.int64)).tolist() == [0, 0, 0, 0]
    assert enc.count_batch(np.zeros(0, np.uint8), np.zeros(1, np.int64)).tolist() == [0]
    assert enc.count_batch_utf16(np.zeros(0, np.uint16), np.zeros(3, np.int64)).tolist() == [0, 0, 0]
    # UTF-16: a lone surrogate, and a surrogate pair cut by a document boundary (each half a lone one)
    texts = ["plain text", "lone \ud800 high", "low \udc00 lone", "pair \U0001F600 whole", "cut \ud83d", "\ude00 here", "", "end"]
    units = [np.frombuffer(t.encode("utf-16-le", "surrogatepass"), np.uint16) for t in texts]
    u = np.concatenate(units)
    uo = np.cumsum([0] + [len(x) for x in units]).astype(np.int64)
    uexp = ctx.expected([t.encode("utf-8", "replace").replace(b"?", b"\xef\xbf\xbd") if any(0xD800 <= ord(ch) <= 0xDFFF for ch in t) else t.encode("utf-8") for t in texts])
    assert enc.count_batch_utf16(u, uo).tolist() == uexp == enc.encode_batch_utf16(u, uo)[1].tolist()


def check_no_id_staging(make_ctx):
    """a fresh encoder that has only made host count calls holds strictly less memory than one that made the same calls through encode_batch"""
    data, offs = parity.pack(host_batch())
    a, b = make_ctx().enc, make_ctx().enc
    for _ in range(2):
        ca = a.count_batch(data, offs)
        cb = b.encode_batch(data, offs)[1]
        assert ca.tolist() == cb.tolist()
    assert 0 < a.workspace_bytes < b.workspace_bytes, (a.workspace_bytes, b.workspace_bytes)


def check_chunks(enc, O, ovocab, pattern, total=20000):
    """(run in a process of its own with TKZ_HOST_CHUNK_BYTES=4096) a host count call of several chunks: only the offsets travel back, rebased"""
    rng = random.Random(7)
    docs = []
    while sum(map(len, docs)) < total:
        docs.append(fill(rng, rng.choice([0, 3, 90, 700, 1500])))
    data, offs = parity.pack(docs)
    exp = parity.oracle_encode_docs(O.Encoder(ovocab, pattern), docs)[1]
    got = enc.count_batch(data, offs).tolist()
    assert got == exp and got == enc.encode_batch(data, offs)[1].tolist()
    texts = [d.decode() for d in docs]
    u = np.frombuffer("".join(texts).encode("utf-16-le"), np.uint16)
    uo = np.cumsum([0] + [len(t) for t in texts]).astype(np.int64)
    assert enc.count_batch_utf16(u, uo).tolist() == exp
    return len(docs)


# ---- 11. single entries ----

SINGLE_LENGTHS = (0, 1, 64, 1024, 1025, 131072, 131073)


def check_single(make_ctx, lengths=SINGLE_LENGTHS):
    ctx = make_ctx({EOT: 50256})
    enc = ctx.enc
    rng = random.Random(11)
    for n in lengths:
        for lit in (False, True):
            body = fill(rng, n).decode()
            if lit and n >= len(EOT):
                at = (n - len(EOT)) // 2
                body = body[:at] + EOT + body[at + len(EOT):]
            text = body.encode()
            assert len(text) == n
            units = [ord(ch) for ch in body]
            c0, s0 = enc.count_calls(), enc.small_path_calls()
            for allowed in ([], [0]):
                want = len(enc.encode_special(text, allowed))
                assert want == len(ctx.oenc.encode(body, [EOT] if allowed else []))
                assert enc.count(text, allowed) == want, (n, lit, allowed)
                assert enc.count_utf16(units, allowed) == want, (n, lit, allowed, "utf16")
            c1, s1 = enc.count_calls(), enc.small_path_calls()
            assert c1[0] - c0[0] == 4
            # the route of the encode calls: two encode and four count calls took the single launch, or none of them did
            assert (s1[0] - s0[0]) * 2 == (c1[1] - c0[1]) * 3, (n, s0, s1, c0, c1)
            assert (c1[1] - c0[1] == 4) == (0 < n <= 131072 and ctx.pattern not in (N.O200K, N.O200K_DOTNET) or 0 < n <= 1024), (n, c0, c1)
    # a lone surrogate in the one text
    units = [ord(ch) for ch in "lone \ud800 and " + EOT + " pair \U0001F600".encode("utf-16-le").decode("utf-16-le")]
    u = []
    for ch in "lone \ud800 and " + EOT + " pair \U0001F600":
        u += list(np.frombuffer(ch.encode("utf-16-le", "surrogatepass"), np.uint16))
    assert enc.count_utf16(u, [0]) == len(enc.encode_special_utf16(u, [0])) and enc.count_utf16(u) == len(enc.encode_utf16(u))


# ---- 12. arguments ----

def check_arguments(ctx, lib, O, raw):
    enc, L = ctx.enc, ctx.enc.lib.L
    docs = [b"hello world", b"it's"]
    data, offs = parity.pack(docs)
    ooff = np.zeros(3, np.int64)
    n = C.c_int64(-1)
    args8 = (data.ctypes.data, offs.ctypes.data, 2, None, 0)
    assert L.tkz_count_batch_utf8(None, *args8, ooff.ctypes.data, None) == N.E_ARG                    # null encoder
    assert L.tkz_count_batch_utf8(enc._h, *args8, None, None) == N.E_ARG                              # null offsets out
    assert L.tkz_count_batch_utf8(enc._h, data.ctypes.data, None, 2, None, 0, ooff.ctypes.data, None) == N.E_ARG      # null offsets in
    assert L.tkz_count_batch_utf8(enc._h, data.ctypes.data, offs.ctypes.data, -1, None, 0, ooff.ctypes.data, None) == N.E_ARG
    assert L.tkz_count_batch_utf8(enc._h, None, offs.ctypes.data, 2, None, 0, ooff.ctypes.data, None) == N.E_ARG      # null bytes, total > 0
    assert L.tkz_count_batch_utf16(None, data.ctypes.data, offs.ctypes.data, 2, None, 0, ooff.ctypes.data, None) == N.E_ARG
    assert L.tkz_count_batch_utf16(enc._h, data.ctypes.data, offs.ctypes.data, 2, None, 0, None, None) == N.E_ARG
    assert L.tkz_count_utf8(None, data.ctypes.data, 5, None, 0, C.byref(n)) == N.E_ARG
    assert L.tkz_count_utf8(enc._h, data.ctypes.data, 5, None, 0, None) == N.E_ARG                    # null n_out
    assert L.tkz_count_utf8(enc._h, data.ctypes.data, -1, None, 0, C.byref(n)) == N.E_ARG
    assert L.tkz_count_utf8(enc._h, None, 5, None, 0, C.byref(n)) == N.E_ARG
    assert L.tkz_count_utf16(enc._h, data.ctypes.data, 2, None, 0, None) == N.E_ARG
    assert L.tkz_count_utf16(enc._h, None, 2, None, 0, C.byref(n)) == N.E_ARG
    assert L.tkz_count_utf8(enc._h, data.ctypes.data, 5, None, -1, C.byref(n)) == N.E_ARG
    b = ctx.device_buffers(docs)
    out = ctx.upload(np.zeros(3, np.int64))
    dev = (b["d_bytes"][1], b["d_offs"][1])
    assert L.tkz_count_batch_device(None, *dev, 2, b["total"], None, 0, out[1], None, None) == N.E_ARG
    assert L.tkz_count_batch_device(enc._h, *dev, 2, b["total"], None, 0, None, None, None) == N.E_ARG
    assert L.tkz_count_batch_device(enc._h, dev[0], None, 2, b["total"], None, 0, out[1], None, None) == N.E_ARG
    assert L.tkz_count_batch_device(enc._h, *dev, -1, b["total"], None, 0, out[1], None, None) == N.E_ARG
    assert L.tkz_count_batch_device(enc._h, None, dev[1], 2, b["total"], None, 0, out[1], None, None) == N.E_ARG
    assert L.tkz_count_batch_device(enc._h, *dev, 2, b["total"], None, 0, out[1], None, None) == N.OK       # total_tokens may be NULL
    assert ctx.back(out[0]).tolist() == ctx.expected(docs)
    c0 = enc.count_calls()
    # invalid UTF-8, on the batch path and through the single launch; a document boundary inside a character
    bad = [b"ok text " * 30, b"broken \xff here", b"fine"]
    for dd in (bad, bad + [b"filler " * 30000], [b"caf\xc3", b"\xa9"]):
        with pytest.raises(N.TkzError) as ei:
            enc.count_batch(*parity.pack(dd))
        assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        ctx.count_device(ctx.device_buffers(bad))
    assert ei.value.code == N.E_INVALID_UTF8
    with pytest.raises(N.TkzError) as ei:
        enc.count(b"broken \xc3")
    assert ei.value.code == N.E_INVALID_UTF8
    # bad offsets
    with pytest.raises(N.TkzError) as ei:
        enc.count_batch(data, np.asarray([0, 12, 11, len(data)], np.int64))
    assert ei.value.code == N.E_ARG
    assert enc.count_calls() == c0                                         # failed calls are not counted
    # a byte outside a partial vocabulary
    pctx = Ctx(lib, O, b"YQ== 0\nYWI= 1\n", pattern=N.P1, upload=ctx.upload)          # 'a', 'ab'
    assert pctx.enc.count(b"aab") == 2 and pctx.count_device(pctx.device_buffers([b"ab", b"aab"])) == [0, 1, 3]
    for call in (lambda: pctx.enc.count(b"abb"), lambda: pctx.enc.count_batch(*parity.pack([b"ab", b"abab" * 40000 + b"b"])),
                 lambda: pctx.count_device(pctx.device_buffers([b"ab", b"aab b"]))):
        with pytest.raises(N.KeyNotFoundError) as ei:
            call()
        assert ei.value.code == N.E_KEY_NOT_FOUND


# ---- 13. two threads ----

def check_threads(make_ctx, rounds=4):
    ctx = make_ctx()
    enc = ctx.enc
    big = host_batch()[:24]
    small = [b"two threads", b"", b"share one encoder, each gets its own result"]
    inputs = []
    for docs in (big, small):
        ids, offs = parity.oracle_encode_docs(ctx.oenc, docs)
        inputs.append((parity.pack(docs), ctx.device_buffers(docs), ids, offs))
    errors = []

    def work(counting):
        try:
            for r in range(rounds):
                for (data, offs), b, eids, eoffs in inputs:
                    if counting:
                        got = (enc.count_batch(data, offs).tolist(), ctx.count_device(b))
                        ok = got == (eoffs, eoffs)
                    else:
                        ids, ooff = enc.encode_batch(data, offs)
                        ok = ids.tolist() == eids and ooff.tolist() == eoffs and ctx.encode_device(b) == eoffs
                    if not ok:
                        errors.append("%s thread, round %d: not the oracle's result" % ("count" if counting else "encode", r))
        except Exception as ex:
            errors.append(repr(ex))
    c0 = enc.count_calls()[0]
    threads = [threading.Thread(target=work, args=(k,)) for k in (True, False)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]
    assert enc.count_calls()[0] - c0 == rounds * 2 * 2


# ---- 14. the Python mirror ----

def check_python_mirror(lib, raw_gpt2, lib_rs_text):
    """TikTokenizer.CountTokens / CountTokensBatch equal len(Encode(...)) / [len(x) for x in EncodeBatch(...)] on the texts of reference_style.run_gpt2_suite"""
    from reference_style import IM_END, IM_START
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {EOT: 50256, IM_START: 50300, IM_END: 50301}
    tok = TokenizerBuilder.CreateTokenizer(raw_gpt2, specials, REGEX_PATTERN_1, lib=lib)
    text = IM_START + "Hello World" + IM_END
    t5 = IM_START + "Hello \u2b50 World" + IM_END
    texts = ["", "Hello World", text, lib_rs_text[:3000], t5, IM_END, " ", "x" * 300, IM_START + IM_END, "a" + IM_START, "<|im_start", EOT + EOT + "x", "a\ud800b"]
    for apply in (True, False, [IM_END], [IM_START, IM_END]):
        want = [len(x) for x in tok.EncodeBatch(texts, apply)]
        assert tok.CountTokensBatch(texts, apply) == want, apply
        assert [tok.CountTokens(t, apply) for t in texts] == want == [len(tok.Encode(t, apply)) for t in texts], apply
    assert tok.CountTokensBatch([]) == [] and tok.CountTokens("") == 0
    assert tok.CountTokens(lib_rs_text, False) == len(tok.Encode(lib_rs_text, False)) and tok.CountTokens(text) == len(tok.Encode("Hello World")) + 2
    # a set of literals the device path does not hold: len(Encode(...)), the host segmentation
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TokenizerBuilder.CreateTokenizer(raw_gpt2, many, REGEX_PATTERN_1, lib=lib)
    t = "a<|s7|>b <|s299|><|s30|"
    assert tok2.CountTokens(t) == len(tok2.Encode(t)) and tok2._special_on_host
    assert tok2.CountTokensBatch([t, "", t]) == [len(x) for x in tok2.EncodeBatch([t, "", t])] and tok2.CountTokens(t, False) == len(tok2.Encode(t, False))
