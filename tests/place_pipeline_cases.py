"""Cases for the load schedule of tkz_place_subtiles (k_place, and k_small's placing phase): a wavefront places four consecutive sub-tiles, requests a
sub-tile's answers and its first 256 records together at its top and the scalars of the sub-tile behind it while it places this one.  The cases are the
smallest shapes at which loads that run ahead across the wavefront's sub-tiles can go wrong (they were written for a pipeline that requested records and
answers a whole sub-tile ahead: profiles/place_pipeline).  Shared by tests/test_emu_place_pipeline.py (the CPU emulator) and
tests/test_gpu_place_pipeline.py (the hardware); every case compares ids and offsets with the oracle.

The vocabulary is built here: the 256 single bytes and three words, so that what a piece costs is known by construction -- " the" (4 bytes),
" abcde" (6) and " abcdefg" (8) are whole-piece hits of one token, any other piece of letters misses and comes back as one token a byte (no pair of
bytes is a key, so nothing merges): a miss of up to 16 bytes is an entry of its sub-tile's short list, a longer one an entry of the long list.
A sub-tile is 1 KiB; a piece belongs to the sub-tile it starts in."""
import base64
import random

import parity
from tokenizer_amd import _native as N

SUB = 1024                                   # kSub
SMALL_MAX = 128 * 1024                       # the single launch (k_small) takes batches up to this size
KEYS = [b" the", b" abcde", b" abcdefg"]
CONS = "bcdfghjklmnpqrstvwxz"


def table():
    keys = [bytes([b]) for b in range(256)] + KEYS
    return b"".join(base64.b64encode(k) + b" " + str(i).encode() + b"\n" for i, k in enumerate(keys))


class Ctx:
    def __init__(self, lib, O, options=()):
        raw = table()
        self.lib, self.O = lib, O
        self.vocab, self.ovocab = N.Vocab(raw, lib), O.Vocab(raw)
        self.oenc = O.Encoder(self.ovocab, N.CL100K)
        self.options = tuple(options)
        self._expected = {}

    def encoder(self, options=()):
        enc = N.Encoder(self.vocab, N.CL100K)
        for opt, val in self.options + tuple(options):
            enc.set_option(opt, val)
        return enc

    def expected(self, docs):
        key = tuple(docs)
        if key not in self._expected:
            self._expected[key] = parity.oracle_encode_docs(self.oenc, list(docs))
        return self._expected[key]

    def check(self, enc, docs, what):
        data, offs = parity.pack(list(docs))
        ids, ooff = enc.encode_batch(data, offs)
        exp, eoff = self.expected(docs)
        assert ooff.tolist() == eoff, what
        assert ids.tolist() == exp, what

    def pieces_per_sub(self, doc):
        """how many pieces start in each sub-tile of a one-document batch (the oracle's split)"""
        n = [0] * ((len(doc) + SUB - 1) // SUB)
        for (a, _len) in self.O.split_utf8(N.CL100K, doc):
            n[a // SUB] += 1
        return n


# ---- sub-tiles of exactly 1 KiB ----
def ordinary():
    return " abcdefg" * 128                                              # 128 pieces, all hits


def short_miss(i):
    return " q" + CONS[i % 20] + CONS[(i // 20) % 20]                       # 4 bytes -> 4 tokens: the entry's quad holds them


def long_miss(i, n=18):
    return " " + "".join(CONS[(i + 7 * k) % 20] for k in range(n - 1))      # n >= 17 bytes -> n tokens, in tmp / the dense region


def crowded(ns, nl, long_len=18, seed=0):
    """a sub-tile with exactly ns short and nl long misses (shuffled among hits)"""
    parts = [short_miss(i) for i in range(ns)] + [long_miss(i, long_len) for i in range(nl)]
    rest = SUB - sum(map(len, parts))
    assert rest >= 0 and rest % 2 == 0 and rest != 2, (ns, nl, long_len, rest)
    parts += [" the"] * ((rest - (6 if rest % 4 == 2 else 0)) // 4) + ([" abcde"] if rest % 4 == 2 else [])
    random.Random(seed * 131 + ns * 7 + nl).shuffle(parts)
    text = "".join(parts)
    assert len(text) == SUB, (ns, nl, len(text))
    return text


def plain_pad(nsub):
    return ordinary() * nsub


def pad_docs(nsub=SMALL_MAX // SUB + 1):
    """hit-only text that lifts a batch past the single launch: k_place itself runs"""
    return (plain_pad(nsub).encode(),)


# ---- batch sizes: the wavefront's four, the next wavefront's first, the batch's last sub-tile ----
def size_batches():
    out = []
    for nsub in (1, 3, 4, 5, 8, 9):
        out.append(("%d sub-tiles" % nsub, "".join(crowded(3 + s, 1 + s % 2, seed=s) for s in range(nsub))))
    for tail in (1, 17):
        out.append(("5 sub-tiles + %d bytes" % tail, "".join(crowded(2 + s, 2, seed=s) for s in range(5)) + " abcdefg abcdefg 1"[-tail:]))
    return out


def check_sizes(ctx, padded):
    enc = ctx.encoder()
    for what, text in size_batches():
        doc = text.encode()
        # (the padding goes in FRONT as a document of its own and behind as another: the batch's last sub-tile is the case's own when it is not padded only)
        docs = (pad_docs() + (doc,)) if padded else (doc,)
        before = enc.small_path_calls()[0]
        ctx.check(enc, docs, what)
        assert (enc.small_path_calls()[0] > before) == (not padded), what
        # ... and cut into documents of 300 bytes: marks in most lanes' records
        cut = tuple(doc[i:i + 300] for i in range(0, len(doc), 300))
        ctx.check(enc, (pad_docs() + cut) if padded else cut, what + ", cut")


# ---- piece counts around the 256 records of a sub-tile's first chunk ----
def count_batch(ctx):
    """one document; sub-tile 4 * i + 1 is the i-th special one, between ordinary sub-tiles of its wavefront (the counts are checked against the oracle's split)"""
    subs, want = [], {}

    def wavefront(special, np_):
        want[len(subs) + 1] = np_
        subs.extend([ordinary(), special, ordinary(), ordinary()])
    wavefront(" abcdefg" + " " + "y" * 1015, 2)                           # (one hit, one piece of 1,016 bytes)
    wavefront(" the" * 254 + " abcdefg", 255)
    wavefront(" the" * 256, 256)
    wavefront(" the" * 255 + "1" + " zq", 257)
    wavefront("1a" * 512, 1024)
    # 1 piece: a piece of 1,016 letters that starts in the sub-tile before fills all but the last 8 bytes; 0 pieces: a sub-tile inside one piece of 2,560 letters
    subs.extend([" abcdefg" * 127 + " " + "z" * 7, "z" * 1016 + " abcdefg", ordinary(), ordinary()])
    want[len(subs) - 3] = 1
    subs.extend([" abcdefg" * 64 + " " + "w" * 511, "w" * SUB, "w" * 1024, "w" * 8 + " abcdefg" * 127])
    want[len(subs) - 3] = 0
    want[len(subs) - 2] = 0
    text = "".join(subs)
    assert len(text) == SUB * len(subs)
    got = ctx.pieces_per_sub(text.encode())
    for s, n in want.items():
        assert got[s] == n, (s, n, got[s])
    return text


def check_piece_counts(ctx, padded):
    doc = count_batch(ctx).encode()
    enc = ctx.encoder()
    ctx.check(enc, (pad_docs() + (doc,)) if padded else (doc,), "piece counts")
    ctx.check(enc, ((doc,) + pad_docs()) if padded else (doc[SUB:],), "piece counts, shifted")


# ---- list lengths around what the two forms keep in LDS (64 / 128 entries), long entries in the top slots ----
LISTS = [(0, 0), (1, 0), (0, 1), (50, 13), (63, 0), (50, 14), (64, 0), (0, 40), (50, 15), (65, 0), (100, 28), (128, 0), (110, 19), (129, 0), (90, 30)]


def list_batch(heavy):
    """every length between ordinary (a few misses) sub-tiles; also a token run of 64 (the fast path's limit), one of 65, and a giant piece.
    heavy: the filler sub-tiles hold 70 entries each, so that the workspace's next batch runs the 128-slot form"""
    filler = (lambda s: crowded(60, 10, seed=s)) if heavy else (lambda s: crowded(3 + s % 5, s % 3, seed=s))
    subs = []
    for i, (ns, nl) in enumerate(LISTS):
        subs.extend([filler(2 * i), crowded(ns, nl, seed=i)] + ([crowded(LISTS[i - 1][0], LISTS[i - 1][1], seed=50 + i)] if i % 3 == 2 else []))
    subs.extend([filler(90), crowded(5, 3, long_len=64), filler(91), crowded(5, 2, long_len=65), crowded(20, 4, long_len=64), filler(92)])
    subs.extend([" abcdefg" * 100 + " " + "g" * 223, "g" * 900 + " zqx" * 31, filler(93)])                  # a giant piece of 1,124 bytes
    text = "".join(subs)
    assert len(text) == SUB * len(subs)
    return text


def check_lists(ctx, padded, heavy):
    """heavy and padded: the call is repeated as parity.check_miss_lists does for the 128-slot form (chosen from the batch before)"""
    enc = ctx.encoder(((N.OPT_PIECE_MEMO, 0),))              # (every miss an entry that a merge kernel answers, call after call)
    doc = list_batch(heavy).encode()
    pad = (("".join(crowded(60, 10, seed=200 + s) for s in range(SMALL_MAX // SUB + 1)).encode(),) if heavy else pad_docs()) if padded else ()
    for rep in range(3 if heavy and padded else 1):
        ctx.check(enc, pad + (doc,), "lists, call %d" % rep)
    enc2 = ctx.encoder()                                        # ... and with the memo answering what repeats
    for rep in range(2):
        ctx.check(enc2, (doc,) + pad, "lists, memo, call %d" % rep)


# ---- the record buffer's end: text with a piece every byte overflows a fresh workspace's records, and the redo sizes them by the count ----
def check_record_buffer(ctx, padded):
    enc = ctx.encoder()
    for tail in (1, 3, 6):
        doc = ("a1" * 2560)[:5 * SUB - 8 + tail].encode()
        ctx.check(enc if tail == 3 else ctx.encoder(), (("a1" * (SMALL_MAX // 2 + 512)).encode(), doc) if padded else (doc,), "a piece every byte, tail %d" % tail)


# ---- promoted pieces in the first chunk of consecutive sub-tiles ----
def check_promoted(ctx, padded):
    rng = random.Random(61)
    lex = sorted({rng.choice(CONS) + rng.choice("aeiou") + rng.choice(["", "x", "z"]) for _ in range(16)})         # with the blank 3 or 4 bytes: 3 or 4 tokens

    def words(n):
        out = []
        while sum(map(len, out)) < n:
            out.append(" " + rng.choice(lex) if rng.random() < 0.5 else " the")
        return "".join(out)
    learn = tuple(words(n).encode() for n in (40000, 60000, 50000))          # (too large for the single launch, which keeps no statistics)
    enc = ctx.encoder(((N.OPT_PROMOTE, 0),))
    ctx.check(enc, learn, "before: the memo fills")
    enc.set_option(N.OPT_PROMOTE, 2)                         # by hand: whatever the memo holds
    enc.set_option(N.OPT_PIECE_STATS, 1)
    enc.piece_stats(reset=True)
    ctx.check(enc, learn, "promoted, the learning text")
    st = enc.piece_stats(reset=True)
    assert st["promoted_pieces_in_tables"] >= len(lex) // 2, st
    enc.set_option(N.OPT_PIECE_STATS, 0)
    # nine sub-tiles whose first 256 records hold promoted pieces in many lanes (two and more in one lane's four), then a sub-tile with none
    body = "".join((words(SUB + 8)[:SUB - 8] + " abcdefg") for _ in range(9)) + ordinary()
    doc = body.encode()
    ctx.check(enc, (pad_docs() + (doc,)) if padded else (doc,), "promoted pieces in consecutive sub-tiles")
    ctx.check(enc, ((doc,) + learn) if padded else (doc[:4 * SUB],), "promoted pieces, again")


# ---- cut lists: a fresh workspace's lists hold 64 entries; the attempt that overflows them is thrown away and the redo must be exact ----
def check_cut_lists(ctx, padded):
    doc = "".join([crowded(3, 1), crowded(200, 0), crowded(60, 30, seed=1), crowded(2, 2), crowded(128, 10), crowded(0, 50), ordinary(), crowded(70, 0), ordinary()]).encode()
    for order in (0, 1):
        enc = ctx.encoder(((N.OPT_PIECE_MEMO, 0),))
        docs = ((pad_docs() + (doc,)) if order else ((doc,) + pad_docs())) if padded else ((doc,) if order else (doc[2 * SUB:],))
        ctx.check(enc, docs, "first call on lists that overflow")
        ctx.check(enc, docs, "the grown lists")
