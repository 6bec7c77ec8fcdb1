"""Cases for the order of the memory requests in k_pretok_rows / tkz_pretok_block / k_pretok_mb_blocks: a block's four chunks a lane, the 16 bytes of the row
behind it and the lane's word of document marks are requested together, then LDS is filled (profiles/wait_order).  And cases for the edges of the main loop of
tkz_probe_subtile, which takes a sub-tile's pieces two batches of 64 an iteration: the same study reordered that loop's gathers and waits, measured no gain
and left the loop as it was -- the cases written for it stay, for whoever changes that loop next.  Nothing of what these kernels compute changed, so every
case compares ids AND offsets with the oracle.  Shared by tests/test_emu_wait_order.py (the CPU emulator) and tests/test_gpu_wait_order.py (the hardware).

Every case runs as a batch small enough for the single launch (k_small: tkz_pretok_block and tkz_probe_subtile<true>) and padded past it (the batch kernels).
Geometry (tkz_kernels.h / tkz_pretok.h): a wavefront of k_pretok_rows owns BLOCK = 62 rows of 64 bytes and stages the row before them, the row behind them and
16 bytes more; a sub-tile of k_probe is SUB = 1024 bytes and is probed 128 pieces (two batches of 64) an iteration.  PAD is a multiple of both and more than
the single launch takes, so a case keeps its place relative to the blocks' and the sub-tiles' edges when the padding goes in front of it."""
import random

import parity
from tokenizer_amd import _native as N

ROW, BLOCK, SUB = 64, 62 * 64, 1024
SMALL_MAX = 128 * 1024
PAD = 5 * 31 * 1024                                   # 158,720 = 40 blocks = 155 sub-tiles
assert PAD % BLOCK == 0 and PAD % SUB == 0 and PAD > SMALL_MAX
WORDS = "the of and to in is that for it with as was on be at by this had not are but from or have an they which one you were her all".split()
CONS = "bcdfghjklmnpqrstvwxz"


def fill(n, seed=0):
    """n bytes of plain words"""
    rng = random.Random(7000 + seed)
    s = ""
    while len(s) < n:
        s += rng.choice(WORDS) + " "
    return s[:n]


class Ctx:
    def __init__(self, lib, O, raw, pattern):
        self.O, self.pattern = O, pattern
        self.vocab, self.ovocab = N.Vocab(raw, lib), O.Vocab(raw)
        self.oenc = O.Encoder(self.ovocab, pattern)
        self.pad = fill(PAD, 99).encode()
        self._expected = {}

    def encoder(self, options=()):
        enc = N.Encoder(self.vocab, self.pattern)
        for opt, val in options:
            enc.set_option(opt, val)
        return enc

    def expected(self, doc):
        if doc not in self._expected:
            self._expected[doc] = self.oenc.encode_bytes(doc)
        return self._expected[doc]

    def check(self, enc, docs, what, padded, pad_behind=False):
        """docs alone (the single launch) or with the padding as a document of its own in front of them (behind them: pad_behind)"""
        docs = [d if isinstance(d, bytes) else d.encode() for d in docs]
        if padded:
            docs = docs + [self.pad] if pad_behind else [self.pad] + docs
        data, offs = parity.pack(docs)
        before = enc.small_path_calls()[0]
        ids, ooff = enc.encode_batch(data, offs)
        exp, eoff = [], [0]
        for d in docs:
            exp += self.expected(d)
            eoff.append(len(exp))
        assert ooff.tolist() == eoff, what
        assert ids.tolist() == exp, what
        if self.pattern in (N.P1, N.CL100K) and len(data):
            assert (enc.small_path_calls()[0] > before) == (not padded), what + ": not the path the case is for"

    def pieces_per_sub(self, doc):
        """how many pieces start in each sub-tile of a one-document batch (the oracle's split)"""
        n = [0] * ((len(doc) + SUB - 1) // SUB)
        for (a, _len) in self.O.split_utf8(self.pattern, doc):
            n[a // SUB] += 1
        return n

    def is_miss(self, piece):
        return len(self.oenc.encode_bytes(piece.encode())) > 1

    def misses(self, n, length, seed=0):
        """n different pieces of `length` bytes (a blank and consonants) that are no keys of the table"""
        rng, out = random.Random(8000 + 31 * length + seed), []
        while len(out) < n:
            w = " " + "".join(rng.choice(CONS) for _ in range(length - 1))
            if w not in out and self.is_miss(w):
                out.append(w)
        return out


# ======== staging ========
def total_cases():
    """the batch ends d bytes behind the k-th block: the last full block, and the 16 bytes of the row behind it present, partial and absent"""
    return [(k, d) for k in (1, 2) for d in (-1, 0, 1, 15, 16, 17, 63, 64)]


def check_totals(ctx, padded):
    enc = ctx.encoder()
    for k, d in total_cases():
        n = BLOCK * k + d
        text = fill(n, 10 * k + d)
        ctx.check(enc, [text], "total = %d blocks %+d bytes" % (k, d), padded)
        ctx.check(enc, [text[:BLOCK - 30], text[BLOCK - 30:]], "total = %d blocks %+d bytes, two documents" % (k, d), padded)


def check_document_starts(ctx, padded):
    """a document at byte 0 (block 0 has no row in front of it: the chunk that would lie before the corpus), one that starts in the first row of block 1
    (the row block 1 stages as context is block 0's last), at the block's edge and on the byte before it"""
    enc = ctx.encoder()
    text = fill(3 * BLOCK + 100, 40)
    for first in (BLOCK + 5, BLOCK, BLOCK - 1, BLOCK + ROW - 1, 1):
        for behind in (False, True):
            ctx.check(enc, [text[:first], text[first:]], "second document at byte %d" % first, padded, pad_behind=behind)
    ctx.check(enc, [text[:BLOCK + 5], "", text[BLOCK + 5:BLOCK + 6], text[BLOCK + 6:]], "documents of 0 and 1 bytes in the first row of block 1", padded, pad_behind=True)


def check_straddling_pieces(ctx, padded):
    """one piece across a block's edge: a run of blanks, a run of letters, digits, line ends"""
    enc = ctx.encoder()
    for run in (" " * 20, "a" * 20, "7" * 20, "\r\n" * 10, " " * 90, "q" * 200):
        for lead in (1, 10, len(run) - 1):
            head = fill(BLOCK - lead - 1, len(run) + lead) + "."
            text = head + run + fill(BLOCK + 77, 41)
            ctx.check(enc, [text], "a run of %r x %d from %d bytes before the edge" % (run[:2], len(run) // len(run[:2]), lead), padded)


def multibyte_docs():
    """one document per character width and position: the character lies across the end of row 60, 61 (the block's edge), 62 or 63 with 1 .. width-1 of its bytes
    in front of the edge -- rows 61 / 62 / 63 of block 0's staging (lane l holds row l - 1), the edge of the block, and the first rows of block 1"""
    out = []
    for ch in ("é", "中", "\U0001F600"):
        b = ch.encode()
        for row_end in (61, 62, 63, 64):
            for ahead in range(1, len(b)):
                at = ROW * row_end - ahead
                raw = bytearray(fill(BLOCK + 3 * ROW + 40, 50 + row_end).encode())
                raw[at - 1:at] = b" "
                raw[at:at + len(b)] = b
                out.append(("U+%04X with %d of its %d bytes before the end of row %d" % (ord(ch), ahead, len(b), row_end - 1), bytes(raw)))
    return out


def check_multibyte(ctx, padded):
    """cl100k / pattern 1: the block evaluator refuses such a block and the row loop takes it; o200k: the char-level evaluator of k_pretok_mb_blocks"""
    enc = ctx.encoder()
    for what, doc in multibyte_docs():
        ctx.check(enc, [doc], what, padded)
    docs = [d for _, d in multibyte_docs()]
    ctx.check(enc, docs[::5], "several such documents in one batch", padded)


# ======== probe ========
def two_byte(i):
    return " " + chr(97 + i % 26)


def subtile_with(ctx, np_, seed=0):
    """a sub-tile of exactly 1 KiB with exactly np_ pieces: two-byte pieces " a", " b", ... and as few longer words (of up to 40 bytes) as fill it"""
    m = 0 if np_ == SUB // 2 else max(1, -(-(SUB - 2 * np_) // 38))
    rest = SUB - 2 * (np_ - m)
    assert 0 <= m <= np_ and (m == 0) == (rest == 0) and (m == 0 or 2 * m <= rest <= 40 * m), (np_, m, rest)
    rng = random.Random(9000 + np_ + seed)
    words = [" " + "".join(rng.choice(CONS) for _ in range(rest // m + (1 if i < rest % m else 0) - 1)) for i in range(m)]
    text = "".join(two_byte(i) for i in range(np_ - m)) + "".join(words)
    assert len(text) == SUB
    return text


FILLS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 512)


def check_piece_counts(ctx, padded):
    """every fill of the iteration of two batches, and the third iteration: all in one document, each between sub-tiles of 128 pieces"""
    subs, want = [], {}
    for np_ in FILLS:
        subs.append(subtile_with(ctx, 128, seed=1))
        want[len(subs)] = np_
        subs.append(subtile_with(ctx, np_))
    subs.append(subtile_with(ctx, 128, seed=2))
    doc = "".join(subs).encode()
    got = ctx.pieces_per_sub(doc)
    for s, n in want.items():
        assert got[s] == n, (s, n, got[s])
    enc = ctx.encoder()
    ctx.check(enc, [doc], "sub-tiles of %s pieces" % (FILLS,), padded)
    for np_ in (64, 129, 257):                           # ... and each alone: the batch's only (k_small) or last (padded) sub-tile
        ctx.check(enc, [subtile_with(ctx, np_)], "one sub-tile of %d pieces" % np_, padded)


def check_miss_batches(ctx, padded):
    """a sub-tile whose last batch of 64 pieces holds misses only (40 short, 24 long: with them the lists are exactly full), and one whose misses overflow
    the 64 entries a fresh workspace's lists hold: that attempt is thrown away and redone with longer lists"""
    short, long_ = ctx.misses(100, 4), ctx.misses(24, 25)
    hits = "".join(two_byte(i) for i in range(128))
    used = len(hits) + 40 * 4 + 23 * 25
    sub = hits + "".join(short[:40]) + "".join(long_[:23]) + " " + "k" * (SUB - used - 1)       # (the 24th long miss takes what is left of the sub-tile)
    assert len(sub) == SUB and ctx.is_miss(sub[used:])
    assert ctx.pieces_per_sub(sub.encode()) == [192]
    enc = ctx.encoder(((N.OPT_PIECE_MEMO, 0),))
    plain = subtile_with(ctx, 128, seed=3)
    ctx.check(enc, [plain + sub + plain], "the last batch of a sub-tile all misses", padded)
    over = "".join(short) + "".join(two_byte(i) for i in range((SUB - 400) // 2))
    assert len(over) == SUB
    for rep in range(2):
        enc2 = ctx.encoder(((N.OPT_PIECE_MEMO, 0),))
        docs = [plain + over + sub, over] if rep else [over + plain]
        ctx.check(enc2, docs, "100 short misses in one sub-tile: the lists overflow", padded)
        ctx.check(enc2, docs, "the grown lists", padded)


def check_key_lengths(ctx, padded):
    """pieces of 12 / 13 bytes (the last length of the SHORT table, the first the pre-pass takes) and 28 / 29 (MID / LONG) in the first and the last lane of a
    batch, as keys where the table has such words and as misses; missed pieces of 13 .. 16 bytes, whose quad for k_merge_short is put together from LDS"""
    enc = ctx.encoder(((N.OPT_PIECE_MEMO, 0),))
    known = {12: " information", 13: " particularly"}
    subs = []
    for length in (12, 13, 28, 29):
        ms = ctx.misses(5, length)
        at = {0: 0, 63: 1, 64: 2, 127: 3, 128: 4}
        pieces = [(known.get(length, ms[at[i]]) if i in (0, 64) else ms[at[i]]) if i in at else two_byte(i) for i in range(300)]
        text = "".join(pieces)
        text += " " + "y" * (SUB - len(text) - 1)
        assert len(text) == SUB
        split = ctx.O.split_utf8(ctx.pattern, text.encode())
        assert [split[i][1] for i in at] == [length] * 5, (length, [split[i] for i in at])
        subs.append(text)
    ctx.check(enc, ["".join(subs)], "pieces of 12 / 13 / 28 / 29 bytes in lanes 0 and 63", padded)
    mid = [w for length in (13, 14, 15, 16) for w in ctx.misses(6, length, seed=1)]
    random.Random(5).shuffle(mid)
    text = "".join(w + two_byte(i) * 3 for i, w in enumerate(mid))
    text += " " + "y" * (SUB - len(text) - 1)
    assert len(text) == SUB
    ctx.check(enc, [subtile_with(ctx, 128, seed=4) + text], "missed pieces of 13 .. 16 bytes", padded)


def check_random_words(ctx, padded):
    """4,096 random lower-case words of 1 .. 12 bytes: first-bucket hits, second-bucket hits and misses in every batch"""
    rng = random.Random(77)
    words = ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(1, 12))) for _ in range(4096)]
    ctx.check(ctx.encoder(), [" ".join(words)], "4,096 random words", padded)


def check_short_last_subtile(ctx, padded):
    """the batch ends inside a sub-tile"""
    enc = ctx.encoder()
    for n in (100, SUB - 1, SUB + 1, 2 * SUB + 300, 3 * SUB - 15):
        ctx.check(enc, [fill(n, 60 + n % 7)], "a batch of %d bytes" % n, padded)
        ctx.check(enc, ["".join(two_byte(i) for i in range(n // 2))], "%d two-byte pieces" % (n // 2), padded)
