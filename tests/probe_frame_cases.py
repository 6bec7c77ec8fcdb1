"""Cases for the frame of tkz_probe_subtile -- what stands around its lookups: the text request (an interior sub-tile asks for its 1,088 bytes without a bound
a lane, the sub-tile the corpus ends in keeps the bounded form), the words of the three bitmaps at a scalar base, the end of the sub-tile's last piece (the batch
kernels search the first word behind the sub-tile on the scalar side and fall back to the 64 lanes' words), the record stores against a 32-bit count, and the
seven key dwords of the 13..28-byte pre-pass (eight LDS dwords, seven v_alignbit, a mask row per length).  Nothing of what the kernels compute changed, so
every case compares ids AND offsets with the oracle (profiles/probe_frame).  Shared by tests/test_emu_probe_frame.py (the CPU emulator) and
tests/test_gpu_probe_frame.py (the hardware).

Every case runs as a batch small enough for the single launch (k_small: tkz_probe_subtile<true>, which keeps the lanes' loads of the bitmap it wrote itself)
and padded past it (k_probe / k_probe_special).  The padding is a multiple of a sub-tile, so a case keeps its place relative to the sub-tiles' and the bitmap
words' edges when the padding goes in front of it -- and the sub-tile the corpus ends in is then not sub-tile 0."""
import base64
import random

import parity
import special_cases as SC
import wait_order_cases as WC
from tokenizer_amd import _native as N

SUB, HALO, WORD = WC.SUB, 64, 64
MID_MIN, MID_MAX = 13, 28
TOTALS = (1, 15, 16, 17, 1023, 1024, 1025, SUB + HALO - 1, SUB + HALO, SUB + HALO + 1, 1984, 2047, 2048, 2049)      # (1,984 = 31 words: the sentinel bit in a word of its own, as at 1,024 and 2,048)
LETTERS = "abcdefghijklmnopqrstuvwxyz"


class Ctx(WC.Ctx):
    def __init__(self, lib, O, raw, pattern, specials=None):
        WC.Ctx.__init__(self, lib, O, raw, pattern)
        self.keys = [base64.b64decode(line.split()[0]) for line in raw.splitlines() if line.strip()]
        self.specials = specials
        if specials:
            self.senc, self.soenc = SC.make_encoders(lib, O, self.vocab, self.ovocab, pattern, specials)

    def run(self, enc, docs, what, padded, pad_behind=False, path=True):
        """WC.Ctx.check; path=False: a batch the single launch may hand back to the batch kernels (a piece beyond its lane mergers, a record buffer that is too
        small), so which path answered is not asserted"""
        if path:
            return self.check(enc, docs, what, padded, pad_behind)
        docs = [d if isinstance(d, bytes) else d.encode() for d in docs]
        if padded:
            docs = docs + [self.pad] if pad_behind else [self.pad] + docs
        data, offs = parity.pack(docs)
        ids, ooff = enc.encode_batch(data, offs)
        exp, eoff = [], [0]
        for d in docs:
            exp += self.expected(d)
            eoff.append(len(exp))
        assert ooff.tolist() == eoff, what
        assert ids.tolist() == exp, what

    def split(self, text):
        return self.O.split_utf8(self.pattern, text if isinstance(text, bytes) else text.encode())

    def word_keys(self, length):
        """the vocabulary's keys of `length` bytes that are a blank and ASCII letters: one piece of the pattern wherever a blank or a digit stands in front"""
        out = []
        for k in self.keys:
            if len(k) == length and k[:1] == b" " and k[1:].isalpha() and k.isascii():
                out.append(k.decode())
        return out

    def near_miss(self, key, rng):
        """`key` with another last letter, no key of the table"""
        for _ in range(200):
            w = key[:-1] + rng.choice(LETTERS)
            if w != key and self.is_miss(w):
                return w
        raise AssertionError("no near-miss of %r" % key)


# ======== the corpus end: the text request's and the bitmap words' edge path ========
def check_totals(ctx, padded):
    """every total, as one document and as two; padded: the padding in front (the sub-tile the corpus ends in is not sub-tile 0) and behind (the case's
    sub-tiles are interior ones and the padding's last is the edge)"""
    enc = ctx.encoder()
    for n in TOTALS:
        text = WC.fill(n, n % 13)
        pieces = "".join(WC.two_byte(i) for i in range(n // 2 + 1))[:n]
        for behind in ((False, True) if padded else (False,)):
            ctx.run(enc, [text], "a batch of %d bytes" % n, padded, pad_behind=behind)
            ctx.run(enc, [pieces], "%d bytes of two-byte pieces" % n, padded, pad_behind=behind)
        if n > 1:
            ctx.run(enc, [text[:n // 2], text[n // 2:]], "a batch of %d bytes, two documents" % n, padded)


# ======== the end of the last piece ========
def last_piece_text(e, behind=True):
    """sub-tile 0 ends inside a run of letters that goes on for e bytes behind it: the run's end is the first piece start at or behind byte 1,024 -- bit e of the
    words behind the sub-tile -- or, with nothing behind the run, the end of the corpus"""
    lead = 7
    head = WC.fill(SUB - lead - 1, e % 11) + " "
    return head + "q" * (lead + e) + (" " + WC.fill(300, 5) if behind else "")


LAST_ENDS = (0, 1, 63, 64, 65, 127, 128, 200)                  # bit 0, bit 63, the second word, the third
LONG_ENDS = (64 * 64 - 1, 64 * 64, 64 * 64 + 1, 5000)          # behind the 64 words a wavefront looks at in one go: a run of more than 4 KiB


def check_last_piece(ctx, padded):
    enc = ctx.encoder()
    for e in LAST_ENDS:
        for behind in (True, False):
            text = last_piece_text(e, behind)
            got = ctx.split(text)
            assert (SUB + e) in [a for a, _ in got] + [len(text)] and not any(SUB <= a < SUB + e for a, _ in got), (e, behind)
            ctx.run(enc, [text], "the last piece of a sub-tile ends %d bytes behind it%s" % (e, "" if behind else ", at the end of the corpus"), padded, path=e <= 200)
            if padded:
                ctx.run(enc, [text], "the same, the padding behind it", padded, pad_behind=True, path=False)


def check_long_runs(ctx, padded):
    """a single-class run of more than 4 KiB: the end of the last piece lies behind the 64 words, and the sub-tiles inside the run hold no piece start at all"""
    enc = ctx.encoder()
    for e in LONG_ENDS:
        for behind in (True, False):
            text = last_piece_text(e, behind)
            starts = [a for a, _ in ctx.split(text)]
            assert not any(SUB <= a < 2 * SUB for a in starts), e            # (sub-tile 1 lies inside the run)
            ctx.run(enc, [text], "a run that ends %d bytes behind its sub-tile%s" % (e, "" if behind else ", at the end of the corpus"), padded, path=False)
    ctx.run(enc, [" " * 6000 + "x", "7" * 4500], "runs of blanks and of digits", padded, path=False)


# ======== piece starts and document marks at the edges of a sub-tile ========
def check_edge_starts(ctx, padded):
    """piece starts at byte 0 and at byte 1,023 of a sub-tile"""
    enc = ctx.encoder()
    first = WC.subtile_with(ctx, 128, seed=11)                      # exactly 1 KiB of whole pieces: the next piece starts at byte 0 of sub-tile 1
    second = "".join(WC.two_byte(i) for i in range(511)) + "." + " zz" + WC.fill(SUB, 3)      # "." at byte 1,022, " zz" from byte 1,023 on
    text = first + second
    starts = [a for a, _ in ctx.split(text)]
    assert SUB in starts and 2 * SUB - 1 in starts and 2 * SUB not in starts, "the case's own layout"
    ctx.run(enc, [text], "piece starts at byte 0 and byte 1,023 of a sub-tile", padded)
    ctx.run(enc, [text[:2 * SUB]], "... and the corpus ends one byte behind the start at byte 1,023", padded)
    ctx.run(enc, [text[:2 * SUB - 1]], "... and the corpus ends at that start", padded)


def check_document_marks(ctx, padded):
    """document marks and empty documents at the first and the last byte of a sub-tile and of the corpus"""
    enc = ctx.encoder()
    t = WC.fill(3 * SUB, 21)
    cuts = [0, 0, 1, SUB - 1, SUB, SUB, SUB + 1, 2 * SUB - 1, 2 * SUB - 1, 2 * SUB, 3 * SUB - 1, 3 * SUB, 3 * SUB]
    docs = [t[a:b] for a, b in zip(cuts, cuts[1:])] + [""]
    for behind in ((False, True) if padded else (False,)):
        ctx.run(enc, docs, "documents that start and end at the edges of the sub-tiles, empty ones among them", padded, pad_behind=behind)
    ctx.run(enc, ["", "", t[:SUB], ""], "empty documents at byte 0 and at the end of a corpus of one sub-tile", padded)
    ctx.run(enc, [t[:SUB - 1], t[SUB - 1:SUB + 63], "", t[SUB + 63:SUB + 64], t[SUB + 64:SUB + 200]], "marks at the last bit of a word and the first of the next", padded)


# ======== the keys of the pre-pass ========
def mid_key_doc(ctx, seed=0):
    """pieces of every length 13 .. 28 at each of the four byte alignments: a key of the table where it has a word of that length (and then a near-miss that
    differs in the key's last byte, and the key with another letter behind it), a miss otherwise; a digit run in front of each sets the alignment, and
    what stands behind a piece (a blank, a line end, a full stop) is the first byte the masks have to drop.  Returns the text and the (start, length,
    is a key) of the pieces it is about."""
    rng = random.Random(600 + seed)
    text, want = "", []
    behind = [" on", "\n", ". a", " 12"]
    for length in range(MID_MIN, MID_MAX + 1):
        keys = ctx.word_keys(length)
        for align in range(4):
            if keys:
                key = keys[rng.randrange(len(keys))]
                items = [(key, True), (ctx.near_miss(key, rng), False), (key + rng.choice(LETTERS), None)]
            else:
                items = [(ctx.misses(1, length, seed=seed + align)[0], False)]
            for piece, is_key in items:
                while (len(text) + 1) % 4 != align or not text:
                    text += "7"                                  # (one more digit: "7", "77", "777", then a piece of its own)
                text += piece[:1]
                want.append((len(text) - 1, len(piece), is_key))
                text += piece[1:] + behind[(length + align) % 4]
    return text, want


def check_mid_keys(ctx, padded):
    enc = ctx.encoder(((N.OPT_PIECE_MEMO, 0),))
    for seed in (0, 1):
        text, want = mid_key_doc(ctx, seed)
        got = set(ctx.split(text))
        seen = set()
        for start, length, is_key in want:
            assert (start, length) in got, ("the case's own layout", start, length)
            if is_key is not None:
                assert (len(ctx.expected(text[start:start + length].encode())) == 1) == is_key, text[start:start + length]
                seen.add((length, start % 4))
        assert seen == {(length, a) for length in range(MID_MIN, MID_MAX + 1) for a in range(4)}
        lead = "" if seed == 0 else WC.fill(517, 8)                # (the same pieces at other places of the sub-tiles)
        ctx.run(enc, [lead + text], "pieces of 13 .. 28 bytes at every alignment", padded)
    assert any(ctx.word_keys(length) for length in range(MID_MIN, MID_MAX + 1)), "the table has no key for the pre-pass"


def check_halo_edge(ctx, padded):
    """the staged text is the sub-tile and 64 bytes more: a piece that ends exactly at byte 1,088, one that ends a byte behind it (read from the corpus, not
    from LDS), one a byte short; and a 28-byte piece from byte 1,023 on, the last one the pre-pass can see start"""
    enc = ctx.encoder(((N.OPT_PIECE_MEMO, 0),))
    for start, length in ((SUB - 24, 24 + HALO), (SUB - 24, 24 + HALO + 1), (SUB - 24, 24 + HALO - 1), (SUB - 1, MID_MAX), (SUB - 1, MID_MAX + 1), (SUB - 1, HALO + 1), (SUB - 1, HALO + 2)):
        rng = random.Random(start + length)
        word = " " + "".join(rng.choice(WC.CONS) for _ in range(length - 1))
        text = WC.fill(start - 1, length) + "." + word + " " + WC.fill(400, 2)
        assert (start, length) in ctx.split(text), (start, length)
        ctx.run(enc, [text], "a piece of %d bytes from byte %d on" % (length, start), padded)
        ctx.run(enc, [text[:start + length]], "... at the end of the corpus", padded)
    long_keys = [k for k in ctx.keys if len(k) > HALO and len(k) <= 200 and len(ctx.split(b"." + k + b"\n")) == 3]
    for k in long_keys[:2]:                                        # (a key of the LONG table across the edge, where the vocabulary has one)
        text = WC.fill(SUB - 10, 4).encode() + b"." + k + b"\n" + WC.fill(300, 6).encode()
        ctx.run(enc, [text], "a key of %d bytes across the halo's edge" % len(k), padded)


# ======== a record buffer that is too small ========
def check_record_capacity(ctx, padded):
    """a fresh workspace holds a record per three bytes; 48 KB of one-byte pieces need one a byte: the attempt's records stop at the buffer's end, the capacity
    is reported and the batch is run again with the exact size (no option is needed to get there)"""
    text = "7." * (24 * SUB)
    assert all(length == 1 for _, length in ctx.split(text[:200]))
    enc = ctx.encoder()
    ctx.run(enc, [text], "one-byte pieces on a fresh workspace", padded, path=False)
    ctx.run(enc, [text[:5 * SUB + 3], text[:77]], "... and on the grown one", padded, path=False)


# ======== k_probe_special ========
def check_special(ctx, padded):
    """the special entry (k_probe_special; unpadded: k_small's special form): literals at the edges of a sub-tile and of the corpus, among the totals' texts and
    the pre-pass's keys"""
    names = list(ctx.specials)
    lit = names[0]
    text, _ = mid_key_doc(ctx, 2)
    body = WC.fill(SUB - 5, 31)
    docs = [lit + body + lit + text + lit, body[:SUB - len(lit)] + lit, "", lit, WC.fill(2049, 3) + lit, last_piece_text(65) + lit + last_piece_text(0, False)]
    if padded:
        docs = [ctx.pad.decode()] + docs
    SC.compare(ctx.senc, ctx.soenc, ctx.specials, names, docs, what="literals around the sub-tiles' edges")
    SC.compare(ctx.senc, ctx.soenc, ctx.specials, [], docs, what="the same text, no literal allowed")
