"""Cases for the document marks' ordinals in k_docoffs: k_docmark records whether a document of the batch is empty (offs[d] == offs[d + 1]); when none is, the
ordinal of document d's mark is d and k_docoffs reads neither the bitmap nor the ordinal bases, otherwise it searches the bitmap as before.  Shared by
tests/test_emu_docmarks.py (the CPU emulator) and tests/test_gpu_docmarks.py (the hardware).

Every case goes through the batch device entry (tkz_encode_batch_device, which always takes the batch path: k_docmark, k_place, k_docoffs), and ids AND
out_offsets are compared with the oracle's.  The shapes are the smallest at which a mark's ordinal can go wrong: a sub-tile is SUB = 1024 bytes (16 words of
the bitmap), the ordinal base is kept per sub-tile, a mark is a bit of a 64-bit word.  `upload` as in count_cases.Ctx.
"""
import numpy as np

import count_cases as CC
import parity
import special_cases as SC
from tokenizer_amd import _native as N

SUB = 1024
EOT = SC.EOT


class Ctx(CC.Ctx):
    def expected_ids(self, docs, allowed=()):
        if self.specials:
            return SC.oracle_docs(self.oenc, [d.decode("utf-8") for d in docs], list(allowed))
        return parity.oracle_encode_docs(self.oenc, docs)

    def encode(self, docs, index=(), enc=None):
        """tkz_encode_batch_device (index: tkz_encode_batch_special_device) -> (ids, out_offsets) as lists"""
        enc = enc or self.enc
        b = self.device_buffers(docs)
        cap = max(1, b["total"])
        ids, out = self.upload(np.full(cap, -7, np.int32)), self.upload(np.full(b["n"] + 1, -5, np.int64))
        args = (b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"])
        if index:
            tot = enc.encode_batch_special_device(*args, list(index), ids[1], cap, out[1])
        else:
            tot = enc.encode_batch_device(*args, ids[1], cap, out[1])
        return self.back(ids[0])[:tot].tolist(), self.back(out[0]).tolist()

    def check(self, docs, what, allowed=(), enc=None):
        index = SC.indices(self.specials, allowed) if self.specials else ()
        ids, offs = self.encode(docs, index, enc)
        eids, eoffs = self.expected_ids(docs, allowed)
        assert offs == eoffs, "%s: offsets differ at document %d" % (what, SC.first_diff(offs, eoffs) - 1)
        assert ids == eids, "%s: ids differ at %d" % (what, SC.first_diff(ids, eids))
        return eoffs


def text(n, seed=0):
    """n bytes of plain words, cut anywhere"""
    rng = CC.generators(1000 + seed)[0]
    return CC.fill(rng, n)


def docs_of(sizes, seed=0):
    return CC.cut(text(sum(sizes), seed), sizes)[:len(sizes)]


# ---- no document is empty: the ordinal is the index ----
def dense_cases():
    return [
        ("1,024 documents of 1 byte: a mark on every bit of a sub-tile", docs_of([1] * 1024)),
        ("1,500 documents of 1 byte: into the second sub-tile", docs_of([1] * 1500, 1)),
        ("documents of 64 bytes: one mark a word, at bit 0", docs_of([64] * 40, 2)),
        ("documents of 1,024 bytes: one mark a sub-tile", docs_of([1024] * 5, 3)),
        ("documents of 3,000 bytes: sub-tiles without a mark", docs_of([3000] * 5, 4)),
        ("starts at bits 63 and 0 of adjacent words", docs_of([63, 1, 127, 1, 700], 5)),
        ("starts at bytes 1023 and 1024", docs_of([1023, 1, 500], 6)),
        ("one document", docs_of([2500], 7)),
        ("one document of one byte", docs_of([1], 8)),
        ("total % 64 == 0", docs_of([300, 340], 9)),
        ("total % 64 == 1", docs_of([300, 341], 10)),
        ("total % 64 == 63", docs_of([300, 403], 11)),
        ("more documents than one workgroup's 256 lanes, of 1..9 bytes", docs_of([1 + (7 * i) % 9 for i in range(700)], 12)),
    ]


def check_dense(ctx):
    for what, docs in dense_cases():
        assert all(len(d) for d in docs)
        ctx.check(docs, what)


# ---- empty documents: several documents share a mark, the ordinal is searched ----
def empty_cases():
    a, b, c = docs_of([700, 1400, 90], 20)
    return [
        ("empty documents at the front, in the middle and two in a row", [b"", a, b"", b, b"", b"", c]),
        ("one empty document in the middle", [a, b"", b]),
        ("a run of empty documents at the end: starts equal to the total", [a, b, b"", b"", b""]),
        ("an empty document at a sub-tile's edge", docs_of([1024], 21) + [b""] + docs_of([1024], 22)),
        ("empty documents among 1-byte ones", [x for i, d in enumerate(docs_of([1] * 300, 23)) for x in ([d, b""] if i % 64 in (0, 62, 63) else [d])]),
        ("every document empty", [b""] * 5),
        ("no document", []),
    ]


def check_empty(ctx):
    for what, docs in empty_cases():
        ctx.check(docs, what)


# ---- the record of one batch is not the next one's ----
def check_flag_does_not_leak(ctx):
    a, b, c = docs_of([500, 64, 1500], 30)
    with_empty, without = [a, b"", b, c], [b, a, c]
    for rep in range(2):
        ctx.check(with_empty, "an empty document, call %d" % rep)
        ctx.check(without, "no empty document, call %d" % rep)
    ctx.check(with_empty, "an empty document, last call")


# ---- a bitmap full of an earlier batch's marks ----
def check_stale_bitmap(ctx):
    n = 8 * SUB
    ctx.check(docs_of([1] * n, 40), "1-byte documents: every bit of the bitmap set")
    ctx.check(docs_of([3000, 3000, n - 6000], 41), "the same size in three documents")
    ctx.check(docs_of([1] * n, 40), "1-byte documents again")
    ctx.check(docs_of([64] * 8 + [256 * 1024] + [64] * 8, 42), "a document of 256 KiB between documents of 64 bytes")
    ctx.check(docs_of([64] * 8, 43) + [b""] + docs_of([3000] * 4, 44), "a shorter batch with an empty document behind it")


# ---- an attempt that is thrown away: the redo starts behind k_docmark, and must still know ----
def check_thrown_away_attempt(make_ctx, with_empty):
    """the first call of a fresh encoder with the memo off: the miss lists of its crowded sub-tiles overflow, the lists grow and the attempt is redone"""
    ctx = make_ctx(options=((N.OPT_PIECE_MEMO, 0),))
    gib = CC.generators(47)[1]
    crowd = CC.cut(gib(50000, 2, 2).encode(), [700, 20000, 9000])
    assert all(len(d) for d in crowd)
    if with_empty:
        crowd = crowd[:2] + [b""] + crowd[2:] + [b""]
    w0 = ctx.enc.workspace_bytes
    ctx.check(crowd, "first call, crowded")
    assert ctx.enc.workspace_bytes > w0                  # (the lists grew: there was a second attempt)
    ctx.check(crowd, "the grown lists")
    # ... and the other kind right behind it on the same encoder
    other = [d for d in crowd if d] if with_empty else crowd[:1] + [b""] + crowd[1:]
    ctx.check(other, "the other kind behind it")


# ---- the count entry and the special-token entry launch the same k_docoffs ----
def check_count_entry(ctx):
    for what, docs in (dense_cases()[0], dense_cases()[4], empty_cases()[0], empty_cases()[2]):
        exp = ctx.expected_ids(docs)[1]
        assert ctx.count_device(ctx.device_buffers(docs)) == exp, what


def check_special_entry(make_ctx):
    ctx = make_ctx({EOT: 50256})
    a, b, c = (d.decode() for d in docs_of([700, 1400, 90], 50))
    dense = [a[:300] + EOT + a[300:], EOT, b, EOT + c + EOT, "x"]
    sparse = [dense[0], "", EOT, "", "", b, c + EOT, ""]
    for allowed in ([EOT], []):
        for what, docs in (("no empty document", dense), ("empty documents", sparse), ("no empty document again", dense)):
            ctx.check([d.encode() for d in docs], "special entry, allowed %r: %s" % (allowed, what), allowed=allowed)
        index = SC.indices(ctx.specials, allowed)
        for docs in (dense, sparse):
            raw = [d.encode() for d in docs]
            assert ctx.count_device(ctx.device_buffers(raw), index) == ctx.expected_ids(raw, allowed)[1]
