"""The row classification of the block scanners (tkz_block_classify: bit planes of a 64-byte row, classes as boolean functions
of the planes) and the flag table of k_pretok_rows' row loop, filled only once a block has been refused.

The same cases run twice: on the CPU build of the kernel sources (tests/hostemu) and, under `-m gpu`, on the device.  Every input is
ONE document of 3 x 4,096 bytes (192 rows of 64 bytes) unless the case is about short documents: k_pretok_rows then evaluates
rows 0..61, 62..123 and 124..185 with the block evaluator (the middle block fully inside the document) and leaves rows 186..191,
whose block is not full, to the row loop.  Piece starts are compared with the oracle's split, as parity.check_pretok does."""
import functools

import numpy as np
import pytest

import emu
import parity
from tokenizer_amd import _native as N

DOC = 3 * 4096
ROWS = DOC // 64
BLOCK_ROWS = 62                      # output rows per block; block b stages rows 62 b - 1 .. 62 b + 62
INSIDE_ROWS = 3 * BLOCK_ROWS         # rows 0..185 go through the block evaluator
PATTERNS = [N.P1, N.CL100K, N.O200K]


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    return emu.library() if request.param == "emu" else N.default_library()


@pytest.fixture(scope="module")
def vocab(lib, gpt2_tiktoken_bytes):
    return N.Vocab(gpt2_tiktoken_bytes, lib)


def ascii_value_docs():
    """Byte value v (0..127) at offset p (0..63) of a row of 'a', all 128 x 64 pairs, one pair per row, on the rows the block
    evaluator takes (the rows behind them are 'a' throughout).  Returns (documents, {(v, p): (document, row)})."""
    pairs = [(v, p) for p in range(64) for v in range(128)]
    docs, where = [], {}
    for d in range(0, len(pairs), INSIDE_ROWS):
        buf = bytearray(b"a" * DOC)
        for row, (v, p) in enumerate(pairs[d:d + INSIDE_ROWS]):
            buf[64 * row + p] = v
            where[(v, p)] = (len(docs), row)
        docs.append(bytes(buf))
    return docs, where


MULTIBYTE = ["é".encode("utf-8"), "中".encode("utf-8"), "\U0001F600".encode("utf-8")]      # 2, 3 and 4 bytes
EDGE_ROWS = [0, 61, 62, 123, 124, 185, 186]      # first row; last output / last staged row of blocks 0, 1; last output row of block 2 and the row behind it


def multibyte_docs():
    """One multi-byte char per row of 'a': at every offset 0..63 (every second row, so that a char which runs over the end of its
    row lands in a row of 'a'), and the offsets at which it straddles two rows once more in the last rows of every block."""
    docs = []
    for ch in MULTIBYTE:
        buf = bytearray(b"a" * DOC)
        for p in range(64):
            at = 64 * (2 * p + 1) + p
            buf[at:at + len(ch)] = ch
        docs.append(bytes(buf))
        for k in range(1, len(ch)):                  # k bytes in its row, the rest in the next one
            buf = bytearray(b"a" * DOC)
            for row in EDGE_ROWS:
                at = 64 * row + 64 - k
                buf[at:at + len(ch)] = ch
            docs.append(bytes(buf))
    assert all(len(d) == DOC for d in docs)
    return docs


def refused_docs():
    """Blocks the evaluator hands to the row loop: a whole row of digits / blanks / line feeds in the middle of block 1, in its
    first staged row (61) and in its last (124); documents whose last block or last row is not full."""
    line = b"lorem ipsum 12 dolor's sit, amet 345\n"
    base = (line * (DOC // len(line) + 1))[:DOC]
    docs = []
    for fill in (b"7", b" ", b"\n"):
        for row in (92, 61, 124):
            buf = bytearray(base)
            buf[64 * row:64 * row + 64] = fill * 64
            docs.append(bytes(buf))
    docs.append(base)                                # rows 186..191: a block of six rows
    docs.append(base[:DOC - 37])                     # ... and a last row of 27 bytes
    return docs


def short_docs():
    line = b"it's 12345 o'clock\r\n  x's\n"
    return [(line * 3)[:n] for n in (0, 1, 63, 64, 65)]


@functools.lru_cache(maxsize=None)
def cases():
    return {"ascii": ascii_value_docs()[0], "multibyte": multibyte_docs(), "refused": refused_docs(), "short": short_docs()}


_expected = {}


def expected(O, pattern, name, i):
    """The oracle's bitmap of document i of a case: computed once, shared by the CPU and the device run."""
    key = (pattern, name, i)
    if key not in _expected:
        bm = parity.oracle_bitmap(O, pattern, [cases()[name][i]])
        bm.setflags(write=False)
        _expected[key] = bm
    return _expected[key]


def check(lib, vocab, O, pattern, name, describe=None):
    enc = N.Encoder(vocab, pattern)
    for i, doc in enumerate(cases()[name]):
        data, offs = parity.pack([doc])
        got = enc.pretokenize(data, offs)
        exp = expected(O, pattern, name, i)
        if not np.array_equal(got, exp):
            at = int(np.nonzero(got != exp)[0][0])
            more = describe(i, at) if describe else ""
            raise AssertionError("pattern %d case %s document %d: %s%s" % (pattern, name, i, parity.explain_bitmap_diff(got, exp, [doc], offs), more))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_ascii_value_at_every_offset(lib, vocab, oracle_mod, pattern):
    def describe(i, at):
        row = min(at // 64, INSIDE_ROWS - 1)
        v, p = (INSIDE_ROWS * i + row) % 128, (INSIDE_ROWS * i + row) // 128
        return "; row %d holds byte value %d at offset %d (dword %d, byte %d)" % (row, v, p, p // 4, p % 4)
    check(lib, vocab, oracle_mod, pattern, "ascii", describe)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_one_multibyte_char_at_every_offset(lib, vocab, oracle_mod, pattern):
    check(lib, vocab, oracle_mod, pattern, "multibyte")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_refused_blocks_reach_the_row_loop(lib, vocab, oracle_mod, pattern):
    check(lib, vocab, oracle_mod, pattern, "refused")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_documents_shorter_than_a_block(lib, vocab, oracle_mod, pattern):
    check(lib, vocab, oracle_mod, pattern, "short")


def test_case_layout():
    """The inputs are what the cases say: every (value, offset) pair on a row of the block evaluator, every char offset, full-size documents."""
    docs, where = ascii_value_docs()
    assert len(where) == 128 * 64 and all(len(d) == DOC for d in docs)
    for (v, p), (d, row) in where.items():
        assert row < INSIDE_ROWS and docs[d][64 * row + p] == v and docs[d][64 * row:64 * row + 64].count(b"a") >= 63
    for j, ch in enumerate(MULTIBYTE):
        doc = multibyte_docs()[sum(len(c) for c in MULTIBYTE[:j])]
        assert all(doc[64 * (2 * p + 1) + p:64 * (2 * p + 1) + p + len(ch)] == ch for p in range(64))
    assert [len(d) for d in refused_docs()] == [DOC] * 10 + [DOC - 37]
    assert ROWS - INSIDE_ROWS == 6
