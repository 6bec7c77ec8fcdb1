"""`not gpu`: the order of the memory requests in the pre-tokenizer's block staging, and the edges of tkz_probe_subtile's loop of two batches
(tests/wait_order_cases.py) -- the real kernel sources on the CPU emulator (tests/hostemu/), ids and offsets against the oracle.  Every case runs as a batch small enough for the single launch (k_small) and
padded past it (the batch kernels).  tests/test_gpu_wait_order.py runs the same cases on the hardware."""
import os
import re

import pytest

import emu
import wait_order_cases as WC
from conftest import ROOT
from tokenizer_amd import _native as N

PADDED = pytest.mark.parametrize("padded", [False, True], ids=["k_small", "batch"])
STAGING = pytest.mark.parametrize("pattern", [N.P1, N.CL100K], ids=["p1", "cl100k"])


@pytest.fixture(scope="module")
def ctxs(oracle_mod, vocab_bytes):
    made = {}

    def get(pattern, table="gpt2"):
        if (pattern, table) not in made:
            made[pattern, table] = WC.Ctx(emu.library(), oracle_mod, vocab_bytes(table), pattern)
        return made[pattern, table]
    return get


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    header = open(os.path.join(src, "tkz_kernels.h")).read()
    assert re.search(r"\bkSub = %d\b" % WC.SUB, header)
    assert re.search(r"\bkRowsPerWave = %d\b" % (WC.BLOCK // WC.ROW), header)
    assert re.search(r"\bkSmallMaxBytes = %d\b" % WC.SMALL_MAX, header)
    assert re.search(r"#define TKZ_PROBE_U 2\b", text)                       # (two batches of 64 pieces an iteration: what check_piece_counts' fills are about)
    # the block's requests stand in front of the LDS fill, the document marks' between them, in all three users; no staging loop is left to stay rolled
    rows = text[text.index("void k_pretok_rows("):text.index("void tkz_pretok_block(")]
    blk = text[text.index("void tkz_pretok_block("):text.index("void k_pretok_mb_blocks(")]
    for body, evaluate in ((rows, "done = tkz_block_eval"), (blk, "if (tkz_block_eval")):
        assert body.index("tkz_pretok_request(") < body.index("docbits[row]") < body.index("tkz_pretok_fill(") < body.index(evaluate)
        assert "c += 64" not in body
    mb = text[text.index("void k_pretok_mb_blocks("):text.index("TKZ_DEV void tkz_seq_emit(")]
    assert mb.index("request(4)") < mb.index("docbits[row]") < mb.index("fill(0, v0)") < mb.index("tkz_block_eval_o200k_mb")
    assert "c += 64" not in mb
    request = text[text.index("void tkz_pretok_request("):text.index("void tkz_pretok_fill(")]
    assert request.count("tkz_load16_or_zero(bytes, ") == 5 and "tpos + 16 <= total" in request


@STAGING
@PADDED
def test_totals(ctxs, pattern, padded):
    WC.check_totals(ctxs(pattern), padded)


@STAGING
@PADDED
def test_document_starts(ctxs, pattern, padded):
    WC.check_document_starts(ctxs(pattern), padded)


@STAGING
@PADDED
def test_straddling_pieces(ctxs, pattern, padded):
    WC.check_straddling_pieces(ctxs(pattern), padded)


@pytest.mark.parametrize("pattern,table", [(N.P1, "gpt2"), (N.CL100K, "gpt2"), (N.O200K, "synth200k")], ids=["p1", "cl100k", "o200k"])
@PADDED
def test_multibyte_across_rows(ctxs, pattern, table, padded):
    WC.check_multibyte(ctxs(pattern, table), padded)


@PADDED
def test_piece_counts(ctxs, padded):
    WC.check_piece_counts(ctxs(N.CL100K), padded)


@PADDED
def test_miss_batches(ctxs, padded):
    WC.check_miss_batches(ctxs(N.CL100K), padded)


@PADDED
def test_key_lengths(ctxs, padded):
    WC.check_key_lengths(ctxs(N.CL100K), padded)


@PADDED
def test_random_words(ctxs, padded):
    WC.check_random_words(ctxs(N.CL100K), padded)


@PADDED
def test_short_last_subtile(ctxs, padded):
    WC.check_short_last_subtile(ctxs(N.CL100K), padded)
