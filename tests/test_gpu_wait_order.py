"""`-m gpu`: the order of the memory requests in the pre-tokenizer's block staging, and the edges of tkz_probe_subtile's loop of two batches
(tests/wait_order_cases.py) through libtkz.so on the hardware, ids and offsets against the oracle.  Every case runs as a batch small enough for the single launch (k_small) and padded past it (the batch
kernels).  The cases of tests/test_emu_wait_order.py; the probe's also on synth100k."""
import pytest

import wait_order_cases as WC
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu
PADDED = pytest.mark.parametrize("padded", [False, True], ids=["k_small", "batch"])
STAGING = pytest.mark.parametrize("pattern", [N.P1, N.CL100K], ids=["p1", "cl100k"])
TABLES = pytest.mark.parametrize("table", ["gpt2", "synth100k"])


@pytest.fixture(scope="module")
def ctxs(oracle_mod, vocab_bytes):
    made = {}

    def get(pattern, table="gpt2"):
        if (pattern, table) not in made:
            made[pattern, table] = WC.Ctx(N.default_library(), oracle_mod, vocab_bytes(table), pattern)
        return made[pattern, table]
    return get


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


@TABLES
@PADDED
def test_piece_counts(ctxs, table, padded):
    WC.check_piece_counts(ctxs(N.CL100K, table), padded)


@TABLES
@PADDED
def test_miss_batches(ctxs, table, padded):
    WC.check_miss_batches(ctxs(N.CL100K, table), padded)


@TABLES
@PADDED
def test_key_lengths(ctxs, table, padded):
    WC.check_key_lengths(ctxs(N.CL100K, table), padded)


@TABLES
@PADDED
def test_random_words(ctxs, table, padded):
    WC.check_random_words(ctxs(N.CL100K, table), padded)


@TABLES
@PADDED
def test_short_last_subtile(ctxs, table, padded):
    WC.check_short_last_subtile(ctxs(N.CL100K, table), padded)
