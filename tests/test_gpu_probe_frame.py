"""`-m gpu`: the frame of tkz_probe_subtile -- text request, bitmap words, the end of the last piece, record stores, the pre-pass's keys
(tests/probe_frame_cases.py) -- through libtkz.so on the hardware, ids and offsets against the oracle.  Every case runs as a batch small enough for the single
launch (k_small) and padded past it (k_probe; the special case: k_probe_special).  The cases of tests/test_emu_probe_frame.py, all of them on both tables."""
import pytest

import probe_frame_cases as PC
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu
PADDED = pytest.mark.parametrize("padded", [False, True], ids=["k_small", "batch"])
TABLES = pytest.mark.parametrize("table", ["gpt2", "synth100k"])


@pytest.fixture(scope="module")
def ctxs(oracle_mod, vocab_bytes):
    made = {}

    def get(table, special=False):
        if (table, special) not in made:
            made[table, special] = PC.Ctx(N.default_library(), oracle_mod, vocab_bytes(table), N.CL100K, PC.SC.SPECIAL_SETS[table] if special else None)
        return made[table, special]
    return get


@TABLES
@PADDED
def test_totals(ctxs, table, padded):
    PC.check_totals(ctxs(table), padded)


@TABLES
@PADDED
def test_last_piece(ctxs, table, padded):
    PC.check_last_piece(ctxs(table), padded)


@TABLES
@PADDED
def test_long_runs(ctxs, table, padded):
    PC.check_long_runs(ctxs(table), padded)


@TABLES
@PADDED
def test_edge_starts(ctxs, table, padded):
    PC.check_edge_starts(ctxs(table), padded)


@TABLES
@PADDED
def test_document_marks(ctxs, table, padded):
    PC.check_document_marks(ctxs(table), padded)


@TABLES
@PADDED
def test_mid_keys(ctxs, table, padded):
    PC.check_mid_keys(ctxs(table), padded)


@TABLES
@PADDED
def test_halo_edge(ctxs, table, padded):
    PC.check_halo_edge(ctxs(table), padded)


@TABLES
@PADDED
def test_record_capacity(ctxs, table, padded):
    PC.check_record_capacity(ctxs(table), padded)


@TABLES
@PADDED
def test_special(ctxs, table, padded):
    PC.check_special(ctxs(table, True), padded)
