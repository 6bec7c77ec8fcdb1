"""`-m gpu`: the marks' ordinals in k_docoffs (the document index when k_docmark saw no empty document, the search of the bitmap otherwise;
tests/docmark_cases.py) through libtkz.so on the hardware, ids and offsets against the oracle.  The cases of tests/test_emu_docmarks.py, on gpt2 and on synth100k."""
import pytest

import docmark_cases as DC
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu
TABLES = pytest.mark.parametrize("table", ["gpt2", "synth100k"])


@pytest.fixture(scope="module")
def upload():
    import torch
    dev = torch.device("cuda", 0)

    def up(a):
        tns = torch.from_numpy(a).to(dev)
        return tns, tns.data_ptr()
    return up


@pytest.fixture(scope="module")
def maker(oracle_mod, vocab_bytes, upload):
    def for_table(table):
        def make_ctx(specials=None, options=()):
            return DC.Ctx(N.default_library(), oracle_mod, vocab_bytes(table), N.CL100K, specials, upload=upload, options=options)
        return make_ctx
    return for_table


@TABLES
def test_no_empty_document(maker, table):
    DC.check_dense(maker(table)())


@TABLES
def test_empty_documents(maker, table):
    DC.check_empty(maker(table)())


@TABLES
def test_the_record_does_not_leak(maker, table):
    DC.check_flag_does_not_leak(maker(table)())


@TABLES
def test_stale_bitmap(maker, table):
    DC.check_stale_bitmap(maker(table)())


@TABLES
@pytest.mark.parametrize("with_empty", [False, True], ids=["no-empty", "empty"])
def test_thrown_away_attempt(maker, table, with_empty):
    DC.check_thrown_away_attempt(maker(table), with_empty)


@TABLES
def test_count_entry(maker, table):
    DC.check_count_entry(maker(table)())


@TABLES
def test_special_entry(maker, table):
    DC.check_special_entry(maker(table))
