"""`-m gpu`: length-bucketed padded rows through libtkz.so (tkz_encode_batch_bucketed_device / _utf8 / _utf16; k_bkt_hist, k_bkt_scatter, k_bkt_table,
k_bkt_write), exact against the rule of tkz.h applied to the oracle's ids: the cases of tests/test_emu_bucketed.py, on gpt2 and on synth100k, and documents of
65,535 / 65,536 / 65,537 tokens, which only the hardware takes in a few seconds."""
import pytest

import bucketed_cases as BK
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu
TABLES = ["gpt2", "synth100k"]


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def upload():
    import torch
    dev = torch.device("cuda", 0)

    def up(a):
        tns = torch.from_numpy(a).to(dev)
        return tns, tns.data_ptr()
    return up


@pytest.fixture(scope="module")
def maker(lib, oracle_mod, vocab_bytes, upload):
    made = {}

    def for_table(table):
        def make_ctx(specials=None, pattern=N.CL100K, options=(), vocab=None):
            return BK.Ctx(lib, oracle_mod, vocab or vocab_bytes(table), pattern, specials, upload=upload, options=options)
        return make_ctx

    def plain(table):                                      # (one encoder a table for the cases that register nothing)
        if table not in made:
            made[table] = for_table(table)()
        return made[table]
    for_table.plain = plain
    return for_table


@pytest.mark.parametrize("table", TABLES)
def test_the_worked_example(maker, table):
    BK.check_worked_example(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_stability_and_ties(maker, table):
    BK.check_ties(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_documents_around_the_sort_tile(maker, table):
    BK.check_sort_tiles(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_digits(maker, table):
    BK.check_digits(maker.plain(table), long_documents=table == "gpt2")


def test_more_documents_and_tiles_than_the_grids_hold(maker, lib):
    BK.check_grid_stride(maker.plain("gpt2"), lib)


@pytest.mark.parametrize("table", TABLES)
def test_buckets(maker, table):
    BK.check_buckets(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_the_writer_geometry(maker, table):
    BK.check_geometry(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens(maker, table):
    BK.check_special(maker(table), BK.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_capacity_and_argument_errors(maker, table):
    BK.check_capacity(maker(table), BK.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_agreement_of_the_entries(maker, lib, table):
    BK.check_agreement(maker(table), lib, BK.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_an_attempt_run_again(maker, table):
    BK.check_retry(maker(table))


def test_python_mirror(lib, oracle_mod, vocab_bytes, lib_rs_bytes):
    BK.check_python_mirror(lib, oracle_mod, vocab_bytes("gpt2"), lib_rs_bytes.decode("utf-8"))
