"""`-m gpu`: token-budget buckets through libtkz.so (tkz_encode_batch_budgeted_device / _utf8 / _utf16; k_tbk_mark, k_tbk_chain, k_tbk_table, k_tbk_write), exact
against the rule of tkz.h restated as the sequential greedy loop over the oracle's ids: the cases of tests/test_emu_budgeted.py, on gpt2 and on synth100k."""
import pytest

import budgeted_cases as TB
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
            return TB.Ctx(lib, oracle_mod, vocab or vocab_bytes(table), pattern, specials, upload=upload, options=options)
        return make_ctx

    def plain(table):                                      # (one encoder a table for the cases that register nothing)
        if table not in made:
            made[table] = for_table(table)()
        return made[table]
    for_table.plain = plain
    return for_table


@pytest.mark.parametrize("table", TABLES)
def test_the_worked_examples(maker, table):
    TB.check_worked_examples(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_one_run_many_buckets(maker, table):
    TB.check_one_run(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("order", [TB.ASC, TB.DESC])
def test_runs(maker, table, order):
    TB.check_runs(maker.plain(table), order)


@pytest.mark.parametrize("table", TABLES)
def test_width_zero(maker, table):
    TB.check_width_zero(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_run_counts_at_the_chain_geometry(maker, table):
    TB.check_run_counts(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_documents_around_the_tiles(maker, table):
    TB.check_tiles(maker.plain(table))


def test_more_documents_than_the_grids_hold(maker, lib):
    TB.check_grid_stride(maker.plain("gpt2"), lib)


@pytest.mark.parametrize("table", TABLES)
def test_only_the_row_cap_binds(maker, table):
    TB.check_row_cap_only(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_random_batches_against_the_greedy_loop(maker, table):
    TB.check_random(maker.plain(table), rounds=120)


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens(maker, table):
    TB.check_special(maker(table), TB.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_capacity_and_argument_errors(maker, table):
    TB.check_capacity(maker(table), TB.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_agreement_of_the_entries(maker, lib, table):
    TB.check_agreement(maker(table), lib, TB.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_an_attempt_run_again(maker, table):
    TB.check_retry(maker(table))


def test_python_mirror(lib, oracle_mod, vocab_bytes, lib_rs_bytes):
    TB.check_python_mirror(lib, oracle_mod, vocab_bytes("gpt2"), lib_rs_bytes.decode("utf-8"))
