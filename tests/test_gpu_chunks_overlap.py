"""`-m gpu`: overlapping token-budget chunks through libtkz.so (tkz_encode_batch_chunks_overlap_device / _utf8 / _utf16, tkz_encode_chunks_overlap_utf8 / _utf16;
k_chunkov_walk, k_chunkov_walk_long, k_chunkov_units), exact against the rule of tkz.h over the oracle's items and the caller's own loop over the two trim
functions: the cases of tests/test_emu_chunks_overlap.py, on gpt2 and on synth100k."""
import pytest

import chunk_cases as CK
import chunk_overlap_cases as CO
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
            return CK.Ctx(lib, oracle_mod, vocab or vocab_bytes(table), pattern, specials, upload=upload, options=options)
        return make_ctx

    def plain(table):                                      # (one encoder a table for the cases that register nothing)
        if table not in made:
            made[table] = for_table(table)()
        return made[table]
    for_table.plain = plain
    return for_table


@pytest.mark.parametrize("table", TABLES)
def test_document_sizes_and_small_budgets(maker, table):
    CO.check_sizes(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_clamp_and_adds_nothing(maker, table):
    CO.check_fallback(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_oversize_items(maker, table):
    CO.check_oversize(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens(maker, table):
    CO.check_special(maker(table), CK.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_units_and_ends(maker, table, pattern):
    CO.check_units(maker(table)(pattern=pattern))


@pytest.mark.parametrize("table", TABLES)
def test_search_widths(maker, table):
    CO.check_widths(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_workgroup_edges(maker, table):
    CO.check_workgroup_edges(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_long_document_form(maker, table):
    CO.check_long_form(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_one_document_beyond_the_piece_stride(maker, table):
    CO.check_stride(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_capacity_and_argument_errors(maker, table):
    CO.check_errors(maker(table), CK.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_agreement_of_the_entries(maker, table):
    CO.check_agreement(maker(table), CK.EOT_ID[table])


def test_python_mirror(lib, oracle_mod, vocab_bytes, lib_rs_bytes):
    CO.check_python_mirror(lib, oracle_mod, vocab_bytes("gpt2"), lib_rs_bytes.decode("utf-8"))
