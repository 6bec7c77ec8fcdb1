"""`-m gpu`: padded rows through libtkz.so (tkz_encode_batch_padded_device / _utf8 / _utf16; k_pad_lens, k_pad_write), exact against the rule of tkz.h applied to
the oracle's ids: the cases of tests/test_emu_padded.py, on gpt2 and on synth100k."""
import pytest

import padded_cases as PD
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
            return PD.Ctx(lib, oracle_mod, vocab or vocab_bytes(table), pattern, specials, upload=upload, options=options)
        return make_ctx

    def plain(table):                                      # (one encoder a table for the cases that register nothing)
        if table not in made:
            made[table] = for_table(table)()
        return made[table]
    for_table.plain = plain
    return for_table


@pytest.mark.parametrize("table", TABLES)
def test_cut_edges(maker, table):
    PD.check_cut_edges(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_width(maker, table):
    PD.check_width(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_tile_and_row_geometry(maker, table):
    PD.check_geometry(maker.plain(table))


def test_more_tiles_and_documents_than_the_grids_hold(maker, lib):
    PD.check_grid_stride(maker.plain("gpt2"), lib)


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens(maker, table):
    PD.check_special(maker(table), PD.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_capacity_and_argument_errors(maker, table):
    PD.check_capacity(maker(table), PD.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_agreement_of_the_entries(maker, lib, table):
    PD.check_agreement(maker(table), lib, PD.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_an_attempt_run_again(maker, table):
    PD.check_retry(maker(table))


def test_python_mirror(lib, oracle_mod, vocab_bytes, lib_rs_bytes):
    PD.check_python_mirror(lib, oracle_mod, vocab_bytes("gpt2"), lib_rs_bytes.decode("utf-8"))
