"""`-m gpu`: pair rows through libtkz.so (tkz_encode_batch_pairs_device / _utf8 / _utf16; k_pair_lens, k_pair_write), exact against the rule of tkz.h applied to
the oracle's ids: the cases of tests/test_emu_pairs.py, on gpt2 and on synth100k."""
import random

import pytest

import pairs_cases as PR
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
            return PR.Ctx(lib, oracle_mod, vocab or vocab_bytes(table), pattern, specials, upload=upload, options=options)
        return make_ctx

    def plain(table):                                      # (one encoder a table for the cases that register nothing)
        if table not in made:
            made[table] = for_table(table)()
        return made[table]
    for_table.plain = plain
    return for_table


@pytest.mark.parametrize("table", TABLES)
def test_the_header_example_on_the_kernels(maker, table):
    rng = random.Random(1)
    docs = [PR.words(rng, 5), PR.words(rng, 3), b"", PR.words(rng, 1)]
    for strategy, kept in ((PR.LONGEST, [3, 2, 0, 1]), (PR.ONLY_FIRST, [2, 3, 0, 1]), (PR.ONLY_SECOND, [5, 0, 0, 1])):
        m = PR.check_device(maker.plain(table), docs, 8, "the header's example", 1, 2, 1, 3, pad=0, strategy=strategy)
        assert (m.W, m.lens, m.n_cut, m.kept) == (8, [8, 4], 1, kept)


@pytest.mark.parametrize("table", TABLES)
def test_strategy_edges(maker, table):
    PR.check_strategy_edges(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_type_ids_and_null_arrays(maker, table):
    PR.check_types_and_nulls(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_width(maker, table):
    PR.check_width(maker.plain(table))


@pytest.mark.parametrize("table", TABLES)
def test_tile_row_and_seam_geometry(maker, table):
    PR.check_geometry(maker.plain(table))


def test_more_tiles_and_pairs_than_the_grids_hold(maker, lib):
    PR.check_grid_stride(maker.plain("gpt2"), lib)


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens(maker, table):
    PR.check_special(maker(table), PR.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_capacity_and_argument_errors(maker, table):
    PR.check_capacity(maker(table), PR.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_agreement_of_the_entries(maker, lib, table):
    PR.check_agreement(maker(table), lib, PR.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_an_attempt_run_again(maker, table):
    PR.check_retry(maker(table))


def test_python_mirror(lib, oracle_mod, vocab_bytes, lib_rs_bytes):
    PR.check_python_mirror(lib, oracle_mod, vocab_bytes("gpt2"), lib_rs_bytes.decode("utf-8"))
