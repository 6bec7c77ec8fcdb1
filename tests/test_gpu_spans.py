"""`-m gpu`: token spans through libtkz.so (tkz_encode_batch_spans_device / _utf8 / _utf16, tkz_encode_spans_utf8 / _utf16; k_tokspan_mark, k_tokspan_count,
k_tokspan_write), exact against positions built from the oracle's ids and the rank file's key lengths: the cases of tests/test_emu_spans.py, on gpt2 and on
synth100k."""
import pytest

import spans_cases as SP
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
    def for_table(table):
        def make_ctx(specials=None, pattern=N.CL100K, options=(), vocab=None):
            return SP.Ctx(lib, oracle_mod, vocab or vocab_bytes(table), pattern, specials, upload=upload, options=options)
        return make_ctx
    return for_table


@pytest.mark.parametrize("table", TABLES)
def test_placement_at_edges(maker, table):
    SP.check_edges(maker(table)())


@pytest.mark.parametrize("table", TABLES)
def test_every_source_of_a_piece_of_several_tokens(maker, table):
    SP.check_sources(maker(table))


@pytest.mark.parametrize("table", TABLES)
def test_promoted_pieces(maker, table):
    SP.check_promoted(maker(table)())


def test_sparse_decode_table(lib, oracle_mod, upload):
    SP.check_sparse_table(lib, oracle_mod, upload)


@pytest.mark.parametrize("table,pattern", [("gpt2", N.CL100K), ("synth100k", N.CL100K), ("synth200k", N.O200K)])
def test_key_lengths(maker, vocab_bytes, table, pattern):
    SP.check_key_lengths(maker(table)(pattern=pattern, vocab=vocab_bytes(table)))


def test_ranks_of_2_21_and_more(lib, oracle_mod, upload):
    """(synth200k's ranks end at 199,997: the table with ranks up to 2^22 is rank_band_cases')"""
    SP.check_rank_band(lib, oracle_mod, upload)


def test_synth200k(maker, vocab_bytes):
    SP.check_units(maker("synth200k")(pattern=N.O200K, vocab=vocab_bytes("synth200k")))


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens(maker, table):
    SP.check_special(maker(table), SP.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens_utf16_with_a_replacement_literal(lib, oracle_mod, vocab_bytes, table):
    SP.check_special_utf16(lib, oracle_mod, vocab_bytes(table))


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_units(maker, table, pattern):
    SP.check_units(maker(table)(pattern=pattern))


@pytest.mark.parametrize("table", TABLES)
def test_a_batch_beyond_the_piece_stride(maker, table):
    SP.check_size(maker(table)())


@pytest.mark.parametrize("table", TABLES)
def test_errors(maker, table, lib, oracle_mod, vocab_bytes):
    SP.check_errors(maker(table), lib, oracle_mod, vocab_bytes(table), SP.EOT_ID[table])


@pytest.mark.parametrize("table", TABLES)
def test_agreement_with_the_special_piece_and_trim_entries(maker, table):
    SP.check_agreement(maker(table), SP.EOT_ID[table])


def test_python_mirror(lib, oracle_mod, vocab_bytes, lib_rs_bytes):
    SP.check_python_mirror(lib, oracle_mod, vocab_bytes("gpt2"), lib_rs_bytes.decode("utf-8"))
