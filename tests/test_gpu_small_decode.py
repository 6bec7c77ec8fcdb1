"""`-m gpu`: Decode(int[]) for one id list in a single launch through libtkz.so (tkz_decode_utf8 / _utf16, k_dec_small), exact against the vocabulary's keys,
the plain UTF-8 reference of tests/u8_decode_cases.py and the batch entries: the cases of tests/test_emu_small_decode.py, every one on both tables."""
import pytest

import small_decode_cases as SD
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def dec(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(table):
        if table not in cache:
            cache[table] = SD.setup(lib, vocab_bytes("gpt2"), oracle_mod, table)
        return cache[table]
    return get


def test_the_tables(dec):
    enc, S = dec("dense")
    assert enc.small_decode_calls() == (0, 0) and len(S.key_of[S.longest]) * SD.TILE == SD.MAX_BYTES        # (gpt2: 128 bytes)
    _, S2 = dec("sparse")
    assert max(S2.specials.values()) >= 1 << 22 and "\U0001F600" in SD.FAR_LITERAL


@pytest.mark.parametrize("table", SD.TABLES)
def test_id_totals(dec, table):
    SD.check_id_totals(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_byte_tile_edges(dec, table):
    SD.check_byte_edges(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_stage_overflow_and_capacity_edges(dec, table):
    SD.check_stage_and_capacity(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_ids_outside_the_vocabulary(dec, table):
    SD.check_outside_ids(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_arguments(dec, table):
    SD.check_arguments(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_capacity_on_every_route(dec, table):
    SD.check_capacity(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_agreement_with_the_batch_entries(dec, table):
    SD.check_agreement(*dec(table), n_lists=60, longest=SD.MAX_IDS)


@pytest.mark.parametrize("table", SD.TABLES)
def test_reuse_and_interleaved_encode_calls(dec, table):
    SD.check_reuse(*dec(table))


@pytest.mark.parametrize("table", SD.TABLES)
def test_two_threads_share_one_encoder(dec, table):
    SD.check_threads(*dec(table), rounds=40)


def test_python_mirror(lib, vocab_bytes, dec):
    SD.check_python_mirror(lib, vocab_bytes("gpt2"), dec("dense")[1])
