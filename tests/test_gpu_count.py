"""`-m gpu`: count calls through libtkz.so (tkz_count_batch_device / _utf8 / _utf16, tkz_count_utf8 / _utf16; k_tokcount), exact against the oracle's token counts
and, entry for entry, against the offsets of the encode entries: the cases of tests/test_emu_count.py, every one on gpt2 and on synth100k."""
import os
import subprocess
import sys

import pytest

import count_cases as CC
from conftest import ROOT
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
            return CC.Ctx(lib, oracle_mod, vocab or vocab_bytes(table), pattern, specials, upload=upload, options=options)
        return make_ctx
    return for_table


@pytest.mark.parametrize("table", TABLES)
def test_marks_and_skipped_sub_tiles(maker, table):
    CC.check_marks(maker(table)())


@pytest.mark.parametrize("table", TABLES)
def test_more_than_256_records_a_sub_tile(maker, table):
    CC.check_many_records(maker(table)())


@pytest.mark.parametrize("table", TABLES)
def test_answers_in_and_beyond_lds(maker, table):
    CC.check_lists(maker(table)())


def test_long_token_runs(lib, oracle_mod, upload):
    CC.check_token_runs(CC.byte_table(lib, oracle_mod, upload))


@pytest.mark.parametrize("table", TABLES)
def test_giant_pieces(maker, table):
    CC.check_giant(maker(table)())


@pytest.mark.parametrize("table", TABLES)
def test_promoted_pieces(maker, table):
    CC.check_promoted(maker(table)())


@pytest.mark.parametrize("table", TABLES)
def test_retry_on_a_fresh_encoder(maker, table):
    CC.check_retry(maker(table))


@pytest.mark.parametrize("table", TABLES)
def test_special_tokens(maker, table):
    CC.check_special(maker(table))


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("pattern,options", [(N.P1, ()), (N.CL100K, ()), (N.O200K, ()), (N.O200K_DOTNET, ()), (N.O200K, ((N.OPT_PRETOK_SEQUENTIAL, 1),))])
def test_patterns(maker, table, pattern, options):
    CC.check_patterns(maker(table)(pattern=pattern, options=options))


@pytest.mark.parametrize("table", TABLES)
def test_host_entries(maker, table):
    CC.check_host(maker(table))


@pytest.mark.parametrize("table", TABLES)
def test_host_count_calls_allocate_no_id_staging(maker, table):
    CC.check_no_id_staging(maker(table))


@pytest.mark.parametrize("table", TABLES)
def test_host_call_of_several_chunks(table):
    """the chunk size is read once per process: a child interpreter with 4 KiB chunks"""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import conftest, gzip, count_cases as CC\n"
            "from tokenizer_amd import _native as N\n"
            "from oracle import oracle as O\n"
            "O.build()\n"
            "raw = gzip.decompress(open(%r, 'rb').read())\n"
            "enc = N.Encoder(N.Vocab(raw), N.CL100K)\n"
            "print('CHUNKS_OK', CC.check_chunks(enc, O, O.Vocab(raw), N.CL100K))\n") % (ROOT, tests, os.path.join(tests, "golden", table + ".tiktoken.gz"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TKZ_HOST_CHUNK_BYTES="4096"), capture_output=True, text=True, timeout=300)
    assert "CHUNKS_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("table", TABLES)
def test_single_text_entries(maker, table):
    CC.check_single(maker(table))


@pytest.mark.parametrize("table", TABLES)
def test_single_text_entries_o200k(maker, table):
    CC.check_single(lambda specials: maker(table)(specials, pattern=N.O200K), lengths=(1024, 1025))


@pytest.mark.parametrize("table", TABLES)
def test_arguments(maker, table, lib, oracle_mod, vocab_bytes):
    CC.check_arguments(maker(table)(), lib, oracle_mod, vocab_bytes(table))


@pytest.mark.parametrize("table", TABLES)
def test_two_threads_share_one_encoder(maker, table):
    CC.check_threads(maker(table), rounds=6)


def test_python_mirror(lib, vocab_bytes, lib_rs_bytes):
    CC.check_python_mirror(lib, vocab_bytes("gpt2"), lib_rs_bytes.decode("utf-8"))
