"""`not gpu`: count calls (tkz_count_batch_device / _utf8 / _utf16, tkz_count_utf8 / _utf16; k_tokcount) -- the real kernel sources on the CPU emulator
(tests/hostemu/), exact against the oracle's token counts and, entry for entry, against the offsets of the encode entries.
tests/test_gpu_count.py runs the same cases on the hardware, every one on gpt2 and on synth100k."""
import os
import re
import subprocess
import sys

import pytest

import count_cases as CC
import emu
from conftest import ROOT
from tokenizer_amd import _native as N


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def raw(vocab_bytes):
    return vocab_bytes("gpt2")


@pytest.fixture(scope="module")
def make(lib, oracle_mod, raw):
    def make_ctx(specials=None, pattern=N.CL100K, options=(), vocab=None):
        return CC.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_constants_and_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.h")).read() + open(os.path.join(src, "tkz_kernels.hip")).read()
    assert re.search(r"\bkSub = %d\b" % CC.SUB, text) and re.search(r"\bkCountSlots = %d\b" % CC.SLOTS, text)
    body = text[text.index("void k_tokcount("):text.index("// giant pieces (")]
    # the count form stores the marks' positions and nothing else: no atomics, no fence, no id buffer, none of the token arrays
    assert "atomic" not in body and "fence" not in body and "asm" not in body
    for name in ("P.mquad", "P.dense", "P.tmp", "P.promo[", "out_cap", "tile_base"):
        assert name not in body, name
    assert body.count("P.doc_tok[") == 2 and body.count("tkz_attempt_failed(P)") == 1


def test_marks_and_skipped_sub_tiles(ctx):
    CC.check_marks(ctx)


def test_more_than_256_records_a_sub_tile(ctx):
    CC.check_many_records(ctx)


def test_answers_in_and_beyond_lds(make):
    CC.check_lists(make())


def test_long_token_runs(lib, oracle_mod):
    CC.check_token_runs(CC.byte_table(lib, oracle_mod))


def test_giant_pieces(ctx):
    CC.check_giant(ctx)


def test_promoted_pieces(make):
    CC.check_promoted(make())


def test_retry_on_a_fresh_encoder(make):
    CC.check_retry(make)


def test_special_tokens(make):
    CC.check_special(make)


@pytest.mark.parametrize("pattern,vocab,options", [(N.P1, "gpt2", ()), (N.CL100K, "synth100k", ()), (N.O200K, "synth200k", ()), (N.O200K_DOTNET, "synth200k", ()),
                                                   (N.O200K, "synth200k", ((N.OPT_PRETOK_SEQUENTIAL, 1),))])
def test_patterns(make, vocab_bytes, pattern, vocab, options):
    CC.check_patterns(make(pattern=pattern, vocab=vocab_bytes(vocab), options=options))


def test_host_entries(make):
    CC.check_host(make)


def test_host_count_calls_allocate_no_id_staging(make):
    CC.check_no_id_staging(make)


def test_host_call_of_several_chunks():
    """the chunk size is read once per process: a child interpreter with 4 KiB chunks"""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gzip, emu, count_cases as CC\n"
            "from tokenizer_amd import _native as N\n"
            "from oracle import oracle as O\n"
            "O.build()\n"
            "raw = gzip.decompress(open(%r, 'rb').read())\n"
            "lib = emu.library()\n"
            "enc = N.Encoder(N.Vocab(raw, lib), N.CL100K)\n"
            "print('CHUNKS_OK', CC.check_chunks(enc, O, O.Vocab(raw), N.CL100K))\n") % (ROOT, tests, os.path.join(tests, "golden", "gpt2.tiktoken.gz"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TKZ_HOST_CHUNK_BYTES="4096"), capture_output=True, text=True, timeout=600)
    assert "CHUNKS_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_single_text_entries(make):
    CC.check_single(make)


def test_single_text_entries_o200k(make, vocab_bytes):
    CC.check_single(lambda specials: make(specials, pattern=N.O200K, vocab=vocab_bytes("synth200k")), lengths=(1024, 1025))


def test_arguments(ctx, lib, oracle_mod, raw):
    CC.check_arguments(ctx, lib, oracle_mod, raw)


def test_two_threads_share_one_encoder(make):
    CC.check_threads(make)


def test_python_mirror(lib, raw, lib_rs_bytes):
    CC.check_python_mirror(lib, raw, lib_rs_bytes.decode("utf-8"))
