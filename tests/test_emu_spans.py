"""`not gpu`: token spans (tkz_encode_batch_spans_device / _utf8 / _utf16, tkz_encode_spans_utf8 / _utf16; k_tokspan_mark, k_tokspan_count, k_tokspan_write) --
the real kernel sources on the CPU emulator (tests/hostemu/), exact against positions built from the oracle's ids and the rank file's key lengths
(tests/spans_cases.py).  tests/test_gpu_spans.py runs the same cases on the hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import emu
import spans_cases as SP
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
        return SP.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    assert re.search(r"\bkSub = %d\b" % SP.SUB, open(os.path.join(src, "tkz_kernels.h")).read())
    body = text[text.index("TKZ_DEV uint32_t tkz_span_bits16("):text.index("// k_small: the WHOLE launch sequence")]
    # plain C++ and the helpers of tkz_simt.h: no assembly, no LDS, no fence; the three kernels are 256-thread workgroups
    assert "asm" not in body and "TKZ_SHARED" not in body and "fence" not in body and "__builtin" not in body
    assert body.count("TKZ_KERNEL(256) void k_tokspan_") == 3


def test_placement_at_edges(ctx):
    SP.check_edges(ctx)


def test_every_source_of_a_piece_of_several_tokens(make):
    SP.check_sources(make)


def test_promoted_pieces(make):
    SP.check_promoted(make())


def test_sparse_decode_table(lib, oracle_mod):
    SP.check_sparse_table(lib, oracle_mod)


@pytest.mark.parametrize("vocab,pattern", [("gpt2", N.CL100K), ("synth200k", N.O200K)])
def test_key_lengths(make, vocab_bytes, vocab, pattern):
    SP.check_key_lengths(make(pattern=pattern, vocab=vocab_bytes(vocab)))


def test_ranks_of_2_21_and_more(lib, oracle_mod):
    """(synth200k's ranks end at 199,997: the table with ranks up to 2^22 is rank_band_cases')"""
    SP.check_rank_band(lib, oracle_mod)


def test_synth200k(make, vocab_bytes):
    SP.check_units(make(pattern=N.O200K, vocab=vocab_bytes("synth200k")))


def test_special_tokens(make):
    SP.check_special(make)


def test_special_tokens_utf16_with_a_replacement_literal(lib, oracle_mod, raw):
    SP.check_special_utf16(lib, oracle_mod, raw)


@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_units(make, pattern):
    SP.check_units(make(pattern=pattern))


def test_a_batch_beyond_the_piece_stride(ctx):
    SP.check_size(ctx)


def test_errors(make, lib, oracle_mod, raw):
    SP.check_errors(make, lib, oracle_mod, raw)


def test_agreement_with_the_special_piece_and_trim_entries(make):
    SP.check_agreement(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    SP.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
