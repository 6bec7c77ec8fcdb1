"""`not gpu`: token-budget chunks (tkz_encode_batch_chunks_device / _utf8 / _utf16, tkz_encode_chunks_utf8 / _utf16; k_chunk_walk, k_chunk_walk_long,
k_chunk_unitcount, k_chunk_units) -- the real kernel sources on the CPU emulator (tests/hostemu/), exact against the caller's own EncodeTrimSuffix loop and against
the rule of tkz.h over the oracle's pieces (tests/chunk_cases.py).  tests/test_gpu_chunks.py runs the same cases on the hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import chunk_cases as CK
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
        return CK.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    head = open(os.path.join(src, "tkz_kernels.h")).read()
    assert re.search(r"\bkChunkLongItems = %d\b" % CK.LONG, head) and re.search(r"\bkSub = %d\b" % CK.SUB, head)
    # the section lies behind the trim kernels and in front of the span helpers; plain C++ and the helpers of tkz_simt.h: no assembly, no LDS, no fence
    first, last = text.index("// Token-budget chunks (tkz_encode_batch_chunks_device)"), text.index("// Token spans (tkz_encode_batch_spans_device)")
    assert text.index("void k_trim_gather(") < first < last < text.index("TKZ_DEV uint32_t tkz_span_bits16(")
    body = text[first:last]
    assert "asm" not in body and "TKZ_SHARED" not in body and "fence" not in body and "__builtin" not in body
    assert body.count("TKZ_KERNEL(256) void k_chunk_") == 4
    # the counting rule is the span helpers': it is not written out a second time
    assert "0xC0" not in body and "0xF0" not in body and "tkz_span_units16(" in body


def test_document_sizes_and_small_budgets(ctx):
    CK.check_sizes(ctx)


def test_oversize_items(ctx):
    CK.check_oversize(ctx)


def test_special_tokens(make):
    CK.check_special(make)


@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_units_at_sub_tile_edges(make, pattern):
    CK.check_units(make(pattern=pattern))


def test_search_widths(ctx):
    CK.check_widths(ctx)


def test_workgroup_edges(ctx):
    CK.check_workgroup_edges(ctx)


def test_long_document_form(ctx):
    CK.check_long_form(ctx)


def test_one_document_beyond_the_piece_stride(ctx):
    CK.check_stride(ctx)


def test_capacity_and_argument_errors(make):
    CK.check_errors(make)


def test_agreement_of_the_entries(make):
    CK.check_agreement(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    CK.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
