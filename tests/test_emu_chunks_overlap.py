"""`not gpu`: overlapping token-budget chunks (tkz_encode_batch_chunks_overlap_device / _utf8 / _utf16, tkz_encode_chunks_overlap_utf8 / _utf16; k_chunkov_walk,
k_chunkov_walk_long, k_chunkov_units) -- the real kernel sources on the CPU emulator (tests/hostemu/), exact against the rule of tkz.h over the oracle's items and,
on small cases, against the caller's own loop over EncodeTrimSuffix and EncodeTrimPrefix (tests/chunk_overlap_cases.py).  tests/test_gpu_chunks_overlap.py runs the
same cases on the hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import chunk_cases as CK
import chunk_overlap_cases as CO
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


def test_the_rule_by_brute_force():
    fbs, worst = CO.check_rule_properties()
    assert fbs == 209911 and worst < 1.0


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    # a section of its own behind the span kernels: the chunk section keeps its four kernels, the new walks and the unit kernel have names of their own
    first, last = text.index("// Overlapping token-budget chunks (tkz_encode_batch_chunks_overlap_device)"), text.index("// k_small: the WHOLE launch sequence")
    assert text.index("void k_tokspan_write(") < first < last
    body = text[first:last]
    assert "asm" not in body and "TKZ_SHARED" not in body and "fence" not in body and "__builtin" not in body
    assert sorted(re.findall(r"TKZ_KERNEL\(256\) void (\w+)\(", body)) == ["k_chunkov_units", "k_chunkov_walk", "k_chunkov_walk_long"]
    # the unit rule and the end of a chunk are the chunk section's: neither is written out a second time
    assert "0xC0" not in body and "0xF0" not in body and "tkz_chunk_units_before(" in body and "tkz_chunk_end(" in body
    assert "k_chunkov" not in text[text.index("// Token-budget chunks (tkz_encode_batch_chunks_device)"):text.index("// Token spans (tkz_encode_batch_spans_device)")]


def test_document_sizes_and_small_budgets(ctx):
    CO.check_sizes(ctx)


def test_clamp_and_adds_nothing(ctx):
    CO.check_fallback(ctx)


def test_oversize_items(ctx):
    CO.check_oversize(ctx)


def test_special_tokens(make):
    CO.check_special(make)


@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_units_and_ends(make, pattern):
    CO.check_units(make(pattern=pattern))


def test_search_widths(ctx):
    CO.check_widths(ctx)


def test_workgroup_edges(ctx):
    CO.check_workgroup_edges(ctx)


def test_long_document_form(ctx):
    CO.check_long_form(ctx)


def test_one_document_beyond_the_piece_stride(ctx):
    CO.check_stride(ctx)


def test_capacity_and_argument_errors(make):
    CO.check_errors(make)


def test_agreement_of_the_entries(make):
    CO.check_agreement(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    CO.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
