"""`not gpu`: the marks' ordinals in k_docoffs (the document index when k_docmark saw no empty document, the search of the bitmap otherwise;
tests/docmark_cases.py) -- the real kernel sources on the CPU emulator (tests/hostemu/), ids and offsets against the oracle.
tests/test_gpu_docmarks.py runs the same cases on the hardware."""
import os
import re

import pytest

import docmark_cases as DC
import emu
from conftest import ROOT
from tokenizer_amd import _native as N


@pytest.fixture(scope="module")
def make(oracle_mod, vocab_bytes):
    def make_ctx(specials=None, options=()):
        return DC.Ctx(emu.library(), oracle_mod, vocab_bytes("gpt2"), N.CL100K, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    assert re.search(r"\bkSub = %d\b" % DC.SUB, open(os.path.join(src, "tkz_kernels.h")).read())
    mark = text[text.index("void k_docmark("):text.index("// k_pretok_rows")]
    offs = text[text.index("void k_docoffs("):text.index("void k_case_equiv_fix(")]
    # the record is a plain store (one atomic in k_docmark: the error bit), and the path without empty documents stands in front of every bitmap load
    assert mark.count("simt::atomic") == 1 and "*has_empty = 1" in mark
    assert offs.index("if (!search)") < offs.index("docord_base[sub]") < offs.index("docbits[w]")
    api = open(os.path.join(src, "tkz_api.cpp")).read()
    block = api[api.index("struct CounterBlock {"):api.index("struct LenCounters")]
    assert re.search(r"\n\s*int32_t has_empty, pad_;[^\n]*\n\};", block), "the last field: a re-run's fill ends in front of it"
    assert "hipMemsetAsync(ws->w_zero.p, 0, kCountersRerun, stream)" in api


def test_no_empty_document(ctx):
    DC.check_dense(ctx)


def test_empty_documents(ctx):
    DC.check_empty(ctx)


def test_the_record_does_not_leak(ctx):
    DC.check_flag_does_not_leak(ctx)


def test_stale_bitmap(make):
    DC.check_stale_bitmap(make())


@pytest.mark.parametrize("with_empty", [False, True], ids=["no-empty", "empty"])
def test_thrown_away_attempt(make, with_empty):
    DC.check_thrown_away_attempt(make, with_empty)


def test_count_entry(ctx):
    DC.check_count_entry(ctx)


def test_special_entry(make):
    DC.check_special_entry(make)
