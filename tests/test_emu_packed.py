"""`not gpu`: packed rows (tkz_encode_batch_packed_device / _utf8 / _utf16; k_pack_count, k_pack_write) -- the real kernel sources on the CPU emulator
(tests/hostemu/), exact against the rule of tkz.h applied to the oracle's ids (tests/packed_cases.py).  tests/test_gpu_packed.py runs the same cases on the
hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import emu
import packed_cases as PK
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
        return PK.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    assert re.search(r"\bkPackTile = %d\b" % PK.K, open(os.path.join(src, "tkz_kernels.h")).read())
    # the section lies behind the trim kernels and in front of the batch decoder; plain C++ and the helpers of tkz_simt.h
    first, last = text.index("// Packed rows (tkz_encode_batch_packed_device"), text.index("// Decode for a batch")
    assert text.index("void k_trim_gather(") < first < last < text.index("// Token-budget chunks (tkz_encode_batch_chunks_device)")
    body = text[first:last]
    assert "asm" not in body and "atomic" not in body and "TKZ_SHARED" not in body and "fence" not in body and "__builtin" not in body
    assert body.count("TKZ_KERNEL(256) void k_pack_") == 2 and body.count("tkz_pack_tiles<") == 2 + 1      # ONE body, instantiated twice
    assert "tkz_load_nt(" in body and "tkz_store_nt(" in body


def test_framing_forms(ctx):
    PK.check_framing(ctx)


def test_row_lengths(ctx):
    PK.check_row_lengths(ctx)


def test_tile_edges(ctx):
    PK.check_tile_edges(ctx)


def test_more_tiles_than_the_grid_has_wavefronts(ctx, lib):
    PK.check_grid_stride(ctx, lib)


def test_coincidence_of_document_and_row_starts(ctx):
    PK.check_coincidence(ctx)


def test_special_tokens(make):
    PK.check_special(make)


def test_capacity_and_argument_errors(make):
    PK.check_capacity(make)


def test_agreement_of_the_entries(make, lib):
    PK.check_agreement(make, lib)


def test_an_attempt_run_again(make):
    PK.check_retry(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    PK.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
