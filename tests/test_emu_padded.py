"""`not gpu`: padded rows (tkz_encode_batch_padded_device / _utf8 / _utf16; k_pad_lens, k_pad_write) -- the real kernel sources on the CPU emulator
(tests/hostemu/), exact against the rule of tkz.h applied to the oracle's ids (tests/padded_cases.py).  tests/test_gpu_padded.py runs the same cases on the
hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import emu
import padded_cases as PD
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
        return PD.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    head = open(os.path.join(src, "tkz_kernels.h")).read()
    assert re.search(r"\bkPadTile = %d\b" % PD.K, head) and re.search(r"\bkPadGridMax = %d\b" % PD.GRID, head) and PD.K % 64 == 0
    # the section is the last of the file, behind the launchers: no older test's window of the file holds it
    first = text.index("// Padded rows (tkz_encode_batch_padded_device")
    assert text.index("void launch_corpus(") < first and text.count("// Padded rows (tkz_encode_batch_padded_device") == 1
    body = text[first:]
    # plain C++ and the helpers of tkz_simt.h: nothing is added up in memory, the one barrier orders the four partial results of a workgroup
    assert "asm" not in body and "atomic" not in body and "fence" not in body and "__builtin" not in body and body.count("simt::sync()") == 1
    assert body.count("TKZ_KERNEL(256) void k_pad_") == 2 and "tkz_load_nt(" in body and body.count("tkz_store_nt(") >= 3
    write = body[body.index("void k_pad_write("):body.index("void launch_pad(")]
    assert "K.offs" not in write and "K.max_len" in write and "K.cut_side" not in write      # the rows come from lens and src, not from the offsets
    assert write.count(" / W") == 2                            # row and column of a tile's first position, and the capacity: nothing is divided per position


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "tkz.h")).read()
    block = text[text.index("/* ---- Padded rows"):text.index("void tkz_encoder_padded_calls(")]
    for needle in ("THE RULE", "TKZ_PAD_RIGHT = 0, TKZ_PAD_LEFT = 1", "B a1 a2 a3 / B P P P / B c1 c2 P", "B a3 a4 a5 / P P P B / P B c1 c2", "0 1 2 3 / 0 0 0 0 / 0 0 1 2",
                   "NOT the reference's whole-item cut", "NEVER the uncut ids", "n_docs * L entries ALWAYS suffice"):
        assert needle in block, needle


def test_cut_edges(ctx):
    PD.check_cut_edges(ctx)


def test_width(ctx):
    PD.check_width(ctx)


def test_tile_and_row_geometry(ctx):
    PD.check_geometry(ctx)


def test_more_tiles_and_documents_than_the_grids_hold(ctx, lib):
    PD.check_grid_stride(ctx, lib)


def test_special_tokens(make):
    PD.check_special(make)


def test_capacity_and_argument_errors(make):
    PD.check_capacity(make)


def test_agreement_of_the_entries(make, lib):
    PD.check_agreement(make, lib)


def test_an_attempt_run_again(make):
    PD.check_retry(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    PD.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
