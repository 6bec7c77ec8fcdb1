"""`not gpu`: length-bucketed padded rows (tkz_encode_batch_bucketed_device / _utf8 / _utf16; k_bkt_hist, k_bkt_scatter, k_bkt_table, k_bkt_write) -- the real
kernel sources on the CPU emulator (tests/hostemu/), exact against the rule of tkz.h applied to the oracle's ids (tests/bucketed_cases.py).
tests/test_gpu_bucketed.py runs the same cases on the hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import bucketed_cases as BK
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
        return BK.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    head = open(os.path.join(src, "tkz_kernels.h")).read()
    assert re.search(r"\bkBktSortTile = %d\b" % BK.T, head) and re.search(r"\bkBktTile = %d\b" % BK.K, head) and BK.T % 256 == 0 and BK.K % 64 == 0
    # the section lies between the launchers and the padded rows' section, which the padded tests read to the end of the file
    first, end = text.index("// Length-bucketed padded rows (tkz_encode_batch_bucketed_device"), text.index("// Padded rows (tkz_encode_batch_padded_device")
    assert text.index("void launch_corpus(") < first < end and text.count("// Length-bucketed padded rows (tkz_encode_batch_bucketed_device") == 1
    body = text[first:end]
    # plain C++ and the helpers of tkz_simt.h; nothing is added up in memory: the sort's ranks come from ballots and three barriers a tile
    assert "asm" not in body and "atomic" not in body and "fence" not in body and "__builtin" not in body and "rocprim" not in body and "hipcub" not in body
    assert body.count("TKZ_KERNEL(256) void k_bkt_") == 4 and body.count("simt::sync()") == 3 and "simt::ballot(" in body
    assert "TKZ_KERNEL(256) void k_pad_lens(PadParams K);" in body              # k_pad_lens is reused as it is: declared here, defined in its own section
    write = body[body.index("void k_bkt_write("):body.index("int bkt_passes(")]
    assert "tkz_load_nt(" in write and write.count("tkz_store_nt(") == 3 and write.count("tkz_last_le(") == 1      # one search a tile, none a lane
    # two constants (wavefronts a workgroup), the tile count and the row of a tile's first position: nothing is divided per position
    assert write.count(" / ") == 4 and write.count("kThreads / 64") == 2 and write.count(" / (int64_t)s.W") == 1 and " % " not in write
    assert "Q.offs" not in write and "Q.cut_side" not in write      # the rows come from order, lens and src
    step = body[body.index("void tkz_bkt_step("):body.index("void k_bkt_write(")]
    assert step.count(" / s.W") == 1 and step.count(" % s.W") == 1      # ... and one 32-bit division where a lane enters a bucket narrower than 64 columns


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "tkz.h")).read()
    block = text[text.index("/* ---- Length-bucketed padded rows"):text.index("void tkz_encoder_bucketed_calls(")]
    for needle in ("THE RULE", "TKZ_BUCKET_ASCENDING = 0, TKZ_BUCKET_DESCENDING = 1", "1 <= B <= 2^31 - 1", 'numpy.argsort(len, kind="stable")', 'numpy.argsort(-len, kind="stable")',
                   "ascending\n *     document index in BOTH directions", "rank[order[r]] = r", "n_buckets = ceil(n_docs / B)", "W_b = min(L, ceil(maxlen_b / M) * M)",
                   "W_b = 0 when maxlen_b == 0", "the last entry is P", "out[bucket_offsets[b] + i * W_b .. + W_b)", "stay in DOCUMENT order",
                   "order 1, 2, 4, 0, 3; rank 3, 0, 1, 4, 2; widths 3, 4, 4; bucket offsets 0, 6, 14, 18; P = 18", "X P P / c1 c2 X | e1 e2 X P / a1 a2 a3 X | d1 d2 d3 X",
                   "order 0, 3, 2, 4, 1; rank 0, 4, 2, 1, 3; widths 4, 3, 1; bucket offsets 0, 8, 14, 15; P = 15", "a1 a2 a3 X / d1 d2 d3 X | c1 c2 X / e1 e2 X | X",
                   "writes 20 positions", "TKZ_E_CAPACITY when out_cap < P", "n_docs * L entries ALWAYS suffice", "NEVER the uncut ids", "TOKEN budget",
                   "no _begin / _end form", "no single-text form", "no device-resident UTF-16"):
        assert needle in block, needle


def test_the_worked_example(ctx):
    BK.check_worked_example(ctx)


def test_stability_and_ties(ctx):
    BK.check_ties(ctx)


def test_documents_around_the_sort_tile(ctx):
    BK.check_sort_tiles(ctx)


def test_digits(ctx):
    BK.check_digits(ctx)


def test_more_documents_and_tiles_than_the_grids_hold(ctx, lib):
    BK.check_grid_stride(ctx, lib)


def test_buckets(ctx):
    BK.check_buckets(ctx)


def test_the_writer_geometry(ctx):
    BK.check_geometry(ctx)


def test_special_tokens(make):
    BK.check_special(make)


def test_capacity_and_argument_errors(make):
    BK.check_capacity(make)


def test_agreement_of_the_entries(make, lib):
    BK.check_agreement(make, lib)


def test_an_attempt_run_again(make):
    BK.check_retry(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    BK.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
