"""`not gpu`: pair rows (tkz_encode_batch_pairs_device / _utf8 / _utf16; k_pair_lens, k_pair_write) -- the real kernel sources on the CPU emulator
(tests/hostemu/), exact against the rule of tkz.h applied to the oracle's ids (tests/pairs_cases.py).  tests/test_gpu_pairs.py runs the same cases on the
hardware, on gpt2 and on synth100k."""
import os
import re

import pytest

import emu
import pairs_cases as PR
from conftest import ROOT
from tokenizer_amd import _native as N

BANNER = "// Pair rows (tkz_encode_batch_pairs_device"
NEXT = "// Token-budget buckets (tkz_encode_batch_budgeted_device"


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def raw(vocab_bytes):
    return vocab_bytes("gpt2")


@pytest.fixture(scope="module")
def make(lib, oracle_mod, raw):
    def make_ctx(specials=None, pattern=N.CL100K, options=(), vocab=None):
        return PR.Ctx(lib, oracle_mod, vocab or raw, pattern, specials, options=options)
    return make_ctx


@pytest.fixture(scope="module")
def ctx(make):
    return make()


def test_the_kernel_text():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    text = open(os.path.join(src, "tkz_kernels.hip")).read()
    head = open(os.path.join(src, "tkz_kernels.h")).read()
    assert re.search(r"\bkPairTile = %d\b" % PR.K, head) and re.search(r"\bkPairGridMax = %d\b" % PR.GRID, head) and PR.K % 64 == 0
    # the section stands between the launchers and the budgeted section: no older test's window of the file holds it
    first = text.index(BANNER)
    assert text.count(BANNER) == 1 and text.index("void launch_corpus(") < first < text.index(NEXT)
    body = text[first:text.index(NEXT)]
    # plain C++ and the helpers of tkz_simt.h: nothing is added up in memory, the one barrier orders the four partial results of a workgroup
    assert "asm" not in body and "atomic" not in body and "fence" not in body and "__builtin" not in body and body.count("simt::sync()") == 1
    assert body.count("TKZ_KERNEL(256) void k_pair_") == 2 and "tkz_load_nt(" in body and body.count("tkz_store_nt(") >= 4
    assert "TKZ_DEV int tkz_pad_wave_max(int v);" in body and "TKZ_DEV int64_t tkz_pad_wave_sum(int64_t v);" in body      # the shuffles of k_pad_lens: declared, not copied
    write = body[body.index("void k_pair_write("):body.index("void launch_pairs(")]
    assert "K.offs" not in write and "K.strategy" not in write and "K.cut_side" not in write      # the rows come from lens, ka and the two sources
    assert write.count(" / W") == 2                            # row and column of a tile's first position, and the capacity: nothing is divided per position
    assert "K.out + q" in write and "K.ids + s" in write and "s < K.ids_cap" in write


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "tkz.h")).read()
    block = text[text.index("/* ---- Pair rows"):text.index("void tkz_encoder_pairs_calls(")]
    for needle in ("THE RULE", "TKZ_PAIR_LONGEST_FIRST = 0, TKZ_PAIR_ONLY_FIRST = 1, TKZ_PAIR_ONLY_SECOND = 2", "C a1 a2 a3 S b1 b2 E / C S d1 E P P P P", "3 2 0 1",
                   "00000111 / 00110000", "C a3 a4 a5 S b2 b3 E", "C a1 a2 S b1 b2 b3 E", "C a1 a2 a3 a4 a5 S E", "00000001", "from the SECOND on a tie",
                   "ka = min(a, max(H, R - b)), kb = min(b, max(h, R - a))", "NEVER the uncut ids", "n_pairs * L entries ALWAYS suffice"):
        assert needle in block, needle


def test_the_header_example():
    """the rows of tkz.h's example, from the model"""
    a, b, d = [11, 12, 13, 14, 15], [21, 22, 23], [31]
    Cc, S, E, P = 1, 2, 3, 0
    m = PR.Model([a, b, [], d], 8, Cc, S, 1, E, P)
    assert (m.W, m.lens, m.n_cut, m.kept) == (8, [8, 4], 1, [3, 2, 0, 1])
    assert m.ids.tolist() == [[Cc, 11, 12, 13, S, 21, 22, E], [Cc, S, 31, E, P, P, P, P]] and m.types.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 0, 0, 0, 0]]
    assert PR.Model([a, b, [], d], 8, Cc, S, 1, E, P, cut=PR.PREFIX).ids[0].tolist() == [Cc, 13, 14, 15, S, 22, 23, E]
    assert PR.Model([a, b, [], d], 8, Cc, S, 1, E, P, PR.ONLY_FIRST).ids[0].tolist() == [Cc, 11, 12, S, 21, 22, 23, E]
    m = PR.Model([a, b, [], d], 8, Cc, S, 1, E, P, PR.ONLY_SECOND)
    assert m.ids[0].tolist() == [Cc, 11, 12, 13, 14, 15, S, E] and m.types[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]


def test_the_closed_forms():
    PR.check_closed_form()


def test_the_header_example_on_the_kernels(ctx):
    import random
    rng = random.Random(1)
    docs = [PR.words(rng, 5), PR.words(rng, 3), b"", PR.words(rng, 1)]
    for strategy, kept in ((PR.LONGEST, [3, 2, 0, 1]), (PR.ONLY_FIRST, [2, 3, 0, 1]), (PR.ONLY_SECOND, [5, 0, 0, 1])):
        m = PR.check_device(ctx, docs, 8, "the header's example", 1, 2, 1, 3, pad=0, strategy=strategy)
        assert (m.W, m.lens, m.n_cut, m.kept) == (8, [8, 4], 1, kept)


def test_strategy_edges(ctx):
    PR.check_strategy_edges(ctx)


def test_type_ids_and_null_arrays(ctx):
    PR.check_types_and_nulls(ctx)


def test_width(ctx):
    PR.check_width(ctx)


def test_tile_row_and_seam_geometry(ctx):
    PR.check_geometry(ctx)


def test_more_tiles_and_pairs_than_the_grids_hold(ctx, lib):
    PR.check_grid_stride(ctx, lib)


def test_special_tokens(make):
    PR.check_special(make)


def test_capacity_and_argument_errors(make):
    PR.check_capacity(make)


def test_agreement_of_the_entries(make, lib):
    PR.check_agreement(make, lib)


def test_an_attempt_run_again(make):
    PR.check_retry(make)


def test_python_mirror(lib, oracle_mod, raw, lib_rs_bytes):
    PR.check_python_mirror(lib, oracle_mod, raw, lib_rs_bytes.decode("utf-8"))
