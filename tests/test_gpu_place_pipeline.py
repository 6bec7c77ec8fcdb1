"""`-m gpu`: the load schedule of tkz_place_subtiles (answers and first records requested at a sub-tile's top, the next sub-tile's scalars while this one
is placed; tests/place_pipeline_cases.py) through libtkz.so on the hardware, ids and offsets against the oracle.
Every case runs as a batch small enough for the single launch (k_small places with the same code) and padded past it (k_place).  The cases of tests/test_emu_place_pipeline.py."""
import pytest

from tokenizer_amd import _native as N
import place_pipeline_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    return PC.Ctx(N.default_library(), oracle_mod)


PADDED = pytest.mark.parametrize("padded", [False, True], ids=["k_small", "k_place"])


@PADDED
def test_batch_sizes(ctx, padded):
    PC.check_sizes(ctx, padded)


@PADDED
def test_piece_counts(ctx, padded):
    PC.check_piece_counts(ctx, padded)


@pytest.mark.parametrize("padded,heavy", [(False, False), (True, False), (True, True)], ids=["k_small", "k_place-64", "k_place-128"])
def test_list_lengths(ctx, padded, heavy):
    PC.check_lists(ctx, padded, heavy)


@PADDED
def test_record_buffer_redo(ctx, padded):
    PC.check_record_buffer(ctx, padded)


@PADDED
def test_promoted_pieces(ctx, padded):
    PC.check_promoted(ctx, padded)


@PADDED
def test_cut_lists(ctx, padded):
    PC.check_cut_lists(ctx, padded)
