"""`not gpu`: the rank-width forms of the merge kernels at their thresholds (tests/rank_band_cases.py) -- the real kernel sources on the CPU emulator
(tests/hostemu/), exact against the oracle's literal loop.  One side of every threshold here (rank_band_cases.MAIN_TOPS: the compact lane forms over a wide
pair table, tkz_bpe_lane_var<true>, <false>, kPromoFlag, TKZ_MAX_RANK), both sides on the GPU (tests/test_gpu_rank_bands.py), where the two very long pieces
run as well: the emulator runs one workgroup at a time.  The promotion gate runs here too, on both sides of kPromoFlag.
No kernel: the header constants against this module's numbers, the band tables' own conditions, the rejection edge of the loader."""
import pytest

import emu
import rank_band_cases as RB

# the forms NO earlier test reaches: the compact lane forms over a wide pair table, tkz_bpe_lane_var<true>, the 27-bit edge (tkz_bpe_lane_var<false> at
# 2^22 - 1 and 2^26 is what parity.check_random_vocab's sparse tables run already; the pieces under those two tops are the GPU module's)
EMU_PIECE_TOPS = (RB.PAIR_CID_LIMIT, RB.VAR_COMPACT_MAX_RANK + 1, RB.MAX_RANK)
EMU_PSEUDO_TOPS = (RB.PAIR_CID_LIMIT - 1, RB.VAR_COMPACT_MAX_RANK + 1, RB.MAX_RANK)          # compact pair entries | tkz_bpe_lane_var<true> | the 27-bit edge
EMU_RANDOM_PSEUDO_TOPS = (RB.VAR_COMPACT_MAX_RANK + 1,)      # (a refusal a call: half a minute a table here)
EMU_BATCH_TOPS = tuple(t for t in RB.MAIN_TOPS if t != RB.VAR_PACKED_MAX_RANK + 1)       # (a quarter of a minute a batch here; all five on the GPU)
EMU_BATCH_BYTES = 200_000


@pytest.fixture(scope="module")
def lib():
    return emu.library()


def test_header_constants():
    """The pins move with the constants: an edit of a threshold in the headers alone fails here, before a case silently tests the wrong side of it."""
    assert RB.header_constants() == RB.module_constants()
    assert sorted(RB.TOPS) == sorted({t + d for t in (RB.PAIR_CID_LIMIT - 1, RB.VAR_COMPACT_MAX_RANK, RB.VAR_PACKED_MAX_RANK, RB.PROMO_FLAG - 1) for d in (0, 1)}
                                     | {RB.MAX_RANK})
    assert RB.OVERFLOW_TOPS == (RB.VAR_COMPACT_MAX_RANK + 2, RB.VAR_PACKED_MAX_RANK + 2)
    assert set(RB.MAIN_TOPS) <= set(RB.TOPS) and set(RB.PSEUDO_TOPS) <= set(RB.TOPS) and set(EMU_PSEUDO_TOPS) <= set(RB.PSEUDO_TOPS) and set(EMU_PIECE_TOPS) <= set(RB.MAIN_TOPS)


@pytest.mark.parametrize("top", RB.TOPS + RB.OVERFLOW_TOPS)
def test_band_tables(oracle_mod, top):
    RB.check_band_table(oracle_mod, top)
    if top in RB.PSEUDO_TOPS:
        RB.check_band_table(oracle_mod, top, drop=b"b")


def test_rejection_edge(lib, oracle_mod):
    RB.check_rejection_edge(lib, oracle_mod)


@pytest.mark.parametrize("latency", RB.LATENCY_FORMS)
@pytest.mark.parametrize("top", EMU_PIECE_TOPS)
def test_pieces(lib, oracle_mod, monkeypatch, top, latency):
    monkeypatch.setenv("TKZ_LATENCY_BYTES", latency)
    RB.check_pieces(lib, oracle_mod, top)


@pytest.mark.parametrize("top", EMU_RANDOM_PSEUDO_TOPS)
def test_pseudo_ids(lib, oracle_mod, top):
    RB.check_pseudo(lib, oracle_mod, top)


@pytest.mark.parametrize("top,latency", list(zip(RB.OVERFLOW_TOPS, RB.LATENCY_FORMS)))
def test_pieces_beyond_the_packed_keys(lib, oracle_mod, monkeypatch, top, latency):
    """2^21 and 2^22: the first ranks a compact / a packed key cannot hold (a long-miss form each here, both on the GPU)."""
    monkeypatch.setenv("TKZ_LATENCY_BYTES", latency)
    RB.check_pieces(lib, oracle_mod, top)


@pytest.mark.parametrize("top", EMU_PSEUDO_TOPS)
def test_pseudo_ids_swallowed(lib, oracle_mod, top):
    RB.check_pseudo_swallowed(lib, oracle_mod, top)


@pytest.mark.parametrize("top", EMU_PSEUDO_TOPS)
def test_pseudo_id_survives_beside_the_memo(lib, oracle_mod, top):
    RB.check_pseudo_survives_memo(lib, oracle_mod, top)


@pytest.mark.parametrize("top", (RB.VAR_COMPACT_MAX_RANK, RB.VAR_COMPACT_MAX_RANK + 1))
def test_rank_equal_to_a_compact_pseudo_id(lib, oracle_mod, top):
    RB.check_pseudo_id_collision(lib, oracle_mod, top)


@pytest.mark.parametrize("top", RB.MAIN_TOPS)
def test_single_launch(lib, oracle_mod, top):
    RB.check_single_launch(lib, oracle_mod, top)


@pytest.mark.parametrize("top", EMU_BATCH_TOPS)
def test_batch_sequence(lib, oracle_mod, top):
    RB.check_batch_sequence(lib, oracle_mod, top, n_docs=35, max_bytes=EMU_BATCH_BYTES)


@pytest.mark.parametrize("top", (RB.PROMO_FLAG - 1, RB.PROMO_FLAG))
def test_promotion_gate(lib, oracle_mod, top):
    RB.check_promotion_gate(lib, oracle_mod, top)
