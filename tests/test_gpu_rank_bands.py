"""`-m gpu`: the rank-width forms of the merge kernels on both sides of every threshold (tests/rank_band_cases.py), exact against the oracle's literal loop:
  pieces of every length class under all nine band tables (and at 2^21 and 2^22, the first ranks the packed keys cannot hold), through both long-miss forms;
  tkz_bpe_long_tail's two very long pieces at 2^21 - 1 and 2^27 - 2
  pseudo ids (a table without the byte b) in the merge forms, the refusals one per call and inside a batch, the memo beside a refused piece
  the single launch and the multi-kernel sequence (twice: the second call answers from the memo), as UTF-16, and back through the sparse-id decode table
  the promotion gate on both sides of kPromoFlag
The emulator runs one side of every threshold (tests/test_emu_rank_bands.py), where the header constants, the tables' own conditions and the rejection edge are."""
import pytest

import rank_band_cases as RB
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu

TAIL_TOPS = (RB.VAR_COMPACT_MAX_RANK + 1, RB.MAX_RANK)
BATCH_DOCS = 300                                             # x 120 words: about 1.4 MB


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.mark.parametrize("latency", RB.LATENCY_FORMS)
@pytest.mark.parametrize("top", RB.TOPS + RB.OVERFLOW_TOPS)
def test_pieces(lib, oracle_mod, monkeypatch, top, latency):
    monkeypatch.setenv("TKZ_LATENCY_BYTES", latency)
    RB.check_pieces(lib, oracle_mod, top, with_tails=top in TAIL_TOPS)


@pytest.mark.parametrize("latency", RB.LATENCY_FORMS)
@pytest.mark.parametrize("top", RB.PSEUDO_TOPS)
def test_pseudo_ids(lib, oracle_mod, monkeypatch, top, latency):
    monkeypatch.setenv("TKZ_LATENCY_BYTES", latency)
    RB.check_pseudo(lib, oracle_mod, top)


@pytest.mark.parametrize("latency", RB.LATENCY_FORMS)
@pytest.mark.parametrize("top", RB.PSEUDO_TOPS)
def test_pseudo_ids_swallowed(lib, oracle_mod, monkeypatch, top, latency):
    monkeypatch.setenv("TKZ_LATENCY_BYTES", latency)
    RB.check_pseudo_swallowed(lib, oracle_mod, top)


@pytest.mark.parametrize("top", RB.PSEUDO_TOPS)
def test_pseudo_id_survives_beside_the_memo(lib, oracle_mod, top):
    RB.check_pseudo_survives_memo(lib, oracle_mod, top)


@pytest.mark.parametrize("top", (RB.VAR_COMPACT_MAX_RANK, RB.VAR_COMPACT_MAX_RANK + 1))
def test_rank_equal_to_a_compact_pseudo_id(lib, oracle_mod, top):
    RB.check_pseudo_id_collision(lib, oracle_mod, top)


@pytest.mark.parametrize("top", RB.MAIN_TOPS)
def test_single_launch(lib, oracle_mod, top):
    RB.check_single_launch(lib, oracle_mod, top)


@pytest.mark.parametrize("top", RB.MAIN_TOPS)
def test_batch_sequence(lib, oracle_mod, top):
    RB.check_batch_sequence(lib, oracle_mod, top, n_docs=BATCH_DOCS)


@pytest.mark.parametrize("top", (RB.PROMO_FLAG - 1, RB.PROMO_FLAG))
def test_promotion_gate(lib, oracle_mod, top):
    RB.check_promotion_gate(lib, oracle_mod, top)
