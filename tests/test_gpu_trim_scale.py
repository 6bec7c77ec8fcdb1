"""`-m gpu`: the piece-granular launch sequence -- tkz_encode_batch_pieces_utf8, tkz_encode_batch_trim_utf8 / _device / _utf16 -- beyond the 256 KiB at which
tests/test_gpu_trim.py and parity.check_piece_granular stop, where the kernels it reuses change form:
  1  launch_scan2 on both sides of kScanSmallMax sub-tiles (k_scan_small | the three-kernel scan, twice over one bsum) with the piece starts as marks
  2  k_scan_top's carry between steps inside the trim scan (more than 256 x kScanBlock documents)
  3  k_trim_gather's two grid strides (more kept ids than 8,192 wavefronts x kTrimTile, more text than 8,192 x kTrimByteTile)
  4  a batch above TKZ_OPT_LATENCY_BYTES through the host entries, UTF-16 included
  5  the side-by-side merge form with a mark on every piece
  6  retries (miss lists, the giant pieces' pool, the record buffer) with c.pieces set, and what a failed attempt leaves of the caller's buffers
Every comparison is exact -- ids, offsets, cut_bytes, cut_units; doc_piece, piece_boffs, piece_toffs -- against the oracle: every batch is made of a small pool
of distinct documents, repeated and shuffled (tests/trim_cases.py), so oracle.TrimOracle's work is bounded by the pool while every document of the batch has its
exact expectation; the plain ids of the same buffers are checked at full size by the oracle in C.  Every case asserts the precondition that puts it in its
regime.  The capacity status and its kept total on the host entry without a retry: tests/test_emu_trim.py::test_capacity; here on the device entry behind a retry.
Not covered: the plain launch_scan's own k_scan_top carry (256 MiB of text) and batches beyond 2^31 bytes through the trim entries."""
import time

import numpy as np
import pytest

import special_cases as SC
import trim_cases as TC
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu

VOCAB, PATTERN = "gpt2", N.CL100K
MIXED_BYTES = 20_000_000


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def setup(lib, vocab_bytes, oracle_mod):
    raw = vocab_bytes(VOCAB)
    specials = SC.SPECIAL_SETS[VOCAB]
    v, ov = N.Vocab(raw, lib), oracle_mod.Vocab(raw)

    def new_encoder():
        enc = N.Encoder(v, PATTERN)
        enc.set_special_tokens(specials)
        return enc
    corpus_doc = lambda kind, d, lo, hi: N.corpus_doc_host(kind, 900 + kind, d, lo, hi, lib=lib)
    return new_encoder, TC.Expect(oracle_mod, ov, PATTERN, specials), ov, specials, corpus_doc


@pytest.fixture(scope="module")
def scale_pool(setup):
    return TC.scale_pool(SC.EOT, setup[4])


@pytest.mark.parametrize("extra,ntiles,one_workgroup", [(0, 8192, True), (1, 8193, False), (1025, 8194, False)])
def test_scan_form_edge(setup, oracle_mod, scale_pool, extra, ntiles, one_workgroup):
    new_encoder, exp, ov, specials, _ = setup
    total = TC.K_SCAN_SMALL_MAX * TC.K_SUB + extra
    assert TC.sub_tiles(total) == ntiles and (ntiles <= TC.K_SCAN_SMALL_MAX) == one_workgroup
    assert (ntiles % TC.K_SCAN_BLOCK != 0) == (not one_workgroup)                      # (the three-kernel form's last block is ragged)
    t0 = time.time()
    idx, data, offs, per_doc = TC.build_batch(scale_pool, 1000 + extra, TC.SCALE_MAXIMA, total_bytes=total)
    assert len(data) == total and (per_doc == 0).any() and (per_doc == TC.HUGE).any()
    enc = new_encoder()
    n_pieces = TC.compare_pieces_pooled(enc, oracle_mod, ov, PATTERN, scale_pool, idx, data, offs, "%d sub-tiles" % ntiles)
    assert n_pieces > total // 8                                                       # (up to 1,024 marks a sub-tile: far more marks than documents)
    for side in TC.SIDES:
        for allowed in ([SC.EOT], []):
            TC.compare_trim_pooled(enc, exp, specials, scale_pool, idx, data, offs, per_doc, allowed, side, "%d sub-tiles" % ntiles, mem=TC.TorchMemory())
    print("scan form edge, %d sub-tiles: %d documents, %d pieces, %.1f s" % (ntiles, len(idx), n_pieces, time.time() - t0))


@pytest.mark.parametrize("n_docs,carries", [(262144, False), (262145, True), (2 * 262144 + 1, True)])
def test_scan_top_carry_in_the_trim_scan(setup, n_docs, carries):
    new_encoder, exp, ov, specials, _ = setup
    assert (n_docs > TC.K_SCAN_TOP_STEP) == carries and n_docs >= TC.K_SCAN_TOP_STEP
    pool = TC.tiny_pool()
    t0 = time.time()
    idx, data, offs, per_doc = TC.build_batch(pool, n_docs, TC.TINY_MAXIMA, n_docs=n_docs)
    assert len(idx) == n_docs and len(data) < 2 << 20 and (per_doc < 0).any() and (per_doc == 0).any()
    enc = new_encoder()
    for side in TC.SIDES:
        kept = TC.compare_trim_pooled(enc, exp, specials, pool, idx, data, offs, per_doc, [], side, "%d documents" % n_docs, mem=TC.TorchMemory())
        assert kept > 0
    print("trim scan, %d documents: %.1f s" % (n_docs, time.time() - t0))


def exp_counts(exp, pool, idx):
    return np.asarray([exp.count(d, []) for d in pool.docs], np.int64)[idx]


def test_gather_strides(setup):
    new_encoder, exp, ov, specials, _ = setup
    pool = TC.dense_pool()
    total = TC.K_TRIM_GATHER_WAVES * TC.K_TRIM_BYTE_TILE + 5000
    t0 = time.time()
    idx, data, offs, per_doc = TC.build_batch(pool, 1, TC.DENSE_MAXIMA, total_bytes=total)
    assert len(data) > TC.K_TRIM_GATHER_WAVES * TC.K_TRIM_BYTE_TILE                     # the unit count goes round its grid twice
    assert -(-total // TC.K_TRIM_TILE) > TC.K_TRIM_GATHER_WAVES                         # (launch_trim's grid -- a wavefront per kTrimTile bytes -- is at its cap)
    enc = new_encoder()
    for side in TC.SIDES:
        kept = TC.compare_trim_pooled(enc, exp, specials, pool, idx, data, offs, per_doc, [], side, "gather strides", mem=TC.TorchMemory())
        assert kept > TC.K_TRIM_GATHER_WAVES * TC.K_TRIM_TILE, kept                      # the id copy goes round its grid twice
        want = TC.expected_from_pool(exp, pool, idx, [], side, per_doc)
        assert (want[3] != want[2]).any() and (np.diff(want[1]) < exp_counts(exp, pool, idx)).any()      # units differ from bytes; some documents are cut
    print("gather strides: %d bytes, %d kept ids, %.1f s" % (total, kept, time.time() - t0))


def test_above_the_latency_threshold(setup, oracle_mod):
    new_encoder, exp, ov, specials, corpus_doc = setup
    pool = TC.mixed_pool(corpus_doc, SC.EOT)
    t0 = time.time()
    idx, data, offs, per_doc = TC.build_batch(pool, 4, TC.MIXED_MAXIMA, total_bytes=MIXED_BYTES)
    assert len(data) > TC.LATENCY_BYTES
    enc = new_encoder()
    TC.compare_pieces_pooled(enc, oracle_mod, ov, PATTERN, pool, idx, data, offs, "20 MB")
    for side in TC.SIDES:
        TC.compare_trim_pooled(enc, exp, specials, pool, idx, data, offs, per_doc, [SC.EOT], side, "20 MB, host entry")
    # UTF-16: well-formed text, so the UTF-8 expectation holds -- the same ids, the same units
    table, starts, lens = pool.units()
    units, uoffs = TC.gather_segments(table, starts, lens, idx)
    ids, ooff, cu = enc.encode_batch_trim_utf16(units, uoffs, SC.indices(specials, [SC.EOT]), N.TRIM_PREFIX, 0, per_doc)
    w_ids, w_offs, _, w_cu = TC.expected_from_pool(exp, pool, idx, [SC.EOT], N.TRIM_PREFIX, per_doc)
    TC.assert_same("20 MB, UTF-16", dict(ids=ids, offsets=ooff, cut_units=cu), dict(offsets=w_offs, cut_units=w_cu, ids=w_ids), offs, want_offs=w_offs)
    print("20 MB: %d documents, %d side-by-side batches, %.1f s" % (len(idx), enc.side_by_side_batches, time.time() - t0))


def test_side_by_side_under_piece_marks(setup, oracle_mod):
    new_encoder, exp, ov, specials, _ = setup
    TC.check_side_by_side_under_piece_marks(new_encoder, exp, oracle_mod, ov, PATTERN, specials, TC.TorchMemory())


def test_retries_with_pieces(setup, oracle_mod, capfd, monkeypatch):
    new_encoder, exp, ov, specials, _ = setup
    TC.check_retries_with_pieces(new_encoder, exp, oracle_mod, ov, PATTERN, specials, TC.TorchMemory(), capfd, monkeypatch)
