"""`not gpu`: the piece-granular launch sequence (tkz_encode_batch_pieces_utf8, tkz_encode_batch_trim_device) where it changes form -- the real kernel sources
on the CPU emulator (tests/hostemu/), exact against the oracle through tests/trim_cases.py's pooled expectations:
  the side-by-side merge form under piece marks, retries with c.pieces set (tests/test_gpu_trim_scale.py cases 5 and 6, at the same sizes),
  k_scan_top's carry inside the trim scan at 262,145 documents (case 2),
  and -- the helper alone, no kernel -- that a pooled expectation equals the oracle's document by document and that one that is wrong by one piece fails the
  comparison of each of the cases 1 to 3.
The scan form edge at 8 MiB, the gather strides at 32 MiB and the 20 MB batch are the GPU module's alone: the emulator runs one workgroup at a time."""
import numpy as np
import pytest

import emu
import special_cases as SC
import trim_cases as TC
from tokenizer_amd import _native as N

VOCAB, PATTERN = "gpt2", N.CL100K


@pytest.fixture(scope="module")
def lib():
    return emu.library()


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


def test_side_by_side_under_piece_marks(setup, oracle_mod):
    new_encoder, exp, ov, specials, _ = setup
    TC.check_side_by_side_under_piece_marks(new_encoder, exp, oracle_mod, ov, PATTERN, specials, TC.HostMemory())


def test_retries_with_pieces(setup, oracle_mod, capfd, monkeypatch):
    new_encoder, exp, ov, specials, _ = setup
    TC.check_retries_with_pieces(new_encoder, exp, oracle_mod, ov, PATTERN, specials, TC.HostMemory(), capfd, monkeypatch)


def test_scan_top_carry_in_the_trim_scan(setup):
    """n_docs = 262,145: k_scan_top's second step holds one block sum and the carry of the first 256"""
    new_encoder, exp, ov, specials, _ = setup
    pool = TC.tiny_pool()
    idx, data, offs, per_doc = TC.build_batch(pool, 262145, TC.TINY_MAXIMA, n_docs=TC.K_SCAN_TOP_STEP + 1)
    assert len(idx) > TC.K_SCAN_TOP_STEP and len(data) < 2 << 20 and (per_doc < 0).any() and (per_doc == 0).any()
    enc = new_encoder()
    for side in TC.SIDES:
        TC.compare_trim_pooled(enc, exp, specials, pool, idx, data, offs, per_doc, [], side, "262,145 documents", mem=TC.HostMemory())


POOLS = {"scale": (lambda cd: TC.scale_pool(SC.EOT, cd), TC.SCALE_MAXIMA, [SC.EOT]),       # case 1
         "tiny": (lambda cd: TC.tiny_pool(), TC.TINY_MAXIMA, []),                           # case 2
         "dense": (lambda cd: TC.dense_pool(), TC.DENSE_MAXIMA, [])}                        # case 3


@pytest.mark.parametrize("which", list(POOLS))
def test_pooled_expectation_and_a_wrong_one(setup, oracle_mod, which):
    """No kernel: expected_from_pool / expected_pieces_from_pool equal the oracle's walk document by document (trim_cases.expected, parity.check_piece_granular's
    loop), and a cached expectation shifted by one piece -- one pooled document, one maximum -- fails assert_same on ids, offsets and cuts."""
    _, exp, ov, specials, corpus_doc = setup
    make, maxima, allowed = POOLS[which]
    pool = make(corpus_doc)
    idx, data, offs, per_doc = TC.build_batch(pool, 9, maxima, n_docs=300)
    docs = [pool.docs[i] for i in idx]
    assert data.tobytes() == "".join(docs).encode("utf-8") and offs.tolist() == np.cumsum([0] + [len(d.encode("utf-8")) for d in docs]).tolist()
    names = ("ids", "offsets", "cut_bytes", "cut_units")
    for side in TC.SIDES:
        pooled = TC.expected_from_pool(exp, pool, idx, allowed, side, per_doc)
        walked = TC.expected(exp, docs, allowed, side, [max(int(m), 0) for m in per_doc])
        TC.assert_same(which, dict(zip(names, pooled)), dict(zip(names, walked)), offs)
        # shift one pooled document's cut by one piece: the first document of the batch that is cut inside its text
        victim = next(k for k in range(len(idx)) if 0 < pooled[2][k] < pool.lens[idx[k]] and pooled[1][k + 1] > pooled[1][k])
        key = (pool.docs[idx[victim]], tuple(allowed), side, max(int(per_doc[victim]), 0))
        ids, cb, cu = exp._trim[key]
        (rel, pstarts, npieces), _, _ = pool.pieces(oracle_mod, ov, PATTERN)
        starts = rel[pstarts[idx[victim]]:pstarts[idx[victim]] + npieces[idx[victim]]].tolist() + [int(pool.lens[idx[victim]])]
        at = starts.index(cb)
        moved = starts[at - 1]                                    # (the boundary one piece in front)
        try:
            exp._trim[key] = (ids[:-1] if side == N.TRIM_SUFFIX else ids, moved, cu - TC.utf16_len(pool.raw[idx[victim]][moved:cb].decode("utf-8")))
            wrong = TC.expected_from_pool(exp, pool, idx, allowed, side, per_doc)
            with pytest.raises(AssertionError):
                TC.assert_same(which, dict(zip(names, pooled)), dict(zip(names, wrong)), offs)
            with pytest.raises(AssertionError):
                TC.assert_same(which, dict(cut_bytes=pooled[2]), dict(cut_bytes=wrong[2]), offs)
        finally:
            exp._trim[key] = (ids, cb, cu)
    # the pieces: against the loop of parity.check_piece_granular, and one piece boundary moved by a byte
    w_ids, w_dpo, w_pbo, w_pto = TC.expected_pieces_from_pool(oracle_mod, ov, PATTERN, pool, idx, offs)
    e_dpo, e_pbo, e_pto, e_ids, pos = [0], [], [0], [], 0
    for d in (pool.raw[i] for i in idx):
        for (a, n) in oracle_mod.split_utf8(PATTERN, d):
            r = ov.rank(d[a:a + n])
            e_ids += [r] if r >= 0 else ov.bpe(d[a:a + n])
            e_pbo.append(pos + a)
            e_pto.append(len(e_ids))
        e_dpo.append(len(e_pbo))
        pos += len(d)
    e_pbo.append(pos)
    pn = ("ids", "doc_piece", "piece_boffs", "piece_toffs")
    TC.assert_same(which, dict(zip(pn, (w_ids, w_dpo, w_pbo, w_pto))), dict(zip(pn, (e_ids, e_dpo, e_pbo, e_pto))), offs)
    wrong = np.array(e_pbo)
    wrong[len(wrong) // 2] += 1
    with pytest.raises(AssertionError):
        TC.assert_same(which, dict(piece_boffs=w_pbo), dict(piece_boffs=wrong), offs)
    TC.crosscheck_plain(oracle_mod, ov, PATTERN, data, offs, w_ids, w_pto[w_dpo])
