"""The rank-width forms of the merge kernels at their thresholds, shared by tests/test_emu_rank_bands.py (CPU emulator) and tests/test_gpu_rank_bands.py.

Several kernels change form with TkzTables::max_rank (tkz_tables.h, tkz_bpe.h):
  TKZ_PAIR_CID_LIMIT   0x1FFF00   the PAIR table is compact (21-bit ids and ranks, pseudo ids as 0x1FFF00 + byte) below it, wide from it on
  kVarCompactMaxRank   2^21 - 2   tkz_bpe_lane_u / tkz_bpe_lane_varc (no ids[]) up to it, the forms with ids[] above
  kVarPackedMaxRank    2^22 - 2   tkz_bpe_lane_var<true> (rank << 10 | pos) up to it, <false> (plain ranks) above
  kPromoFlag           2^26       bit 26 of a piece record is a promotion code below it and part of a rank from it on: the host promotes nothing
  TKZ_MAX_RANK         2^27 - 2   the largest rank that loads
A band table (band_table) is a rank table whose largest rank is exactly `top`, its other ranks just below: TOPS holds both sides of every threshold.
Every comparison is exact against the oracle's literal loop -- Vocab.rank / Vocab.bpe for pieces, Encoder.encode_bytes for documents."""
import base64
import os
import random
import re

import numpy as np
import pytest

import parity
from tokenizer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tokenizer_amd", "csrc")

# the thresholds as this module's cases assume them (test_emu_rank_bands.py::test_header_constants compares them with the headers' text)
PAIR_CID_LIMIT = 0x1FFF00
VAR_POS_BITS = 10
VAR_COMPACT_MAX_RANK = (1 << 21) - 2
VAR_PACKED_MAX_RANK = (1 << (32 - VAR_POS_BITS)) - 2
PROMO_FLAG = 1 << 26
MAX_RANK = (1 << 27) - 2
SMALL_MAX_BYTES = 131072                  # kSmallMaxBytes (tkz_kernels.h): the largest batch the single launch takes
SMALL_LANE_PIECE = 256                    # kSmallLanePiece: a longer missed piece sends a small call back to the batch path

TOPS = (PAIR_CID_LIMIT - 1, PAIR_CID_LIMIT, VAR_COMPACT_MAX_RANK, VAR_COMPACT_MAX_RANK + 1, VAR_PACKED_MAX_RANK, VAR_PACKED_MAX_RANK + 1,
        PROMO_FLAG - 1, PROMO_FLAG, MAX_RANK)
# one side of every threshold, each form once: compact over a wide pair table | var<true> | var<false> | no promotion | the 27-bit edge
MAIN_TOPS = (PAIR_CID_LIMIT, VAR_COMPACT_MAX_RANK + 1, VAR_PACKED_MAX_RANK + 1, PROMO_FLAG, MAX_RANK)
PSEUDO_TOPS = (PAIR_CID_LIMIT - 1, PAIR_CID_LIMIT, VAR_COMPACT_MAX_RANK + 1, VAR_PACKED_MAX_RANK + 1, MAX_RANK)
# The two packed-key thresholds are conservative by one: rank 2^21 - 1 still fits a live compact key (rank << 10 | pos stays below kVarDead) and 2^22 - 1 a packed
# one, so a threshold that drifts up by a few is invisible at TOPS.  The first ranks the packed keys can NOT hold pin the forms from the other side.
OVERFLOW_TOPS = (1 << (31 - VAR_POS_BITS), 1 << (32 - VAR_POS_BITS))
LATENCY_FORMS = ("0", str(16 << 20))      # $TKZ_LATENCY_BYTES: the class queue (k_merge_long_q) | the chunk form (k_merge_latency)

# SHORT / MID / LONG key edges (12|13, 28|29), tkz_bpe_lane_f<16> / <32> (16|17, 32|33), tkz_bpe_lane_u / tkz_bpe_lane_varc / the arena (64|65, 128|129),
# k_merge_coop (256|257 .. 1024) and the giant pieces (1025)
PIECE_LENS = (2, 9, 12, 13, 16, 17, 28, 29, 32, 33, 64, 65, 128, 129, 256, 257, 320, 1024, 1025)
TAIL_LENS = (18_000, 34_000)              # tkz_bpe_long_tail with the ids in LDS and in the pool, and its window sweep
WORD_LENS = (1, 2, 3, 5, 8, 11, 12, 13, 15, 16, 17, 27, 28, 29, 33, 64, 65, 130, 250)       # all <= kSmallLanePiece: k_small keeps the call


def header_constants():
    """The thresholds as tkz_tables.h / tkz_bpe.h / tkz_kernels.h define them, read out of the headers' text."""
    text = {name: open(os.path.join(CSRC, name), encoding="utf-8").read() for name in ("tkz_tables.h", "tkz_bpe.h", "tkz_kernels.h")}
    out = {}

    def take(name, header, pattern):
        m = re.search(pattern, text[header], re.M)
        assert m, "%s: no definition of %s found" % (header, name)
        expr = re.sub(r"(?<=[0-9a-fA-F])[uU]\b", "", m.group(1))
        out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))          # noqa: S307 (an integer expression of the project's own header)
    take("TKZ_PAIR_CID_LIMIT", "tkz_tables.h", r"^#define\s+TKZ_PAIR_CID_LIMIT\s+(.+?)\s*(?:/[/*].*)?$")
    take("TKZ_MAX_RANK", "tkz_tables.h", r"^#define\s+TKZ_MAX_RANK\s+(.+?)\s*(?:/[/*].*)?$")
    take("kPromoFlag", "tkz_tables.h", r"\bkPromoFlag\s*=\s*([^,;]+)[,;]")
    take("kVarPosBits", "tkz_bpe.h", r"\bkVarPosBits\s*=\s*([^,;]+);")
    take("kVarPackedMaxRank", "tkz_bpe.h", r"\bkVarPackedMaxRank\s*=\s*([^,;]+);")
    take("kVarCompactMaxRank", "tkz_bpe.h", r"\bkVarCompactMaxRank\s*=\s*([^,;]+);")
    take("kSmallLanePiece", "tkz_kernels.h", r"\bkSmallLanePiece\s*=\s*([^,;]+);")
    take("kSmallMaxBytes", "tkz_kernels.h", r"\bkSmallMaxBytes\s*=\s*([^,;]+)[,;]")
    return out


def module_constants():
    return {"TKZ_PAIR_CID_LIMIT": PAIR_CID_LIMIT, "TKZ_MAX_RANK": MAX_RANK, "kPromoFlag": PROMO_FLAG, "kVarPosBits": VAR_POS_BITS,
            "kVarPackedMaxRank": VAR_PACKED_MAX_RANK, "kVarCompactMaxRank": VAR_COMPACT_MAX_RANK, "kSmallLanePiece": SMALL_LANE_PIECE,
            "kSmallMaxBytes": SMALL_MAX_BYTES}


# ---- band tables ---------------------------------------------------------------------------------------------------------------------
def table_lines(ranks):
    return b"".join(base64.b64encode(k) + b" " + str(r).encode() + b"\n" for k, r in ranks.items())


def band_ranks(top, drop=b"", n_random=200, n_spaced=60, seed=None):
    """{key: rank}: all single bytes but those of `drop`, n_random keys of 2..6 bytes over abc, n_spaced of them once more behind a blank (cl100k pieces
    such as " abca" are whole keys); distinct ranks drawn from [top - 4n, top), and `top` itself on a two-byte key -- a rank the PAIR table holds, so in the
    band [TKZ_PAIR_CID_LIMIT, kVarCompactMaxRank] the wide pair table has ranks on both sides of the compact limit whatever the draw.  Seeded from top (the soaks of tools/ pass a seed of their own: another table of the same band every round)."""
    rng = random.Random(top if seed is None else top * 1_000_003 + seed)
    multi = set()
    while len(multi) < n_random:
        multi.add(bytes(rng.choice(b"abc") for _ in range(rng.randint(2, 6))))
    multi = sorted(multi)
    spaced = [b" " + k for k in rng.sample(multi, n_spaced)]
    keys = [bytes([b]) for b in range(256) if b not in drop] + multi + spaced
    n = len(keys)
    at_top = rng.choice([k for k in multi if len(k) == 2])
    keys.remove(at_top)
    rng.shuffle(keys)
    ranks = dict(zip(keys, rng.sample(range(top - 4 * n, top), n - 1)))
    ranks[at_top] = top
    return ranks


def band_table(top, drop=b"", seed=None):
    """A .tiktoken image whose largest rank is exactly `top` (band_ranks)."""
    return table_lines(band_ranks(top, drop, seed=seed))


def pair_derived_ranks(ranks):
    """The ranks the PAIR table holds: keys with a split into two parts that are keys or single bytes (tkz_vocab.cpp: build_tables)."""
    part = lambda s: s in ranks or len(s) == 1
    return [r for k, r in ranks.items() if any(part(k[:p]) and part(k[p:]) for p in range(1, len(k)))]


def check_band_table(O, top, drop=b""):
    """What makes a band table a test of its band, asserted on the table itself."""
    ranks = band_ranks(top, drop)
    raw = table_lines(ranks)
    assert raw == band_table(top, drop), "the generator is deterministic"
    vals = sorted(ranks.values())
    assert vals[-1] == top and len(set(vals)) == len(vals) and vals[0] >= top - 4 * len(vals) and vals[0] >= 0
    assert sum(1 for k in ranks if len(k) == 1) == 256 - len(drop) and not any(bytes([b]) in ranks for b in drop)
    assert len(ranks) == 256 - len(drop) + 260 and sum(1 for k in ranks if k[:1] == b" " and len(k) > 1) == 60
    if PAIR_CID_LIMIT <= top <= VAR_COMPACT_MAX_RANK:          # the compact lane forms over a WIDE pair table that holds both kinds of rank
        pr = pair_derived_ranks(ranks)
        assert max(pr) >= PAIR_CID_LIMIT and min(pr) < PAIR_CID_LIMIT and vals[0] < PAIR_CID_LIMIT
    if top == PROMO_FLAG:                                      # bit 26 set and clear
        assert any(r & PROMO_FLAG for r in vals) and any(not (r & PROMO_FLAG) for r in vals)
    ov = O.Vocab(raw)
    assert len(ov) == len(ranks) and all(ov.rank(k) == r for k, r in list(ranks.items())[::17])


_tables = {}


def tables(lib, O, top, drop=b""):
    """(device vocabulary, oracle vocabulary) of a band table, built once per library."""
    key = (id(lib), top, bytes(drop))
    if key not in _tables:
        raw = band_table(top, drop)
        _tables[key] = (N.Vocab(raw, lib), O.Vocab(raw))
    return _tables[key]


# ---- pieces --------------------------------------------------------------------------------------------------------------------------
def band_pieces(top, n=120, lens=PIECE_LENS):
    """n random pieces over a / ab / abc, every length of `lens` in turn."""
    rng = random.Random(top * 31 + 7)
    out = []
    for i in range(n):
        alpha = rng.choice([b"a", b"ab", b"abc"])
        out.append(bytes(rng.choice(alpha) for _ in range(lens[i % len(lens)])))
    return out


def tail_pieces(top):
    rng = random.Random(top * 31 + 11)
    return [bytes(rng.choice(b"abc") for _ in range(n)) for n in TAIL_LENS]


def oracle_piece(O, ov, p):
    """The reference's answer for one piece: its ids, or None where BytePairEncode throws KeyNotFoundException (a byte that is no key survives)."""
    r = ov.rank(p)
    if r >= 0:
        return [r]
    try:
        return ov.bpe(p)
    except O.OracleError as ex:
        assert ex.code == O.E_KEY_NOT_FOUND, ex.code
        return None


_expected = {}


def expected_pieces(O, ov, key, pcs):
    """oracle_piece of every piece, computed once per key and left unchanged."""
    if key not in _expected:
        _expected[key] = tuple(oracle_piece(O, ov, p) for p in pcs)
    return _expected[key]


def compare_pieces(enc, pcs, want, what):
    data, offs = parity.pack(pcs)
    ids, ooff = enc.encode_pieces(data, offs)
    for i, p in enumerate(pcs):
        g = ids[ooff[i]:ooff[i + 1]].tolist()
        assert g == want[i], "%s piece %d (len %d) %r: got %r expected %r" % (what, i, len(p), p[:40], g[:12], want[i][:12])
    assert ooff.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist() and len(ids) == ooff[-1], what


def check_pieces(lib, O, top, with_tails=False):
    """120 pieces of every length class through tkz_encode_pieces under a table whose largest rank is `top`.  $TKZ_LATENCY_BYTES, read when the encoder is
    created, is the caller's: both long-miss forms take the same pieces."""
    v, ov = tables(lib, O, top)
    pcs = band_pieces(top)
    want = list(expected_pieces(O, ov, (top, "pieces"), pcs))
    if with_tails:
        tails = tail_pieces(top)
        pcs, want = pcs + tails, want + list(expected_pieces(O, ov, (top, "tails"), tails))
    assert all(w is not None for w in want)
    assert max(max(w) for w in want) <= top
    enc = N.Encoder(v, N.CL100K)
    compare_pieces(enc, pcs, want, "top %#x latency %s" % (top, os.environ.get("TKZ_LATENCY_BYTES")))


# ---- pseudo ids: a byte that is no key ----------------------------------------------------------------------------------------------
def expect_key_not_found(enc, pcs):
    data, offs = parity.pack(pcs)
    with pytest.raises(N.KeyNotFoundError) as ei:
        enc.encode_pieces(data, offs)
    assert ei.value.code == N.E_KEY_NOT_FOUND


def check_pseudo(lib, O, top):
    """The band table without the byte `b`: a piece either merges every b away (equal ids) or a b survives (KeyNotFoundError, as BytePairEncoder.cs:17,73
    throws) -- one per call, inside a batch of good pieces, and the encoder answers a good piece correctly after every refusal."""
    v, ov = tables(lib, O, top, drop=b"b")
    pcs = band_pieces(top)
    want = expected_pieces(O, ov, (top, "pseudo"), pcs)
    good = [i for i, w in enumerate(want) if w is not None]
    bad = [i for i, w in enumerate(want) if w is None]
    # (what keeps the test honest: the oracle alone accepts and refuses enough of them, whatever the device says)
    assert len(good) >= 40 and len(bad) >= 10, (top, len(good), len(bad))
    assert any(b"b" in pcs[i] for i in good), "no accepted piece holds the dropped byte"
    enc = N.Encoder(v, N.CL100K)
    what = "top %#x without b" % top
    compare_pieces(enc, [pcs[i] for i in good], [want[i] for i in good], what)
    for k, i in enumerate(bad):
        expect_key_not_found(enc, [pcs[i]])
        j = good[k % len(good)]                                  # nothing is left behind: a good piece of another length class every time
        compare_pieces(enc, [pcs[j]], [want[j]], what + " after a refusal")
    mixed = [pcs[i] for i in good[:7]] + [pcs[bad[0]]] + [pcs[i] for i in good[7:20]] + [pcs[i] for i in bad[1:4]] + [pcs[i] for i in good[20:25]]
    expect_key_not_found(enc, mixed)
    expect_key_not_found(enc, pcs)
    compare_pieces(enc, [pcs[i] for i in good], [want[i] for i in good], what + " after the refused batches")


def swallow_ranks(top):
    """{a, ab, abab} and every single byte but b, the three keys at the top of the band."""
    ranks = {bytes([c]): top - 600 + c for c in range(256) if c != ord("b")}
    ranks.update({b"a": top - 2, b"ab": top - 1, b"abab": top})
    return ranks


def check_pseudo_swallowed(lib, O, top):
    """Hand-made case 1: under {a, ab, abab} without b, "ab" * k encodes -- every b is swallowed into an ab -- and "ab" * k + "b" must raise, at lengths that
    reach tkz_bpe_lane_f (8, 20, 32), tkz_bpe_lane_u (34, 64), tkz_bpe_lane_varc (80, 128), the arena form (200), k_merge_coop (300, 800) and the giant
    pieces (1200); as pieces and as one cl100k string (k_small's chunk form)."""
    raw = table_lines(swallow_ranks(top))
    v, ov = N.Vocab(raw, lib), O.Vocab(raw)
    enc = N.Encoder(v, N.CL100K)
    oenc = O.Encoder(ov, N.CL100K)
    reps = (4, 10, 16, 17, 32, 40, 64, 100, 150, 400, 600)
    good = [b"ab" * k for k in reps]
    want = [oracle_piece(O, ov, p) for p in good]
    assert all(w is not None and set(w) <= {top - 1, top} for w in want)
    compare_pieces(enc, good, want, "swallowed, top %#x" % top)
    for p, w in zip(good, want):
        bad = p + b"b"
        assert oracle_piece(O, ov, bad) is None
        expect_key_not_found(enc, [bad])
        compare_pieces(enc, [p], [w], "swallowed, after a refusal")
        if len(p) <= SMALL_LANE_PIECE:
            assert enc.encode_utf8(p) == oenc.encode_bytes(p)
            with pytest.raises(N.KeyNotFoundError):
                enc.encode_utf8(bad)
    expect_key_not_found(enc, good[:5] + [good[5] + b"b"] + good[6:])
    compare_pieces(enc, good, want, "swallowed, after the refused batch")


def check_pseudo_survives_memo(lib, O, top):
    """Hand-made case 2: a 12-byte and a 16-byte piece whose last b survives (k_merge_short's lane and its memo round).  They raise, and raise again: the memo
    must not answer for a piece it was never allowed to store; their good neighbours (which the memo does store) keep their ids."""
    raw = table_lines(swallow_ranks(top))
    v, ov = N.Vocab(raw, lib), O.Vocab(raw)
    enc = N.Encoder(v, N.CL100K)
    for n in (12, 16):
        bad = b"ab" * (n // 2 - 1) + b"bb"
        good = b"ab" * (n // 2)
        assert len(bad) == n and oracle_piece(O, ov, bad) is None
        w = oracle_piece(O, ov, good)
        assert enc.memo_bucket(bad) >= 0
        for rep in range(3):
            expect_key_not_found(enc, [bad])
            compare_pieces(enc, [good, b"a" * n], [w, oracle_piece(O, ov, b"a" * n)], "memo round %d" % rep)
            expect_key_not_found(enc, [good, bad, good])
            with pytest.raises(N.KeyNotFoundError):
                enc.encode_utf8(bad)


def collision_ranks(top, byte=ord("b")):
    """Every single byte but b; "aa" at the rank that equals b's compact pseudo id (TKZ_PAIR_CID_LIMIT + 'b'); "bc", "cb" as keys through the pseudo id."""
    cid = PAIR_CID_LIMIT + byte
    assert top - 600 > 0 and cid <= top
    ranks = {bytes([c]): top - 900 + c for c in range(256) if c != byte}
    ranks.update({b"aa": cid, b"bc": top - 3, b"cb": top - 2, b"cc": top})
    assert len(set(ranks.values())) == len(ranks)
    return ranks


def check_pseudo_id_collision(lib, O, top):
    """Hand-made case 3 (tops from TKZ_PAIR_CID_LIMIT + 'b' on): a key whose RANK equals the compact form's id of the missing byte.  Only a wide pair table
    tells (aa, c) from (b, c): "aac" is [aa, c], never [.., bc]."""
    raw = table_lines(collision_ranks(top))
    v, ov = N.Vocab(raw, lib), O.Vocab(raw)
    enc = N.Encoder(v, N.CL100K)
    rng = random.Random(top)
    pcs = [b"aac", b"caa", b"aacaa", b"bcaac", b"aacb"] + [b"".join(rng.choice([b"aa", b"c", b"bc", b"cb", b"a"]) for _ in range(n)) for n in (5, 9, 14, 30, 60, 150, 500)]
    want = [oracle_piece(O, ov, p) for p in pcs]
    assert want[0] == [PAIR_CID_LIMIT + ord("b"), top - 900 + ord("c")]
    good = [i for i, w in enumerate(want) if w is not None]
    assert len(good) >= 6
    compare_pieces(enc, [pcs[i] for i in good], [want[i] for i in good], "pseudo-id collision, top %#x" % top)
    for i in range(len(pcs)):
        if want[i] is None:
            expect_key_not_found(enc, [pcs[i]])


# ---- the batch sequence and the single launch -------------------------------------------------------------------------------------
def word_pool(top):
    rng = random.Random(top * 31 + 13)
    return ["".join(rng.choice("abc") for _ in range(WORD_LENS[i % len(WORD_LENS)])) for i in range(50)]


def make_docs(top, n_docs, n_words, salt):
    pool = word_pool(top)
    rng = random.Random(top * 31 + salt)
    return [" ".join(rng.choice(pool) for _ in range(n_words)).encode() for _ in range(n_docs)]


def long_run_word(O, ov, top, n=250, min_tokens=70):
    """One piece over abc that merges into a run of at least 70 tokens: more than k_place's fast path takes (64)."""
    rng = random.Random(top * 31 + 17)
    for _ in range(50):
        w = bytes(rng.choice(b"abc") for _ in range(n))
        if ov.rank(w) < 0 and len(ov.bpe(w)) >= min_tokens:
            return w
    raise AssertionError("no %d-byte piece of %d tokens under top %#x" % (n, min_tokens, top))


_batches = {}


def batch_case(O, ov, top, which, n_docs):
    """(documents, expected ids, expected offsets) of the small call (`small`: 3 documents of 40 words) or of the batch just too large for the single launch
    (`batch`: n_docs documents of 120 words, a 70-token run, a 300-byte missed word), against the oracle once."""
    key = (top, which, n_docs)
    if key not in _batches:
        if which == "small":
            docs = make_docs(top, 3, 40, 19)
        else:
            rng = random.Random(top * 31 + 23)
            miss300 = bytes(rng.choice(b"abc") for _ in range(300))
            assert ov.rank(miss300) < 0
            docs = make_docs(top, n_docs, 120, 29) + [long_run_word(O, ov, top), b"a " + miss300 + b" c"]
        at_top = next(k for k, r in band_ranks(top).items() if r == top)
        docs[0] += b" " + at_top                                 # (a whole-key hit at the largest rank itself: k_probe's record at its edge)
        exp, eoff = parity.oracle_encode_docs(O.Encoder(ov, N.CL100K), docs)
        _batches[key] = (docs, exp, eoff)
    return _batches[key]


def compare_docs(got, docs, exp, eoff, what):
    ids, ooff = got
    if ids.tolist() != exp or ooff.tolist() != eoff:
        for i in range(len(docs)):
            g, x = ids[ooff[i]:ooff[i + 1]].tolist(), exp[eoff[i]:eoff[i + 1]]
            assert g == x and ooff[i] == eoff[i], "%s doc %d (len %d): got %r... expected %r..." % (what, i, len(docs[i]), g[:12], x[:12])
        raise AssertionError(what + ": trailing mismatch")


def check_single_launch(lib, O, top):
    """3 documents of 40 pool words: k_small takes the call and keeps it (its chunk form of the long-miss merger, its memo round), twice with one encoder."""
    v, ov = tables(lib, O, top)
    docs, exp, eoff = batch_case(O, ov, top, "small", 3)
    assert max(exp) == top and sum(map(len, docs)) <= SMALL_MAX_BYTES
    enc = N.Encoder(v, N.CL100K)
    data, offs = parity.pack(docs)
    for rep in range(2):
        c0 = enc.small_path_calls()
        compare_docs(enc.encode_batch(data, offs), docs, exp, eoff, "single launch, top %#x, call %d" % (top, rep))
        c1 = enc.small_path_calls()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0), "call %d: taken by the single launch and not handed back: %r -> %r" % (rep, c0, c1)


def check_batch_sequence(lib, O, top, n_docs, max_bytes=None):
    """A batch just too large for the single launch: k_probe's records, k_merge_short's memo round (the second call hits the memo), k_place's fast and general
    paths under ranks up to `top`; the same batch as UTF-16 and back through the sparse-id decode table."""
    v, ov = tables(lib, O, top)
    docs, exp, eoff = batch_case(O, ov, top, "batch", n_docs)
    total = sum(map(len, docs))
    assert total > SMALL_MAX_BYTES and (max_bytes is None or total <= max_bytes), total
    assert max(exp) == top and max(np.diff(eoff[-3:])) >= 70
    enc = N.Encoder(v, N.CL100K)
    enc.set_option(N.OPT_PROMOTE, 0)                             # (the promotion gate has its own test: here the memo answers)
    data, offs = parity.pack(docs)
    c0 = enc.small_path_calls()
    for rep in range(2):
        compare_docs(enc.encode_batch(data, offs), docs, exp, eoff, "batch sequence, top %#x, call %d" % (top, rep))
    assert enc.small_path_calls() == c0, "the single launch must not take %d bytes" % total
    units = data.astype(np.uint16)                               # (ASCII: a code unit a byte)
    compare_docs(enc.encode_batch_utf16(units, offs), docs, exp, eoff, "batch sequence as UTF-16, top %#x" % top)
    back, boffs = enc.decode_batch(np.asarray(exp, np.int32), np.asarray(eoff, np.int64))
    assert back.tobytes() == data.tobytes() and boffs.tolist() == offs.tolist(), "decode(encode(x)) != x under top %#x" % top


# ---- the promotion gate ------------------------------------------------------------------------------------------------------------
def promo_batches(top, n_batches, nbytes=160_000):
    """The same repeated text for both sides of kPromoFlag: words over abc that miss the table and merge into a few tokens."""
    rng = random.Random(PROMO_FLAG * 31 + 5)
    lex = sorted({"".join(rng.choice("abc") for _ in range(rng.randint(4, 11))) for _ in range(300)})
    out = []
    for _ in range(n_batches):
        docs, size = [], 0
        while size < nbytes:
            n = rng.choice([300, 2000, 9000])
            words = []
            while sum(map(len, words)) < n:
                words.append(rng.choice([" ", " ", "\n", ", "]) + rng.choice(lex))
            docs.append("".join(words).encode())
            size += len(docs[-1])
        out.append(docs)
    return out


def check_promotion_gate(lib, O, top, n_batches=4):
    """Below kPromoFlag the learning batch promotes hot memo entries into the key tables; from kPromoFlag on bit 26 of a record is part of a rank, and the host
    promotes nothing -- automatically or by hand.  The ids are the oracle's before and after."""
    assert top in (PROMO_FLAG - 1, PROMO_FLAG)
    v, ov = tables(lib, O, top)
    oenc = O.Encoder(ov, N.CL100K)
    enc = N.Encoder(v, N.CL100K)
    enc.set_option(N.OPT_PROMOTE_MIN_BYTES, 100_000)
    seen = []
    for k, docs in enumerate(promo_batches(top, n_batches)):
        data, offs = parity.pack(docs)
        exp, eoff = parity.oracle_encode_docs(oenc, docs)
        compare_docs(enc.encode_batch(data, offs), docs, exp, eoff, "promotion gate, top %#x, batch %d" % (top, k))
        seen.append(enc.adapt_stats())
    st = seen[-1]
    if top < PROMO_FLAG:
        assert st["promotions"] == 1 and st["promoted_pieces"] > 0, seen
        first = next(k for k, s in enumerate(seen) if s["promotions"] == 1)
        assert first < n_batches - 1, "no batch ran on the installed tables: %r" % (seen,)
    else:
        assert all(s["promotions"] == 0 and s["promoted_pieces"] == 0 for s in seen), seen
        enc.set_option(N.OPT_PROMOTE, 2)                         # by hand: whatever the memo holds -- still nothing
        st = enc.adapt_stats()
        assert st["promotions"] == 0 and st["promoted_pieces"] == 0, st
        enc.set_option(N.OPT_PIECE_STATS, 1)
        enc.piece_stats(reset=True)
        compare_docs(enc.encode_batch(data, offs), docs, exp, eoff, "promotion gate, top %#x, after a promotion by hand" % top)
        assert enc.piece_stats()["promoted_pieces_in_tables"] == 0


# ---- the rejection edge ------------------------------------------------------------------------------------------------------------
def check_rejection_edge(lib, O):
    """TKZ_MAX_RANK is the DEVICE's own bound -- (rank << 5 | 31) in tkz_bpe_lane_f<32>, rank | len << 27 in the SHORT / MID slots, the 28-bit rank field of a
    piece record --; the reference and the oracle take any int."""
    line = lambda key, rank: base64.b64encode(key) + b" " + str(rank).encode() + b"\n"
    good = b"".join(line(bytes([b]), 1000 + b) for b in range(256))
    over = MAX_RANK + 1
    for raw, lineno in ((line(b"ab", over), 1), (good + line(b"ab", over), 257)):
        with pytest.raises(N.UnsupportedError) as ei:
            N.Vocab(raw, lib)
        assert ei.value.code == N.E_UNSUPPORTED and "(line %d)" % lineno in str(ei.value) and str(over) in str(ei.value), str(ei.value)
        assert O.Vocab(raw).rank(b"ab") == over                  # (no such limit there)
    v = N.Vocab(good + line(b"ab", MAX_RANK), lib)
    assert len(v) == 257 and v.rank(b"ab") == MAX_RANK
    for neg in (-1, -MAX_RANK):
        with pytest.raises(N.TkzError) as ei:
            N.Vocab(good + line(b"ab", neg), lib)
        assert ei.value.code in (N.E_UNSUPPORTED, N.E_FORMAT) and "(line 257)" in str(ei.value)
    for big in (1 << 31, 1 << 32, (1 << 32) + 5, 10 ** 19, 10 ** 30):        # beyond int: int.TryParse fails, a FormatException in the reference
        with pytest.raises(N.FormatError) as ei:
            N.Vocab(good + line(b"ab", big), lib)
        assert ei.value.code == N.E_FORMAT and "(line 257)" in str(ei.value), str(ei.value)
