"""Encode(text, allowedSpecial) for ONE string in a single launch (tkz_encode_special_utf8 / _utf16, k_small's special form): the cases the emulated (CPU)
and the GPU test modules share.  Every result is compared with the oracle's encode(text, allowed), one text per call; where it says so a case also pins
the ROUTE the call took, read from tkz_encoder_small_path_calls (calls, handed back) and tkz_encoder_special_stats (batches, literals)."""
import base64
import random
import threading

import numpy as np
import pytest

import parity
import special_cases as SC
import u16_special_cases as UC
from tokenizer_amd import _native as N

SMALL_MAX, SMALL_MAX_O200K_DOC = 131072, 1024      # tkz_kernels.h: kSmallMaxBytes, kSmallMaxDoc (o200k's single-launch limit for one document)
LIT_BLOCK = 2048                                   # tkz_kernels.hip: kSmallLitBlock, the text stage of the literal scan inside k_small
LAUNCH, HANDED, BATCH = (1, 0), (1, 1), (0, 0)     # what a call adds to small_path_calls


def single_call(enc):
    """the single-text entry as a special_cases.compare() call on a batch of one document"""
    def call(data, offs, index):
        assert len(offs) == 2
        ids = enc.encode_special(np.asarray(data, np.uint8).tobytes(), index)
        return np.asarray(ids, np.int64), np.asarray([0, len(ids)], np.int64)
    return call


def single_call_u16(enc):
    def call(flat, offs, index):
        assert len(offs) == 2
        ids = enc.encode_special_utf16([int(u) for u in flat], index)
        return np.asarray(ids, np.int64), np.asarray([0, len(ids)], np.int64)
    return call


def eligible(pattern, nbytes):
    """small_eligible for one document, as tkz_api.cpp states it"""
    return 0 < nbytes <= (SMALL_MAX if pattern in (1, 2) else SMALL_MAX_O200K_DOC)


def check(enc, oenc, specials, allowed, doc, what, route=None, count_literals=False):
    """one text through the single entry against the oracle; route: None, or what the call must add to small_path_calls"""
    c0, s0 = enc.small_path_calls(), enc.special_stats()
    SC.compare(enc, oenc, specials, allowed, [doc], what, call=single_call(enc))
    c1, s1 = enc.small_path_calls(), enc.special_stats()
    moved = (c1[0] - c0[0], c1[1] - c0[1])
    if route is not None:
        assert moved == route, "%s: small_path_calls moved by %s, expected %s" % (what, moved, route)
    index = SC.indices(specials, allowed)
    if not index:
        assert s1 == s0, "%s: a call that allows nothing moved the special stats" % what
    else:
        assert s1[0] - s0[0] == 1, "%s: special batches moved by %d" % (what, s1[0] - s0[0])
        if count_literals:
            ids = set(specials[a] for a in allowed)
            n_lit = sum(1 for i in oenc.encode(doc, list(allowed)) if i in ids)
            assert s1[1] - s0[1] == n_lit, "%s: special literals moved by %d, the oracle's result holds %d" % (what, s1[1] - s0[1], n_lit)
    return moved


# ---- a. edge documents --------------------------------------------------------------------------------------------------------------------------------------

GIANT_EDGE = ("x" * 1500, " " * 1500, "=" * 1200)      # the edge documents with a piece of more than 1024 bytes: handed back


def check_edge_docs(lib, O, v, ov, name, pattern):
    specials = SC.SPECIAL_SETS[name]
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    for allowed in SC.allowed_choices(specials):
        for k, doc in enumerate(SC.edge_docs(specials, o200k=pattern in (3, 4))):
            n = len(doc.encode("utf-8"))
            if not eligible(pattern, n):
                route = BATCH
            elif any(g in doc for g in GIANT_EDGE):
                route = HANDED
            else:
                route = LAUNCH
            check(enc, oenc, specials, allowed, doc, "%s pattern %d allowed %s document %d" % (name, pattern, allowed, k), route, count_literals=True)


# ---- b. order and overlaps ----------------------------------------------------------------------------------------------------------------------------------

def check_order(lib, O, v, ov, pattern):
    for specials, allowed_sets, docs in SC.order_cases():
        enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
        for allowed in allowed_sets:
            for doc in docs:
                check(enc, oenc, specials, allowed, doc, "%s allowed %s pattern %d %r" % (list(specials), allowed, pattern, doc[:40]))
    # a run that one lane walks: every second byte of 8 KiB heads a candidate, all of them one run
    specials = {"aa": 2001}
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    for n in (8192, 8191):
        check(enc, oenc, specials, ["aa"], "a" * n, "a run of %d" % n, LAUNCH if pattern in (1, 2) else BATCH)


# ---- c. seams -----------------------------------------------------------------------------------------------------------------------------------------------

def seam_docs(full):
    """the literal at every offset across a 64-byte row, a sub-tile, the literal scan's text stage inside k_small, a pre-tokenizer block, a k_merge_short group
    and the sixteen text stages of one round of the literal scan
    (full: every offset everywhere -- the GPU; else the two large ones at the offsets where the literal touches, straddles and leaves the edge)"""
    some = None if full else (0, 1, 6, 12, 13)
    return SC.boundary_docs(SC.EOT, (64, 1024, LIT_BLOCK)) + SC.boundary_docs(SC.EOT, (4096, 16384, 16 * LIT_BLOCK), shifts=some)


def check_seams(lib, O, v, ov, pattern, full):
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    for doc in seam_docs(full):
        check(enc, oenc, specials, [SC.EOT], doc, "boundary, %d bytes, pattern %d" % (len(doc), pattern), LAUNCH if eligible(pattern, len(doc)) else BATCH, count_literals=True)


def check_64k(lib, O, v, ov, pattern):
    """one document with the literal across byte 65,536: patterns 1 and 2 take the launch, o200k the batch path; the ids are the oracle's either way"""
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    doc = SC.boundary_docs(SC.EOT, (65536,), shifts=(6,))[0]
    assert len(doc) < SMALL_MAX
    check(enc, oenc, specials, [SC.EOT], doc, "65,536 boundary, pattern %d" % pattern, LAUNCH if pattern in (1, 2) else BATCH, count_literals=True)


# ---- d. segments --------------------------------------------------------------------------------------------------------------------------------------------

def check_segments(lib, O, v, ov, pattern):
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    E = SC.EOT
    docs = [E + "tail of it", "head of it" + E, E, E + E, "x" + E + E + "y",
            "a   " + E + "   b", "\n\n" + E + "\n", "a   " + E, E + "   b", "a \n " + E + " \n b", "1234" + E + "5678", "it" + E + "'s"]
    for doc in docs:
        check(enc, oenc, specials, [E], doc, "segments pattern %d %r" % (pattern, doc), LAUNCH, count_literals=True)
        check(enc, oenc, specials, [], doc, "segments, nothing allowed, pattern %d %r" % (pattern, doc), LAUNCH)


# ---- e. literals outside the vocabulary ---------------------------------------------------------------------------------------------------------------------

def check_outside_vocabulary(lib, O):
    raw = b"".join(base64.b64encode(k) + b" %d\n" % r for r, k in enumerate([b"a", b"b", b"c", b" ", b"ab", b"bc", b" a", b"abc", b"ca"]))      # a tiny rank table
    v, ov = N.Vocab(raw, lib), O.Vocab(raw)
    specials = {"<|z|>": 900, "zz": 901}
    for pattern in SC.PATTERNS:
        enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
        for doc in ["abc<|z|>cab", "<|z|>", "zzabzz", "a zz b<|z|>"]:
            check(enc, oenc, specials, list(specials), doc, "pattern %d %r" % (pattern, doc), LAUNCH, count_literals=True)      # allowed: the ids come from the table
        c0 = enc.small_path_calls()
        with pytest.raises(N.KeyNotFoundError):                  # not allowed: text whose bytes no key holds -- the kernel hands the call back, the batch path names the error
            enc.encode_special(b"abc<|z|>cab", [1])
        c1 = enc.small_path_calls()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == HANDED


# ---- f. hand-back -------------------------------------------------------------------------------------------------------------------------------------------

def check_hand_back(lib, O, v, ov, pattern):
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    rng = random.Random(9)
    giant = "q" * 1100                                            # one piece of more than 1024 bytes
    missed = "".join(rng.choice("bcdfghjklmnpqrstvwxz") for _ in range(300))        # one piece of 300 bytes that no key holds: over kSmallLanePiece
    for doc in ("go " + SC.EOT + giant + " on", giant + SC.EOT, "go " + SC.EOT + " " + missed + " on" + SC.EOT):
        check(enc, oenc, specials, [SC.EOT], doc, "hand-back pattern %d, %d bytes" % (pattern, len(doc)), HANDED, count_literals=True)


# ---- g. the UTF-16 entry ------------------------------------------------------------------------------------------------------------------------------------

def check_u16(lib, O, v, ov, pattern):
    """the lone-surrogate documents, one string per call: with a literal that holds U+FFFD registered (the replaced-byte bitmap travels to the kernel) and with
    none (nothing is built)"""
    for specials, sets in ((UC.FFFD_SPECIALS, ([UC.A, UC.B, UC.C], [UC.A], [UC.A, UC.C], [UC.B], [UC.C])), ({UC.B: 60002, "<|e|>": 60009}, ([UC.B, "<|e|>"], [UC.B]))):
        enc = N.Encoder(v, pattern)
        enc.set_special_tokens(specials)
        exp = UC.Expect(O, ov, pattern, specials)
        docs = UC.lone_docs() + [UC.units("x") + [UC.HI], [UC.LO] + UC.units("x"), UC.units("x�"), UC.units("a <|e|> b"), UC.fill(LIT_BLOCK - 1) + UC.units("x") + [UC.HI] + UC.units("x�")]
        for allowed in sets:
            for k, d in enumerate(docs):
                c0, s0 = enc.small_path_calls(), enc.special_stats()
                UC.compare_special(enc, exp, specials, allowed, [d], "UTF-16 pattern %d allowed %s document %d" % (pattern, allowed, k), call=single_call_u16(enc))
                c1, s1 = enc.small_path_calls(), enc.special_stats()
                assert (c1[0] - c0[0], c1[1] - c0[1]) == (LAUNCH if eligible(pattern, UC.utf8_len(d)) else BATCH) and s1[0] - s0[0] == 1
    if pattern == 1:      # what the bitmap is there for, stated without the oracle
        UC.lone_expectations(UC.Expect(O, ov, pattern, UC.FFFD_SPECIALS))


# ---- h. memo and promotions ---------------------------------------------------------------------------------------------------------------------------------

def check_memo(lib, O, v, ov):
    specials = {"<|q|>": 60001, "zqzq": 60002}
    enc, oenc = SC.make_encoders(lib, O, v, ov, 2, specials)
    enc.set_option(N.OPT_PIECE_STATS, 1)
    enc.set_option(N.OPT_PROMOTE, 0)
    enc.piece_stats(reset=True)
    check(enc, oenc, specials, list(specials), "<|q|>zqzq" * 500, "dense in literals", LAUNCH)
    st = enc.piece_stats(reset=True)
    assert (st["pieces"], st["short_misses"], st["long_misses"], st["memo_lookups"]) == (1000, 0, 0, 0), st


# ---- i. arguments -------------------------------------------------------------------------------------------------------------------------------------------

def check_arguments(lib, O, v, ov):
    text = b"hello <|endoftext|> you"
    u = UC.units(text.decode())
    for specials in ({"<|s%d|>" % i: 70000 + i for i in range(257)}, {"<|" + "x" * 126 + "|>": 70000, SC.EOT: 50256}, {"<|big|>": 1 << 26}):
        enc, oenc = SC.make_encoders(lib, O, v, ov, 1, specials)
        with pytest.raises(N.UnsupportedError):
            enc.encode_special(text, [0])
        with pytest.raises(N.UnsupportedError):
            enc.encode_special_utf16(u, [0])
        assert enc.encode_special(text, []) == enc.encode_utf8(text) and enc.special_stats() == (0, 0)
    specials = SC.SPECIAL_SETS["synth100k"]
    enc, oenc = SC.make_encoders(lib, O, v, ov, 1, specials)
    eot = SC.indices(specials, [SC.EOT])
    for bad in ([5], [-1], [0, 0], [1, 2, 1]):
        for call, arg in ((enc.encode_special, text), (enc.encode_special_utf16, u)):
            with pytest.raises(N.TkzError) as ei:
                call(arg, bad)
            assert ei.value.code == N.E_ARG
    assert enc.special_stats() == (0, 0)
    # nothing allowed: the plain entries' ids by the plain entries' launch; the special stats do not move
    c0 = enc.small_path_calls()
    assert enc.encode_special(text, []) == enc.encode_utf8(text) == oenc.encode(text.decode(), [])
    assert enc.encode_special_utf16(u, []) == enc.encode_utf16(u) == oenc.encode(text.decode(), [])
    c1 = enc.small_path_calls()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (4, 0) and enc.special_stats() == (0, 0)
    # nothing registered
    bare = N.Encoder(v, 1)
    assert bare.encode_special(text, [0]) == bare.encode_utf8(text) and bare.special_stats() == (0, 0)
    # a capacity that is too small: the required count; the launch's and the batch path's
    want = oenc.encode(text.decode(), [SC.EOT])
    for body in (text, text + b" " + b"q" * 1100):              # (a piece of more than 1024 bytes: handed back)
        n = len(oenc.encode(body.decode(), [SC.EOT]))
        for call, arg in ((enc.encode_special, body), (enc.encode_special_utf16, UC.units(body.decode()))):
            with pytest.raises(N.TkzError) as ei:
                call(arg, eot, out_cap=n - 1)
            assert ei.value.code == N.E_CAPACITY and ei.value.needed == n
            assert len(call(arg, eot, out_cap=n)) == n
    assert enc.encode_special(text, eot) == want and enc.encode_special_utf16(u, eot) == want
    # no text at all
    assert enc.encode_special(b"", eot) == [] and enc.encode_special_utf16([], eot) == [] and enc.encode_special(b"", []) == []


# ---- j. threads ---------------------------------------------------------------------------------------------------------------------------------------------

def check_threads(lib, O, v, ov, pattern):
    specials = {SC.EOT: 50256}
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    docs = SC.side_by_side_inputs()[0]
    expect = {True: [oenc.encode(d, [SC.EOT]) for d in docs], False: [oenc.encode(d, []) for d in docs]}
    assert expect[True] != expect[False]
    errors = []

    def work(special):
        try:
            for r in range(SC.ROUNDS):
                for k, d in enumerate(docs):
                    got = enc.encode_special(d.encode(), [0]) if special else enc.encode_utf8(d.encode())
                    if got != expect[special][k]:
                        errors.append("%s call, text %d, round %d: not the oracle's result" % ("special" if special else "plain", k, r))
        except Exception as ex:          # (a thread's exception would otherwise be lost)
            errors.append(repr(ex))
    c0 = enc.small_path_calls()
    threads = [threading.Thread(target=work, args=(s,)) for s in (True, False)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]
    c1 = enc.small_path_calls()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2 * SC.ROUNDS * len(docs), 0)
    assert enc.special_stats() == (SC.ROUNDS * len(docs), SC.ROUNDS * len(docs))


# ---- k. the Python mirror -----------------------------------------------------------------------------------------------------------------------------------

def check_python_mirror(lib, O, raw):
    from tokenizer_amd.tokenizer import TikTokenizer, REGEX_CL100K
    specials = SC.SPECIAL_SETS["synth100k"]
    tok = TikTokenizer(raw, specials, REGEX_CL100K, lib=lib)
    oenc = O.Encoder(O.Vocab(raw), 2, specials=specials)
    names = list(specials)
    text = "Hello <|endoftext|> World<|fim_prefix|>"
    for allowed in (True, names, names[:2], [names[4]]):
        want = names if allowed is True else allowed
        c0, s0 = tok._encoder.small_path_calls(), tok._encoder.special_stats()
        assert tok.Encode(text, allowed) == oenc.encode(text, want)
        c1, s1 = tok._encoder.small_path_calls(), tok._encoder.special_stats()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == LAUNCH and s1[0] - s0[0] == 1, allowed      # ONE launch
    # a set beyond the device path: the host segmentation, same ids
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TikTokenizer(raw, many, REGEX_CL100K, lib=lib)
    oenc2 = O.Encoder(O.Vocab(raw), 2, specials=many)
    t = "a<|s7|>b <|s299|><|s30|"
    assert tok2.Encode(t, True) == oenc2.encode(t, list(many)) and tok2._special_on_host and tok2._encoder.special_stats() == (0, 0)
    assert tok2.Encode(t, ["<|s7|>"]) == oenc2.encode(t, ["<|s7|>"])
    # a lone surrogate while a literal holds U+FFFD: the host segmentation, as EncodeBatchFlat has it
    fffd = {"<�>": 300001}
    tok3 = TikTokenizer(raw, fffd, REGEX_CL100K, lib=lib)
    assert tok3.Encode("a<�>b", True) == O.Encoder(O.Vocab(raw), 2, specials=fffd).encode("a<�>b", list(fffd))
    assert tok3._encoder.special_stats()[0] == 1
    assert 300001 not in tok3.Encode("a<\ud800>b", True) and tok3._encoder.special_stats()[0] == 1


# ---- l. random ----------------------------------------------------------------------------------------------------------------------------------------------

def check_random(lib, O, v, ov, name, pattern, seeds, n_docs=6):
    specials = SC.SPECIAL_SETS[name]
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    for seed in range(seeds):
        rng = random.Random(7000 * pattern + seed)
        allowed = rng.choice(SC.allowed_choices(specials))
        for k, doc in enumerate(SC.random_docs(rng, specials, n_docs, 3000)):
            n = len(doc.encode("utf-8"))
            moved = check(enc, oenc, specials, allowed, doc, "%s pattern %d seed %d document %d allowed %s" % (name, pattern, seed, k, allowed), count_literals=True)
            assert moved[0] == (1 if eligible(pattern, n) else 0)
