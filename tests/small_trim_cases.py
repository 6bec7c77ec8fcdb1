"""EncodeTrimSuffix / EncodeTrimPrefix for ONE string in a single launch (tkz_encode_trim_utf8 / _utf16, k_small's trim form): the cases the emulated (CPU)
and the GPU test modules share.  Every result -- kept ids, cut_bytes, cut_units -- is compared exactly with trim_cases.Expect / u16_special_cases.Expect
(oracle.TrimOracle), one text per call; where it says so a case also pins the ROUTE the call took, read from tkz_encoder_small_path_calls (calls, handed back)."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import small_special_cases as SS
import special_cases as SC
import trim_cases as TC
import u16_special_cases as UC
from tokenizer_amd import _native as N

LAUNCH, HANDED, BATCH = SS.LAUNCH, SS.HANDED, SS.BATCH
SIDES = TC.SIDES
HUGE = 1 << 40
K_SUB = TC.K_SUB
TRIM_MAX = 98304                                   # tkz_kernels.h: kSmallTrimMaxBytes -- the trim entries take the launch up to 96 KiB, not the plain entries' 128 KiB


def eligible(pattern, nbytes):
    """what the trim entries send through the launch (tkz_api.cpp: trim_small): small_eligible for one document, and at most kSmallTrimMaxBytes"""
    return SS.eligible(pattern, nbytes) and nbytes <= TRIM_MAX


def moved(c0, c1):
    return (c1[0] - c0[0], c1[1] - c0[1])


def check(enc, exp, specials, allowed, doc, side, mx, what, route=None):
    """one text through the single entry against the oracle; route: None, or what the call must add to small_path_calls.  Returns (ids, cut_bytes, cut_units)."""
    c0 = enc.small_path_calls()
    got = enc.encode_trim(doc.encode("utf-8"), SC.indices(specials, allowed), side, mx)
    c1 = enc.small_path_calls()
    want = exp.trim(doc, allowed, side, mx)
    what = "%s, side %d, max %d, allowed %s" % (what, side, mx, allowed)
    for name, g, w in zip(("cut_bytes", "cut_units", "ids"), (got[1], got[2], got[0]), (want[1], want[2], want[0])):
        assert g == w, "%s: %s differ: got %s, expected %s" % (what, name, g if name != "ids" else g[:12], w if name != "ids" else w[:12])
    if route is not None:
        assert moved(c0, c1) == route, "%s: small_path_calls moved by %s, expected %s" % (what, moved(c0, c1), route)
    return got


def route_of(pattern, doc):
    n = len(doc.encode("utf-8"))
    if not eligible(pattern, n):
        return BATCH
    return HANDED if any(g in doc for g in SS.GIANT_EDGE) else LAUNCH


# ---- a. sweep -----------------------------------------------------------------------------------------------------------------------------------------------

def sweep_maxima(count, full):
    """full: every maximum from 0 to count + 1 and one far above -- every text that takes the LAUNCH on the GPU, whatever its token count.  Else the maxima
    around 0 and around the count: every text on the emulator, and the texts that never reach the new cut phase -- the edge documents with a piece of more
    than 1024 bytes (400 .. 1,300 tokens), which the kernel hands back in front of it, and a text beyond the launch's limit: their results are the batch
    path's, which tests/test_*_trim.py sweep."""
    if full:
        return list(range(count + 2)) + [HUGE]
    return sorted(set([0, 1, 2] + [m for m in (count // 2, count - 1, count, count + 1) if m >= 0])) + [HUGE]


def check_sweep(lib, O, v, ov, name, pattern, full):
    specials = SC.SPECIAL_SETS[name]
    enc, _ = SC.make_encoders(lib, O, v, ov, pattern, specials)
    exp = TC.Expect(O, ov, pattern, specials)
    docs = TC.REFERENCE_TEXTS + [d for d in SC.edge_docs(specials, o200k=pattern in (3, 4)) if d]
    choices = SC.allowed_choices(specials)
    for allowed in (choices if full else choices[:2]):
        for k, doc in enumerate(docs):
            route = route_of(pattern, doc)
            for mx in sweep_maxima(exp.count(doc, allowed), full and route == LAUNCH):
                for side in SIDES:
                    check(enc, exp, specials, allowed, doc, side, mx, "%s pattern %d document %d" % (name, pattern, k), route)


# ---- b. items that are never split ----------------------------------------------------------------------------------------------------------------------------

def check_items(lib, O, v, ov, pattern):
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, _ = SC.make_encoders(lib, O, v, ov, pattern, specials)
    exp = TC.Expect(O, ov, pattern, specials)
    E = SC.EOT
    # a piece of several tokens astride the maximum: dropped whole for suffix, the boundary for prefix
    emoji = "ab 😀 cd"
    n_head, n_piece = exp.count("ab", []), exp.count(" 😀", [])
    assert n_piece >= 2, "the reference's example piece has several tokens"
    for mx in range(n_head + n_piece + 2):
        ids, cb, cu = check(enc, exp, specials, [], emoji, N.TRIM_SUFFIX, mx, "multi-token piece, pattern %d" % pattern, LAUNCH)
        if n_head <= mx < n_head + n_piece:
            assert (len(ids), cb) == (n_head, 2), (mx, ids, cb)                   # not one token of the piece is kept
        ids, cb, cu = check(enc, exp, specials, [], emoji, N.TRIM_PREFIX, mx, "multi-token piece, pattern %d" % pattern, LAUNCH)
        total = exp.count(emoji, [])
        if total - n_head - n_piece < mx < total - n_head:
            assert cb == 2 + len(" 😀".encode()), (mx, cb)                        # the whole piece goes with what is in front of it
    # an allowed literal exactly at the maximum, one before it and one after it; not allowed, it is plain text of several tokens
    doc = "one two" + E + "three four"
    n_front = exp.count("one two", [])
    assert exp.count(E, []) >= 2
    for allowed in ([E], []):
        for mx in (n_front - 1, n_front, n_front + 1, n_front + 2):
            for side in SIDES:
                ids, cb, cu = check(enc, exp, specials, allowed, doc, side, mx, "literal at the maximum, pattern %d" % pattern, LAUNCH)
                if side == N.TRIM_SUFFIX and allowed and mx == n_front + 1:
                    assert ids[-1] == specials[E] and cb == len("one two" + E)     # ONE item of ONE token
                if side == N.TRIM_SUFFIX and not allowed and mx == n_front + 1:
                    assert cb == len("one two")                                     # several tokens: it does not fit


# ---- c. seams of the cut ----------------------------------------------------------------------------------------------------------------------------------------

UNIT = "ab cd "


def seam_text(O, pattern, length, target):
    """(text, piece starts) of `length` bytes of the repeated unit, shifted so that a piece starts at byte `target`"""
    for shift in range(len(UNIT)):
        text = (UNIT * (length // len(UNIT) + 3))[shift:shift + length]
        starts = set(a for a, _ in O.split_utf8(pattern, text.encode()))
        if target in starts:
            return text, starts
    raise AssertionError("no shift of the unit puts a piece start at byte %d" % target)


def check_cut_at(enc, exp, specials, text, target, what):
    """the maximum from the oracle's count of the prefix: the cut must sit at byte `target`, both sides"""
    front, count = exp.count(text[:target], []), exp.count(text, [])
    assert 0 < front < count
    n = len(text)
    ids, cb, cu = check(enc, exp, specials, [], text, N.TRIM_SUFFIX, front, what, LAUNCH if eligible(exp.oracle.pattern, n) else BATCH)
    assert (cb, cu, len(ids)) == (target, target, front), (what, cb, cu, len(ids), target, front)
    ids, cb, cu = check(enc, exp, specials, [], text, N.TRIM_PREFIX, count - front, what, LAUNCH if eligible(exp.oracle.pattern, n) else BATCH)
    assert (cb, cu, len(ids)) == (target, target, count - front), (what, cb, cu, len(ids), target, count - front)


def check_seams(lib, O, v, ov, pattern, full):
    """the cut on, one before and one after a bitmap word edge (64), a sub-tile edge (1,024: tile_base takes over from doc_tok), 4,096 bytes (the workgroup goes
    from 256 to 1,024 threads, nsub 4 -> 5: the text is made to END just behind the seam as well), a k_merge_short group (16,384) and 65,536; o200k: the first
    two.  full False: the two large seams on the edge only."""
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, _ = SC.make_encoders(lib, O, v, ov, pattern, specials)
    exp = TC.Expect(O, ov, pattern, specials)
    seams = (64, 1024) if pattern in (3, 4) else (64, 1024, 4096, 16384, 65536)
    for B in seams:
        for delta in ((-1, 0, 1) if full or B <= 4096 else (0,)):
            length = B + 150                                     # (o200k at 1,024: beyond its launch -- the batch path, the same result)
            if B + delta + 3 >= length:
                continue
            text, _ = seam_text(O, pattern, length, B + delta)
            check_cut_at(enc, exp, specials, text, B + delta, "cut at %d%+d of %d bytes, pattern %d" % (B, delta, length, pattern))
    if pattern in (1, 2):
        # the text's own end around 4,096: 4 sub-tiles and 256 threads up to it, 5 and 1,024 behind it; the cut in the last piece's front
        for length in (4095, 4096, 4097, 4100):
            text, starts = seam_text(O, pattern, length, 4090)
            check_cut_at(enc, exp, specials, text, 4090, "text of %d bytes, cut at 4090, pattern %d" % (length, pattern))
    # a piece that starts in one sub-tile and ends in the next: the cut at its front and at its back
    text = (UNIT * 400)[:K_SUB + 200] if pattern in (1, 2) else (UNIT * 400)[:SS.SMALL_MAX_O200K_DOC]
    if pattern in (3, 4):
        text = text[:1020] + "wxyz"                              # (o200k: 1 KiB in all -- the straddling piece is made at a 64-byte row's edge instead)
        edge = 960
    else:
        edge = K_SUB
    pieces = O.split_utf8(pattern, text.encode())
    across = [(a, n) for a, n in pieces if a < edge < a + n]
    assert len(across) == 1, across
    a, n = across[0]
    for target in (a, a + n):
        if 0 < target < len(text):
            check_cut_at(enc, exp, specials, text, target, "a piece across byte %d, cut at %d, pattern %d" % (edge, target, pattern))


# ---- d. cut_units -----------------------------------------------------------------------------------------------------------------------------------------------

def check_units(lib, O, v, ov, pattern):
    """texts of 2-, 3- and 4-byte characters, every maximum on both sides: the cut falls inside, at the end of and just past a 16-byte quad (asserted), a
    4-byte character -- two units -- is the last kept and the first dropped item at some maximum; all-ASCII text: units equal bytes"""
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, _ = SC.make_encoders(lib, O, v, ov, pattern, specials)
    exp = TC.Expect(O, ov, pattern, specials)
    for ch in ("é", "中", "😀"):
        seen = set()
        for head in ("", "a", "ab", "abc"):
            text = head + (" " + ch) * 14 + " end"
            for side in SIDES:
                for mx in range(exp.count(text, []) + 2):
                    ids, cb, cu = check(enc, exp, specials, [], text, side, mx, "%r-text, pattern %d" % (ch, pattern), LAUNCH)
                    seen.add(cb % 16)
                    assert cu == TC.utf16_len(text.encode()[:cb].decode())
        assert 0 in seen and 1 in seen and len(seen - {0, 1}) >= 2, (ch, seen)
    # the 4-byte character as the last kept item (suffix) and the first dropped one: two units each
    text = "ab" + "😀" + " cd"
    front = exp.count("ab", [])
    n_emoji = exp.count("ab😀", []) - front
    got = check(enc, exp, specials, [], text, N.TRIM_SUFFIX, front + n_emoji, "emoji last kept, pattern %d" % pattern, LAUNCH)
    assert (got[1], got[2]) == (6, 4)
    got = check(enc, exp, specials, [], text, N.TRIM_SUFFIX, front + n_emoji - 1, "emoji first dropped, pattern %d" % pattern, LAUNCH)
    assert (got[1], got[2]) == (2, 2)
    text = TC.prose(700)
    for mx in (0, 1, 50, 120, HUGE):
        for side in SIDES:
            got = check(enc, exp, specials, [], text, side, mx, "ASCII, pattern %d" % pattern, LAUNCH)
            assert got[1] == got[2]


# ---- e. route limits --------------------------------------------------------------------------------------------------------------------------------------------

def check_limits(lib, O, v, ov, pattern):
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, _ = SC.make_encoders(lib, O, v, ov, pattern, specials)
    exp = TC.Expect(O, ov, pattern, specials)
    # (the trim launch stops at TRIM_MAX, where the measured crossover with the batch trim path lies -- profiles/small_trim/README.md --, not at the plain
    #  launch's SMALL_MAX: the texts at and just above that limit take the batch path, with the oracle's results like every other)
    limit = TRIM_MAX if pattern in (1, 2) else SS.SMALL_MAX_O200K_DOC
    for n, route in ((limit, LAUNCH), (limit + 1, BATCH)) + (((SS.SMALL_MAX, BATCH), (SS.SMALL_MAX + 1, BATCH)) if pattern in (1, 2) else ()):
        text = TC.prose(n)
        for side in SIDES:
            check(enc, exp, specials, [SC.EOT], text, side, 1000 if pattern in (1, 2) else 100, "%d bytes, pattern %d" % (n, pattern), route)
    # no text at all
    c0 = enc.small_path_calls()
    for side in SIDES:
        for allowed in ([], [0]):
            assert enc.encode_trim(b"", allowed, side, 5) == ([], 0, 0)
            assert enc.encode_trim_utf16([], allowed, side, 5) == ([], 0)
    assert moved(c0, enc.small_path_calls()) == (0, 0)
    # one piece
    for mx in (0, 1, 2):
        for side in SIDES:
            check(enc, exp, specials, [], "hello", side, mx, "one piece, pattern %d" % pattern, LAUNCH)
            check(enc, exp, specials, [SC.EOT], SC.EOT, side, mx, "one literal, pattern %d" % pattern, LAUNCH)


# ---- f. hand-back -----------------------------------------------------------------------------------------------------------------------------------------------

def hand_back_docs():
    """small_special_cases.check_hand_back's three texts"""
    rng = random.Random(9)
    giant = "q" * 1100                                            # one piece of more than 1024 bytes
    missed = "".join(rng.choice("bcdfghjklmnpqrstvwxz") for _ in range(300))        # one piece of 300 bytes that no key holds: over kSmallLanePiece
    return ["go " + SC.EOT + giant + " on", giant + SC.EOT, "go " + SC.EOT + " " + missed + " on" + SC.EOT]


def check_hand_back(lib, O, v, ov, pattern):
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, _ = SC.make_encoders(lib, O, v, ov, pattern, specials)
    exp = TC.Expect(O, ov, pattern, specials)
    for doc in hand_back_docs():
        count = exp.count(doc, [SC.EOT])
        for mx in (count - 1, count, count + 1, 2):
            for side in SIDES:
                check(enc, exp, specials, [SC.EOT], doc, side, mx, "hand-back pattern %d, %d bytes" % (pattern, len(doc)), HANDED)


# ---- g. the UTF-16 entry ----------------------------------------------------------------------------------------------------------------------------------------

def check_u16(lib, O, v, ov, pattern):
    """the lone-surrogate documents and the text with a literal that holds U+FFFD, one string per call, every maximum 0..6 on both sides: with such a literal
    registered (the replaced-byte bitmap travels to the kernel) and with none.  A lone surrogate counts as one unit; the literal is not taken over a replaced
    surrogate (UC.Expect searches the string)."""
    for specials, sets in ((UC.FFFD_SPECIALS, ([UC.A, UC.B, UC.C], [UC.A], [UC.C])), ({UC.B: 60002, "<|e|>": 60009}, ([UC.B, "<|e|>"],))):
        enc = N.Encoder(v, pattern)
        enc.set_special_tokens(specials)
        exp = UC.Expect(O, ov, pattern, specials)
        docs = UC.lone_docs() + [UC.units("a <|e|> b \U0001F600 c")]
        for allowed in sets:
            index = SC.indices(specials, allowed)
            for k, d in enumerate(docs):
                route = LAUNCH if eligible(pattern, UC.utf8_len(d)) else BATCH
                for side in SIDES:
                    for mx in range(7):
                        c0 = enc.small_path_calls()
                        ids, cu = enc.encode_trim_utf16(d, index, side, mx)
                        assert moved(c0, enc.small_path_calls()) == route
                        want = exp.trim(d, allowed, side, mx)
                        assert (ids, cu) == (want[0], want[1]), ("UTF-16 pattern %d allowed %s document %d side %d max %d" % (pattern, allowed, k, side, mx), ids, cu, want)
    if pattern == 1:      # stated without the oracle: `x` + a lone high half -- two units, the surrogate one of them --, A allowed alone: plain text
        enc = N.Encoder(v, pattern)
        enc.set_special_tokens(UC.FFFD_SPECIALS)
        ids, cu = enc.encode_trim_utf16(UC.units("a x") + [UC.HI], [0], N.TRIM_SUFFIX, HUGE)
        assert cu == 4 and UC.FFFD_SPECIALS[UC.A] not in ids
        ids, cu = enc.encode_trim_utf16(UC.units("a x�"), [0], N.TRIM_SUFFIX, HUGE)
        assert cu == 4 and ids[-1] == UC.FFFD_SPECIALS[UC.A]


# ---- h. arguments and capacity ----------------------------------------------------------------------------------------------------------------------------------

def check_arguments(lib, O, v, ov):
    text = b"hello <|endoftext|> you"
    u = UC.units(text.decode())
    for specials in ({"<|s%d|>" % i: 70000 + i for i in range(257)}, {"<|" + "x" * 126 + "|>": 70000, SC.EOT: 50256}, {"<|big|>": 1 << 26}):
        enc, _ = SC.make_encoders(lib, O, v, ov, 1, specials)
        with pytest.raises(N.UnsupportedError):
            enc.encode_trim(text, [0], N.TRIM_SUFFIX, 3)
        with pytest.raises(N.UnsupportedError):
            enc.encode_trim_utf16(u, [0], N.TRIM_PREFIX, 3)
    specials = SC.SPECIAL_SETS["synth100k"]
    enc, _ = SC.make_encoders(lib, O, v, ov, 1, specials)
    exp = TC.Expect(O, ov, 1, specials)
    eot = SC.indices(specials, [SC.EOT])
    bad_calls = [(b, N.TRIM_SUFFIX, 3) for b in ([5], [-1], [0, 0], [1, 2, 1])] + [(eot, 2, 3), (eot, -1, 3), (eot, N.TRIM_SUFFIX, -1), (eot, N.TRIM_PREFIX, -7), ([], 5, 3), ([], N.TRIM_PREFIX, -1)]
    for index, side, mx in bad_calls:
        for call, arg in ((enc.encode_trim, text), (enc.encode_trim_utf16, u)):
            with pytest.raises(N.TkzError) as ei:
                call(arg, index, side, mx)
            assert ei.value.code == N.E_ARG, (index, side, mx)
    assert enc.special_stats() == (0, 0) and enc.small_path_calls() == (0, 0)
    # nothing allowed, nothing registered: the plain trim, and the special stats do not move
    bare = N.Encoder(v, 1)
    for side in SIDES:
        for mx in (0, 2, 4, HUGE):
            want = exp.trim(text.decode(), [], side, mx)
            assert enc.encode_trim(text, [], side, mx) == tuple(want) == bare.encode_trim(text, [0], side, mx)
            assert enc.encode_trim_utf16(u, [], side, mx) == (want[0], want[2]) == bare.encode_trim_utf16(u, [0], side, mx)
    assert enc.special_stats() == (0, 0) and bare.special_stats() == (0, 0)
    # a 5,000-token text cut to 3: room for 3 is enough, room for 2 reports 3 -- on the launch and on a text that is handed back
    long_text = "a\n" * 2500
    assert exp.count(long_text, []) == 5000
    for body, route in ((long_text, LAUNCH), ("a\n" * 1250 + "q" * 1100 + "\na" * 1250, HANDED)):       # (the giant piece in the middle: either side keeps 3)
        for side in SIDES:
            for call, arg in ((enc.encode_trim, body.encode()), (enc.encode_trim_utf16, UC.units(body))):
                c0 = enc.small_path_calls()
                got = call(arg, eot, side, 3, out_cap=3)
                assert got[0] == exp.trim(body, [SC.EOT], side, 3)[0] and len(got[0]) == 3
                with pytest.raises(N.TkzError) as ei:
                    call(arg, eot, side, 3, out_cap=2)
                assert ei.value.code == N.E_CAPACITY and ei.value.needed == 3
                m = moved(c0, enc.small_path_calls())
                assert m == (2 * route[0], 2 * route[1]), (m, route)
    # a capacity failure moves the special stats by what it moves them through the batch entry (the literals are counted, the batch is not)
    lit_text = (SC.EOT + " a") * 40
    data, offs2 = np.frombuffer(lit_text.encode(), np.uint8), np.asarray([0, len(lit_text)], np.int64)
    deltas = []
    for call in (lambda: enc.encode_batch_trim(data, offs2, eot, N.TRIM_PREFIX, 9, out_cap=4), lambda: enc.encode_trim(lit_text.encode(), eot, N.TRIM_PREFIX, 9, out_cap=4)):
        s0 = enc.special_stats()
        with pytest.raises(N.TkzError) as ei:
            call()
        assert ei.value.code == N.E_CAPACITY and ei.value.needed == 9
        s1 = enc.special_stats()
        deltas.append((s1[0] - s0[0], s1[1] - s0[1]))
    assert deltas[0] == deltas[1] == (0, 40), deltas
    # cut_bytes / cut_units NULL through the raw export
    ids = np.zeros(8, np.int32)
    n = C.c_int64(0)
    buf = np.frombuffer(text, np.uint8)
    uu = np.asarray(u, np.uint16)
    idx = np.asarray(eot, np.int32)
    want = exp.trim(text.decode(), [SC.EOT], N.TRIM_SUFFIX, 2)
    lib.check(lib.L.tkz_encode_trim_utf8(enc._h, buf.ctypes.data, len(text), idx.ctypes.data, len(idx), N.TRIM_SUFFIX, 2, ids.ctypes.data, 8, C.byref(n), None, None))
    assert ids[:n.value].tolist() == want[0]
    lib.check(lib.L.tkz_encode_trim_utf16(enc._h, uu.ctypes.data, len(uu), idx.ctypes.data, len(idx), N.TRIM_SUFFIX, 2, ids.ctypes.data, 8, C.byref(n), None))
    assert ids[:n.value].tolist() == want[0]
    assert lib.L.tkz_encode_trim_utf8(enc._h, buf.ctypes.data, len(text), idx.ctypes.data, len(idx), N.TRIM_SUFFIX, 2, ids.ctypes.data, 8, None, None, None) == N.E_ARG


# ---- i. agreement with the batch entry ----------------------------------------------------------------------------------------------------------------------------

def check_agreement(lib, O, v, ov, name, pattern, n_docs=12):
    """the new entry and encode_batch_trim on a batch of one: ids, both cuts and what each call adds to special_stats"""
    specials = SC.SPECIAL_SETS[name]
    enc, _ = SC.make_encoders(lib, O, v, ov, pattern, specials)
    rng = random.Random(8100 + pattern)
    for k, doc in enumerate(SC.random_docs(rng, specials, n_docs, 3000)):
        raw = doc.encode("utf-8")
        allowed = rng.choice(SC.allowed_choices(specials))
        index = SC.indices(specials, allowed)
        data, offs = np.frombuffer(raw, np.uint8), np.asarray([0, len(raw)], np.int64)
        for side in SIDES:
            for mx in (0, rng.randrange(1, 40), rng.randrange(40, 900), HUGE):
                s0 = enc.special_stats()
                ids, ooff, cb, cu = enc.encode_batch_trim(data, offs, index, side, mx)
                s1 = enc.special_stats()
                got = enc.encode_trim(raw, index, side, mx)
                s2 = enc.special_stats()
                what = "%s pattern %d document %d side %d max %d allowed %s" % (name, pattern, k, side, mx, allowed)
                assert got == (ids.tolist(), int(cb[0]), int(cu[0])), what
                assert (s2[0] - s1[0], s2[1] - s1[1]) == (s1[0] - s0[0], s1[1] - s0[1]), (what, s0, s1, s2)


# ---- j. threads -------------------------------------------------------------------------------------------------------------------------------------------------

def check_threads(lib, O, v, ov, pattern):
    specials = {SC.EOT: 50256}
    enc, oenc = SC.make_encoders(lib, O, v, ov, pattern, specials)
    exp = TC.Expect(O, ov, pattern, specials)
    docs = SC.side_by_side_inputs()[0]
    trims = [(d, SIDES[k % 2], 5 + 3 * k) for k, d in enumerate(docs)]
    expect_trim = [tuple(exp.trim(d, [SC.EOT], side, mx)) for d, side, mx in trims]
    expect_plain = [oenc.encode(d, []) for d in docs]
    errors = []

    def work(trim):
        try:
            for r in range(SC.ROUNDS):
                for k, d in enumerate(docs):
                    if trim:
                        ok = enc.encode_trim(d.encode(), [0], trims[k][1], trims[k][2]) == expect_trim[k]
                    else:
                        ok = enc.encode_utf8(d.encode()) == expect_plain[k]
                    if not ok:
                        errors.append("%s call, text %d, round %d: not the oracle's result" % ("trim" if trim else "plain", k, r))
        except Exception as ex:          # (a thread's exception would otherwise be lost)
            errors.append(repr(ex))
    c0 = enc.small_path_calls()
    threads = [threading.Thread(target=work, args=(s,)) for s in (True, False)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]
    assert moved(c0, enc.small_path_calls()) == (2 * SC.ROUNDS * len(docs), 0)
    assert enc.special_stats() == (SC.ROUNDS * len(docs), SC.ROUNDS * len(docs))


# ---- k. the Python mirror -----------------------------------------------------------------------------------------------------------------------------------------

def check_python_mirror(lib, O, raw):
    from tokenizer_amd.tokenizer import TikTokenizer, REGEX_CL100K
    specials = SC.SPECIAL_SETS["synth100k"]
    tok = TikTokenizer(raw, specials, REGEX_CL100K, lib=lib)
    ov = O.Vocab(raw)
    oracle = O.TrimOracle(ov, 2, specials)
    names = list(specials)
    text = "Hello <|endoftext|> World 😀😀 done<|fim_prefix|> and a tail of it"
    for mx in (0, 1, 3, 5, 8, 100):
        for allowed in (names, names[:1]):
            c0 = tok._encoder.small_path_calls()
            assert tok.EncodeTrimSuffix(text, allowed, mx) == tuple(oracle.encode_trim_suffix(text, allowed, mx)), (mx, allowed)
            assert tok.EncodeTrimPrefix(text, allowed, mx) == tuple(oracle.encode_trim_prefix(text, allowed, mx)), (mx, allowed)
            assert moved(c0, tok._encoder.small_path_calls()) == (2, 0)              # ONE launch each
        c0 = tok._encoder.small_path_calls()
        assert tok.EncodeTrimSuffix(text, mx) == tuple(oracle.encode_trim_suffix(text, names, mx))          # (text, maxTokenCount, applySpecialTokens = true)
        assert tok.EncodeTrimPrefix(text, mx, False) == tuple(oracle.encode_trim_prefix(text, None, mx))
        assert moved(c0, tok._encoder.small_path_calls()) == (2, 0)
    # a set beyond the device path: the host walk, same result
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TikTokenizer(raw, many, REGEX_CL100K, lib=lib)
    o2 = O.TrimOracle(ov, 2, many)
    t = "a<|s7|>b <|s299|><|s30| and more of it"
    assert tok2.EncodeTrimSuffix(t, 4) == tuple(o2.encode_trim_suffix(t, list(many), 4)) and tok2._special_on_host
    assert tok2.EncodeTrimPrefix(t, 4) == tuple(o2.encode_trim_prefix(t, list(many), 4)) and tok2._encoder.special_stats() == (0, 0)
    # a lone surrogate while a literal holds U+FFFD: the host walk
    fffd = {"<�>": 300001}
    tok3 = TikTokenizer(raw, fffd, REGEX_CL100K, lib=lib)
    o3 = O.TrimOracle(ov, 2, fffd)
    c0 = tok3._encoder.small_path_calls()
    lone = "a<\ud800>b c d"
    assert tok3.EncodeTrimSuffix(lone, 3) == tuple(o3.encode_trim_suffix(lone, list(fffd), 3))
    assert tok3.EncodeTrimPrefix(lone, 3) == tuple(o3.encode_trim_prefix(lone, list(fffd), 3))
    assert tok3._encoder.special_stats()[0] == 0
    assert tok3.EncodeTrimSuffix("a<�>b c d", 2) == tuple(o3.encode_trim_suffix("a<�>b c d", list(fffd), 2)) and tok3._encoder.special_stats()[0] == 1
    # a negative maximum: the reference's quirk, kept on the host (suffix keeps nothing, prefix returns the whole text)
    c0 = tok._encoder.small_path_calls()
    assert tok.EncodeTrimSuffix(text, -1) == tuple(oracle.encode_trim_suffix(text, names, -1))
    assert tok.EncodeTrimPrefix(text, -1) == tuple(oracle.encode_trim_prefix(text, names, -1))
    assert moved(c0, tok._encoder.small_path_calls()) == (0, 0)
