"""Decode(int[]) for ONE id list in a single launch (tkz_decode_utf8 / tkz_decode_utf16: k_dec_small): the cases and comparisons the emulated (CPU) and the GPU
test modules share.  Every comparison is exact equality of bytes / code units.

Expected values come from what is independent of the new kernel: the vocabulary's keys and the registered literals (u16_cases.decode_ids) for the bytes,
u8_decode_cases.get_string (short results) / python_codec for the units, and the batch entries (tkz_decode_batch / _utf16 with one document) for agreement.

The route of a call is read from tkz_encoder_small_decode_calls: LAUNCH (the kernel ran and answered), HANDED (it ran and handed the list back: more than
MAX_BYTES decoded bytes; the batch path answered), BATCH (more than MAX_IDS ids: no launch).  The constants are the kernels' (test_constants_are_the_kernels
reads them out of the sources):
  MAX_IDS 32768, MAX_BYTES 131072   tkz_kernels.h: kDecSmallMaxIds, kDecSmallMaxBytes -- what the page-locked block holds
  STAGE 5120                        tkz_kernels.hip: kDecSmallStage -- bytes of LDS stage per wavefront; a tile of more bytes is copied directly
  WAVES_SMALL 4, WAVES 16           the workgroup is 256 threads for up to 4 id tiles and 1024 beyond
The tables are gpt2 with the specials of u16_cases.DecodeSetup ("dense") and gpt2 with a special id far above the vocabulary, whose literal holds a 4-byte char
("sparse": the decode table's sorted, binary-searched form).  Both hold all 256 single-byte keys, so a list of single-byte ids puts byte q at id q.
"""
import ctypes as C
import random
import threading

import numpy as np

import u16_cases as U
import u8_decode_cases as D
from tokenizer_amd import _native as N

MAX_IDS, MAX_BYTES, STAGE, TILE = 32768, 131072, 5120, 1024
WAVES_SMALL, WAVES = 4, 16
LAUNCH, HANDED, BATCH = (1, 0), (1, 1), (0, 0)
TABLES = ["dense", "sparse"]
FAR_ID = 5_000_000                    # beyond 2^22: the decode table takes its sparse form
FAR_LITERAL = "<|\U0001F600 far|>"
# 0, the lane and tile edges, the last id of the 256-thread form and the first of the 1024-thread one (a fifth tile), a wavefront's second tile, the capacity
ID_TOTALS = (0, 1, 15, 16, 17, 1023, 1024, 1025, WAVES_SMALL * TILE - 1, WAVES_SMALL * TILE, WAVES_SMALL * TILE + 1, WAVES * TILE - 1, WAVES * TILE,
             WAVES * TILE + 1, MAX_IDS, MAX_IDS + 1)
# F0 9F 98 41, ED A0 80, F4 90 80 80, stray 80s: u8_decode_cases.PROBES
EDGE_PROBES = [D.PROBES[i] for i in (4, 6, 8, 11)]
# a 16-byte lane group edge, a 64-byte edge, the last group edge of a tile, the tile edge, inside later tiles (256-thread form: fewer than 4 * 1024 ids) ...
EDGES_AT = [16, 64, 1008, 1024, 2064, 3072]
# ... and one byte on (the sequence straddles 1024 / 1025), up to a sixth tile (1024-thread form)
EDGES_BEHIND = [e + 1 for e in EDGES_AT] + [4112, 5121]


def setup(lib, raw, O, table):
    """(encoder, DecodeSetup) of a table"""
    S = U.DecodeSetup(O.Vocab(raw).entries())
    if table == "sparse":
        S.specials = {"<|endoftext|>": S.max_id + 1, FAR_LITERAL: FAR_ID, "shadow": S.known[5]}
        S.strays = [S.strays[0], S.max_id + 1000, -3, 2**31 - 1, FAR_ID + 1]
    enc = N.Encoder(N.Vocab(raw, lib), N.CL100K)
    enc.set_special_tokens(S.specials)
    S.lut = D.byte_ids(S)
    S.longest = max(S.known, key=lambda i: (len(S.key_of[i]), -i))
    return enc, S


def moved(c0, c1):
    return (c1[0] - c0[0], c1[1] - c0[1])


def ids_of_bytes(S, flat):
    return S.lut[np.frombuffer(bytes(flat), np.uint8)]


def raw_call(enc, utf16, ids, cap, guard=8):
    """tkz_decode_utf8 / _utf16 with room for `cap` items: (status, n_out, the output array with `guard` items behind the capacity)"""
    ids = np.ascontiguousarray(ids, np.int32)
    out = np.full(max(1, cap) + guard, 0xAAAA if utf16 else 0xAA, np.uint16 if utf16 else np.uint8)
    n = C.c_int64(-7)
    fn = enc.lib.L.tkz_decode_utf16 if utf16 else enc.lib.L.tkz_decode_utf8
    st = fn(enc._h, ids.ctypes.data if len(ids) else None, len(ids), out.ctypes.data, cap, C.byref(n))
    return st, n.value, out


def expect(S, ids):
    """(bytes, units uint16) of the reference"""
    data = U.decode_ids(ids, S.key_of, S.specials)
    units = D.get_string(data) if len(data) <= 8192 else D.python_codec(data)
    return data, np.asarray(units, np.uint16)


def route_of(n_ids, n_bytes):
    if n_ids == 0 or n_ids > MAX_IDS: return BATCH
    return LAUNCH if n_bytes <= MAX_BYTES else HANDED


def check_one(enc, S, ids, what, route=None, batch=True):
    """Both forms at a capacity of exactly the reference length: status, total, items, nothing written behind them, the route; the batch entries agree."""
    ids = np.asarray(ids, np.int32)
    data, units = expect(S, ids)
    if route is None: route = route_of(len(ids), len(data))
    for utf16, want in ((False, np.frombuffer(data, np.uint8)), (True, units)):
        c0 = enc.small_decode_calls()
        st, n, out = raw_call(enc, utf16, ids, len(want))
        assert (st, n) == (N.OK, len(want)), (what, utf16, st, n, len(want))
        assert np.array_equal(out[:n], want), "%s utf16=%s: items differ at %d" % (what, utf16, U.first_diff(out[:n].tolist(), want.tolist()))
        assert (out[n:] == (0xAAAA if utf16 else 0xAA)).all(), "%s: items behind the result were written" % what
        assert moved(c0, enc.small_decode_calls()) == route, (what, utf16, moved(c0, enc.small_decode_calls()), route)
    if batch:
        offs = np.asarray([0, len(ids)], np.int64)
        b8, o8 = enc.decode_batch(ids, offs)
        b16, o16 = enc.decode_batch_utf16(ids, offs)
        assert b8.tobytes() == data and o8.tolist() == [0, len(data)] and np.array_equal(b16, units) and o16.tolist() == [0, len(units)], what
    return len(data), len(units)


# ---- a. id totals -------------------------------------------------------------------------------------------------------------------------------------------

def check_id_totals(enc, S, totals=ID_TOTALS):
    """single-byte ids (a byte an id: the filler's 1-, 2- and 3-byte chars, a 4-byte char around every tile edge), every total on its route"""
    for t in totals:
        flat = D.filler(t, phase=t)
        for e in range(TILE, t - 4, TILE):
            flat[e - 2:e + 2] = bytes.fromhex("F0 9F 98 80")
        nb, nu = check_one(enc, S, ids_of_bytes(S, flat), "%d single-byte ids" % t)
        assert nb == t and (t == 0 or 0 < nu <= t)
    # multi-byte keys: lists that decode to more bytes than ids
    for t in (17, 1025, WAVES_SMALL * TILE + 1, WAVES * TILE + 1):
        if t in totals:
            nb, _ = check_one(enc, S, S.ordinary(t, seed=t), "%d ordinary ids" % t)
            assert nb > t


# ---- b. byte tile edges -------------------------------------------------------------------------------------------------------------------------------------

def edge_cases(S):
    out = [D.sweep_case(S, p, back, "inside", edges) for p in EDGE_PROBES for back in D.BACKS for edges in (EDGES_AT, EDGES_BEHIND)]
    assert {len(c.ids) <= WAVES_SMALL * TILE for c in out} == {True, False}          # both workgroup sizes
    return out


def check_byte_edges(enc, S):
    for case in edge_cases(S):
        check_one(enc, S, case.ids, case.name)
    for case in D.ragged_tail_cases(S):                       # a list that ends inside a char, as a trimmed list does
        _, nu = check_one(enc, S, case.ids, case.name)
        assert nu > 0
    for case in D.unit_extreme_cases(S)[:2] + D.split_char_cases(S)[:2]:
        check_one(enc, S, case.ids, case.name)


# ---- c. stage overflow, capacity edges ------------------------------------------------------------------------------------------------------------------------

def exact_capacity_ids(S, extra=0):
    """whole tiles of the longest key, then single-byte ids: MAX_BYTES + extra decoded bytes"""
    L = len(S.key_of[S.longest])
    k = min(MAX_BYTES // L, TILE)
    rest = MAX_BYTES + extra - k * L
    assert 0 <= rest and k + rest <= MAX_IDS
    return [S.longest] * k + ids_of_bytes(S, D.filler(rest, phase=5)).tolist()


def check_stage_and_capacity(enc, S):
    L = len(S.key_of[S.longest])
    assert TILE * L > STAGE
    # a tile of 1024 ids of the longest key: the direct-copy branch -- between two staged tiles, under the byte capacity ...
    mid = [S.longest] * min(TILE, (MAX_BYTES - 4 * TILE) // L)
    mid += ids_of_bytes(S, D.filler(TILE - len(mid), phase=1)).tolist()
    ids = ids_of_bytes(S, D.filler(TILE, phase=2)).tolist() + mid + ids_of_bytes(S, D.filler(TILE + 9, phase=3)).tolist()
    nb, _ = check_one(enc, S, ids, "a tile beyond the stage between two staged tiles", route=LAUNCH)
    assert STAGE < nb - 2 * TILE - 9 <= MAX_BYTES
    # ... and over it: a hand-back, the batch entry's result
    over = [S.longest] * TILE + ids_of_bytes(S, D.filler(TILE + 9, phase=3)).tolist()
    if TILE * L + TILE + 9 > MAX_BYTES:
        check_one(enc, S, over, "a tile beyond the stage, beyond the capacity", route=HANDED)
    # a tile of exactly STAGE bytes and one of a byte more (both branches at their limit)
    for extra in (0, 1):
        k = (STAGE + extra - TILE) // (L - 1)
        tile = [S.longest] * k + ids_of_bytes(S, D.filler(TILE - k, phase=7)).tolist()
        pad = STAGE + extra - (k * L + TILE - k)
        assert len(tile) == TILE and 0 <= pad < L - 1 and pad <= TILE - k
        if pad:                                                # (two-byte keys in the place of single-byte ids: a byte more each)
            tile[-pad:] = [S.by_len[2][0]] * pad
        assert len(U.decode_ids(tile, S.key_of, S.specials)) == STAGE + extra
        check_one(enc, S, S.ordinary(700, 3) + tile, "a tile of %d bytes behind a ragged one" % (STAGE + extra))       # (700 + 1024 ids: the tile in question straddles two id tiles)
        check_one(enc, S, tile + S.ordinary(11, 4), "a first tile of %d bytes" % (STAGE + extra))
    # decoded bytes exactly MAX_BYTES: the launch; one more byte: a hand-back
    nb, nu = check_one(enc, S, exact_capacity_ids(S), "exactly the byte capacity", route=LAUNCH)
    assert nb == MAX_BYTES
    nb, _ = check_one(enc, S, exact_capacity_ids(S, 1), "one byte beyond the byte capacity", route=HANDED)
    assert nb == MAX_BYTES + 1
    # MAX_BYTES single-char units: every byte a unit of its own is the most units the block holds
    ascii_ids = [S.by_len[4][0]] * (MAX_BYTES // 4)
    if all(b < 0x80 for b in S.key_of[S.by_len[4][0]]):
        nb, nu = check_one(enc, S, ascii_ids, "as many units as bytes at the capacity", route=LAUNCH)
        assert nb == nu == MAX_BYTES


# ---- d. ids outside the vocabulary ----------------------------------------------------------------------------------------------------------------------------

def check_outside_ids(enc, S):
    special_ids = sorted(set(S.specials.values()) - set(S.key_of))
    for n in (40, TILE + 50, 3 * TILE + 5):
        ids = S.ordinary(n, seed=n)
        for i in range(0, n, 5):
            ids[i] = (S.strays + special_ids)[(i // 5) % (len(S.strays) + len(special_ids))]
        nb, _ = check_one(enc, S, ids, "strays and specials in %d ids" % n)
        assert nb > 0
    unknown = [S.strays[k % 4] for k in range(TILE + 50)]
    assert check_one(enc, S, unknown, "only unknown ids", route=LAUNCH) == (0, 0)
    assert check_one(enc, S, unknown[:3], "three unknown ids", route=LAUNCH) == (0, 0)
    # every special on its own and side by side: a literal's 4-byte char is a pair
    for sid in special_ids:
        check_one(enc, S, [sid], "special %d alone" % sid)
    check_one(enc, S, special_ids * 700, "specials only, three tiles")


# ---- e. arguments and capacity --------------------------------------------------------------------------------------------------------------------------------

def check_arguments(enc, S):
    L = enc.lib.L
    ids = ids_of_bytes(S, D.filler(40))
    c0 = enc.small_decode_calls()
    for fn, dtype in ((L.tkz_decode_utf8, np.uint8), (L.tkz_decode_utf16, np.uint16)):
        out = np.zeros(64, dtype)
        n = C.c_int64(-7)
        rows = [(None, ids.ctypes.data, 40, out.ctypes.data, 64, C.byref(n)),               # a null encoder
                (enc._h, ids.ctypes.data, 40, out.ctypes.data, 64, None),                    # a null n_out
                (enc._h, ids.ctypes.data, -1, out.ctypes.data, 64, C.byref(n)),              # a negative n_ids
                (enc._h, ids.ctypes.data, 40, out.ctypes.data, -1, C.byref(n)),              # a negative out_cap
                (enc._h, None, 40, out.ctypes.data, 64, C.byref(n)),                         # null ids with n_ids > 0
                (enc._h, ids.ctypes.data, 40, None, 64, C.byref(n))]                         # a null output with out_cap > 0
        for row in rows:
            assert fn(*row) == N.E_ARG, row[1:5]
        # no ids: OK and 0, null arrays or not, nothing launched
        assert fn(enc._h, None, 0, None, 0, C.byref(n)) == N.OK and n.value == 0
        n.value = -7
        assert fn(enc._h, ids.ctypes.data, 0, out.ctypes.data, 64, C.byref(n)) == N.OK and n.value == 0
        # a null output with no capacity asks for the size
        assert fn(enc._h, ids.ctypes.data, 40, None, 0, C.byref(n)) == N.E_CAPACITY and n.value > 0
    assert moved(c0, enc.small_decode_calls()) == (2, 0)          # (the two size queries)
    check_one(enc, S, ids, "after bad arguments")


def check_capacity(enc, S):
    """one item short: E_CAPACITY and the exact total; then exactly that many: OK -- on the launch, on a hand-back and on the batch route"""
    soup = D.soup_cases(S)[0].ids
    lists = [(soup, LAUNCH), (np.asarray(exact_capacity_ids(S, 1), np.int32), HANDED), (ids_of_bytes(S, D.filler(MAX_IDS + 1, phase=4)), BATCH)]
    for ids, route in lists:
        data, units = expect(S, ids)
        assert route_of(len(ids), len(data)) == route
        for utf16, want in ((False, np.frombuffer(data, np.uint8)), (True, units)):
            for cap in (len(want) - 1, len(want) // 2, 0):
                c0 = enc.small_decode_calls()
                st, n, _ = raw_call(enc, utf16, ids, cap)
                assert (st, n) == (N.E_CAPACITY, len(want)), (route, utf16, cap, st, n, len(want))
                assert moved(c0, enc.small_decode_calls()) == route
            st, n, out = raw_call(enc, utf16, ids, n)
            assert (st, n) == (N.OK, len(want)) and np.array_equal(out[:n], want)
    try:
        enc.decode(soup, out_cap=3)
        raise AssertionError("a short capacity did not raise")
    except N.TkzError as ex:
        assert ex.code == N.E_CAPACITY


# ---- f. agreement and re-use ----------------------------------------------------------------------------------------------------------------------------------

def soup_lists(S, seed, n_lists, longest):
    """seeded lists of ids: keys of every length, strays, specials, single bytes of the boundary alphabet"""
    rng = random.Random(seed)
    pool = S.known + S.strays + sorted(S.specials.values()) + [int(S.lut[b]) for b in D.BOUNDARY] * 40
    return [[rng.choice(pool) for _ in range(rng.choice((1, 2, 7, 16, 63, 700, TILE, TILE + 1, longest)))] for _ in range(n_lists)]


def check_agreement(enc, S, n_lists=12, longest=3 * TILE + 17):
    for k, ids in enumerate(soup_lists(S, 20251019, n_lists, longest)):
        ids = np.asarray(ids, np.int32)
        offs = np.asarray([0, len(ids)], np.int64)
        b8, _ = enc.decode_batch(ids, offs)
        b16, _ = enc.decode_batch_utf16(ids, offs)
        c0 = enc.small_decode_calls()
        assert np.array_equal(enc.decode(ids), b8) and np.array_equal(enc.decode_utf16(ids), b16), "list %d of %d ids" % (k, len(ids))
        m = moved(c0, enc.small_decode_calls())          # (a call more where the wrapper's first capacity, 8 items an id, was short)
        assert 2 <= m[0] <= 4 and m[1] == (m[0] if len(b8) > MAX_BYTES else 0), m          # (more bytes than the block holds: every launch hands back)


def check_reuse(enc, S, large=WAVES * TILE + 1):
    """a large call, a small one, a large one again on one encoder; single decode and single encode calls interleaved"""
    big = ids_of_bytes(S, D.filler(large, phase=2))
    small = S.ordinary(9, seed=1)
    for k, ids in enumerate((big, small, big, small, S.ordinary(large // 8, seed=2))):
        check_one(enc, S, ids, "call %d of the re-use sequence" % k, batch=False)
    texts = ["Hello, world", "naïve → 中文 \U0001F600 done", "ab " * 300 + "tail", "x"]
    for r in range(3):
        for t in texts:
            e0, d0 = enc.small_path_calls(), enc.small_decode_calls()
            ids = enc.encode_utf8(t.encode())
            assert enc.decode(np.asarray(ids, np.int32)).tobytes() == t.encode()
            assert enc.decode_utf16(np.asarray(ids, np.int32)).astype("<u2").tobytes() == t.encode("utf-16-le")
            assert moved(e0, enc.small_path_calls()) == (1, 0) and moved(d0, enc.small_decode_calls()) == (2, 0)


def check_threads(enc, S, rounds=6):
    """two host threads share one encoder: one decodes to bytes, the other to units, each on its own leased workspace"""
    lists = [np.asarray(x, np.int32) for x in soup_lists(S, 7, 6, TILE + 300)]
    want = [expect(S, x) for x in lists]
    errors = []

    def work(utf16):
        try:
            for r in range(rounds):
                for k, ids in enumerate(lists):
                    got = enc.decode_utf16(ids) if utf16 else enc.decode(ids)
                    ok = np.array_equal(got, want[k][1]) if utf16 else got.tobytes() == want[k][0]
                    if not ok:
                        errors.append("utf16=%s list %d round %d: not the reference's result" % (utf16, k, r))
        except Exception as ex:          # (a thread's exception would otherwise be lost)
            errors.append(repr(ex))
    c0 = enc.small_decode_calls()
    threads = [threading.Thread(target=work, args=(u,)) for u in (False, True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]
    assert moved(c0, enc.small_decode_calls()) == (2 * rounds * len(lists), 0)


# ---- g. the Python mirror -------------------------------------------------------------------------------------------------------------------------------------

def check_python_mirror(lib, raw, S):
    from tokenizer_amd.tokenizer import REGEX_CL100K, TikTokenizer
    tok = TikTokenizer(raw, dict(S.specials), REGEX_CL100K, lib=lib)
    lists = [c.ids.tolist() for c in D.ragged_tail_cases(S)[:6] + D.soup_cases(S)[:1]] + [S.ordinary(50, 1) + S.strays, [], [2**40, -2**40]]
    for ids in lists:
        c0 = tok._encoder.small_decode_calls()
        a, b = tok.Decode(ids), tok.DecodeUtf16(ids)
        assert moved(c0, tok._encoder.small_decode_calls()) == ((2, 0) if ids else (0, 0))          # ONE launch each; no ids, no launch
        assert a == b == tok.DecodeBatch([ids])[0] == tok.DecodeBatchUtf16([ids])[0], ids[:8]
        assert moved(c0, tok._encoder.small_decode_calls()) == ((2, 0) if ids else (0, 0))          # (the batch methods are the batch entries still)
    text = "Hello <|endoftext|> wörld \U0001F600"
    assert tok.Decode(tok.Encode(text, list(S.specials))) == text
