"""`not gpu`: Decode to UTF-16 (tkz_decode_batch_utf16: the k_dec_* family, then k_u8_len / k_u8_write / k_u8_docoffs) at the tile, lane-group and bitmap-word
edges of the decoded bytes -- the real kernel sources on the CPU emulator (tests/hostemu/), exact against the plain reference of tests/u8_decode_cases.py.
tests/test_gpu_u8_decode.py runs the same cases through libtkz.so, the sweep on every multiple of 16."""
import os
import random
import re

import numpy as np
import pytest

import emu
import u16_cases as U
import u8_decode_cases as D
from conftest import ROOT
from tokenizer_amd import _native as N

TABLES = ["dense", "sparse"]


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def dec(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(table):
        if table not in cache:
            raw = vocab_bytes("gpt2") if table == "dense" else U.sparse_vocab_bytes()
            S = U.DecodeSetup(oracle_mod.Vocab(raw).entries())
            enc = N.Encoder(N.Vocab(raw, lib), N.CL100K)
            enc.set_special_tokens(S.specials)
            cache[table] = (enc, S)
        return cache[table]
    return get


def run_cases(dec, table, cases):
    enc, S = dec(table)
    assert cases
    for case in cases:
        D.check_case(enc, S, case)


# ---- the reference and the constants ----------------------------------------------------------------------------------------------------------------------

def test_reference_by_hand():
    for hexes, units in D.HAND:
        data = bytes.fromhex(hexes)
        assert D.get_string(data) == units, hexes
        assert D.python_codec(data) == units, hexes


def test_reference_agrees_with_pythons_codec_on_a_boundary_soup():
    rng = random.Random(20250117)
    seen = set()
    for _ in range(120_000):
        data = bytes(rng.choice(D.BOUNDARY) for _ in range(rng.randint(0, 9)))
        assert D.get_string(data) == D.python_codec(data), data.hex()
        seen.add(len(data))
    assert seen == set(range(10))


def test_reference_agrees_with_pythons_codec_on_every_case(dec):
    enc, S = dec("dense")
    cases = [c for kind in D.KINDS for c in D.sweep_cases(S, kind, D.WORD)] + D.split_char_cases(S) + D.ragged_tail_cases(S) + D.unit_extreme_cases(S) + \
        D.odd_shape_cases(S) + D.soup_cases(S) + [D.scan_edge_case(S)]
    n = 0
    for case in cases:
        for data in D.documents(S, case):
            assert D.get_string(data) == D.python_codec(data), case
            n += 1
    assert n > 5000


def test_constants_are_the_kernels():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    hip = open(os.path.join(src, "tkz_kernels.hip")).read()

    def const(name):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, hip)
        assert m, name
        return int(m.group(1))
    assert const("kU8Tile") == D.TILE and const("kU8Lane") == D.GROUP
    # one classification, shared by the three kernels (k_u8_len and k_u8_write through tkz_u8_lane, k_u8_docoffs through tkz_u8_units_at)
    assert hip.count("int tkz_u8_item(") == 1 and hip.count("tkz_u8_item(") == 4
    for kernel in ("k_u8_len", "k_u8_write", "k_u8_docoffs"):
        assert re.search(r"TKZ_KERNEL\(256\) void %s\(" % kernel, hip), kernel
    # the scan of the tile sums is launch_scan, as for the families it mirrors
    api = open(os.path.join(src, "tkz_api.cpp")).read()
    assert re.search(r"launch_scan\(L, ws->d8_tsum", api)


def test_the_tables_hold_every_single_byte_key(dec):
    for table in TABLES:
        _, S = dec(table)
        assert len(D.byte_ids(S)) == 256
    assert sorted(D.split_keys(dec("dense")[1])) == [3, 4]            # (gpt2 holds proper prefixes of 3- and of 4-byte chars as keys)


def test_filler_and_edges():
    assert len(D.FILLER) % 2 == 1
    edges = D.sweep_edges(D.WORD)
    assert set(range(64, 4096 + 64 + 1, 64)) <= set(edges) and {16, 32, 48, 976, 1008, 1040, 1072, 4048, 4080, 4112, 4144} <= set(edges)
    assert D.sweep_edges(D.GROUP) == list(range(16, 4096 + 16 + 1, 16))
    assert len(D.PROBES) == 12 and D.BACKS == (1, 2, 3)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("table", TABLES)
def test_probe_at_every_edge(dec, table, kind):
    """(the emulator runs the sweep on the multiples of 64 and the group edges inside the first and last word of a tile and of a workgroup; the GPU module on
    every multiple of 16)"""
    cases = D.sweep_cases(dec(table)[1], kind, D.WORD)
    assert len(cases) == 36
    run_cases(dec, table, cases)


def test_char_split_across_two_keys(dec):
    cases = D.split_char_cases(dec("dense")[1])
    assert len(cases) == 20
    run_cases(dec, "dense", cases)


@pytest.mark.parametrize("table", TABLES)
def test_ragged_tail_in_a_truncated_char(dec, table):
    run_cases(dec, table, D.ragged_tail_cases(dec(table)[1]))


@pytest.mark.parametrize("table", TABLES)
def test_boundary_soup(dec, table):
    run_cases(dec, table, D.soup_cases(dec(table)[1]))


@pytest.mark.parametrize("table", TABLES)
def test_fewest_and_most_units_of_a_tile(dec, table):
    enc, S = dec(table)
    a, b, c = D.unit_extreme_cases(S)
    want, _ = D.expect(S, a)
    assert len(want) == 2 * D.TILE + 6 + D.TILE // 2 + 1              # (the boundary at 1024 + 6 cuts one char into a prefix and two stray bytes: 3 units for 2)
    assert D.expect(S, b)[0][:D.TILE + 1].tolist() == [ord("x")] * (D.TILE - 1) + [0xD83D, 0xDE00]
    run_cases(dec, table, [a, b, c])


@pytest.mark.parametrize("table", TABLES)
def test_unknown_ids_and_empty_documents(dec, table):
    enc, S = dec(table)
    unknown, one_in_last, all_empty, one_empty = D.odd_shape_cases(S)
    for case in (unknown, all_empty, one_empty):
        assert D.check_case(enc, S, case) == 0
        out, offs = enc.decode_batch_utf16(case.ids, case.offs)
        assert len(out) == 0 and offs.tolist() == [0] * len(case.offs)
    assert D.check_case(enc, S, one_in_last) > D.TILE


def test_second_scan_workgroup(dec):
    enc, S = dec("dense")
    case = D.scan_edge_case(S)
    assert len(case.ids) > D.SCAN_BLOCK * D.TILE
    assert D.check_case(enc, S, case) > 0


@pytest.mark.parametrize("table", TABLES)
def test_capacity_one_unit_short(dec, table):
    enc, S = dec(table)
    D.check_capacity(enc, S, D.soup_cases(S)[1])
    D.check_capacity(enc, S, D.unit_extreme_cases(S)[1])


@pytest.mark.parametrize("table", TABLES)
def test_bad_id_offsets(dec, table):
    D.check_bad_offsets(*dec(table))


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------------------------

def test_python_mirror_gives_the_strings_of_decode_batch(lib, vocab_bytes, dec):
    from tokenizer_amd.tokenizer import REGEX_CL100K, TikTokenizer
    _, S = dec("dense")
    tok = TikTokenizer(vocab_bytes("gpt2"), dict(S.specials), REGEX_CL100K, lib=lib)
    for case in D.quick_cases(S) + D.split_char_cases(S)[:6] + D.odd_shape_cases(S):
        batches = [case.ids[int(a):int(b)].tolist() for a, b in zip(case.offs, case.offs[1:])]
        got = tok.DecodeBatchUtf16(batches)
        assert got == tok.DecodeBatch(batches), case
        assert got == [bytes(d).decode("utf-8", "replace") for d in D.documents(S, case)], case
        assert tok.DecodeUtf16(batches[0]) == tok.Decode(batches[0]) == got[0]
    assert tok.DecodeUtf16([2**40, -2**40]) == "" and tok.DecodeBatchUtf16([]) == []


def test_special_literals_beyond_the_bmp_come_out_as_pairs(lib, vocab_bytes, dec):
    _, S = dec("dense")
    specials = {"<|\U0001F600|>": S.max_id + 1, "\U00010000\U0010FFFF": S.max_id + 2, "<|é中|>": S.max_id + 3}
    enc = N.Encoder(N.Vocab(vocab_bytes("gpt2"), lib), N.CL100K)
    enc.set_special_tokens(specials)
    lut = D.byte_ids(S)
    ids = [int(lut[ord("a")]), S.max_id + 1, S.max_id + 2, int(lut[0xF0]), S.max_id + 3, S.max_id + 9, S.max_id + 2]
    units, offs = enc.decode_batch_utf16(np.asarray(ids, np.int32), np.asarray([0, 2, 2, 6, 7], np.int64))
    docs = ["a<|\U0001F600|>", "", "\U00010000\U0010FFFF\uFFFD<|é中|>", "\U00010000\U0010FFFF"]
    assert offs.tolist() == np.cumsum([0] + [len(d.encode("utf-16-le")) // 2 for d in docs]).tolist()
    assert units.tobytes() == "".join(docs).encode("utf-16-le")
    assert units.tolist()[3:5] == [0xD83D, 0xDE00] and units.tolist()[7:11] == [0xD800, 0xDC00, 0xDBFF, 0xDFFF]
