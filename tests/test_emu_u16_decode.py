"""`not gpu`: the UTF-16 transcoder (k_u16_len / k_u16_write / k_u16_docoffs behind tkz_encode_batch_utf16) and the batch decoder (k_dec_len / k_dec_write /
k_dec_docoffs behind tkz_decode_batch) at their tile, lane-group and bitmap-word edges -- the real kernel sources on the CPU emulator (tests/hostemu/), exact
against the plain reference of tests/u16_cases.py.  CL100K in full; tests/test_gpu_u16_decode.py runs the same cases under both patterns of the C# entry."""
import os
import re
import subprocess
import sys

import pytest

import emu
import u16_cases as U
from conftest import ROOT
from tokenizer_amd import _native as N

PATTERN, VOCAB = N.CL100K, "synth100k"


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def u16(lib, vocab_bytes, oracle_mod):
    raw = vocab_bytes(VOCAB)
    return N.Encoder(N.Vocab(raw, lib), PATTERN), oracle_mod.Encoder(oracle_mod.Vocab(raw), PATTERN)


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


# ---- the reference and the constants ----------------------------------------------------------------------------------------------------------------------

def test_reference_agrees_with_pythons_codec():
    n = 0
    for cases in U.utf16_case_groups().values():
        for case in cases:
            for units, ref in zip(case.docs, case.ref):
                assert ref == U.python_codec(units), case
                n += 1
    docs, ref, _ = U.chunk_cut_case(6000, 3, block_len=41)
    for units, b in zip(docs, ref):
        assert b == U.python_codec(units)
    assert n > 1500
    # by hand: 1, 2 and 3 bytes, a pair, each lone half, a reversed pair, a high half at the very end
    assert U.get_bytes([0x41, 0xE9, 0x4E2D, 0xD83D, 0xDE00, 0xDE00, 0xD83D, 0x42, 0xDE00, 0xD83D, 0xD83D]) == \
        b"A\xC3\xA9\xE4\xB8\xAD\xF0\x9F\x98\x80" + b"\xEF\xBF\xBD" * 2 + b"B" + b"\xEF\xBF\xBD" * 3


def test_decode_reference_by_hand():
    key_of = {0: b"a", 1: b"bc", 5: b"\xE4\xB8"}
    specials = {"<|s|>": 9, "shadow": 1}
    assert U.decode_ids([0, 9, 7, -3, 1, 2**31 - 1, 5, 5], key_of, specials) == b"a<|s|>bc\xE4\xB8\xE4\xB8"
    assert U.decode_ids([], key_of, specials) == b"" and U.decode_ids([7, 8], key_of, specials) == b""


def test_constants_are_the_kernels():
    src = os.path.join(ROOT, "tokenizer_amd", "csrc")
    hip = open(os.path.join(src, "tkz_kernels.hip")).read()
    hdr = open(os.path.join(src, "tkz_kernels.h")).read()

    def const(text, name):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        assert m, name
        return int(m.group(1))
    assert const(hip, "kU16Tile") == const(hip, "kDecTile") == U.TILE
    assert const(hip, "kU16Lane") == const(hip, "kDecLane") == U.GROUP
    assert const(hip, "kDecStage") == U.DEC_STAGE
    assert const(hdr, "kThreads") // 64 == U.WG_TILES and const(hdr, "kScanBlock") == U.SCAN_BLOCK
    assert "p0 >> 6" in hip and "p0 & 63" in hip and "sh == 48" in hip and U.WORD == 64
    # both families scan their tile sums with launch_scan, which never takes the one-kernel form (u16_cases' docstring)
    api = open(os.path.join(src, "tkz_api.cpp")).read()
    assert re.search(r"launch_scan\(L, U\.tsum", api) and re.search(r"launch_scan\(L, ws->d_tsum", api)
    body = hip[hip.index("void launch_scan(const Launch& L, const int32_t* tile_count"):]
    assert "k_scan_small" not in body[:body.index("\n}\n")]


# ---- UTF-16 --------------------------------------------------------------------------------------------------------------------------------------------------

def run_cases(u16, cases):
    enc, oenc = u16
    assert cases
    for case in cases:
        U.check_utf16_case(enc, oenc, case)


@pytest.mark.parametrize("kind", U.PAIR_KINDS)
def test_utf16_pair_across_every_group_edge(u16, kind):
    """(the emulator runs the sweep on the multiples of 64 -- the bitmap-word edges, every fourth group edge -- and the tile edges; the GPU module on every
    multiple of 16)"""
    cases = [U.pair_case(e, kind) for e in U.pair_positions(U.WORD)]
    assert len(cases) == 66
    run_cases(u16, cases)


@pytest.mark.parametrize("kind", U.PAIR_KINDS)
def test_utf16_pair_across_group_edges_inside_a_word(u16, kind):
    """the group edges that are no word edges (bits 16, 32 and 48 of a word), in the first and the last word of a tile and of a workgroup"""
    edges = [w + g for w in (0, U.TILE - U.WORD, U.TILE, U.WG_UNITS - U.WORD, U.WG_UNITS) for g in (16, 32, 48)]
    run_cases(u16, [U.pair_case(e, kind) for e in edges])


def test_utf16_document_start_in_the_carried_bitmap_bit(u16):
    run_cases(u16, U.utf16_case_groups()["bitmap_carry"])


def test_utf16_ragged_tail(u16):
    run_cases(u16, U.utf16_case_groups()["ragged_tail"])


def test_utf16_document_starts_mid_group(u16):
    run_cases(u16, U.utf16_case_groups()["mid_group_starts"])


def test_utf16_surrogate_soup_at_group_edges(u16):
    run_cases(u16, U.utf16_case_groups()["soup_at_edges"])


def test_utf16_capacity_one_id_short(u16):
    U.check_utf16_capacity(*u16)


def test_utf16_chunk_cut_between_facing_halves(vocab_bytes, oracle_mod):
    """the chunk size is read once per process: a child interpreter with 4 KiB chunks cuts 6,000 units into three, each cut between a high and a low half"""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gzip, emu, u16_cases as U\n"
            "from tokenizer_amd import _native as N\n"
            "from oracle import oracle as O\n"
            "raw = gzip.decompress(open(%r, 'rb').read())\n"
            "lib = emu.library()\n"
            "enc = N.Encoder(N.Vocab(raw, lib), N.CL100K)\n"
            "n_docs, cuts = U.check_chunk_cut(enc, O, O.Vocab(raw), N.CL100K, 6000, 3, block_len=41)\n"
            "assert cuts == [2007, 4014], cuts\n"
            "print('CHUNK_CUT_OK', n_docs)\n") % (ROOT, tests, os.path.join(tests, "golden", "gpt2.tiktoken.gz"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TKZ_HOST_CHUNK_BYTES="4096"), capture_output=True, text=True, timeout=600)
    assert "CHUNK_CUT_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- decode --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["dense", "sparse"])
def test_decode_document_start_behind_an_unknown_id(dec, table):
    enc, S = dec(table)
    for case in U.residue_cases(S):
        U.check_decode_case(enc, S, case)


def test_decode_tile_either_side_of_the_stage_limit(dec):
    enc, S = dec("dense")
    for case in U.stage_limit_cases(S):
        U.check_decode_case(enc, S, case)


@pytest.mark.parametrize("table", ["dense", "sparse"])
def test_decode_tile_counts_with_a_partly_empty_workgroup(dec, table):
    enc, S = dec(table)
    for case in U.tile_count_cases(S):
        U.check_decode_case(enc, S, case)


def test_decode_second_scan_workgroup(dec):
    enc, S = dec("dense")
    for case in U.scan_edge_cases(S):
        U.check_decode_case(enc, S, case)


@pytest.mark.parametrize("table", ["dense", "sparse"])
def test_decode_capacity_one_byte_short(dec, table):
    enc, S = dec(table)
    U.check_decode_capacity(enc, S, U.residue_cases(S)[0])
    if table == "dense":
        for case in U.stage_limit_cases(S):                      # (the direct store path refuses as the staged one does)
            U.check_decode_capacity(enc, S, case)


@pytest.mark.parametrize("table", ["dense", "sparse"])
def test_decode_only_unknown_ids_and_an_empty_last_document(dec, table):
    enc, S = dec(table)
    unknown, one_in_last = U.odd_shape_cases(S)
    assert U.check_decode_case(enc, S, unknown) == 0
    out, offs = enc.decode_batch(unknown.ids, unknown.offs)
    assert len(out) == 0 and offs.tolist() == [0] * len(unknown.offs)
    assert U.check_decode_case(enc, S, one_in_last) > 2 * U.TILE
