"""`-m gpu`: the UTF-16 transcoder and the batch decoder through libtkz.so at their tile, lane-group and bitmap-word edges -- tkz_encode_batch_utf16 under the two
patterns the C# entry uses, tkz_decode_batch and tkz_decode_batch_device (on a side stream) -- exact against the plain reference of tests/u16_cases.py.  The
cases are those of tests/test_emu_u16_decode.py, the pair sweep on every multiple of 16; one case the emulator cannot reach in-process is added: a batch large
enough for the host to cut it into two chunks, the cut between two facing surrogate halves."""
import os

import numpy as np
import pytest

import u16_cases as U
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu

VOCAB_OF = {N.CL100K: "synth100k", N.O200K_DOTNET: "synth200k"}
PATTERNS = (N.CL100K, N.O200K_DOTNET)


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def u16(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(pattern):
        if pattern not in cache:
            raw = vocab_bytes(VOCAB_OF[pattern])
            ov = oracle_mod.Vocab(raw)
            cache[pattern] = (N.Encoder(N.Vocab(raw, lib), pattern), oracle_mod.Encoder(ov, pattern), ov)
        return cache[pattern]
    return get


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


def device_decode(enc):
    """tkz_decode_batch_device on torch buffers and a side stream, as a u16_cases.check_decode_case() call.  The bytes behind the result must be left alone."""
    import torch

    def call(ids, offs, cap):
        n = len(offs) - 1
        d_ids = torch.zeros(max(1, len(ids)), dtype=torch.int32, device="cuda")
        if len(ids):
            d_ids[:len(ids)] = torch.from_numpy(np.array(ids, dtype=np.int32)).cuda()
        d_offs = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
        out = torch.full((cap + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        ooff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        nb = enc.decode_batch_device(d_ids.data_ptr(), d_offs.data_ptr(), n, len(ids), out.data_ptr(), cap, ooff.data_ptr(), stream=stream.cuda_stream)
        assert nb <= cap and bool((out[nb:] == 0xAA).all()), "bytes behind the result were written"
        return out[:nb].cpu().numpy(), ooff.cpu().numpy()
    return call


# ---- UTF-16 --------------------------------------------------------------------------------------------------------------------------------------------------

def run_cases(u16, pattern, cases):
    enc, oenc, _ = u16(pattern)
    assert cases
    for case in cases:
        U.check_utf16_case(enc, oenc, case)


@pytest.mark.parametrize("kind", U.PAIR_KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_utf16_pair_across_every_group_edge(u16, pattern, kind):
    cases = [c for c in U.utf16_case_groups()["pair_sweep"] if c.name.endswith("_" + kind)]
    assert len(cases) == (U.WG_UNITS + U.WORD) // U.GROUP + 1              # (every multiple of 16 up to 4096 + 64, and 5120)
    run_cases(u16, pattern, cases)


@pytest.mark.parametrize("group", ["bitmap_carry", "ragged_tail", "mid_group_starts", "soup_at_edges"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_utf16_positioned_cases(u16, pattern, group):
    run_cases(u16, pattern, U.utf16_case_groups()[group])


@pytest.mark.parametrize("pattern", PATTERNS)
def test_utf16_capacity_one_id_short(u16, pattern):
    enc, oenc, _ = u16(pattern)
    U.check_utf16_capacity(enc, oenc)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_utf16_chunk_cut_between_facing_halves(u16, oracle_mod, pattern):
    """6.5 M code units (13 MB) are cut into two chunks; the cut falls between a document ending in a high half and one starting with a low half, 3,250,007 units
    into the batch -- no multiple of 16."""
    enc, _, ov = u16(pattern)
    n_docs, cuts = U.check_chunk_cut(enc, oracle_mod, ov, pattern, 6_500_000, 2, threads=min(16, os.cpu_count() or 1))
    assert cuts == [3_250_007] and n_docs > 300


# ---- decode --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["dense", "sparse"])
def test_decode_document_start_behind_an_unknown_id(dec, table):
    enc, S = dec(table)
    for case in U.residue_cases(S):
        U.check_decode_case(enc, S, case, device=device_decode(enc))


def test_decode_tile_either_side_of_the_stage_limit(dec):
    enc, S = dec("dense")
    for case in U.stage_limit_cases(S):
        U.check_decode_case(enc, S, case, device=device_decode(enc))


@pytest.mark.parametrize("table", ["dense", "sparse"])
def test_decode_tile_counts_with_a_partly_empty_workgroup(dec, table):
    enc, S = dec(table)
    for case in U.tile_count_cases(S):
        U.check_decode_case(enc, S, case, device=device_decode(enc))


def test_decode_second_scan_workgroup(dec):
    enc, S = dec("dense")
    for case in U.scan_edge_cases(S):
        U.check_decode_case(enc, S, case, device=device_decode(enc))


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
    assert U.check_decode_case(enc, S, unknown, device=device_decode(enc)) == 0
    out, offs = enc.decode_batch(unknown.ids, unknown.offs)
    assert len(out) == 0 and offs.tolist() == [0] * len(unknown.offs)
    assert U.check_decode_case(enc, S, one_in_last, device=device_decode(enc)) > 2 * U.TILE
