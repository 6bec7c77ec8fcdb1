"""`-m gpu`: Decode to UTF-16 through libtkz.so -- tkz_decode_batch_utf16 and tkz_decode_batch_utf16_device (torch buffers, a side stream) -- at the tile,
lane-group and bitmap-word edges of the decoded bytes, exact against the plain reference of tests/u8_decode_cases.py.  The cases are those of
tests/test_emu_u8_decode.py, the probe sweep on every multiple of 16; one round trip is added: UTF-16 documents encoded by tkz_encode_batch_utf16 come back
from tkz_decode_batch_utf16 unit for unit."""
import numpy as np
import pytest

import u16_cases as U
import u8_decode_cases as D
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu

TABLES = ["dense", "sparse"]


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


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
    """tkz_decode_batch_utf16_device on torch buffers and a side stream, as a u8_decode_cases.check_case() call.  The units behind the result must be left alone."""
    import torch

    def call(ids, offs, cap):
        n = len(offs) - 1
        d_ids = torch.zeros(max(1, len(ids)), dtype=torch.int32, device="cuda")
        if len(ids):
            d_ids[:len(ids)] = torch.from_numpy(np.array(ids, dtype=np.int32)).cuda()
        d_offs = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
        out = torch.full((cap + 64,), 0x2AAA, dtype=torch.int16, device="cuda")
        ooff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        nu = enc.decode_batch_utf16_device(d_ids.data_ptr(), d_offs.data_ptr(), n, len(ids), out.data_ptr(), cap, ooff.data_ptr(), stream=stream.cuda_stream)
        assert nu <= cap and bool((out[nu:] == 0x2AAA).all()), "units behind the result were written"
        return out[:nu].cpu().numpy().view(np.uint16), ooff.cpu().numpy()
    return call


def run_cases(dec, table, cases, device=True):
    enc, S = dec(table)
    assert cases
    for case in cases:
        D.check_case(enc, S, case, device=device_decode(enc) if device else None)


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("table", TABLES)
def test_probe_at_every_multiple_of_16(dec, table, kind):
    cases = D.sweep_cases(dec(table)[1], kind, D.GROUP)
    assert len(cases) == 36 and len(D.sweep_edges(D.GROUP)) == 257
    run_cases(dec, table, cases)


@pytest.mark.parametrize("kind", D.KINDS)
def test_probe_at_the_edges_of_the_emulated_sweep(dec, kind):
    """(the edges of the `not gpu` module as well: 4160 and the group edges of the word behind a workgroup are beyond 4096 + 16)"""
    run_cases(dec, "dense", D.sweep_cases(dec("dense")[1], kind, D.WORD), device=False)


def test_char_split_across_two_keys(dec):
    run_cases(dec, "dense", D.split_char_cases(dec("dense")[1]))


@pytest.mark.parametrize("table", TABLES)
def test_positioned_cases(dec, table):
    S = dec(table)[1]
    run_cases(dec, table, D.ragged_tail_cases(S) + D.soup_cases(S) + D.unit_extreme_cases(S))


@pytest.mark.parametrize("table", TABLES)
def test_unknown_ids_and_empty_documents(dec, table):
    enc, S = dec(table)
    unknown, one_in_last, all_empty, one_empty = D.odd_shape_cases(S)
    for case in (unknown, all_empty, one_empty):
        assert D.check_case(enc, S, case, device=device_decode(enc)) == 0
        out, offs = enc.decode_batch_utf16(case.ids, case.offs)
        assert len(out) == 0 and offs.tolist() == [0] * len(case.offs)
    assert D.check_case(enc, S, one_in_last, device=device_decode(enc)) > D.TILE


def test_second_scan_workgroup(dec):
    enc, S = dec("dense")
    assert D.check_case(enc, S, D.scan_edge_case(S), device=device_decode(enc)) > 0


@pytest.mark.parametrize("table", TABLES)
def test_capacity_and_bad_id_offsets(dec, table):
    import torch
    enc, S = dec(table)
    case = D.soup_cases(S)[1]
    D.check_capacity(enc, S, case)
    D.check_capacity(enc, S, D.unit_extreme_cases(S)[1])
    D.check_bad_offsets(enc, S)
    # the device entry: one unit short, and offsets that do not end at the id count
    want, _ = D.expect(S, case)
    d_ids = torch.from_numpy(case.ids).cuda()
    ooff = torch.empty(len(case.offs), dtype=torch.int64, device="cuda")
    out = torch.full((len(want) + 8,), 0x2AAA, dtype=torch.int16, device="cuda")
    tot = N.C.c_int64(0)
    for offs, cap, status, total in ((case.offs, len(want) - 1, N.E_CAPACITY, len(want)), (case.offs[:-1], len(want), N.E_ARG, None), (case.offs, len(want), N.OK, len(want))):
        d_offs = torch.from_numpy(np.ascontiguousarray(offs)).cuda()
        st = enc.lib.L.tkz_decode_batch_utf16_device(enc._h, d_ids.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(case.ids), out.data_ptr(), cap, ooff.data_ptr(), None,
                                                     N.C.byref(tot))
        assert st == status and (total is None or tot.value == total), (cap, st, tot.value)
    assert np.array_equal(out[:len(want)].cpu().numpy().view(np.uint16), want)


def test_python_mirror_gives_the_strings_of_decode_batch(lib, vocab_bytes, dec):
    from tokenizer_amd.tokenizer import REGEX_CL100K, TikTokenizer
    _, S = dec("dense")
    tok = TikTokenizer(vocab_bytes("gpt2"), dict(S.specials), REGEX_CL100K, lib=lib)
    for case in D.quick_cases(S) + D.split_char_cases(S)[:6] + D.odd_shape_cases(S):
        batches = [case.ids[int(a):int(b)].tolist() for a, b in zip(case.offs, case.offs[1:])]
        got = tok.DecodeBatchUtf16(batches)
        assert got == tok.DecodeBatch(batches), case
        assert got == [bytes(d).decode("utf-8", "replace") for d in D.documents(S, case)], case


def test_round_trip_of_utf16_documents(lib, vocab_bytes):
    """~1 MB: well-formed UTF-16 documents of u16_cases' filler with pairs -> tkz_encode_batch_utf16 -> tkz_decode_batch_utf16: the same units and offsets"""
    enc = N.Encoder(N.Vocab(vocab_bytes("synth100k"), lib), N.CL100K)
    block = U.filler(4099, phase=5)
    for q in range(10, 4090, 97):
        block[q], block[q + 1] = U.HI, U.LO
    docs, n = [], 0
    while n < 500_000:
        ln = 1 + (len(docs) * 7919) % 9001
        start = (len(docs) * 131) % 1000
        d = (block * 4)[start:start + ln]
        if U.LO == d[0]: d = d[1:]                      # (no document starts or ends inside a pair)
        if d and U.HI == d[-1]: d = d[:-1]
        docs.append(d)
        n += len(d)
    docs[3:3] = [[], []]
    flat, offs = U.pack_units(docs)
    assert 2 * len(flat) > 1_000_000 and flat.tobytes().decode("utf-16-le").encode("utf-16-le") == flat.tobytes()
    ids, ooff = enc.encode_batch_utf16(flat, offs)
    units, uoffs = enc.decode_batch_utf16(ids, ooff)
    assert uoffs.tolist() == offs.tolist()
    assert np.array_equal(units, flat), U.first_diff(units.tolist(), flat.tolist())
