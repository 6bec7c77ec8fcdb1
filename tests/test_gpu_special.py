"""`-m gpu`: special tokens on the device through libtkz.so -- tkz_encode_batch_special_utf8 / _device against the oracle's restatement of
EncodeInternal, bit-exact.  The cases of tests/test_emu_special.py at full size, plus what needs the hardware: batches above 16 MB, the
16 MB chunk cuts of the host entry, page-locked buffers."""
import ctypes as C
import random

import numpy as np
import pytest

import parity
import special_cases as SC
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def vocabs(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            raw = vocab_bytes(name)
            cache[name] = (N.Vocab(raw, lib), oracle_mod.Vocab(raw))
        return cache[name]
    return get


def device_call(enc):
    """the device entry on torch buffers, as a compare() call"""
    import torch

    def call(data, offs, index):
        d = torch.from_numpy(np.array(data, dtype=np.uint8)).cuda() if len(data) else torch.zeros(16, dtype=torch.uint8, device="cuda")
        o = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
        ids = torch.empty(max(1, len(data)), dtype=torch.int32, device="cuda")
        ooff = torch.empty(len(offs), dtype=torch.int64, device="cuda")
        n = enc.encode_batch_special_device(d.data_ptr(), o.data_ptr(), len(offs) - 1, len(data), index, ids.data_ptr(), len(data), ooff.data_ptr())
        torch.cuda.synchronize()
        return ids[:n].cpu().numpy(), ooff.cpu().numpy()
    return call


@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("name", list(SC.SPECIAL_SETS))
def test_edge_cases(lib, vocabs, oracle_mod, name, pattern):
    v, ov = vocabs(name)
    specials = SC.SPECIAL_SETS[name]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
    docs = SC.edge_docs(specials, o200k=pattern in (3, 4))
    for allowed in SC.allowed_choices(specials):
        SC.compare(enc, oenc, specials, allowed, docs, "%s pattern %d allowed %s (host entry)" % (name, pattern, allowed))
        SC.compare(enc, oenc, specials, allowed, docs, "%s pattern %d allowed %s (device entry)" % (name, pattern, allowed), call=device_call(enc))
    data, offs = parity.pack([d.encode("utf-8") for d in ["no literal here", "", "nor < | here |>"]])
    ids0, off0 = enc.encode_batch(data, offs)
    ids1, off1 = enc.encode_batch_special(data, offs, SC.indices(specials, list(specials)))
    assert ids0.tolist() == ids1.tolist() and off0.tolist() == off1.tolist()


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_registration_order_and_overlaps(lib, vocabs, oracle_mod, pattern, sequential):
    v, ov = vocabs("gpt2")
    for specials, allowed_sets, docs in SC.order_cases():
        enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
        enc.set_option(N.OPT_PRETOK_SEQUENTIAL, sequential)
        for allowed in allowed_sets:
            SC.compare(enc, oenc, specials, allowed, docs, "%s allowed %s pattern %d" % (list(specials), allowed, pattern))
            SC.compare(enc, oenc, specials, allowed, ["".join(docs) * 40], "joined, %s allowed %s" % (list(specials), allowed), call=device_call(enc))


def test_literal_bytes_outside_the_vocabulary(lib, oracle_mod):
    import base64
    raw = b"".join(base64.b64encode(k) + b" %d\n" % r for r, k in enumerate([b"a", b"b", b"c", b" ", b"ab", b"bc", b" a", b"abc", b"ca"]))
    v, ov = N.Vocab(raw, lib), oracle_mod.Vocab(raw)
    specials = {"<|z|>": 900, "zz": 901}
    for pattern in SC.PATTERNS:
        enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
        docs = ["abc<|z|>cab", "<|z|>", "zzabzz", "a zz b<|z|>"] * 50
        SC.compare(enc, oenc, specials, list(specials), docs, "pattern %d" % pattern)
        data, offs = parity.pack([d.encode() for d in docs])
        with pytest.raises(N.KeyNotFoundError):
            enc.encode_batch_special(data, offs, [1])


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_literals_across_kernel_boundaries(lib, vocabs, oracle_mod, pattern):
    """64-byte row, 1 KiB sub-tile, 4 KiB block, 16 sub-tile group, 64 sub-tile chunk: the literal at every offset across each."""
    v, ov = vocabs("gpt2")
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
    for doc in SC.boundary_docs(SC.EOT, (64, 1024, 4096, 16384, 65536)):
        SC.compare(enc, oenc, specials, [SC.EOT], [doc], "boundary, %d bytes" % len(doc))
    SC.compare(enc, oenc, specials, [SC.EOT], SC.boundary_docs(SC.EOT, (64, 1024, 4096, 16384, 65536)), "all boundary documents as one batch", call=device_call(enc))


@pytest.mark.parametrize("name,pattern", [("gpt2", 1), ("synth100k", 2), ("synth200k", 3), ("synth200k", 4), ("gpt2", 2), ("synth100k", 1)])
def test_random_batches(lib, vocabs, oracle_mod, name, pattern):
    v, ov = vocabs(name)
    specials = SC.SPECIAL_SETS[name]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
    for seed in range(25):
        rng = random.Random(1000 * pattern + seed)
        docs = SC.random_docs(rng, specials, rng.choice([1, 7, 60]), 40000)
        allowed = rng.choice(SC.allowed_choices(specials))
        SC.compare(enc, oenc, specials, allowed, docs, "%s pattern %d seed %d allowed %s" % (name, pattern, seed, allowed), call=device_call(enc) if seed & 1 else None)


def test_throughput_form_on_small_batches(lib, vocabs, oracle_mod, monkeypatch):
    monkeypatch.setenv("TKZ_LATENCY_BYTES", "0")
    v, ov = vocabs("gpt2")
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 2, specials)
    rng = random.Random(77)
    for seed in range(6):
        SC.compare(enc, oenc, specials, [SC.EOT], SC.random_docs(rng, specials, 40, 40000), "throughput form, round %d" % seed, call=device_call(enc) if seed & 1 else None)


def big_docs(rng, specials, total):
    docs, n = [], 0
    base = SC.random_docs(rng, specials, 200, 40000)
    while n < total:
        d = rng.choice(base)
        docs.append(d)
        n += len(d.encode("utf-8"))
    return docs


def test_large_batch_device_entry(lib, vocabs, oracle_mod):
    """One batch above 16 MB (the large batches' launch sequence) through the device entry; the oracle on every document."""
    v, ov = vocabs("synth100k")
    specials = SC.SPECIAL_SETS["synth100k"]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 2, specials)
    docs = big_docs(random.Random(3), specials, 20 << 20)
    SC.compare(enc, oenc, specials, list(specials), docs, "20 MB, device entry", call=device_call(enc))


def test_large_batch_host_entry_chunks(lib, vocabs, oracle_mod):
    """At least 32 MB through the host entry on page-locked buffers: 16 MB chunks, with a chunk cut falling right before and right after a literal."""
    v, ov = vocabs("gpt2")
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 1, specials)
    rng = random.Random(9)
    docs = big_docs(rng, specials, 34 << 20)
    # documents that are a literal alone / begin / end with one, where the cuts fall (the planner cuts at the document that reaches total / nchunks * k)
    enc_docs = [d.encode("utf-8") for d in docs]
    total = sum(map(len, enc_docs))
    nch = max(2, (total + (8 << 20)) // (16 << 20))
    pos, k = 0, 1
    out = []
    for d in docs:
        if k < nch and pos + len(d.encode("utf-8")) >= total // nch * k:
            out += [d + SC.EOT, SC.EOT, SC.EOT + d]
            k += 1
        else:
            out.append(d)
        pos += len(d.encode("utf-8"))
    docs = out
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    bufs = []

    def pinned(n, dt):
        p = C.c_void_p()
        lib.check(lib.L.tkz_host_alloc(max(64, n * np.dtype(dt).itemsize), C.byref(p)))
        bufs.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(max(1, n),))
    try:
        pd = pinned(len(data), np.uint8); pd[:len(data)] = data
        po = pinned(len(offs), np.int64); po[:] = offs
        pi = pinned(len(data), np.int32)
        poo = pinned(len(offs), np.int64)
        dl0 = enc.engine_downloads

        def call(_d, _o, index):
            return enc.encode_batch_special(pd[:len(data)], po, index, out=(pi, poo))
        SC.compare(enc, oenc, specials, [SC.EOT], docs, "34 MB, host entry, page-locked", call=call)
        print("copy-engine downloads:", enc.engine_downloads - dl0)
    finally:
        for p in bufs:
            lib.L.tkz_host_free(p)


def test_memo_and_promotions_never_hold_a_literal(lib, vocabs, oracle_mod):
    v, ov = vocabs("gpt2")
    specials = {"<|q|>": 60001, "zqzq": 60002}
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 2, specials)
    enc.set_option(N.OPT_PIECE_STATS, 1)
    rng = random.Random(5)
    docs = ["".join(rng.choice(["<|q|>", "zqzq", " word", " zqz", "qzq "]) for _ in range(3000)) for _ in range(700)]      # a learning window's worth (8 MB)
    for _ in range(2):
        SC.compare(enc, oenc, specials, list(specials), docs, "dense in literals")
    enc.set_option(N.OPT_PROMOTE, 2)
    SC.compare(enc, oenc, specials, list(specials), docs, "after a promotion")
    enc2, _ = SC.make_encoders(lib, oracle_mod, v, ov, 2, specials)
    enc2.set_option(N.OPT_PIECE_STATS, 1)
    enc2.set_option(N.OPT_PROMOTE, 0)
    data, offs = parity.pack([("<|q|>zqzq" * 5000).encode()])
    enc2.encode_batch_special(data, offs, [0, 1])
    st = enc2.piece_stats(reset=True)
    assert (st["pieces"], st["short_misses"], st["long_misses"], st["memo_lookups"]) == (10000, 0, 0, 0), st


def test_limits_and_arguments(lib, vocabs, oracle_mod):
    v, ov = vocabs("gpt2")
    data, offs = parity.pack([b"hello <|endoftext|> you"])
    for specials in ({"<|s%d|>" % i: 70000 + i for i in range(257)}, {"<|" + "x" * 126 + "|>": 70000, SC.EOT: 50256}, {"<|big|>": 1 << 26}):
        enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 1, specials)
        with pytest.raises(N.UnsupportedError):
            enc.encode_batch_special(data, offs, [0])
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 1, SC.SPECIAL_SETS["synth100k"])
    for bad in ([5], [-1], [0, 0], [1, 2, 1]):
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_special(data, offs, bad)
        assert ei.value.code == N.E_ARG


def test_python_mirror(lib, vocab_bytes, oracle_mod):
    from tokenizer_amd.tokenizer import TikTokenizer, REGEX_CL100K
    raw = vocab_bytes("synth100k")
    specials = SC.SPECIAL_SETS["synth100k"]
    tok = TikTokenizer(raw, specials, REGEX_CL100K, lib=lib)
    oenc = oracle_mod.Encoder(oracle_mod.Vocab(raw), 2, specials=specials)
    rng = random.Random(11)
    texts = ["Hello <|endoftext|> World<|fim_prefix|>", "", "<|endofprompt|><|endofprompt|>x", "plain", "a   <|endoftext|>b"] + SC.random_docs(rng, specials, 300, 3000)
    names = list(specials)
    for allowed in (True, names, names[:2], False):
        want = names if allowed is True else (allowed or [])
        b0, l0 = tok._encoder.special_stats()
        got = tok.EncodeBatch(texts, allowed)
        exp = [oenc.encode(t, want) for t in texts]
        assert got == exp, allowed
        b1, l1 = tok._encoder.special_stats()
        n_lit = sum(1 for e in exp for i in e if i in [specials[w] for w in want])
        assert (b1 - b0, l1 - l0) == ((1, n_lit) if want else (0, 0)), allowed
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TikTokenizer(raw, many, REGEX_CL100K, lib=lib)
    oenc2 = oracle_mod.Encoder(oracle_mod.Vocab(raw), 2, specials=many)
    t = "a<|s7|>b <|s299|><|s30|"
    assert tok2.Encode(t, True) == oenc2.encode(t, list(many)) and tok2._special_on_host


def test_reference_unit_tests_through_the_device_path(lib, gpt2_tiktoken_bytes, lib_rs_bytes, oracle_mod, oracle_gpt2):
    import reference_style
    reference_style.run_gpt2_suite(lib, gpt2_tiktoken_bytes, lib_rs_bytes.decode("utf-8"), oracle_mod, oracle_gpt2)


@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_special_and_plain_calls_side_by_side(lib, vocabs, oracle_mod, pattern):
    """Special calls on one thread, plain calls of the same buffers on another, and both kinds in turn on one thread around a batch in flight."""
    import torch
    dev = torch.device("cuda", 0)

    def upload(a):
        tns = torch.from_numpy(a).to(dev)
        return tns, tns.data_ptr()
    v, ov = vocabs("gpt2")
    SC.check_special_beside_plain(lib, oracle_mod, v, ov, pattern, upload=upload)
