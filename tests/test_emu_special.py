"""`not gpu`: special tokens on the device (tkz_encode_batch_special_utf8 and the kernels behind it: k_lit_scan, k_lit_resolve, k_lit_fix,
k_probe_special) -- the real kernel sources on the CPU emulator (tests/hostemu/), bit-exact against the oracle's restatement of EncodeInternal.
Small sizes; tests/test_gpu_special.py runs the same cases at full size."""
import random

import numpy as np
import pytest

import emu
import parity
import special_cases as SC
from tokenizer_amd import _native as N


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def vocabs(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            raw = vocab_bytes(name)
            cache[name] = (N.Vocab(raw, lib), oracle_mod.Vocab(raw))
        return cache[name]
    return get


@pytest.mark.parametrize("pattern", SC.PATTERNS)
@pytest.mark.parametrize("name", list(SC.SPECIAL_SETS))
def test_edge_cases(lib, vocabs, oracle_mod, name, pattern):
    v, ov = vocabs(name)
    specials = SC.SPECIAL_SETS[name]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
    docs = SC.edge_docs(specials, o200k=pattern in (3, 4))
    b0, l0 = enc.special_stats()
    for allowed in SC.allowed_choices(specials):
        SC.compare(enc, oenc, specials, allowed, docs, "%s pattern %d allowed %s" % (name, pattern, allowed))
    assert enc.special_stats()[0] > b0 and enc.special_stats()[1] > l0          # (the device path was taken)
    # nothing allowed / no literal in the text: the plain entry's result
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    ids0, off0 = enc.encode_batch(data, offs)
    ids1, off1 = enc.encode_batch_special(data, offs, [])
    assert ids0.tolist() == ids1.tolist() and off0.tolist() == off1.tolist()
    plain_docs = ["no literal here", "", "nor < | here |>"]
    data, offs = parity.pack([d.encode("utf-8") for d in plain_docs])
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
            SC.compare(enc, oenc, specials, allowed, ["".join(docs)], "joined, %s allowed %s" % (list(specials), allowed))


def test_literal_bytes_outside_the_vocabulary(lib, oracle_mod):
    """A literal whose bytes are not all vocabulary keys: as plain text it raises KeyNotFound, as a special token it is its id."""
    import base64
    raw = b"".join(base64.b64encode(k) + b" %d\n" % r for r, k in enumerate([b"a", b"b", b"c", b" ", b"ab", b"bc", b" a", b"abc", b"ca"]))      # a tiny rank table
    v, ov = N.Vocab(raw, lib), oracle_mod.Vocab(raw)
    specials = {"<|z|>": 900, "zz": 901}
    for pattern in SC.PATTERNS:
        enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
        docs = ["abc<|z|>cab", "<|z|>", "zzabzz", "a zz b<|z|>"]
        SC.compare(enc, oenc, specials, list(specials), docs, "pattern %d" % pattern)
        data, offs = parity.pack([d.encode() for d in docs])
        with pytest.raises(N.KeyNotFoundError):
            enc.encode_batch_special(data, offs, [1])


@pytest.mark.parametrize("pattern", SC.PATTERNS)
def test_literals_across_kernel_boundaries(lib, vocabs, oracle_mod, pattern):
    """64-byte row, 1 KiB sub-tile, 4 KiB pre-tokenizer / scan block, 16 sub-tile group: the literal at every offset across each."""
    v, ov = vocabs("gpt2")
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
    for doc in SC.boundary_docs(SC.EOT, (64, 1024, 4096)) + SC.boundary_docs(SC.EOT, (16384,), shifts=(0, 1, 6, 12, 13)):
        SC.compare(enc, oenc, specials, [SC.EOT], [doc], "boundary, %d bytes" % len(doc))
    # ... and with documents ending right there
    docs = []
    for B in (64, 1024, 4096):
        for k in (0, 1, 7, 13):
            docs += ["x" * (B - k - sum(map(len, docs)) % B), SC.EOT, "", SC.EOT[:k]]
    SC.compare(enc, oenc, specials, [SC.EOT], docs, "documents ending at boundaries")


@pytest.mark.parametrize("name,pattern", [("gpt2", 1), ("synth100k", 2), ("synth200k", 3), ("synth200k", 4), ("gpt2", 2)])
def test_random_batches(lib, vocabs, oracle_mod, name, pattern, monkeypatch):
    v, ov = vocabs(name)
    specials = SC.SPECIAL_SETS[name]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, pattern, specials)
    for seed in range(25):
        rng = random.Random(1000 * pattern + seed)
        docs = SC.random_docs(rng, specials, rng.choice([1, 3, 12]), 3000)
        allowed = rng.choice(SC.allowed_choices(specials))
        SC.compare(enc, oenc, specials, allowed, docs, "%s pattern %d seed %d allowed %s" % (name, pattern, seed, allowed))


def test_throughput_form_and_chunks(lib, vocabs, oracle_mod, monkeypatch):
    """TKZ_OPT_LATENCY_BYTES = 0 (the large batches' form of the merge kernels) and a host batch cut into chunks, a cut right before / after a literal."""
    monkeypatch.setenv("TKZ_LATENCY_BYTES", "0")
    v, ov = vocabs("gpt2")
    specials = SC.SPECIAL_SETS["gpt2"]
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 2, specials)
    rng = random.Random(77)
    for seed in range(4):
        docs = SC.random_docs(rng, specials, 10, 3000)
        SC.compare(enc, oenc, specials, [SC.EOT], docs, "throughput form, round %d" % seed)


def test_memo_and_promotions_never_hold_a_literal(lib, vocabs, oracle_mod):
    v, ov = vocabs("gpt2")
    specials = {"<|q|>": 60001, "zqzq": 60002}
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 2, specials)
    enc.set_option(N.OPT_PIECE_STATS, 1)
    enc.set_option(N.OPT_PROMOTE_MIN_BYTES, 4096)
    rng = random.Random(5)
    docs = ["".join(rng.choice(["<|q|>", "zqzq", " word", " zqz", "qzq "]) for _ in range(300)) for _ in range(8)]
    for _ in range(3):
        SC.compare(enc, oenc, specials, list(specials), docs, "dense in literals")
    enc.set_option(N.OPT_PROMOTE, 2)
    SC.compare(enc, oenc, specials, list(specials), docs, "after a promotion")
    # as plain text the literals are pieces that miss the vocabulary; as special tokens they never reach a miss list: the same text with the
    # literals allowed counts fewer misses than with none allowed
    enc2, _ = SC.make_encoders(lib, oracle_mod, v, ov, 2, specials)
    enc2.set_option(N.OPT_PIECE_STATS, 1)
    enc2.set_option(N.OPT_PROMOTE, 0)
    data, offs = parity.pack([("<|q|>" * 50).encode()])
    enc2.encode_batch_special(data, offs, [0, 1])
    st = enc2.piece_stats(reset=True)
    assert (st["pieces"], st["short_misses"], st["long_misses"], st["memo_lookups"]) == (50, 0, 0, 0), st       # 50 pieces, no miss of any length, no memo lookup


def test_limits_and_arguments(lib, vocabs, oracle_mod):
    from tokenizer_amd.tokenizer import TikTokenizer, REGEX_PATTERN_1
    v, ov = vocabs("gpt2")
    data, offs = parity.pack([b"hello <|endoftext|> you"])
    for specials in ({"<|s%d|>" % i: 70000 + i for i in range(257)}, {"<|" + "x" * 126 + "|>": 70000, SC.EOT: 50256}, {"<|big|>": 1 << 26}):
        enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 1, specials)
        with pytest.raises(N.UnsupportedError):
            enc.encode_batch_special(data, offs, [0])
        assert enc.encode_batch_special(data, offs, [])[0].tolist() == enc.encode_batch(data, offs)[0].tolist()
    enc = N.Encoder(v, 1)
    ids = np.asarray([5, 6], np.int32)
    blob = np.frombuffer(b"ab", np.uint8)
    lib.check(lib.L.tkz_encoder_set_special_tokens(enc._h, N._ptr(ids), N._ptr(blob), N._ptr(np.asarray([0, 0, 2], np.int64)), 2))      # an empty literal
    with pytest.raises(N.UnsupportedError):
        enc.encode_batch_special(data, offs, [1])
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 1, SC.SPECIAL_SETS["synth100k"])
    for bad in ([5], [-1], [0, 0], [1, 2, 1]):
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_special(data, offs, bad)
        assert ei.value.code == N.E_ARG
    # 128 bytes exactly is held
    specials = {"<|" + "y" * 124 + "|>": 70001}
    enc, oenc = SC.make_encoders(lib, oracle_mod, v, ov, 1, specials)
    SC.compare(enc, oenc, specials, list(specials), ["a" + list(specials)[0] + "b", list(specials)[0][:-1], "x" * 1000 + list(specials)[0]], "128-byte literal")


def test_python_mirror(lib, vocab_bytes, oracle_mod):
    """TikTokenizer.Encode / EncodeBatch / EncodeBatchFlat with True and with a list: ONE device call, counted by tkz_encoder_special_stats; the fallback
    for a set the device does not hold; the lone-surrogate edge."""
    from tokenizer_amd.tokenizer import TikTokenizer, REGEX_CL100K
    raw = vocab_bytes("synth100k")
    specials = SC.SPECIAL_SETS["synth100k"]
    tok = TikTokenizer(raw, specials, REGEX_CL100K, lib=lib)
    oenc = oracle_mod.Encoder(oracle_mod.Vocab(raw), 2, specials=specials)
    texts = ["Hello <|endoftext|> World<|fim_prefix|>", "", "<|endofprompt|><|endofprompt|>x", "plain", "a   <|endoftext|>b"]
    names = list(specials)
    for allowed in (True, names, names[:2], [names[4]], False, []):
        want = names if allowed is True else (allowed or [])
        b0, l0 = tok._encoder.special_stats()
        got = tok.EncodeBatch(texts, allowed)
        assert got == [oenc.encode(t, want) for t in texts], allowed
        b1, l1 = tok._encoder.special_stats()
        n_lit = sum(1 for t in texts for i in oenc.encode(t, want) if i in [specials[w] for w in want])
        assert (b1 - b0, l1 - l0) == ((1, n_lit) if want else (0, 0)), allowed
        assert tok.Encode(texts[0], allowed) == oenc.encode(texts[0], want)
        ids, offs = tok.EncodeBatchFlat(texts, allowed)
        assert [ids[offs[d]:offs[d + 1]].tolist() for d in range(len(texts))] == got
    # a set beyond the device path: the host segmentation, same ids
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TikTokenizer(raw, many, REGEX_CL100K, lib=lib)
    oenc2 = oracle_mod.Encoder(oracle_mod.Vocab(raw), 2, specials=many)
    t = "a<|s7|>b <|s299|><|s30|"
    assert tok2.Encode(t, True) == oenc2.encode(t, list(many)) and tok2._special_on_host and tok2._encoder.special_stats() == (0, 0)
    # a lone surrogate while a literal holds U+FFFD: the host route (the reference searches UTF-16)
    fffd = {"<�>": 300001}
    tok3 = TikTokenizer(raw, fffd, REGEX_CL100K, lib=lib)
    assert tok3.Encode("a<�>b", True) == oracle_mod.Encoder(oracle_mod.Vocab(raw), 2, specials=fffd).encode("a<�>b", list(fffd))
    assert tok3._encoder.special_stats()[0] == 1
    lone = tok3.Encode("a<\ud800>b", True)
    assert tok3._encoder.special_stats()[0] == 1 and 300001 not in lone


def test_reference_unit_tests_through_the_device_path(lib, gpt2_tiktoken_bytes, lib_rs_bytes, oracle_mod, oracle_gpt2):
    """The reference's own unit tests as tests/reference_style.py restates them (special tokens honoured by default, allow-sets, adjacent and trailing
    specials, EncodeBatch[Flat]): the mirror now sends them through the device's special entry."""
    import reference_style
    reference_style.run_gpt2_suite(lib, gpt2_tiktoken_bytes, lib_rs_bytes.decode("utf-8"), oracle_mod, oracle_gpt2)


@pytest.mark.parametrize("pattern", [N.P1, N.CL100K])
def test_special_and_plain_calls_side_by_side(lib, vocabs, oracle_mod, pattern):
    """Special calls on one thread, plain calls of the same buffers on another, and both kinds in turn on one thread around a batch in flight."""
    v, ov = vocabs("gpt2")
    SC.check_special_beside_plain(lib, oracle_mod, v, ov, pattern)
