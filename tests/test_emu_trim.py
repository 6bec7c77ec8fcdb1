"""`not gpu`: EncodeTrimSuffix / EncodeTrimPrefix for a batch on the device (tkz_encode_batch_trim_utf8 and the kernels behind it: the piece-granular
launch sequence with the literal kernels, k_trim_cut, the scan of the kept lengths, k_trim_gather) -- the real kernel sources on the CPU emulator
(tests/hostemu/), exact against oracle.TrimOracle's restatement of TikTokenizer.cs:288-579.  Small sizes; tests/test_gpu_trim.py runs the shapes at
which the kernels take their other paths."""
import numpy as np
import pytest

import emu
import parity
import special_cases as SC
import trim_cases as TC
from tokenizer_amd import _native as N

# pattern -> the vocabulary it runs with (tests/conftest.py: vocab_bytes)
VOCAB_OF = {1: "gpt2", 2: "synth100k", 4: "synth200k"}
PATTERNS = (1, 2, 4)
SHORT_TOKENS = 14          # documents of at most this many tokens take part in the maximum sweeps; longer ones are cut at a few maxima


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def setup(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(pattern, specials=None):
        key = (pattern, None if specials is None else tuple(specials.items()))
        if key not in cache:
            name = VOCAB_OF[pattern]
            raw = vocab_bytes(name)
            sp = SC.SPECIAL_SETS[name] if specials is None else specials
            ov = oracle_mod.Vocab(raw)
            cache[key] = (N.Vocab(raw, lib), sp, TC.Expect(oracle_mod, ov, pattern, sp), oracle_mod.Encoder(ov, pattern, specials=sp))
        return cache[key]
    return get


def make_encoder(v, pattern, specials, sequential=0):
    enc = N.Encoder(v, pattern)
    enc.set_special_tokens(specials)
    enc.set_option(N.OPT_PRETOK_SEQUENTIAL, sequential)
    return enc


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_maximum_sweep(setup, pattern, sequential):
    """Every maximum from 0 past the token count: a limit that falls on a boundary, inside a piece of several tokens, on a literal; a literal as the first,
    the last and the only item, the item that overflows, and -- under the smaller allowed sets -- as plain text."""
    v, specials, exp, _ = setup(pattern)
    enc = make_encoder(v, pattern, specials, sequential)
    docs = SC.edge_docs(specials, o200k=pattern == 4) + TC.REFERENCE_TEXTS
    if pattern == 1:
        assert exp.count(" 😀", []) == 2                     # (a piece of two tokens: the limit 1 falls inside it)
    for allowed in SC.allowed_choices(specials):
        short = [d for d in docs if exp.count(d, allowed) <= SHORT_TOKENS]
        long_ = [d for d in docs if exp.count(d, allowed) > SHORT_TOKENS]
        assert len(short) >= 30 and long_
        for side in TC.SIDES:
            what = "pattern %d sequential %d allowed %s" % (pattern, sequential, allowed)
            assert 8 <= TC.sweep(enc, exp, specials, allowed, short, side, what) <= SHORT_TOKENS + 1
            for mx in (SHORT_TOKENS + 3, 200):
                TC.compare(enc, exp, specials, allowed, long_, side, mx, what + ", the long documents")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_batch_shapes(setup, pattern):
    v, specials, exp, _ = setup(pattern)
    enc = make_encoder(v, pattern, specials)
    names = list(specials)
    a = names[0]
    docs = ["", "Hello World" + a, "", "", a + " it's 12345 tokens " + a + a, "", " 😀 漢字かな " + a, a, "", "plain text without a literal, long enough to be cut", ""]
    for side in TC.SIDES:
        # a batch equals its documents one by one
        for mx in (0, 1, 3, 7):
            data, offs = parity.pack([d.encode("utf-8") for d in docs])
            ids, ooff, cb, cu = enc.encode_batch_trim(data, offs, [0], side, mx)
            for d, doc in enumerate(docs):
                one = parity.pack([doc.encode("utf-8")])
                i1, o1, b1, u1 = enc.encode_batch_trim(one[0], one[1], [0], side, mx)
                assert ids[ooff[d]:ooff[d + 1]].tolist() == i1.tolist() and (int(cb[d]), int(cu[d])) == (int(b1[0]), int(u1[0])), (side, mx, d)
            TC.compare(enc, exp, specials, [a], docs, side, mx, "batch of documents")
        # a maximum per document: 0, small and huge ones, and a negative one the wrapper may not pass (the host entry refuses it)
        per_doc = np.asarray([0, 2, 5, 1 << 40, 3, 0, 1, 0, 7, 4, 1 << 62], np.int64)
        TC.compare(enc, exp, specials, names, docs, side, -1, "a maximum per document", per_doc=per_doc)
        TC.compare(enc, exp, specials, [], docs, side, 99, "a maximum per document, plain", per_doc=per_doc[::-1].copy())
        data, offs = parity.pack([d.encode("utf-8") for d in docs])
        for bad in (dict(max_tokens=-1), dict(max_tokens=5, per_doc=np.where(per_doc == 3, -3, per_doc))):
            with pytest.raises(N.TkzError) as ei:
                enc.encode_batch_trim(data, offs, [0], side, **bad)
            assert ei.value.code == N.E_ARG
    # an empty batch, a batch of empty documents
    for docs0 in ([], ["", "", ""]):
        data, offs = parity.pack([d.encode() for d in docs0])
        ids, ooff, cb, cu = enc.encode_batch_trim(data, offs, [0], N.TRIM_PREFIX, 4)
        assert len(ids) == 0 and ooff.tolist() == [0] * (len(docs0) + 1) and cb.tolist() == [0] * len(docs0) and cu.tolist() == [0] * len(docs0)
    # the side and the allowed set are checked as the special entry checks them
    data, offs = parity.pack([b"hello"])
    for bad in (dict(allowed_index=[0], side=2), dict(allowed_index=[len(names)], side=0), dict(allowed_index=[0, 0], side=1)):
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_trim(data, offs, bad["allowed_index"], bad["side"], 3)
        assert ei.value.code == N.E_ARG


def test_capacity(setup):
    v, specials, exp, oenc = setup(1)
    enc = make_encoder(v, 1, specials)
    docs = ["The quick brown fox jumps over the lazy dog, %d times. " % k * 6 for k in range(12)] + ["", SC.EOT]
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    untrimmed = sum(len(oenc.encode(d, [SC.EOT])) for d in docs)
    for side in TC.SIDES:
        want = TC.expected(exp, docs, [SC.EOT], side, [4] * len(docs))
        kept = len(want[0])
        assert 0 < kept < untrimmed // 10                        # (far below the untrimmed token count)
        ids, ooff, _, _ = enc.encode_batch_trim(data, offs, [0], side, 4, out_cap=kept)      # exactly the kept total
        assert ids.tolist() == want[0] and ooff.tolist() == want[1]
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_trim(data, offs, [0], side, 4, out_cap=kept - 1)
        assert ei.value.code == N.E_CAPACITY and ei.value.needed == kept
        ids, ooff, _, _ = enc.encode_batch_trim(data, offs, [0], side, 4, out_cap=kept + 5)
        assert ids.tolist() == want[0]
        # the wrapper's default capacity is the bound of tkz.h: min(bytes, documents * maximum)
        assert enc.encode_batch_trim(data, offs, [0], side, 4)[0].tolist() == want[0]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_leaves_the_plain_path_alone(setup, pattern):
    v, specials, exp, _ = setup(pattern)
    enc = make_encoder(v, pattern, specials)
    docs = SC.edge_docs(specials, o200k=pattern == 4)
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    everything = SC.indices(specials, list(specials))
    stats0 = enc.special_stats()
    plain = enc.encode_batch(data, offs)
    for side in TC.SIDES:
        ids, ooff, cb, cu = enc.encode_batch_trim(data, offs, [], side, len(data))
        assert ids.tolist() == plain[0].tolist() and ooff.tolist() == plain[1].tolist()
        lens = [len(d.encode("utf-8")) for d in docs]
        assert cb.tolist() == (lens if side == N.TRIM_SUFFIX else [0] * len(docs))
        assert cu.tolist() == ([TC.utf16_len(d) for d in docs] if side == N.TRIM_SUFFIX else [0] * len(docs))
    assert enc.special_stats() == stats0                          # (n_allowed == 0: no literal kernel ran, nothing was counted)
    special = enc.encode_batch_special(data, offs, everything)
    stats1 = enc.special_stats()
    for side in TC.SIDES:
        ids, ooff, _, _ = enc.encode_batch_trim(data, offs, everything, side, len(data))
        assert ids.tolist() == special[0].tolist() and ooff.tolist() == special[1].tolist()
    assert enc.special_stats() == (stats1[0] + 2, stats1[1] + 2 * (stats1[1] - stats0[1]))
    after = enc.encode_batch(data, offs)
    assert after[0].tolist() == plain[0].tolist() and after[1].tolist() == plain[1].tolist()


def test_mirrors(lib, vocab_bytes, oracle_mod):
    """EncodeTrimSuffixBatch / EncodeTrimPrefixBatch against TrimOracle text by text: one device call for the batch, the cut inside a surrogate pair's
    neighbourhood, a lone surrogate, both overload shapes; the fallbacks to the host walk."""
    from tokenizer_amd.tokenizer import TikTokenizer, REGEX_CL100K
    raw = vocab_bytes("synth100k")
    specials = SC.SPECIAL_SETS["synth100k"]
    tok = TikTokenizer(raw, specials, REGEX_CL100K, lib=lib)
    oracle = oracle_mod.TrimOracle(oracle_mod.Vocab(raw), 2, specials)
    names = list(specials)
    texts = ["Hello <|endoftext|> World<|fim_prefix|> tail", "", "ab \U0001F600\U0001F600 cd \U0001F600", "x\U0001D400y\U0001D401z", "a \ud800 b \udc00c", names[4] * 3 + "x",
             "plain text only", "中文 <|endoftext|>中文"]
    for mx in (0, 1, 2, 3, 5, 8, 1000):
        for allowed in (names, names[:1], None):
            b0 = tok._encoder.special_stats()[0]
            assert tok.EncodeTrimSuffixBatch(texts, allowed or [], mx) == [oracle.encode_trim_suffix(t, allowed, mx) for t in texts], (mx, allowed)
            assert tok.EncodeTrimPrefixBatch(texts, allowed or [], mx) == [oracle.encode_trim_prefix(t, allowed, mx) for t in texts], (mx, allowed)
            assert tok._encoder.special_stats()[0] - b0 == (2 if allowed else 0)          # one device call per batch
        assert tok.EncodeTrimSuffixBatch(texts, mx) == [oracle.encode_trim_suffix(t, names, mx) for t in texts]
        assert tok.EncodeTrimPrefixBatch(texts, mx, False) == [oracle.encode_trim_prefix(t, None, mx) for t in texts]
        for t in texts[:4]:
            assert tok.EncodeTrimSuffix(t, names, mx) == oracle.encode_trim_suffix(t, names, mx)
            assert tok.EncodeTrimPrefix(t, names, mx) == oracle.encode_trim_prefix(t, names, mx)
    assert tok.EncodeTrimSuffixBatch([], 3) == [] and tok.EncodeTrimPrefixBatch([], names, 3) == []
    # a negative maximum: the host walk keeps the reference's answers (suffix: nothing; prefix: the whole text)
    assert tok.EncodeTrimSuffixBatch(texts[:1], names, -1) == [oracle.encode_trim_suffix(texts[0], names, -1)]
    assert tok.EncodeTrimPrefixBatch(texts[:1], names, -1) == [oracle.encode_trim_prefix(texts[0], names, -1)]
    # a set beyond the device path: the host walk, from here on
    many = {"<|s%d|>" % i: 200000 + i for i in range(300)}
    tok2 = TikTokenizer(raw, many, REGEX_CL100K, lib=lib)
    oracle2 = oracle_mod.TrimOracle(oracle_mod.Vocab(raw), 2, many)
    t = "a<|s7|>b <|s299|><|s30|"
    assert tok2.EncodeTrimSuffixBatch([t, "x"], 3) == [oracle2.encode_trim_suffix(t, list(many), 3), oracle2.encode_trim_suffix("x", list(many), 3)]
    assert tok2._special_on_host and tok2._encoder.special_stats() == (0, 0)
    assert tok2.EncodeTrimPrefixBatch([t], 2) == [oracle2.encode_trim_prefix(t, list(many), 2)]
    # a lone surrogate while a literal holds U+FFFD: the host walk (the reference searches UTF-16)
    fffd = {"<�>": 300001}
    tok3 = TikTokenizer(raw, fffd, REGEX_CL100K, lib=lib)
    oracle3 = oracle_mod.TrimOracle(oracle_mod.Vocab(raw), 2, fffd)
    for t in ("a<�>b c", "a<\ud800>b c"):
        for mx in (1, 2, 9):
            assert tok3.EncodeTrimSuffixBatch([t], mx) == [oracle3.encode_trim_suffix(t, list(fffd), mx)]
            assert tok3.EncodeTrimPrefixBatch([t], mx) == [oracle3.encode_trim_prefix(t, list(fffd), mx)]
    assert tok3._encoder.special_stats()[0] == 6                 # (the text with the literal went to the device, the one with the lone surrogate did not)


def test_single_text_methods_pass_the_reference_suite(lib, gpt2_tiktoken_bytes, lib_rs_bytes, oracle_mod, oracle_gpt2):
    """tests/reference_style.py's trim suite, unchanged, over the single-text methods -- which are now the batch methods with one text."""
    import reference_style as RS
    from tokenizer_amd import REGEX_PATTERN_1, TokenizerBuilder
    specials = {"<|endoftext|>": 50256, RS.IM_START: 50300, RS.IM_END: 50301}
    tok = TokenizerBuilder.CreateTokenizer(gpt2_tiktoken_bytes, specials, REGEX_PATTERN_1, lib=lib)
    b0 = tok._encoder.special_stats()[0]
    RS.run_trim_suite(tok, oracle_mod.TrimOracle(oracle_gpt2, oracle_mod.P1, specials), specials, lib_rs_bytes.decode("utf-8"))
    assert tok._encoder.special_stats()[0] > b0                   # (through the device's trim entry)


def test_cpp_mirror_batch_methods(lib, tmp_path, gpt2_tiktoken_bytes):
    """include/tkz_tokenizer.hpp: EncodeTrimSuffixBatch / EncodeTrimPrefixBatch against the header's own host walk (tests/cpp/test_trim_batch.cpp)."""
    import os
    import subprocess
    from conftest import ROOT
    libdir, libname = os.path.dirname(emu.EMU_LIB), "tkz_hostemu"
    (tmp_path / "gpt2.tiktoken").write_bytes(gpt2_tiktoken_bytes)
    exe = str(tmp_path / "test_trim_batch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_trim_batch.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "gpt2.tiktoken")], capture_output=True, text=True)
    assert out.returncode == 0 and "cpp trim batch ok" in out.stdout, out.stdout + out.stderr
