"""`not gpu`: special tokens and trimming for UTF-16 batches (tkz_encode_batch_special_utf16 / tkz_encode_batch_trim_utf16: the transcoder's replaced-byte
bitmap, the literal kernels that read it, k_probe_special's lookup of the literal's id) -- the real kernel sources on the CPU emulator (tests/hostemu/), exact
against oracle.TrimOracle on the strings the code units are.  tests/test_gpu_u16_special.py runs the same builders through libtkz.so."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
import parity
import special_cases as SC
import trim_cases as TC
import u16_special_cases as US
from conftest import ROOT
from tokenizer_amd import _native as N

VOCAB_OF = {1: "gpt2", 2: "synth100k", 4: "synth200k"}
PATTERNS = (1, 2, 4)


@pytest.fixture(scope="module")
def lib():
    return emu.library()


@pytest.fixture(scope="module")
def setup(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(pattern, specials=None):
        name = VOCAB_OF[pattern]
        sp = SC.SPECIAL_SETS[name] if specials is None else specials
        key = (pattern, tuple(sp.items()))
        if key not in cache:
            raw = vocab_bytes(name)
            cache[key] = (N.Vocab(raw, lib), sp, US.Expect(oracle_mod, oracle_mod.Vocab(raw), pattern, sp))
        return cache[key]
    return get


def make_encoder(v, pattern, specials, sequential=0):
    enc = N.Encoder(v, pattern)
    enc.set_special_tokens(specials)
    enc.set_option(N.OPT_PRETOK_SEQUENTIAL, sequential)
    return enc


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_agrees_with_the_utf8_entries(setup, pattern, sequential):
    """SC.edge_docs / SC.order_cases / the trim tests' texts, as units: the UTF-8 entries' results on the same texts, and the oracle's."""
    v, specials, exp = setup(pattern)
    enc = make_encoder(v, pattern, specials, sequential)
    strs = SC.edge_docs(specials, o200k=pattern == 4) + TC.REFERENCE_TEXTS
    for allowed in SC.allowed_choices(specials):
        what = "pattern %d sequential %d allowed %s" % (pattern, sequential, allowed)
        US.agree_with_utf8(enc, specials, allowed, strs, what)
        US.compare_special(enc, exp, specials, allowed, US.as_units(strs), what)
    short = [s for s in strs if len(s) < 60]
    for side in US.SIDES:
        for mx in (1, 4):
            US.compare_trim(enc, exp, specials, list(specials), US.as_units(short), side, mx, "pattern %d" % pattern)
    if pattern == 1:
        for sp, allowed_sets, docs in SC.order_cases():
            v1, _, exp1 = setup(1, sp)
            enc1 = make_encoder(v1, 1, sp, sequential)
            for allowed in allowed_sets:
                US.agree_with_utf8(enc1, sp, allowed, docs, "order cases %s allowed %s" % (list(sp), allowed))
                US.compare_special(enc1, exp1, sp, allowed, US.as_units(docs), "order cases %s allowed %s" % (list(sp), allowed))


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_lone_surrogates_against_a_fffd_literal(setup, pattern, sequential):
    v, specials, exp = setup(pattern, US.FFFD_SPECIALS)
    enc = make_encoder(v, pattern, specials, sequential)
    docs = US.lone_expectations(exp)
    b0, l0 = enc.special_stats()
    for allowed in ([US.A, US.B, US.C], [US.A], [US.B], [US.A, US.C], [US.C]):
        US.check_both(enc, exp, specials, allowed, docs, "pattern %d sequential %d allowed %r" % (pattern, sequential, allowed))
        for d in docs:                                        # ... and every document as a batch of its own
            US.compare_special(enc, exp, specials, allowed, [d], "one document %r, allowed %r" % (US.text(d), allowed))
    b1, l1 = enc.special_stats()
    assert b1 > b0 and l1 > l0                                # (the device path was taken)
    # the case the bitmap exists for, spelled out: `x` + a lone high half with only A allowed is plain text, with B allowed it is B
    flat, offs = US.pack([docs[0]])
    ida, idb = specials[US.A], specials[US.B]
    assert ida not in enc.encode_batch_special_utf16(flat, offs, [0])[0].tolist()
    assert idb in enc.encode_batch_special_utf16(flat, offs, [0, 1])[0].tolist() and ida not in enc.encode_batch_special_utf16(flat, offs, [0, 1])[0].tolist()
    flat, offs = US.pack([docs[1]])
    assert ida in enc.encode_batch_special_utf16(flat, offs, [0])[0].tolist()


@pytest.mark.parametrize("pattern", [1, 4])
def test_edge_positions(setup, pattern):
    v, specials, exp = setup(pattern, US.EDGE_SPECIALS)
    enc = make_encoder(v, pattern, specials)
    batches = US.edge_batches()
    US.edge_smoke(batches)
    for what, allowed_sets, docs in batches:
        for allowed in allowed_sets:
            US.compare_special(enc, exp, specials, allowed, docs, "%s, allowed %r" % (what, allowed))
        for side in US.SIDES:
            tokens = len(exp.encode(docs[0], allowed_sets[0]))
            for mx in (tokens - 3, tokens - 1):               # (around the items at the end of the first document: the pattern and its tail)
                US.compare_trim(enc, exp, specials, allowed_sets[0], docs, side, max(mx, 0), what)


def test_chunk_pipeline(setup):
    """the chunk size is read once per process: a child interpreter with 4 KiB chunks (several chunks, an empty one, chunks that end in a lone high half)"""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gzip, emu, u16_special_cases as US\n"
            "from tokenizer_amd import _native as N\n"
            "from oracle import oracle as O\n"
            "raw = gzip.decompress(open(%r, 'rb').read())\n"
            "lib = emu.library()\n"
            "enc = N.Encoder(N.Vocab(raw, lib), N.CL100K)\n"
            "enc.set_special_tokens(US.FFFD_SPECIALS)\n"
            "n = US.check_chunks(enc, US.Expect(O, O.Vocab(raw), N.CL100K, US.FFFD_SPECIALS), US.FFFD_SPECIALS)\n"
            "print('U16_SPECIAL_CHUNKS_OK', n)\n") % (ROOT, tests, os.path.join(tests, "golden", "gpt2.tiktoken.gz"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TKZ_HOST_CHUNK_BYTES="4096"), capture_output=True, text=True, timeout=600)
    assert "U16_SPECIAL_CHUNKS_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split("U16_SPECIAL_CHUNKS_OK")[1].split()[0]) * 2 > 5 * 4096        # (more than five chunks' worth of upload)


def test_error_paths(setup):
    v, specials, exp = setup(1, US.FFFD_SPECIALS)
    enc = make_encoder(v, 1, specials)
    docs = US.lone_docs()
    flat, offs = US.pack(docs)
    want = US.compare_special(enc, exp, specials, [US.A, US.B, US.C], docs, "capacity")
    # TKZ_E_CAPACITY with *needed; exactly enough is enough
    ids, _ = enc.encode_batch_special_utf16(flat, offs, [0, 1, 2], out_cap=len(want))
    assert ids.tolist() == want
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_special_utf16(flat, offs, [0, 1, 2], out_cap=len(want) - 1)
    assert ei.value.code == N.E_CAPACITY and ei.value.needed == len(want)
    for side in US.SIDES:
        kept = US.compare_trim(enc, exp, specials, [US.A, US.B, US.C], docs, side, 2, "capacity")
        assert 0 < len(kept) < len(want)
        assert enc.encode_batch_trim_utf16(flat, offs, [0, 1, 2], side, 2, out_cap=len(kept))[0].tolist() == kept
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_trim_utf16(flat, offs, [0, 1, 2], side, 2, out_cap=len(kept) - 1)
        assert ei.value.code == N.E_CAPACITY and ei.value.needed == len(kept)
    # a bad allowed index, a bad side, a negative maximum
    for bad in ([3], [-1], [0, 0]):
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_special_utf16(flat, offs, bad)
        assert ei.value.code == N.E_ARG
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_trim_utf16(flat, offs, bad, N.TRIM_SUFFIX, 3)
        assert ei.value.code == N.E_ARG
    for kw in (dict(side=2, max_tokens=3), dict(side=0, max_tokens=-1), dict(side=1, max_tokens=3, per_doc=np.asarray([1] * (len(docs) - 1) + [-2], np.int64))):
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_trim_utf16(flat, offs, [0], **kw)
        assert ei.value.code == N.E_ARG
    # unit offsets that do not end at the unit count / are not monotone
    for bad_offs in (np.asarray([0, 5, 3, len(flat)], np.int64),):
        with pytest.raises(N.TkzError) as ei:
            enc.encode_batch_trim_utf16(flat, bad_offs, [0], N.TRIM_SUFFIX, 3)
        assert ei.value.code == N.E_ARG
    # a maximum per document
    per_doc = np.asarray([0, 2, 5, 1 << 40, 3, 0, 1, 0, 7, 4, 1 << 62, 2], np.int64)
    for side in US.SIDES:
        US.compare_trim(enc, exp, specials, [US.A, US.B, US.C], docs, side, -1, "a maximum per document", per_doc=per_doc)
    # more than 256 literals: TKZ_E_UNSUPPORTED from both entries; nothing allowed is still the plain entry
    many = {"<|s%d|>" % i: 70000 + i for i in range(257)}
    enc2 = make_encoder(v, 1, many)
    with pytest.raises(N.UnsupportedError):
        enc2.encode_batch_special_utf16(flat, offs, [0])
    with pytest.raises(N.UnsupportedError):
        enc2.encode_batch_trim_utf16(flat, offs, [0], N.TRIM_PREFIX, 3)
    assert enc2.encode_batch_special_utf16(flat, offs, [])[0].tolist() == enc2.encode_batch_utf16(flat, offs)[0].tolist()
    # n_docs == 0, all-empty documents
    for docs0 in ([], [[], [], []]):
        f0, o0 = US.pack(docs0)
        ids, ooff = enc.encode_batch_special_utf16(f0, o0, [0, 1])
        assert len(ids) == 0 and ooff.tolist() == [0] * (len(docs0) + 1)
        for side in US.SIDES:
            ids, ooff, cu = enc.encode_batch_trim_utf16(f0, o0, [0, 1], side, 4)
            assert len(ids) == 0 and ooff.tolist() == [0] * (len(docs0) + 1) and cu.tolist() == [0] * len(docs0)
    # n_allowed == 0 is tkz_encode_batch_utf16, and counts as no special call
    s0 = enc.special_stats()
    a = enc.encode_batch_special_utf16(flat, offs, [])
    b = enc.encode_batch_utf16(flat, offs)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and enc.special_stats() == s0
    for side in US.SIDES:
        ids, ooff, cu = enc.encode_batch_trim_utf16(flat, offs, [], side, 3 * len(flat))
        assert ids.tolist() == b[0].tolist() and ooff.tolist() == b[1].tolist()
        assert cu.tolist() == ([len(d) for d in docs] if side == N.TRIM_SUFFIX else [0] * len(docs))
    assert enc.special_stats() == s0


def test_utf8_entries_untouched(setup):
    """the UTF-8 special entry launches what it launched: the same kernel launch counts per bracket before and after UTF-16 special calls, with a U+FFFD
    literal registered; and its result on text that holds a real U+FFFD is what it was (no bitmap: the bytes decide)"""
    v, specials, exp = setup(2, US.FFFD_SPECIALS)
    enc = make_encoder(v, 2, specials)
    strs = ["a x� b", "plain <�> text", "x", "", "no literal"] + [US._WORDS * 40]
    data, offs = parity.pack([s.encode("utf-8") for s in strs])
    flat, uoffs = US.pack(US.lone_docs())
    before = enc.encode_batch_special(data, offs, [0, 1, 2])
    enc.set_profiling(True)
    try:
        enc.kernel_ms(reset=True)
        enc.encode_batch_special(data, offs, [0, 1, 2])
        launches0 = enc.kernel_ms(reset=True)
        enc.encode_batch_special_utf16(flat, uoffs, [0, 1, 2])
        enc.encode_batch_trim_utf16(flat, uoffs, [0, 1, 2], N.TRIM_SUFFIX, 3)
        enc.kernel_ms(reset=True)
        enc.encode_batch_special(data, offs, [0, 1, 2])
        launches1 = enc.kernel_ms(reset=True)
    finally:
        enc.set_profiling(False)
    count = lambda r: [n for _, n in r.values()]
    assert count(launches0) == count(launches1)
    after = enc.encode_batch_special(data, offs, [0, 1, 2])
    assert before[0].tolist() == after[0].tolist() and before[1].tolist() == after[1].tolist()
    US.compare_special(enc, exp, specials, [US.A, US.B, US.C], US.as_units(strs), "the same texts as units")


def test_cpp_mirror_utf16_methods(lib, tmp_path, gpt2_tiktoken_bytes):
    """include/tkz_tokenizer.hpp: the std::u16string methods against the header's own host walk (tests/cpp/test_u16_special.cpp)."""
    libdir, libname = os.path.dirname(emu.EMU_LIB), "tkz_hostemu"
    (tmp_path / "gpt2.tiktoken").write_bytes(gpt2_tiktoken_bytes)
    exe = str(tmp_path / "test_u16_special")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_u16_special.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "gpt2.tiktoken")], capture_output=True, text=True)
    assert out.returncode == 0 and "cpp u16 special ok" in out.stdout, out.stdout + out.stderr
