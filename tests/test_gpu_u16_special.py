"""`-m gpu`: special tokens and trimming for UTF-16 batches through libtkz.so -- tkz_encode_batch_special_utf16 / tkz_encode_batch_trim_utf16 against the
oracle, exact.  The builders of tests/u16_special_cases.py at the smallest shapes at which the hardware can differ from the emulator: the replaced-byte
bitmap's atomics at tile, lane-group, bitmap-word and scan-block edges, thousands of short documents beside one long one, page-locked and pageable buffers,
two chunks through the real pipeline.  Every batch but the last is at most about 256 KiB."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import special_cases as SC
import u16_special_cases as US
from conftest import ROOT
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu

VOCAB_OF = {1: "gpt2", 2: "synth100k", 4: "synth200k"}


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def setup(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(pattern, specials):
        key = (pattern, tuple(specials.items()))
        if key not in cache:
            raw = vocab_bytes(VOCAB_OF[pattern])
            enc = N.Encoder(N.Vocab(raw, lib), pattern)
            enc.set_special_tokens(specials)
            cache[key] = (enc, US.Expect(oracle_mod, oracle_mod.Vocab(raw), pattern, specials))
        return cache[key]
    return get


def corpus_units(kind, seed, n_docs, min_len, max_len):
    return [US.units(N.corpus_doc_host(kind, seed, d, min_len, max_len).decode("utf-8")) for d in range(n_docs)]


def splice(docs, patterns, every=10):
    """a lone-surrogate pattern / a literal into every tenth document: in front, in the middle, at the end in turn (a cut inside a pair makes two more lone halves)"""
    out = [list(d) for d in docs]
    for k, d in enumerate(range(0, len(out), every)):
        t = out[d]
        at = (0, len(t) // 2, len(t))[k % 3]
        out[d] = t[:at] + patterns[k % len(patterns)] + t[at:]
    return out


@pytest.mark.parametrize("pattern", [1, 4])
def test_lone_surrogates_against_a_fffd_literal(setup, pattern):
    enc, exp = setup(pattern, US.FFFD_SPECIALS)
    docs = US.lone_expectations(exp)
    b0, l0 = enc.special_stats()
    for allowed in ([US.A, US.B, US.C], [US.A], [US.A, US.C]):
        US.check_both(enc, exp, US.FFFD_SPECIALS, allowed, docs, "pattern %d allowed %r" % (pattern, allowed))
    b1, l1 = enc.special_stats()
    assert b1 > b0 and l1 > l0


def test_edge_positions(setup):
    enc, exp = setup(1, US.EDGE_SPECIALS)
    for what, allowed_sets, docs in US.edge_batches():
        for allowed in allowed_sets[:2]:
            US.compare_special(enc, exp, US.EDGE_SPECIALS, allowed, docs, "%s, allowed %r" % (what, allowed))
        tokens = len(exp.encode(docs[0], allowed_sets[0]))
        for side in US.SIDES:
            US.compare_trim(enc, exp, US.EDGE_SPECIALS, allowed_sets[0], docs, side, max(tokens - 2, 0), what)


@pytest.mark.parametrize("kind,pattern", [(1, 1), (2, 2)])
def test_many_documents_beside_a_long_one(setup, kind, pattern):
    """a few thousand short documents beside one of 100 KiB, lone-surrogate patterns and real literals spliced into every tenth: special and trim, both sides"""
    enc, exp = setup(pattern, US.FFFD_SPECIALS)
    small = corpus_units(kind, 31, 3000, 1, 40)
    big = corpus_units(kind, 32, 1, 100 << 10, 100 << 10)[0][:50 << 10]  # 100 KiB as the caller holds it: 51,200 code units
    if 0xD800 <= big[-1] < 0xDC00:                                      # (the cut is not to add a lone half of its own)
        big = big[:-1]
    pats = [US.P_XHI[0], US.P_XREAL[0], US.P_CLO[0], US.P_CREAL[0], US.units(" x") + [US.LO], [US.HI]]
    docs = splice(small[:1500] + [big] + small[1500:], pats)
    assert len(docs[1500]) >= (50 << 10) - 1 and sum(len(d) for d in docs) * 2 <= 256 << 10
    allowed = [US.A, US.B, US.C]
    US.compare_special(enc, exp, US.FFFD_SPECIALS, allowed, docs, "skew, kind %d" % kind)
    US.compare_special(enc, exp, US.FFFD_SPECIALS, [US.A, US.C], docs, "skew, kind %d, without B" % kind)
    per_doc = np.full(len(docs), 4, np.int64)
    per_doc[1500] = 9000
    per_doc[::7] = 0
    for side in US.SIDES:
        US.compare_trim(enc, exp, US.FFFD_SPECIALS, allowed, docs, side, 3, "skew, kind %d" % kind)
        US.compare_trim(enc, exp, US.FFFD_SPECIALS, allowed, docs, side, 0, "skew, kind %d" % kind, per_doc=per_doc)


def test_page_locked_and_pageable_buffers_and_determinism(lib, setup):
    enc, exp = setup(2, US.FFFD_SPECIALS)
    pats = [US.P_XHI[0], US.P_XREAL[0], US.P_CLO[0], US.P_CREAL[0]]
    docs = splice(corpus_units(2, 5, 400, 0, 600), pats)
    flat, offs = US.pack(docs)
    n = len(docs)
    allowed = [0, 1, 2]
    a = enc.encode_batch_special_utf16(flat, offs, allowed)                 # pageable numpy buffers
    b = enc.encode_batch_special_utf16(flat, offs, allowed)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    US.compare_special(enc, exp, US.FFFD_SPECIALS, [US.A, US.B, US.C], docs, "pageable buffers", call=lambda f, o, i: a)
    for side in US.SIDES:
        t0 = enc.encode_batch_trim_utf16(flat, offs, allowed, side, 20)
        t1 = enc.encode_batch_trim_utf16(flat, offs, allowed, side, 20)
        assert all(np.array_equal(x, y) for x, y in zip(t0, t1))
    # the same call on page-locked buffers (tkz_host_alloc): units, offsets, ids, output offsets
    sizes = [flat.nbytes + 64, offs.nbytes, 4 * 3 * len(flat), 8 * (n + 1)]
    ptrs = []
    try:
        for nb in sizes:
            p = C.c_void_p()
            lib.check(lib.L.tkz_host_alloc(nb, C.byref(p)))
            ptrs.append(p)
        view = lambda p, nb, dt: np.frombuffer((C.c_char * nb).from_address(p.value), dtype=dt)
        hu, ho, hi, hoo = (view(p, nb - nb % 8, dt) for p, nb, dt in zip(ptrs, sizes, (np.uint16, np.int64, np.int32, np.int64)))
        hu[:len(flat)] = flat
        ho[:] = offs
        needed = C.c_int64(0)
        idx = np.asarray(allowed, np.int32)
        lib.check(lib.L.tkz_encode_batch_special_utf16(enc._h, ptrs[0], ptrs[1], n, idx.ctypes.data, len(idx), ptrs[2], 3 * len(flat), ptrs[3], C.byref(needed)))
        assert hi[:needed.value].tolist() == a[0].tolist() and hoo[:n + 1].tolist() == a[1].tolist()
    finally:
        for p in ptrs:
            lib.L.tkz_host_free(p)


def test_two_chunks_through_the_real_pipeline(setup, oracle_mod, vocab_bytes):
    """6.3 M code units -- 12 MiB of upload, the smallest size the planner cuts in two -- of well-formed text with <|endoftext|> between documents, through
    the real pipeline (no TKZ_HOST_CHUNK_BYTES); checked by the C oracle.  A U+FFFD literal is registered, so both chunks carry a bitmap."""
    specials = {US.A: 60001, SC.EOT: 50256}
    enc, exp = setup(2, specials)
    doc = N.corpus_doc_host(1, 77, 0, 60 << 10, 60 << 10).decode("utf-8")
    body = US.units(doc + SC.EOT + " x� tail ")
    reps = ((12 << 20) // 2 + len(body) - 1) // len(body)
    flat = np.tile(np.asarray(body, np.uint16), reps)
    offs = np.arange(reps + 1, dtype=np.int64) * len(body)
    assert flat.nbytes >= 12 << 20
    ids, ooff = enc.encode_batch_special_utf16(flat, offs, [0, 1])
    want = exp.encode(body, [US.A, SC.EOT])
    assert 60001 in want and 50256 in want
    assert ooff.tolist() == [len(want) * d for d in range(reps + 1)]
    assert np.array_equal(ids.reshape(reps, len(want)), np.tile(np.asarray(want, np.int32), (reps, 1)))


def test_cpp_mirror_utf16_methods(tmp_path, gpt2_tiktoken_bytes):
    """include/tkz_tokenizer.hpp: the std::u16string methods against the header's own host walk (tests/cpp/test_u16_special.cpp)."""
    libdir, libname = os.path.join(ROOT, "tokenizer_amd", "lib"), "tkz"
    (tmp_path / "gpt2.tiktoken").write_bytes(gpt2_tiktoken_bytes)
    exe = str(tmp_path / "test_u16_special")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_u16_special.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "gpt2.tiktoken")], capture_output=True, text=True)
    assert out.returncode == 0 and "cpp u16 special ok" in out.stdout, out.stdout + out.stderr
