"""`-m gpu`: EncodeTrimSuffix / EncodeTrimPrefix for a batch through libtkz.so -- tkz_encode_batch_trim_utf8 / _device against oracle.TrimOracle, exact.
The smallest shapes at which k_trim_cut, the scan of the kept lengths and k_trim_gather can still go wrong on the hardware: cuts across sub-tiles, a document
over more than 64 sub-tiles, thousands of documents beside one long one, a piece of more than 1024 bytes, a side stream with a maximum per document.
Every batch is at most about 256 KiB; the oracle is pure Python, so the long documents are cut at one or two maxima."""
import numpy as np
import pytest

import parity
import special_cases as SC
import trim_cases as TC
from tokenizer_amd import _native as N

pytestmark = pytest.mark.gpu

VOCAB_OF = {1: "gpt2", 2: "synth100k", 4: "synth200k"}


@pytest.fixture(scope="module")
def lib():
    return N.default_library()


@pytest.fixture(scope="module")
def setup(lib, vocab_bytes, oracle_mod):
    cache = {}

    def get(pattern):
        if pattern not in cache:
            name = VOCAB_OF[pattern]
            raw = vocab_bytes(name)
            sp = SC.SPECIAL_SETS[name]
            ov = oracle_mod.Vocab(raw)
            enc = N.Encoder(N.Vocab(raw, lib), pattern)
            enc.set_special_tokens(sp)
            cache[pattern] = (enc, sp, TC.Expect(oracle_mod, ov, pattern, sp))
        return cache[pattern]
    return get


def device_call(enc, side_stream=False, per_doc_on_device=True):
    """the device entry on torch buffers, as a trim_cases.compare() call; the results are read after the call has returned"""
    import torch

    def call(data, offs, index, side, mx, per_doc):
        n = len(offs) - 1
        d = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
        if len(data):
            d[:len(data)] = torch.from_numpy(np.array(data, dtype=np.uint8)).cuda()
        o = torch.from_numpy(np.array(offs, dtype=np.int64)).cuda()
        dm = torch.from_numpy(np.array(per_doc, dtype=np.int64)).cuda() if per_doc is not None else None
        cap = max(1, len(data))
        ids = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
        ooff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        cb = torch.empty(max(1, n), dtype=torch.int64, device="cuda")
        cu = torch.empty(max(1, n), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream() if side_stream else None
        got = enc.encode_batch_trim_device(d.data_ptr(), o.data_ptr(), n, len(data), index, side, mx, dm.data_ptr() if dm is not None else 0,
                                           ids.data_ptr(), cap, ooff.data_ptr(), cb.data_ptr(), cu.data_ptr(), stream=stream.cuda_stream if stream else 0)
        return ids[:got].cpu().numpy(), ooff.cpu().numpy(), cb[:n].cpu().numpy(), cu[:n].cpu().numpy()
    return call


def corpus_docs(kind, seed, n_docs, min_len, max_len):
    return [N.corpus_doc_host(kind, seed, d, min_len, max_len).decode("utf-8") for d in range(n_docs)]


def splice(docs, literal, every=10):
    """the literal into every tenth document: in front, in the middle (at a character boundary), at the end in turn"""
    out = list(docs)
    for k, d in enumerate(range(0, len(out), every)):
        t = out[d]
        at = (0, len(t) // 2, len(t))[k % 3]
        out[d] = t[:at] + literal + t[at:]
    return out


@pytest.mark.parametrize("side", TC.SIDES)
def test_sub_tile_and_chunk_boundaries(setup, side):
    enc, specials, exp = setup(1)
    words = "the quick brown fox it's 2024 tokens => x don't Hello 12345 (a+b) "
    text = lambda n: (words * (n // len(words) + 1))[:n]
    # the first document ends in the last byte but one of a sub-tile, the second starts in its last byte; cuts that lie sub-tiles behind the document's start;
    # one document over more than 64 sub-tiles (a chunk of the class queue), cut near its end and near its start
    docs = [text(1023), "z" + text(3000) + SC.EOT + text(500), text(70 * 1024), "", text(2500)]
    assert len(docs[0]) == 1023
    for mx in (5, 700):
        TC.compare(enc, exp, specials, [SC.EOT], docs, side, mx, "boundaries")
    per_doc = [3, 650, 15000, 4, 600]                                   # (the cut of document 2 lies ~60 sub-tiles behind its start)
    TC.compare(enc, exp, specials, [SC.EOT], docs, side, 0, "boundaries, a maximum per document", per_doc=np.asarray(per_doc, np.int64), call=device_call(enc))


@pytest.mark.parametrize("side", TC.SIDES)
def test_many_documents_beside_a_long_one(setup, side):
    """~5,000 documents of 1..40 bytes -- the scan of the kept lengths spans several workgroups -- and one of 100 KiB: the kept ids cross several output
    tiles, some inside the one long document, some over hundreds of short ones."""
    enc, specials, exp = setup(2)
    small = corpus_docs(1, 11, 5000, 1, 40)
    big = corpus_docs(1, 12, 1, 100 << 10, 100 << 10)
    docs = small[:2500] + big + small[2500:]
    assert sum(len(d.encode("utf-8")) for d in docs) <= 256 << 10
    TC.compare(enc, exp, specials, [], docs, side, 3, "skew, maximum 3")
    per_doc = np.full(len(docs), 4, np.int64)
    per_doc[2500] = 9000                                                # (the long document keeps 9,000 ids: more than four output tiles)
    per_doc[::7] = 0
    n = TC.compare(enc, exp, specials, [], docs, side, 0, "skew, a maximum per document", per_doc=per_doc, call=device_call(enc))
    assert n > 3 * 2048 + 9000


@pytest.mark.parametrize("side", TC.SIDES)
def test_giant_piece(setup, side):
    enc, specials, exp = setup(1)
    giant = "a" * 1500                                                  # one piece of more than 1024 bytes
    docs = ["head " + giant + " tail words", giant, "x", giant + SC.EOT]
    count = exp.count(giant, [])
    assert count > 3
    for mx in (count - 1, count + 1):
        TC.compare(enc, exp, specials, [SC.EOT], docs, side, mx, "giant piece")
    ids, ooff, cb, cu = enc.encode_batch_trim(*parity.pack([giant.encode()]), [], side, count - 1)
    # suffix: the piece does not fit, nothing is kept; prefix: the piece goes as a whole, nothing is left
    assert len(ids) == 0 and int(cb[0]) == (0 if side == N.TRIM_SUFFIX else 1500)


@pytest.mark.parametrize("with_literals", [0, 1])
@pytest.mark.parametrize("kind,pattern", [(1, 1), (2, 2), (2, 4), (1, 4)])
def test_text_kinds_and_patterns(setup, kind, pattern, with_literals):
    enc, specials, exp = setup(pattern)
    docs = corpus_docs(kind, 100 + pattern, 120, 0, 900)
    names = list(specials)
    allowed = names if with_literals else []
    if with_literals:
        docs = splice(docs, names[-1])
    mean = sum(exp.count(d, allowed) for d in docs) // len(docs)
    for side in TC.SIDES:
        TC.compare(enc, exp, specials, allowed, docs, side, max(1, mean // 2), "kind %d pattern %d" % (kind, pattern))
        TC.compare(enc, exp, specials, allowed, docs, side, mean, "kind %d pattern %d (device entry)" % (kind, pattern), call=device_call(enc))


def test_determinism_and_the_plain_entry(setup):
    enc, specials, exp = setup(2)
    docs = splice(corpus_docs(2, 5, 300, 0, 600), list(specials)[0])
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    plain0 = enc.encode_batch(data, offs)
    for side in TC.SIDES:
        a = enc.encode_batch_trim(data, offs, [0], side, 20)
        b = enc.encode_batch_trim(data, offs, [0], side, 20)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    plain1 = enc.encode_batch(data, offs)
    assert np.array_equal(plain0[0], plain1[0]) and np.array_equal(plain0[1], plain1[1])
    # the plain entry launches what it launched: the same kernel launch counts per bracket before and after trim calls
    enc.set_profiling(True)
    try:
        enc.kernel_ms(reset=True)
        enc.encode_batch(data, offs)
        launches0 = enc.kernel_ms(reset=True)
        enc.encode_batch_trim(data, offs, [0], N.TRIM_SUFFIX, 20)
        enc.kernel_ms(reset=True)
        enc.encode_batch(data, offs)
        launches1 = enc.kernel_ms(reset=True)
    finally:
        enc.set_profiling(False)
    count = lambda r: [n for _, n in r.values()]
    assert count(launches0) == count(launches1)


@pytest.mark.parametrize("side", TC.SIDES)
def test_device_entry_on_a_side_stream(setup, side):
    enc, specials, exp = setup(1)
    docs = splice(corpus_docs(1, 21, 400, 0, 500), SC.EOT)
    rng = np.random.RandomState(3)
    per_doc = rng.choice([0, 1, 5, 40, 1 << 50, -2], size=len(docs)).astype(np.int64)       # (a negative entry in a device array counts as 0)
    TC.compare(enc, exp, specials, [SC.EOT], docs, side, 0, "side stream", per_doc=per_doc, call=device_call(enc, side_stream=True))


def test_cpp_mirror_batch_methods(tmp_path, gpt2_tiktoken_bytes):
    """include/tkz_tokenizer.hpp: EncodeTrimSuffixBatch / EncodeTrimPrefixBatch against the header's own host walk (tests/cpp/test_trim_batch.cpp)."""
    import os
    import subprocess
    from conftest import ROOT
    libdir, libname = os.path.join(ROOT, "tokenizer_amd", "lib"), "tkz"
    (tmp_path / "gpt2.tiktoken").write_bytes(gpt2_tiktoken_bytes)
    exe = str(tmp_path / "test_trim_batch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_trim_batch.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe, str(tmp_path / "gpt2.tiktoken")], capture_output=True, text=True)
    assert out.returncode == 0 and "cpp trim batch ok" in out.stdout, out.stdout + out.stderr
