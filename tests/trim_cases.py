"""EncodeTrimSuffix / EncodeTrimPrefix for a batch on the device (tkz_encode_batch_trim_utf8 / _device): the expected values and the comparison the
emulated (CPU) and the GPU test modules share.  Every comparison is exact -- kept ids, offsets, cut_bytes, cut_units -- against oracle.TrimOracle's
restatement of TikTokenizer.cs:288-579, text by text."""
import numpy as np

import parity
import special_cases as SC
from tokenizer_amd import _native as N

SIDES = (N.TRIM_SUFFIX, N.TRIM_PREFIX)
IM_START, IM_END = "<|im_start|>", "<|im_end|>"
# the texts of the reference's unit tests (TikTokenizerUnitTest.cs:128-225) and around them
REFERENCE_TEXTS = [IM_START + "Hello World" + IM_END, IM_START + "Hello TempWorld" + IM_END, IM_START + "HelloTemp World" + IM_END,
                   "Hello ⭐ World 😀😀 done" + IM_END + " tail", " 😀", "a 😀 b", "x" + " 😀" * 3]


def utf16_len(s):
    return len(s.encode("utf-16-le", "surrogatepass")) // 2


class Expect:
    """TrimOracle per text, remembered: (kept ids, cut_bytes, cut_units) for (text, allowed, side, max), and the untrimmed token count of (text, allowed)."""

    def __init__(self, O, ovocab, pattern, specials):
        self.oracle = O.TrimOracle(ovocab, pattern, specials)
        self.enc = O.Encoder(ovocab, pattern, specials=specials)
        self._trim, self._count = {}, {}

    def count(self, text, allowed):
        key = (text, tuple(allowed))
        if key not in self._count:
            self._count[key] = len(self.enc.encode(text, list(allowed)))
        return self._count[key]

    def trim(self, text, allowed, side, mx):
        key = (text, tuple(allowed), side, mx)
        if key not in self._trim:
            if side == N.TRIM_SUFFIX:
                ids, kept = self.oracle.encode_trim_suffix(text, list(allowed) or None, mx)
                part = kept                                   # the kept text
            else:
                ids, kept = self.oracle.encode_trim_prefix(text, list(allowed) or None, mx)
                n = utf16_len(text) - utf16_len(kept)         # the dropped text is what is in front of the kept one
                part = text.encode("utf-16-le", "surrogatepass")[:2 * n].decode("utf-16-le", "surrogatepass")
            self._trim[key] = ([int(i) for i in ids], len(part.encode("utf-8")), utf16_len(part))
        return self._trim[key]


def expected(exp, docs, allowed, side, maxima):
    ids, offs, cb, cu = [], [0], [], []
    for d, mx in zip(docs, maxima):
        i, b, u = exp.trim(d, allowed, side, mx)
        ids += i
        offs.append(len(ids))
        cb.append(b)
        cu.append(u)
    return ids, offs, cb, cu


def compare(enc, exp, specials, allowed, docs, side, mx, what="", per_doc=None, call=None):
    """docs: str documents.  mx: the uniform maximum, or -- per_doc -- ignored in favour of one maximum per document.
    call(data, offs, index, side, mx, per_doc) -> (ids, offsets, cut_bytes, cut_units): the entry under test (default: the host entry)."""
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    index = SC.indices(specials, allowed)
    got = (call or enc.encode_batch_trim)(data, offs, index, side, mx, per_doc)
    maxima = [max(int(m), 0) for m in per_doc] if per_doc is not None else [mx] * len(docs)
    want = expected(exp, docs, allowed, side, maxima)
    for name, g, w in zip(("offsets", "cut_bytes", "cut_units", "ids"), (got[1], got[2], got[3], got[0]), (want[1], want[2], want[3], want[0])):
        g = [int(x) for x in g]
        if g != w:
            k = SC.first_diff(g, w)
            raise AssertionError("%s side %d max %s: %s differ at %d: got %s, expected %s" % (what, side, mx if per_doc is None else "per document", name, k, g[max(0, k - 2):k + 6], w[max(0, k - 2):k + 6]))
    return len(want[0])


def sweep(enc, exp, specials, allowed, docs, side, what=""):
    """Every maximum from 0 to one past the longest document's token count, the whole batch at each (a document that is shorter is kept whole)."""
    top = max([exp.count(d, allowed) for d in docs] + [0]) + 1
    for mx in range(top + 1):
        compare(enc, exp, specials, allowed, docs, side, mx, what)
    return top


# ---- batches beyond what the oracle can walk document by document: a small pool of distinct documents, repeated and shuffled (tests/test_gpu_trim_scale.py,
# tests/test_emu_trim_scale.py).  Expect caches by text, so the oracle's work is bounded by the pool; every document of the batch still has an exact
# expectation, and the repetitions land on every row, sub-tile and tile alignment. ----

# The kernels' constants the scale tests place their batches by, mirrored here and nowhere else: a test asserts that its batch lies on the side of each
# constant it means to cover, so a later change of one of them makes the test fail rather than quietly stop covering the regime.
K_THREADS = 256                                     # tkz_kernels.h:11      kThreads
K_SUB = 1024                                        # tkz_kernels.h:12      kSub: bytes of text per sub-tile
K_SCAN_BLOCK = 1024                                 # tkz_kernels.h:34      kScanBlock: entries per workgroup of a scan
K_SCAN_SMALL_MAX = 8192                             # tkz_kernels.hip:2387  kScanSmallMax: launch_scan2 takes k_scan_small up to this many sub-tiles
K_SCAN_TOP_STEP = K_THREADS * K_SCAN_BLOCK          # tkz_kernels.hip:2425  k_scan_top: kThreads block sums a step -- it carries beyond 262,144 entries
K_TRIM_TILE, K_TRIM_BYTE_TILE = 2048, 4096          # tkz_kernels.hip:2980  kTrimTile, kTrimByteTile
K_TRIM_GATHER_WAVES = 2048 * (K_THREADS // 64)      # tkz_kernels.hip:3643  launch_trim: k_trim_gather's grid is capped at 2,048 workgroups of 4 wavefronts
LATENCY_BYTES = 16 << 20                            # tkz_api.cpp:247       TKZ_OPT_LATENCY_BYTES as an encoder starts: larger batches take the throughput forms
HUGE = 1 << 40                                      # a maximum above any document's token count


def sub_tiles(total):
    return (total + K_SUB - 1) // K_SUB


def gather_segments(table, starts, lens, keys):
    """table[starts[k] : starts[k] + lens[k]] for every k of keys, concatenated, and the segments' offsets -- by index arithmetic, no loop over keys"""
    n = lens[keys]
    offs = np.zeros(len(keys) + 1, np.int64)
    np.cumsum(n, out=offs[1:])
    pos = np.repeat(starts[keys] - offs[:-1], n) + np.arange(int(offs[-1]), dtype=np.int64)
    return table[pos], offs


def _tables(arrays, dtype):
    lens = np.asarray([len(a) for a in arrays], np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(arrays) else np.zeros(0, np.int64)
    table = np.concatenate([np.asarray(a, dtype) for a in arrays]) if len(arrays) and lens.sum() else np.zeros(0, dtype)
    return table, starts, lens


class Pool:
    """the distinct documents of a batch: str, their bytes, their UTF-16 units"""

    def __init__(self, docs):
        self.docs = list(docs)
        self.raw = [d.encode("utf-8") for d in self.docs]
        self.bytes, self.starts, self.lens = _tables([np.frombuffer(r, np.uint8) for r in self.raw], np.uint8)
        self._pieces = {}

    def __len__(self):
        return len(self.docs)

    def units(self):
        """(table, starts, lens) of the documents' UTF-16 code units"""
        return _tables([np.frombuffer(d.encode("utf-16-le"), np.uint16) for d in self.docs], np.uint16)

    def pieces(self, O, ovocab, pattern):
        """the oracle's pieces of every pool document, once: O.split_utf8, then the whole-piece rank or else bpe (as parity.check_piece_granular has it)"""
        key = (id(ovocab), pattern)
        if key not in self._pieces:
            rel, ntok, ids = [], [], []
            for r in self.raw:
                a_, n_, i_ = [], [], []
                for (a, n) in O.split_utf8(pattern, r):
                    p = r[a:a + n]
                    rank = ovocab.rank(p)
                    t = [rank] if rank >= 0 else ovocab.bpe(p)
                    a_.append(a)
                    n_.append(len(t))
                    i_ += t
                rel.append(a_)
                ntok.append(n_)
                ids.append(i_)
            self._pieces[key] = (_tables(rel, np.int64), _tables(ntok, np.int64), _tables(ids, np.int32))
        return self._pieces[key]


def build_batch(pool, seed, maxima, total_bytes=None, n_docs=None):
    """A batch of pool documents drawn at random (seeded): n_docs of them, or as many as give EXACTLY total_bytes (the tail is filled with the longest
    documents that still fit, one-byte documents last).  maxima: at most six distinct values; every document draws one.
    Returns (pool indices, packed bytes, offsets, the maximum of every document)."""
    assert len(set(maxima)) <= 6 and (n_docs is None) != (total_bytes is None)
    rng = np.random.RandomState(seed)
    if n_docs is not None:
        idx = rng.randint(0, len(pool), n_docs).astype(np.int64)
    else:
        draw = rng.randint(0, len(pool), int(total_bytes / max(1.0, pool.lens.mean()) * 1.3) + 64).astype(np.int64)
        cs = np.cumsum(pool.lens[draw])
        assert cs[-1] >= total_bytes
        k = int(np.searchsorted(cs, total_bytes, side="right"))
        rest = total_bytes - (int(cs[k - 1]) if k else 0)
        by_len = sorted((int(n), d) for d, n in enumerate(pool.lens) if n > 0)
        assert by_len[0][0] == 1, "the pool needs a one-byte document to hit a byte count exactly"
        tail = []
        while rest > 0:
            n, d = max(e for e in by_len if e[0] <= rest)
            tail.append(d)
            rest -= n
        idx = np.concatenate([draw[:k], np.asarray(tail, np.int64)])
    data, offs = gather_segments(pool.bytes, pool.starts, pool.lens, idx)
    assert total_bytes is None or len(data) == total_bytes
    per_doc = np.asarray(list(maxima), np.int64)[rng.randint(0, len(maxima), len(idx))]
    return idx, data, offs, per_doc


def expected_from_pool(exp, pool, idx, allowed, side, per_doc):
    """(ids, offsets, cut_bytes, cut_units) of the whole batch: the oracle once per (pool document, maximum) that occurs, then numpy -- the cached arrays
    concatenated by index, the cumulative sum of their lengths.  A negative maximum counts as 0 (the device entry's rule)."""
    values, which = np.unique(np.maximum(np.asarray(per_doc, np.int64), 0), return_inverse=True)
    assert len(values) <= 6
    keys = np.asarray(idx, np.int64) * len(values) + which
    nk = len(pool) * len(values)
    chunks = [[] for _ in range(nk)]
    cb, cu = np.zeros(nk, np.int64), np.zeros(nk, np.int64)
    for k in np.unique(keys).tolist():
        d, v = divmod(k, len(values))
        chunks[k], cb[k], cu[k] = exp.trim(pool.docs[d], allowed, side, int(values[v]))
    table, starts, lens = _tables(chunks, np.int32)
    ids, offs = gather_segments(table, starts, lens, keys)
    return ids, offs, cb[keys], cu[keys]


def expected_pieces_from_pool(O, ovocab, pattern, pool, idx, offs):
    """(ids, doc_piece, piece_boffs, piece_toffs) of the piece-granular entry for the whole batch: the pool's pieces, byte and token offsets shifted per occurrence"""
    (rel, pstarts, npieces), (ntok, _, _), (ids, istarts, nids) = pool.pieces(O, ovocab, pattern)
    idx = np.asarray(idx, np.int64)
    rel_b, doc_piece = gather_segments(rel, pstarts, npieces, idx)
    pbo = np.concatenate([rel_b + np.repeat(np.asarray(offs[:-1], np.int64), npieces[idx]), [int(offs[-1])]])
    tok_b, _ = gather_segments(ntok, pstarts, npieces, idx)
    pto = np.zeros(len(tok_b) + 1, np.int64)
    np.cumsum(tok_b, out=pto[1:])
    all_ids, _ = gather_segments(ids, istarts, nids, idx)
    return all_ids, doc_piece, pbo, pto


def crosscheck_plain(O, ovocab, pattern, data, offs, ids, tok_offs):
    """the plain ids of the same buffers at full size, every document, by the oracle in C on all cores (as test_device_corpus_properties_and_sample has it)"""
    import os
    bad, first_bad, otok = O.check_batch(ovocab, pattern, data, offs, ids, tok_offs, threads=max(1, min(64, os.cpu_count() or 1)))
    assert (bad, first_bad, otok) == (0, -1, len(ids)), "%d of %d documents differ from the oracle, first %d" % (bad, len(offs) - 1, first_bad)


def assert_same(what, got, want, offs=None, want_offs=None):
    """got / want: dicts name -> array.  The first differing entry, its document and where that document lies among the sub-tiles."""
    for name, w in want.items():
        g, w = np.asarray(got[name]), np.asarray(w)
        if g.shape == w.shape and np.array_equal(g, w):
            continue
        n = min(len(g), len(w))
        bad = np.nonzero(g[:n] != w[:n])[0]
        k = int(bad[0]) if len(bad) else n
        where = ""
        if offs is not None:
            d = k if name in ("cut_bytes", "cut_units", "offsets", "doc_piece") else int(np.searchsorted(want_offs, k, side="right")) - 1 if name == "ids" and want_offs is not None else None
            if d is not None and 0 <= d < len(offs) - 1:
                where = "; document %d, bytes [%d, %d), sub-tile %d + %d" % (d, offs[d], offs[d + 1], offs[d] // K_SUB, offs[d] % K_SUB)
        raise AssertionError("%s: %s differ at %d of %d / %d: got %s, expected %s%s" % (what, name, k, len(g), len(w), g[max(0, k - 2):k + 6].tolist(), w[max(0, k - 2):k + 6].tolist(), where))


class HostMemory:
    """the emulated build: "device" memory is the host's"""

    def up(self, arr):
        a = np.array(arr, copy=True, order="C")
        return a, a.ctypes.data

    def down(self, owner):
        return owner


class TorchMemory:
    def up(self, arr):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        return t, t.data_ptr()

    def down(self, owner):
        return owner.cpu().numpy()


SENTINEL_ID, SENTINEL_64 = -7, -0x5A5A5A5A5A5A5A5B
PAD = 16


def device_trim(enc, mem, data, offs, index, side, per_doc, out_cap=None, max_tokens=0):
    """tkz_encode_batch_trim_device on buffers of `mem`.  Every output buffer is pre-filled with a sentinel and PAD entries longer than the call may write.
    Returns dict(got=the kept total returned, ids, offsets, cut_bytes, cut_units -- what the call wrote --, and untouched=whether everything behind that
    is still the sentinel)."""
    n, total = len(offs) - 1, len(data)
    padded = np.zeros(total + 64, np.uint8)
    padded[:total] = data
    (d_keep, d_ptr), (o_keep, o_ptr) = mem.up(padded), mem.up(np.asarray(offs, np.int64))
    m_keep, m_ptr = mem.up(np.asarray(per_doc, np.int64)) if per_doc is not None else (None, 0)
    cap = max(1, total) if out_cap is None else out_cap
    ids, ids_ptr = mem.up(np.full(max(1, cap) + PAD, SENTINEL_ID, np.int32))
    ooff, ooff_ptr = mem.up(np.full(n + 1 + PAD, SENTINEL_64, np.int64))
    cb, cb_ptr = mem.up(np.full(n + PAD, SENTINEL_64, np.int64))
    cu, cu_ptr = mem.up(np.full(n + PAD, SENTINEL_64, np.int64))
    try:
        got = enc.encode_batch_trim_device(d_ptr, o_ptr, n, total, index, side, max_tokens, m_ptr, ids_ptr, cap, ooff_ptr, cb_ptr, cu_ptr)
        failed = None
    except N.TkzError as ex:
        got, failed = ex.needed, ex
    ids, ooff, cb, cu = mem.down(ids), mem.down(ooff), mem.down(cb), mem.down(cu)
    wrote = 0 if failed else got
    untouched = bool((ids[wrote:] == SENTINEL_ID).all() and (ooff[n + 1:] == SENTINEL_64).all() and (cb[n:] == SENTINEL_64).all() and (cu[n:] == SENTINEL_64).all())
    del d_keep, o_keep, m_keep
    return dict(got=got, failed=failed, ids=ids[:wrote], offsets=ooff[:n + 1], cut_bytes=cb[:n], cut_units=cu[:n], untouched=untouched)


# ---- the pools ----

def _gib(rng, n, lo, hi, cons="bcdfghjklmnpqrstvwxz"):
    out = []
    while sum(map(len, out)) < n:
        out.append(" " + "".join(rng.choice(cons) for _ in range(rng.randint(lo, hi))))
    return "".join(out)[:n]


WORDS = "the quick brown fox it's 2024 tokens => x don't Hello 12345 (a+b) "
CJK = "漢字かな交じり文、한국어 텍스트 😀👍🏽 naïve café １２３４５ "


def prose(n):
    return (WORDS * (n // len(WORDS) + 1))[:n]


def scale_pool(literal, corpus_doc=None):
    """The pool of the scan-form and the retry cases: empty and one-byte documents, documents that end one byte before, on and one byte behind a sub-tile
    edge, CJK and emoji (cut_units != cut_bytes), the literal alone / in front / in the middle / at the end, one piece of 1,500 bytes, crowded text
    (parity.check_miss_lists' gib(n, 2, 2)), dense one-byte pieces; corpus_doc(kind, d, lo, hi) -> bytes adds generated documents of kinds 1 and 2."""
    import random
    rng = random.Random(77)
    docs = ["", "", "a", "\n", prose(K_SUB - 1), prose(K_SUB), prose(K_SUB + 1), prose(37), prose(700), prose(3 * K_SUB + 5),
            CJK * 3, CJK * 14, "😀" * 40 + " a 😀 b", "x" + " 😀" * 3,
            literal, literal + prose(300), prose(200) + literal + prose(150), prose(400) + literal, "中文" + literal + literal + "中文 " + prose(90),
            "a" * 1500, "head " + "b" * 1500 + " tail words",
            _gib(rng, 2500, 2, 2), _gib(rng, 1100, 2, 2), _gib(rng, 600, 2, 3) + prose(500),
            "a\nb\nc\nd\n" * 300, "".join(rng.choice("bcdfgh") + "\n" for _ in range(700)), "é\nü\n" * 100]
    if corpus_doc is not None:
        docs += [corpus_doc(kind, d, lo, hi).decode("utf-8") for kind in (1, 2) for d, (lo, hi) in enumerate([(40, 200), (900, 1100), (2000, 3000)])]
    assert len(docs) <= 48 and sum(len(d.encode("utf-8")) for d in docs) <= 200_000
    return Pool(docs)


SCALE_MAXIMA = (0, 1, 7, 60, 400, HUGE)


def tiny_pool():
    """documents of 0..3 bytes: a batch of 262,144 of them stays below 2 MiB"""
    docs = ["", "a", "\n", " b", "qz", "é", "c d", "x\n\n", "中", " é", "12", "a b"]
    assert all(len(d.encode("utf-8")) <= 3 for d in docs)
    return Pool(docs)


TINY_MAXIMA = (0, -2, 1, 2, HUGE, -(1 << 40))            # (a negative entry counts as 0 on the device entry)


def dense_pool():
    """dense one-byte pieces -- a token per byte, nearly --, some of the characters of two, three and four bytes: the units differ from the bytes"""
    import random
    rng = random.Random(78)
    line = lambda n, alpha: "".join(rng.choice(alpha) + "\n" for _ in range(n))
    docs = ["a", line(2048, "abcdefgh"), line(1500, "abcdefghxyz"), line(511, "abc") + "z", line(1200, "abcdefgé"), line(900, "abc中"), line(700, "ab😀"), "a\nb\nc\nd\n" * 700]
    return Pool(docs)


DENSE_MAXIMA = (HUGE, HUGE - 1, HUGE - 2, 1000, 100, 0)    # (most documents kept whole, some cut)


def mixed_pool(corpus_doc, literal):
    """kinds 1 and 2 of the corpus generator, the literal in some of them"""
    docs = [corpus_doc(kind, d, lo, hi).decode("utf-8") for kind in (1, 2) for d, (lo, hi) in enumerate([(0, 60), (100, 400), (900, 1200), (1500, 2500), (3000, 5000), (200, 2000)] * 3)]
    docs = [d if k % 5 else (literal + d, d[:len(d) // 2] + literal + d[len(d) // 2:], d + literal)[k // 5 % 3] for k, d in enumerate(docs)] + ["", "a"]
    return Pool(docs)


MIXED_MAXIMA = (0, 3, 50, 300, HUGE)


def side_by_side_pool():
    """parity.check_side_by_side's documents: short, 17..128-byte, 129..1,024-byte and giant missed pieces"""
    import random
    import regex_crosscheck as RC
    alpha = RC.alphabet()
    rng = random.Random(71)
    cons = "bcdfghjklmnpqrstvwxz"
    docs = ["", "a"]
    for _ in range(22):
        parts = []
        for _ in range(rng.randint(1, 12)):
            r = rng.random()
            if r < 0.4: parts.append(parity.gen_text(rng, "mix", rng.choice([5, 80, 700]), alpha))
            elif r < 0.7: parts.append(" " + "".join(rng.choice(cons) for _ in range(rng.choice([3, 9, 17, 30, 64, 100, 128]))))
            elif r < 0.9: parts.append(" " + "".join(rng.choice(cons) for _ in range(rng.choice([129, 300, 1024]))))
            else: parts.append(" " + "".join(rng.choice("ab") for _ in range(rng.choice([1025, 2500]))))
        docs.append("".join(parts))
    return Pool(docs)


SIDE_MAXIMA = (0, 2, 30, 200, HUGE)


# ---- the comparisons at scale and the cases the emulated and the GPU module share ----

def compare_pieces_pooled(enc, O, ovocab, pattern, pool, idx, data, offs, what, crosscheck=True):
    """tkz_encode_batch_pieces_utf8 against the pooled piece expectation, exact: doc_piece, piece_boffs, piece_toffs, ids.  Returns the piece count."""
    ids, dpo, pbo, pto = enc.encode_batch_pieces(data, offs)
    w_ids, w_dpo, w_pbo, w_pto = expected_pieces_from_pool(O, ovocab, pattern, pool, idx, offs)
    assert_same(what + ", pieces", dict(doc_piece=dpo, piece_boffs=pbo, piece_toffs=pto, ids=ids), dict(doc_piece=w_dpo, piece_boffs=w_pbo, piece_toffs=w_pto, ids=w_ids),
                offs, want_offs=w_pto[w_dpo])
    if crosscheck:
        crosscheck_plain(O, ovocab, pattern, data, offs, ids, pto[dpo])
    return len(w_pbo) - 1


def compare_trim_pooled(enc, exp, specials, pool, idx, data, offs, per_doc, allowed, side, what, mem=None):
    """the trim entry against the pooled expectation, exact: ids, offsets, cut_bytes, cut_units; the last offset is the kept total returned.
    mem: the device entry on buffers of that kind (per_doc may hold negative entries there); None: the host entry.  Returns the kept total."""
    index = SC.indices(specials, allowed)
    w_ids, w_offs, w_cb, w_cu = expected_from_pool(exp, pool, idx, allowed, side, per_doc)
    what = "%s, side %d, allowed %s" % (what, side, allowed)
    if mem is None:
        ids, ooff, cb, cu = enc.encode_batch_trim(data, offs, index, side, 0, per_doc)
        got = dict(got=len(ids), ids=ids, offsets=ooff, cut_bytes=cb, cut_units=cu, untouched=True)
    else:
        got = device_trim(enc, mem, data, offs, index, side, per_doc)
        assert got["failed"] is None, got["failed"]
    assert_same(what, got, dict(offsets=w_offs, cut_bytes=w_cb, cut_units=w_cu, ids=w_ids), offs, want_offs=w_offs)
    assert got["got"] == int(got["offsets"][-1]) == len(w_ids), (what, got["got"], int(got["offsets"][-1]), len(w_ids))
    assert got["untouched"], what + ": the call wrote behind what it returned"
    return got["got"]


def check_side_by_side_under_piece_marks(new_encoder, exp, O, ovocab, pattern, specials, mem, rounds=4):
    """TKZ_OPT_LATENCY_BYTES 0: every batch of an encoder after its first runs the three merge stages side by side, the sub-tiles' token counts summed with
    atomics (P.tc_atomic) -- here with a mark on every PIECE, so every piece's token position depends on those sums.  parity.check_side_by_side's documents,
    pooled; several batches on one encoder through the piece entry, then through the trim entry; the encoder must report the form for all but the first."""
    pool = side_by_side_pool()
    enc = new_encoder()
    enc.set_option(N.OPT_LATENCY_BYTES, 0)
    literal = list(specials)[0]
    before = enc.side_by_side_batches
    for it in range(rounds):
        idx, data, offs, _ = build_batch(pool, 100 + it, SIDE_MAXIMA, n_docs=(30, 60, 3, 40)[it % 4])
        compare_pieces_pooled(enc, O, ovocab, pattern, pool, idx, data, offs, "side by side, round %d" % it)
    assert enc.side_by_side_batches - before >= rounds - 1, (before, enc.side_by_side_batches, rounds)
    enc = new_encoder()
    enc.set_option(N.OPT_LATENCY_BYTES, 0)
    before, calls = enc.side_by_side_batches, 0
    for it in range(rounds):
        idx, data, offs, per_doc = build_batch(pool, 200 + it, SIDE_MAXIMA, n_docs=(40, 3, 60, 30)[it % 4])
        for side in SIDES:
            compare_trim_pooled(enc, exp, specials, pool, idx, data, offs, per_doc, [literal] if it % 2 else [], side, "side by side, round %d" % it, mem=mem)
            calls += 1
    assert enc.side_by_side_batches - before >= calls - 1, (before, enc.side_by_side_batches, calls)


def attempts_of(err):
    import re
    got = [int(m) for m in re.findall(r"(\d+) attempt", err)]
    assert got, err
    return got[-1]


def retry_scenarios():
    """(name, a first batch the fresh encoder sees or None, the pool, attempts of the call under test): what makes the launch sequence run again.
      crowded   a sub-tile misses more pieces than a fresh list's 64 entries (parity.check_miss_lists' gib(n, 2, 2)): overflow, again
      giant     the pool of the giant pieces is sized by a workspace's FIRST batch (24 bytes per byte of it); a later batch whose giant pieces need more
                overflows it: grown, again
      records   a piece per byte: more records than a fresh buffer's one per three bytes: sized exactly, again"""
    import random
    rng = random.Random(41)
    crowded = Pool([_gib(rng, 5000, 2, 2), prose(700), "", _gib(rng, 1500, 2, 2) + CJK, "a"])
    giant = Pool(["head " + "a" * 1500 + " tail", "b" * 3000, "x", "", "qz" * 900 + CJK])
    records = Pool(["a\nb\nc\nd\n" * 2500, "", "é\n" * 300, "x"])
    return [("crowded", None, crowded, 2), ("giant", prose(300), giant, 2), ("records", None, records, 2)]


# The attempts of the three corpora of parity.check_sizing_attempt through the PIECE sequence.  The sizing sample is a plain call's alone -- encode_device
# (tkz_api.cpp): `nsample = attempt == 0 && ... && c.plain_encode() ? sizing_sample(ntiles) : -1`, and a Pieces / Trim call is no plain_encode() -- so the
# first attempt of a piece or trim call is a whole one:
#   crowded everywhere   plain: sample (sizes the lists), whole = 2     pieces: whole (overflows), again = 2
#   crowded tail         plain: sample, whole (overflows), again = 3    pieces: whole (overflows), again = 2
#   ordinary text        plain: sample, whole = 2                       pieces: whole = 1
SIZING_ATTEMPTS_PIECES = (2, 2, 1)
RETRY_MAXIMA = (0, 5, 90, HUGE)


def check_retries_with_pieces(new_encoder, exp, O, ovocab, pattern, specials, mem, capfd, monkeypatch):
    """Every reason for which the launch sequence runs again, with c.pieces set: enqueue_attempt waits for n_pieces, sizes p_boffs / p_toffs, runs
    k_piece_index again on the bitmaps the failed attempt left, and k_trim_cut / k_trim_gather of the failed attempt leave the caller's buffers alone.  Fresh
    encoders, the piece entry and the trim device entry on both sides: the results exact, the attempts off the TKZ_LOG_SLOW_MS line (first call and the call
    after it, which takes one), nothing written behind the kept ids, and -- one id short of the kept total -- the capacity status with the kept total."""
    monkeypatch.setenv("TKZ_SIZING_MIN_SUB", "128")
    monkeypatch.setenv("TKZ_LOG_SLOW_MS", "0")
    literal = list(specials)[0]
    cases = [(name, first, pool, np.arange(len(pool), dtype=np.int64), attempts) for name, first, pool, attempts in retry_scenarios()]
    for (docs, plain_attempts), attempts in zip(parity.sizing_corpora(), SIZING_ATTEMPTS_PIECES):
        assert attempts <= plain_attempts
        cases.append(("sizing corpus, %d attempts as a plain call" % plain_attempts, None, Pool([d.decode("utf-8") for d in docs]), None, attempts))

    def fresh(first):
        enc = new_encoder()
        if first is not None:
            enc.encode_batch_pieces(*parity.pack([first.encode("utf-8")]))
        capfd.readouterr()
        return enc
    for name, first, pool, idx, attempts in cases:
        if idx is None:
            idx = np.arange(len(pool), dtype=np.int64)
        else:
            idx = np.concatenate([idx, idx[::-1], idx])
        rng = np.random.RandomState(len(name))
        per_doc = np.asarray(RETRY_MAXIMA, np.int64)[rng.randint(0, len(RETRY_MAXIMA), len(idx))]
        data, offs = gather_segments(pool.bytes, pool.starts, pool.lens, idx)
        enc = fresh(first)
        for want in (attempts, 1):
            compare_pieces_pooled(enc, O, ovocab, pattern, pool, idx, data, offs, name)
            assert attempts_of(capfd.readouterr().err) == want, (name, "pieces", want)
        for side in SIDES:
            allowed = [literal] if side == SIDES[0] else []
            enc = fresh(first)
            for want in (attempts, 1):
                kept = compare_trim_pooled(enc, exp, specials, pool, idx, data, offs, per_doc, allowed, side, name, mem=mem)
                assert attempts_of(capfd.readouterr().err) == want, (name, "trim", side, want)
            # one id short, on a fresh encoder: the attempt that fails leaves the ids alone, the one that succeeds has no room for them
            assert kept > 0
            enc = fresh(first)
            got = device_trim(enc, mem, data, offs, SC.indices(specials, allowed), side, per_doc, out_cap=kept - 1)
            assert attempts_of(capfd.readouterr().err) == attempts, (name, "trim, one id short", side)
            assert got["failed"] is not None and got["failed"].code == N.E_CAPACITY and got["got"] == kept, (name, side, got["failed"], got["got"], kept)
            assert got["untouched"], (name, side, "ids written by a call that failed")
