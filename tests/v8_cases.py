"""The split as V8 cuts it -- the engine the TypeScript reference compiles its patterns with (`new RegExp(pattern, "gu")`) -- shared by the oracle,
the emulated and the GPU test modules.  The fixtures are written by tests/golden/make_v8_fixtures.py on a machine that has Node; which text is a
legitimate expectation for which pattern is decided THERE (its docstring has the rules) -- nothing here filters a record, and nothing here starts
`node` or reads the reference.

A record is {pattern, table, kind, text, starts}: `starts` are the UTF-8 byte offsets of V8's pieces; `table` is "builtin" (the record holds under the
library's own Unicode 13.0 class table) or "v8" (it holds once V8's table, v8_unicode_classes.bin.gz, has been handed over with
tkz_encoder_set_unicode_classes -- every code point for o200k, the first 65,536 entries for the patterns .NET reads by code unit)."""
import gzip
import json
import os

import numpy as np

import parity
from tokenizer_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATTERNS = (1, 2, 3)
TABLES = ("builtin", "v8")
BATCH_SIZES = (1, 3, 20)
_cache = {}


def fixture():
    if "fx" not in _cache:
        with open(os.path.join(GOLDEN, "splits_v8.json.gz"), "rb") as f:
            _cache["fx"] = json.loads(gzip.decompress(f.read()).decode("utf-8"))
    return _cache["fx"]


def versions():
    with open(os.path.join(GOLDEN, "v8_versions.json")) as f:
        return json.load(f)


def v8_table():
    """uint8[0x110000]: V8's class of every code point (read-only)."""
    if "tab" not in _cache:
        with open(os.path.join(GOLDEN, "v8_unicode_classes.bin.gz"), "rb") as f:
            t = np.frombuffer(gzip.decompress(f.read()), np.uint8)
        assert len(t) == 0x110000
        _cache["tab"] = t
    return _cache["tab"]


def table_for(pattern):
    """What a host on V8 hands the encoder of that pattern."""
    return v8_table() if pattern == N.O200K else v8_table()[:65536]


def records(pattern, table):
    """The records of one (pattern, table) in fixture order, each with `bytes` (the text's UTF-8 form) beside it."""
    key = ("rec", pattern, table)
    if key not in _cache:
        out = [dict(r, bytes=r["text"].encode("utf-8")) for r in fixture()["records"] if r["pattern"] == pattern and r["table"] == table]
        _cache[key] = out
    return _cache[key]


def changed_code_points():
    """The code points V8's table and the built-in one class differently (the census of v8_versions.json)."""
    out = set()
    for r in versions()["census"]["changed_ranges"]:
        a, _, b = r.partition("..")
        out.update(range(int(a[2:], 16), int((b or a)[2:], 16) + 1))
    return out


def table_sensitive_records(pattern):
    """The "v8" records of a pattern that hold a code point whose class differs between the two tables."""
    ch = changed_code_points()
    return [r for r in records(pattern, "v8") if any(ord(c) in ch for c in r["text"])]


def slice_for_emulator(recs):
    """A fixed slice, chosen by index and length alone: every document of at most 4,097 bytes and every tenth short text."""
    docs = [r for r in recs if r["kind"] == "doc" and len(r["bytes"]) <= 4097]
    shorts = [r for r in recs if r["kind"] == "short"]
    return docs + shorts[::10]


def batches(recs):
    """The records packed 1, 3 and 20 to a batch, in turn: every record is in exactly one batch."""
    out, i, k = [], 0, 0
    while i < len(recs):
        n = BATCH_SIZES[k % len(BATCH_SIZES)]
        out.append(recs[i:i + n])
        i += n
        k += 1
    return out


def bitmap(batch):
    """The piece-start bitmap V8's pieces give for a batch (the layout of Encoder.pretokenize: one entry per byte and the sentinel)."""
    total = sum(len(r["bytes"]) for r in batch)
    bm = np.zeros(total + 1, bool)
    bm[total] = True
    pos = 0
    for r in batch:
        assert (r["starts"][0] == 0 and r["starts"][-1] < len(r["bytes"])) if r["bytes"] else r["starts"] == []
        bm[pos + np.asarray(r["starts"], np.int64)] = True
        bm[pos] = True
        pos += len(r["bytes"])
    return bm


def device_bitmaps(enc, recs):
    """[(batch, docs, offsets, device bitmap, V8's bitmap)] over batches(recs)."""
    out = []
    for batch in batches(recs):
        docs = [r["bytes"] for r in batch]
        data, offs = parity.pack(docs)
        out.append((batch, docs, offs, enc.pretokenize(data, offs), bitmap(batch)))
    return out


def make_encoder(vocab, pattern, table, sequential=0):
    enc = N.Encoder(vocab, pattern)
    if sequential:
        enc.set_option(N.OPT_PRETOK_SEQUENTIAL, 1)
    if table == "v8":
        enc.set_unicode_classes(table_for(pattern))
    return enc


def check_splits(vocab, pattern, sequential, table, recs):
    """enc.pretokenize bit for bit against V8's pieces."""
    assert recs
    enc = make_encoder(vocab, pattern, table, sequential)
    for batch, docs, offs, got, exp in device_bitmaps(enc, recs):
        assert np.array_equal(got, exp), "pattern %d seq=%d table=%s, batch of %d: %s" % (
            pattern, sequential, table, len(batch), parity.explain_bitmap_diff(got, exp, docs, offs))


def check_table_is_honoured(vocab, pattern):
    """The "v8" records that hold a re-classed code point, through an encoder left on the BUILT-IN table: the device bitmap differs from V8's for at
    least one of them (else the "v8" mode would say nothing about the table being read) -- and equals it once the table is handed over."""
    recs = table_sensitive_records(pattern)
    assert len(recs) >= 100, len(recs)
    enc = N.Encoder(vocab, pattern)
    differing = sum(1 for _b, _d, _o, got, exp in device_bitmaps(enc, recs) if not np.array_equal(got, exp))
    assert differing > 0
    enc.set_unicode_classes(table_for(pattern))
    for batch, docs, offs, got, exp in device_bitmaps(enc, recs):
        assert np.array_equal(got, exp), parity.explain_bitmap_diff(got, exp, docs, offs)
    return differing


def check_one_class_flipped(vocab, O, pattern=N.O200K):
    """V8's table with ONE entry changed -- a non-ASCII letter that first occurs beyond byte 4096 of a document becomes a digit --: the device bitmap now
    differs from V8's in the 4 KiB block of that first occurrence and nowhere before it (a letter and a digit are both \\S and both outside
    [^\\s\\p{L}\\p{N}], so no piece that ends in front of the char can end elsewhere), and is what the oracle makes of the same table.  The document
    and the letter are the first ones, in fixture order, for which the oracle says the block is affected."""
    tab = v8_table()
    try:
        for r in records(pattern, "v8"):
            if r["kind"] != "doc" or len(r["bytes"]) < 9000:
                continue
            pos, first = 0, {}
            for c in r["text"]:
                first.setdefault(c, pos)
                pos += len(c.encode("utf-8"))
            exp = bitmap([r])
            for at, ch in sorted((p, c) for c, p in first.items() if p > 4096 and ord(c) >= 0x80 and 1 <= tab[ord(c)] <= 5):
                flipped = table_for(pattern).copy()
                flipped[ord(ch)] = 7
                O.set_unicode_classes(flipped)
                want = parity.oracle_bitmap(O, pattern, [r["bytes"]])
                bad = np.nonzero(want != exp)[0]
                if len(bad) and bad[0] // 4096 == at // 4096:
                    break
            else:
                continue
            break
        else:
            raise AssertionError("no document with a non-ASCII letter that first occurs beyond byte 4096")
    finally:
        O.set_unicode_classes(None)
    assert at <= bad[0]
    data, offs = parity.pack([r["bytes"]])
    for seq in (0, 1):
        enc = make_encoder(vocab, pattern, "v8", seq)
        assert np.array_equal(enc.pretokenize(data, offs), exp)
        enc.set_unicode_classes(flipped)
        got = enc.pretokenize(data, offs)
        assert np.array_equal(got[:at], exp[:at]) and not np.array_equal(got, exp), (ch, at)
        assert int(np.nonzero(got != exp)[0][0]) // 4096 == at // 4096
        assert np.array_equal(got, want), parity.explain_bitmap_diff(got, want, [r["bytes"]], offs)


def check_table_read_back(vocab, pattern):
    """After set_unicode_classes(V8's table) the DEVICE's table, read back for all 0x110000 code points, is the fixture's -- apart from the documented
    rules (tkz.h): ASCII keeps the built-in classes, a surrogate code unit is class 0, and what lies beyond the entries handed over stays built-in."""
    enc = N.Encoder(vocab, pattern)
    base = enc.unicode_classes(0, 0x110000).copy()
    tab = table_for(pattern)
    enc.set_unicode_classes(tab)
    got = enc.unicode_classes(0, 0x110000)
    want = base.copy()
    want[:len(tab)] = tab
    want[:128] = base[:128]
    want[0xD800:0xE000] = 0
    assert np.array_equal(got, want), [hex(int(c)) for c in np.nonzero(got != want)[0][:10]]
    assert np.array_equal(want[:128], tab[:128]) and not tab[0xD800:0xE000].any()       # (so for o200k `want` IS the fixture, entry for entry)
    if pattern == N.O200K:
        assert np.array_equal(got, tab)
    assert not np.array_equal(got, base)
    enc.set_unicode_classes(None)
    assert np.array_equal(enc.unicode_classes(0, 0x110000), base)


def v8_ids(ovocab, r):
    """Encode restated over V8's pieces: [rank] where the whole piece is a key, its byte-pair merge otherwise."""
    b, ends = r["bytes"], r["starts"][1:] + [len(r["bytes"])]
    ids = []
    for a, e in zip(r["starts"], ends):
        rank = ovocab.rank(b[a:e])
        ids += [rank] if rank >= 0 else ovocab.bpe(b[a:e])
    return ids


def check_ids(vocab, ovocab, pattern, table, recs, single_docs):
    """enc.encode_batch, document by document, against v8_ids: what the probe, merge and place stages make of the boundaries.  `single_docs` short
    documents go one per call (the single-launch path, which must report having run); then every record in ONE batch (the multi-kernel path)."""
    enc = make_encoder(vocab, pattern, table)
    want = [v8_ids(ovocab, r) for r in recs]
    shorts = [i for i, r in enumerate(recs) if r["kind"] == "short" and r["bytes"]][:single_docs]
    before = enc.small_path_calls()[0]
    for i in shorts:
        data, offs = parity.pack([recs[i]["bytes"]])
        ids, ooff = enc.encode_batch(data, offs)
        assert ids.tolist() == want[i] and ooff.tolist() == [0, len(want[i])], (pattern, table, recs[i]["text"])
    assert enc.small_path_calls()[0] - before == len(shorts) > 0
    data, offs = parity.pack([r["bytes"] for r in recs])
    assert len(data) > (128 << 10)                      # beyond the single launch
    before = enc.small_path_calls()[0]
    ids, ooff = enc.encode_batch(data, offs)
    assert enc.small_path_calls()[0] == before
    for i, w in enumerate(want):
        g = ids[ooff[i]:ooff[i + 1]].tolist()
        assert g == w, "pattern %d table %s doc %d (%d bytes): got %r... expected %r..." % (pattern, table, i, len(recs[i]["bytes"]), g[:12], w[:12])
    assert int(ooff[-1]) == len(ids) == sum(map(len, want))
