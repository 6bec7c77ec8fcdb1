#!/usr/bin/env python3
"""Pin the split on V8, the regex engine the TypeScript reference runs (run by hand in the build container only, after build();
never imported by a test, never run on a GPU machine -- the convention of make_golden.py).

tests/golden/v8_split.js is driven with /usr/bin/node; it reads the three pattern strings out of the reference's
tokenizer_ts/src/tokenizerBuilder.ts at run time (none is copied here; their SHA-256s go into the fixtures' headers) and compiles them as
tikTokenizer.ts:100 does, `new RegExp(pattern, "gu")`.  Written, reproducibly (fixed seeds, gzip mtime 0):

  v8_unicode_classes.bin.gz   0x110000 bytes, V8's class of every code point in the coding of tkz_unicode_classes (0 other, 1 Lu, 2 Ll, 3 Lt,
                              4 Lm, 5 Lo, 6 M, 7 N, 8 = V8's \\s; surrogates 0), from /\\p{Lu}/u ... /\\s/u tested on each code point
  v8_versions.json            process.versions.{node,v8,icu,unicode}, the pattern SHA-256s, and the census: how many code points V8's table and
                              the built-in one (Unicode 13.0) class differently, as ranges, and the \\s differences
  splits_v8.json.gz           {"header": ..., "records": [{pattern, table, kind, text, starts}]}: `starts` = the UTF-8 byte offset of every piece
                              V8 produced (converted from its UTF-16 indices; the pieces tile the text, asserted here).  `table` names the class
                              table under which the record is a valid expectation: "builtin" (the library's own 13.0 table) or "v8" (the table
                              above handed over with tkz_encoder_set_unicode_classes: all of it for o200k, its first 65,536 entries otherwise)

WHICH TEXT IS LEGITIMATE FOR WHICH PATTERN (the tests apply no filter: these rules live here)
  TKZ_PATTERN_O200K (3): V8 is the defining engine, any well-formed text qualifies.  "builtin" records draw only on code points whose class AS O200K
      READS THE BUILT-IN TABLE (tkz.h: U+FEFF is white space, U+0085 is not -- ECMAScript's \\s) equals V8's; "v8" records draw on everything and
      oversample the code points that differ between the two tables, U+0085, U+FEFF, U+2028 / U+2029 and U+180E.
  Patterns 1 and cl100k (2): libtkz implements .NET's code-UNIT reading; V8 is a reference only where the two readings coincide:
      * the alphabet is the BMP plus supplementary code points V8 classes 0 (both surrogate halves are "other" units in .NET, and no alternative can
        end between them); supplementary letters / digits / marks are left out;
      * every code point on which V8's \\s and the built-in table's class 8 differ is left out (computed below: U+0085 and U+FEFF), in both modes;
      * cl100k only: a supplementary char directly in front of a letter is left out.  V8 takes the whole char as the optional one-char prefix
        [^\\r\\n\\p{L}\\p{N}]? of the word ("a\U0001F600b" -> "a", "\U0001F600b"); .NET can take only its high half, fails on the low one and
        cuts the char off ("a", "\U0001F600", "b": TikTokenizer.cs:77 compiles the string with System.Text.RegularExpressions, one class test per
        code unit; tests/hand_splits.py has the case).  Pattern 1 has no such prefix.  Both facts are asserted below on that pair of texts;
      * cl100k only: the TypeScript string spells (?i:'s|'t|'re|...) out, lists 'eR where 'rE belongs and folds nothing beyond ASCII: after an
        apostrophe, a following rE, eR, U+017F, U+212A, U+0130 or U+0131 is replaced by a digit.
  TKZ_PATTERN_O200K_DOTNET (4) is the o200k string read by another engine: V8 does not pin it (splits_o200k_dotnet.json does).

Texts come from the generators the suite already uses -- regex_crosscheck.alphabet() / random_text, parity.gen_text (every kind, `runs` included) and
parity.o200k_gen -- and are stored verbatim.  Shapes: short texts of 0..40 chars, and documents of 63 .. 20,000 bytes around the 64-byte rows and
the 4 KiB blocks of the device scanners, with runs that cross a row and a block boundary and a multi-byte char straddling byte 64 and byte 4096.
"""
import gzip
import json
import os
import random
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NODE = "/usr/bin/node"
TS = "/root/reference/tokenizer_ts/src/tokenizerBuilder.ts"
JS = os.path.join(HERE, "v8_split.js")
N_SHORT = 1400                         # short texts per (pattern, table)
DOC_LENS = [63, 64, 65, 127, 128, 129, 1000, 4095, 4096, 4097, 9000, 20000]
LIMIT = 1 << 20


def node(mode, stdin=None):
    return subprocess.run([NODE, JS, TS, mode], input=stdin, stdout=subprocess.PIPE, check=True).stdout


def to_byte_starts(p, t, flat):
    """V8's matches [index, length, ...] in UTF-16 units -> the pieces' starts in UTF-8 bytes; the pieces tile the text (asserted)."""
    u8 = [0]                                                # UTF-16 unit index -> UTF-8 byte offset
    for ch in t:
        n8 = len(ch.encode("utf-8"))
        if ord(ch) >= 0x10000:
            u8 += [None, u8[-1] + n8]
        else:
            u8.append(u8[-1] + n8)
    pos, starts = 0, []
    for at, ln in zip(flat[0::2], flat[1::2]):
        assert at == pos and ln > 0, (p, t, flat)           # no gap, no empty piece
        starts.append(u8[at])
        pos = at + ln
    assert pos == len(u8) - 1 and None not in starts, (p, t, flat)
    return starts


def v8_split(items):
    """[(pattern, text)] -> [starts in UTF-8 bytes]."""
    lines = "".join(json.dumps({"p": p, "t": t}) + "\n" for p, t in items)
    out = node("split", lines.encode("ascii")).decode().splitlines()
    assert len(out) == len(items)
    return [to_byte_starts(p, t, json.loads(line)) for (p, t), line in zip(items, out)]


def ranges(cps):
    out = []
    for cp in cps:
        if out and out[-1][1] == cp - 1:
            out[-1][1] = cp
        else:
            out.append([cp, cp])
    return out


class Domain:
    """The rules of the docstring for one (pattern, table)."""

    def __init__(self, pattern, table, v8, builtin):
        self.pattern, self.table = pattern, table
        same = v8 == builtin
        ws_differs = (v8 == 8) != (builtin == 8)
        if pattern == 3:
            as_o200k = builtin.copy()
            as_o200k[0xFEFF], as_o200k[0x85] = 8, 0
            ok = (v8 == as_o200k) if table == "builtin" else np.ones(len(v8), bool)
        else:
            ok = (same if table == "builtin" else np.ones(len(v8), bool)) & ~ws_differs
            ok[0x10000:] &= (v8[0x10000:] == 0)
            if table == "builtin":
                ok[0x10000:] &= (builtin[0x10000:] == 0)
        ok[0xD800:0xE000] = False
        self.ok, self.v8 = ok, v8

    def clean(self, text):
        out = [ch for ch in text if self.ok[ord(ch)]]
        if self.pattern == 2:
            for i in range(len(out) - 1):
                if out[i] == "'":
                    if out[i + 1] in "\u017f\u212a\u0130\u0131" or (i + 2 < len(out) and out[i + 1] + out[i + 2] in ("rE", "eR")):
                        out[i + 1] = "7"
                if ord(out[i]) >= 0x10000 and 1 <= self.v8[ord(out[i + 1])] <= 5:
                    out[i + 1] = "7"
        return "".join(out)


def fit(text, nbytes, straddle=(), wide="\u4e2d", pad="a"):
    """Exactly nbytes of UTF-8 out of text (padded with `pad`), with a multi-byte char (`wide`, or U+00E9 where that does not fit) across every
    byte offset in `straddle`, a pad char in front of it."""
    out, off = [], 0
    marks = []
    for b in straddle:
        w = wide if b - 1 + len(wide.encode()) <= nbytes else "\u00e9"
        if b + 1 <= nbytes:
            marks.append((b, w))
    for ch in text:
        n8 = len(ch.encode("utf-8"))
        if marks and off + n8 > marks[0][0] - 2:
            b, w = marks.pop(0)
            out.append(pad * (b - 1 - off) + w)
            off = b - 1 + len(w.encode())
        if off + n8 > nbytes:
            break
        out.append(ch)
        off += n8
    assert not marks, (nbytes, straddle)
    s = "".join(out) + pad * (nbytes - off)
    assert len(s.encode("utf-8")) == nbytes
    for b in straddle:
        if b + 1 <= nbytes:
            assert (s.encode("utf-8")[b] & 0xC0) == 0x80, b                  # byte b is inside a char
    return s


def crafted_runs(n, variant):
    """Single-class runs placed across byte 64 (a row) and bytes 3968 / 4096 (a block and its neighbour), cut to n chars (ASCII: n bytes)."""
    if variant == 0:
        s = "ab " + "7" * 90 + " x" + " " * 70 + "\ny" + "=" * 80 + "'s"
        s += "z" * (3900 - len(s)) + "5" * 300 + " end" + " " * 4200 + "\n" + "ab 12.\n" * 200
    else:
        s = "q" * 40 + " " * 60 + "\r\n" + "\n" * 70 + "9" * 65 + "a "
        s += "/" * (3950 - len(s)) + "\n" * 100 + " \t" * 100 + "A" * 4300 + "1" * 4100 + " " * 300 + "x"
    s = s * (n // len(s) + 1)
    return s[:n]


def tables():
    """(node's versions and pattern hashes, V8's class table, the built-in one)."""
    from tokenizer_amd import _native as N
    info = json.loads(node("info"))
    v8 = np.frombuffer(node("classes"), np.uint8).copy()
    assert len(v8) == 0x110000 and v8.max() == 8 and not v8[0xD800:0xE000].any()
    builtin = np.zeros(0x110000, np.uint8)
    N.default_library().L.tkz_unicode_classes(0, 0x110000, builtin.ctypes.data)
    return info, v8, builtin


class Drawer:
    """Texts of one Domain from the suite's generators; under the "v8" table the code points the two tables class differently and the \\s edge cases
    (U+0085, U+FEFF, U+2028, U+2029, U+180E) are mixed in wherever the domain admits them."""
    def __init__(self, dom, v8, builtin):
        import parity
        import regex_crosscheck as RC
        self.parity, self.dom = parity, dom
        self.alpha = RC.alphabet()
        self.kinds = ["mix"] * 3 + list(parity.SMALL_ALPHAS) + ["runs"]
        self.okinds = ["cjk", "case", "emoji", "upper", "all", "mark", "slash", "chain"]
        changed = [chr(cp) for cp in np.nonzero(v8 != builtin)[0].tolist()] + ["\x85", "\ufeff", "\u2028", "\u2029", "\u180e"]
        self.hot = hot = [c for c in changed if dom.ok[ord(c)]] if dom.table == "v8" else []
        assert dom.table == "builtin" or len(hot) > 50
        self.wide = self.alpha + (hot * (1 + len(self.alpha) // max(1, len(hot))))[:len(self.alpha)]      # (half of the draws are changed / edge code points)

    def text(self, rng, n, i):
        """n chars of the i-th kind (before Domain.clean)."""
        parity, hot = self.parity, self.hot
        if self.dom.pattern == 3 and i % 3 == 2:
            a = parity.O200K_ALPHAS[self.okinds[(i // 3) % len(self.okinds)]]
            return parity.o200k_gen(rng, a + (rng.sample(hot, 8) if hot else []), n)
        kind = self.kinds[i % len(self.kinds)]
        if hot and kind != "mix" and kind != "runs":
            base = parity.gen_text(rng, kind, n, self.alpha)
            return "".join(rng.choice(hot) if rng.random() < 0.15 else ch for ch in base)
        return parity.gen_text(rng, kind, n, self.wide)


def main():
    import parity
    from oracle import oracle as O

    info, v8, builtin = tables()
    with open(os.path.join(HERE, "v8_unicode_classes.bin.gz"), "wb") as f:
        f.write(gzip.compress(v8.tobytes(), 9, mtime=0))

    changed = np.nonzero(v8 != builtin)[0].tolist()
    ws_diff = np.nonzero((v8 == 8) != (builtin == 8))[0].tolist()
    census = {"code_points_classed_differently": len(changed), "changed_ranges": ["U+%04X" % a if a == b else "U+%04X..U+%04X" % (a, b) for a, b in ranges(changed)],
              "whitespace_differences": [{"cp": "U+%04X" % cp, "v8": int(v8[cp]), "builtin": int(builtin[cp])} for cp in ws_diff]}
    assert 0x85 in ws_diff and 0xFEFF in ws_diff
    versions = dict(info, census=census)
    with open(os.path.join(HERE, "v8_versions.json"), "w") as f:
        json.dump(versions, f, indent=1, sort_keys=True)
        f.write("\n")

    # the domain argument for supplementary chars under .NET's reading, on a pair of texts: pattern 1 cuts "a😀b" as V8 does, cl100k does not
    pair = "a\U0001F600b"
    got = v8_split([(1, pair), (2, pair)])
    assert got[0] == [0, 1, 5] == [a for a, _ in O.split_utf8(1, pair.encode())]
    assert got[1] == [0, 1] and [a for a, _ in O.split_utf8(2, pair.encode())] == [0, 1, 5]

    items, meta = [], []

    def add(dom, kind, text):
        assert dom.clean(text) == text
        items.append((dom.pattern, text))
        meta.append({"pattern": dom.pattern, "table": dom.table, "kind": kind, "text": text})

    for pattern in (1, 2, 3):
        for table in ("builtin", "v8"):
            dom = Domain(pattern, table, v8, builtin)
            draw = Drawer(dom, v8, builtin)
            rng = random.Random(20000 + 100 * pattern + (table == "v8"))
            text_of = lambda n, i: draw.text(rng, n, i)
            for i in range(N_SHORT):
                add(dom, "short", dom.clean(text_of(rng.randint(0, 40), i))[:40])
            for li, nbytes in enumerate(DOC_LENS):
                four = "\U0001F600" if pattern == 3 else "\u4e2d"
                pad = "7" if pattern == 2 else "a"
                # a mixed document with a multi-byte char across bytes 64 and 4096 (where it is that long), one of another kind, and ASCII runs
                add(dom, "doc", fit(dom.clean(text_of(nbytes, 2 * li)), nbytes, (64, 4096), four, pad))
                add(dom, "doc", fit(dom.clean(text_of(nbytes, 2 * li + 1 + pattern)), nbytes, (64,) if li % 2 else (), pad=pad))
                add(dom, "doc", fit(dom.clean(crafted_runs(nbytes, li % 2)), nbytes, pad=pad))
                if nbytes >= 1000:
                    add(dom, "doc", fit(dom.clean(parity.gen_runs(rng, nbytes)), nbytes, pad=pad))

    for m, starts in zip(meta, v8_split(items)):
        m["starts"] = starts
    header = {k: info[k] for k in ("node", "v8", "icu", "unicode", "pattern_sha256")}
    blob = json.dumps({"header": header, "records": meta}, ensure_ascii=False, separators=(",", ":"), sort_keys=True).encode("utf-8")
    packed = gzip.compress(blob, 9, mtime=0)
    with open(os.path.join(HERE, "splits_v8.json.gz"), "wb") as f:
        f.write(packed)
    assert len(packed) <= LIMIT, len(packed)
    print("V8 %s (node %s, ICU %s, Unicode %s): %d code points classed differently from the built-in table, \\s differs on %s" % (
        info["v8"], info["node"], info["icu"], info["unicode"], len(changed), [w["cp"] for w in census["whitespace_differences"]]))
    print("%d records, %d bytes of JSON, %d gzipped" % (len(meta), len(blob), len(packed)))


if __name__ == "__main__":
    main()
