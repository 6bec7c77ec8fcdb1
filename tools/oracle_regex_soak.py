"""Soak of the oracle's hand-written split (oracle/tkz_oracle.c: all four patterns) against the independent backtracking engine of tests/regex_crosscheck.py
(Python `regex` fed UTF-16 code units with .NET's / ECMAScript's \\s): random texts over the wide alphabet and over the adversarial small alphabets of
tests/parity.py (white space, digits, apostrophes and contraction suffixes, case transitions, CR / LF / '/', long runs), 0..400 chars, for a wall-clock budget.
What stands behind the cl100k / o200k split while the reference's own id vectors cannot run offline.  usage: oracle_regex_soak.py [seconds] [seed]

--engine v8 [texts per pattern and table] [seed]: the same oracle against V8 itself, the engine the TypeScript reference compiles its patterns with --
one `node` child (tests/golden/v8_split.js, which reads the pattern strings out of the reference's source) is streamed the texts.  Patterns 1, cl100k
and o200k, under the built-in class table and under V8's own; the texts and the domain on which V8 is a valid reference for each pattern are those of
tests/golden/make_v8_fixtures.py (short texts of 0..40 chars, one in ten up to 400).  Prints the count and every disagreement.  Needs Node and the
reference: the build machine only."""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity
import regex_crosscheck as RC
from oracle import oracle as O


def soak_v8(n_texts, seed):
    import json, subprocess
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_v8_fixtures as G
    info, v8, builtin = G.tables()
    print("oracle vs V8 %s (node %s, ICU %s, Unicode %s), %d texts per pattern and table, seed %d" % (info["v8"], info["node"], info["icu"], info["unicode"], n_texts, seed))
    child = subprocess.Popen([G.NODE, G.JS, G.TS, "split"], stdin=subprocess.PIPE, stdout=subprocess.PIPE)
    bad_total = 0
    try:
        for pattern in (1, 2, 3):
            for table in ("builtin", "v8"):
                dom = G.Domain(pattern, table, v8, builtin)
                draw = G.Drawer(dom, v8, builtin)
                rng = random.Random(seed * 1000 + 10 * pattern + (table == "v8"))
                O.set_unicode_classes((v8 if pattern == 3 else v8[:65536]) if table == "v8" else None)
                t0 = time.time(); done = bad = nbytes = 0
                while done < n_texts:
                    chunk = [dom.clean(draw.text(rng, rng.randint(0, 40) if rng.random() < 0.9 else rng.randint(41, 400), rng.randrange(1 << 20)))
                             for _ in range(min(500, n_texts - done))]
                    child.stdin.write("".join(json.dumps({"p": pattern, "t": t}) + "\n" for t in chunk).encode("ascii")); child.stdin.flush()
                    for t in chunk:
                        want = G.to_byte_starts(pattern, t, json.loads(child.stdout.readline()))
                        b = t.encode("utf-8")
                        got = [a for a, _ in O.split_utf8(pattern, b)]
                        if got != want:
                            bad += 1
                            print("DISAGREEMENT pattern %d table %s %r\n oracle %r\n v8     %r" % (pattern, table, t, got, want))
                        nbytes += len(b)
                    done += len(chunk)
                print("pattern %d table %-7s: %d texts, %d bytes, %d disagreements, %.0f s" % (pattern, table, done, nbytes, bad, time.time() - t0), flush=True)
                bad_total += bad
    finally:
        O.set_unicode_classes(None)
        child.stdin.close(); child.wait()
    print("oracle vs V8: %d disagreements in all" % bad_total)
    sys.exit(1 if bad_total else 0)


if "--engine" in sys.argv:
    rest = [a for a in sys.argv[1:] if a not in ("--engine", "v8")]
    assert sys.argv[sys.argv.index("--engine") + 1] == "v8", "engines: v8 (the default is Python's `regex`)"
    soak_v8(int(rest[0]) if rest else 200000, int(rest[1]) if len(rest) > 1 else 1)

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 300.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = random.Random(seed)
alpha = RC.alphabet()
kinds = ["mix"] * 4 + [k for k in parity.SMALL_ALPHAS]
t0 = time.time(); n = 0; units_total = 0; per = {1: 0, 2: 0, 3: 0, 4: 0}
while time.time() - t0 < budget:
    kind = rng.choice(kinds)
    ln = rng.choice([0, 1, 2, 5, 12, 40, 40, 100, 400])
    s = RC.random_text(rng, alpha, ln) if kind == "mix" else parity.gen_text(rng, kind, ln, alpha)
    # (the small alphabets hold chars whose classes Python's tables and Unicode 13 may disagree on: keep what the cross-check's own filter accepts)
    s = "".join(ch for ch in s if ord(ch) < 0x80 or RC._agree(ord(ch)))
    units = RC.to_units(s)
    for pattern in (1, 2, 3, 4):
        a, b = O.split_utf16(pattern, units), RC.split_units_regex(pattern, units)
        if a != b:
            print("MISMATCH pattern", pattern, "kind", kind, repr(s)); print(" oracle", a[:20]); print(" regex ", b[:20]); sys.exit(1)
        per[pattern] += 1
    n += 1; units_total += len(units)
print("oracle vs regex ok: %d texts x 4 patterns, %d code units, seed %d" % (n, units_total, seed))
