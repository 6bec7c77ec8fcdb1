#!/usr/bin/env python3
"""What Encode(text, allowedSpecial) on ONE string costs through the single-launch kernel's special form, beside the routes it replaces.  Per vocabulary
(gpt2 with pattern 1, synth100k with cl100k) and per input -- 64 bytes with one literal, a 2 KB chat prompt with six, 32 KB with forty -- three routes,
alternating in ONE loop after warm-up calls of all three, a host clock around calls that end in the entry's own synchronisation, the median of --calls calls:
  (a) tkz_encode_special_utf8                            the new entry
  (b) tkz_encode_batch_special_utf8 with one document    the parent's route for the same text (page-locked buffers: the entry allows them)
  (c) tkz_encode_utf8 on the text without its literals   the plain single call
and the phase stamps of tkz_encoder_small_path_phases for the special launch (shader-clock ticks between the stamps).  The results of (a) and (b) are compared.
Then the plain path beside the parent commit (--parent-lib: a libtkz.so built from the parent's sources): tkz_encode_utf8 on 64 bytes and on 1 MB of
literal-free text, in child processes that alternate between the two libraries, --runs of each; the README states the difference of the medians beside the
spread of the parent's runs against one another.
Writes README.md and raw.jsonl into --out.
usage: python tools/small_special_probe.py [--calls 2000] [--warmup 200] [--parent-lib PATH] [--runs 5] [--out profiles/small_special]"""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPECIALS = ["<|endoftext|>", "<|im_start|>", "<|im_end|>"]
WORDS = ["the", "quick", "brown", "fox", "it's", "2024", "tokens", "=>", "x", "don't", "Hello", "12345", "(a+b)", "jumps", "over", "lazy", "dog."]
PHASES = ["input", "document marks", "literal scan", "literal resolve", "pre-tokenizer", "literal fix", "counts + scans", "probe", "merge short", "merge long",
          "token scan", "place", "document offsets"]


def filler(n, seed):
    import random
    rng = random.Random(seed)
    s = ""
    while len(s) < n:
        s += rng.choice(WORDS) + " "
    return s[:n]


def make_inputs():
    """(name, text with literals, the same text without them)"""
    out = []
    body = filler(64 - len(SPECIALS[0]), 1)
    out.append(("64 B, 1 literal", body[:30] + SPECIALS[0] + body[30:]))
    turns = [("system", 300), ("user", 700), ("assistant", 800)]                       # <|im_start|>role\n ... <|im_end|>\n, three turns: six literals
    chat = "".join("<|im_start|>%s\n%s<|im_end|>\n" % (role, filler(n, 10 + k)) for k, (role, n) in enumerate(turns))
    chat += filler(2048 - len(chat), 20)
    out.append(("2 KB chat prompt, 6 literals", chat))
    part = (32768 - 40 * len(SPECIALS[0])) // 40
    big = "".join(filler(part, 100 + k) + SPECIALS[0] for k in range(40))
    out.append(("32 KB, 40 literals", big + filler(32768 - len(big), 99)))
    res = []
    for name, text in out:
        plain = text
        for s in SPECIALS:
            plain = plain.replace(s, "")
        res.append((name, text.encode(), plain.encode()))
    assert [len(t) for _, t, _ in res] == [64, 2048, 32768]
    return res


def median_us(ns):
    return round(statistics.median(ns) / 1000.0, 2)


def spread(ns):
    q = statistics.quantiles(ns, n=10)
    return {"median_us": median_us(ns), "p10_us": round(q[0] / 1000.0, 2), "p90_us": round(q[-1] / 1000.0, 2)}


def load(lib_path, vocab_name, pattern):
    from tokenizer_amd import _native as N
    lib = N.Library(lib_path) if lib_path else N.default_library()
    raw = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", vocab_name + ".tiktoken.gz"), "rb").read())
    return N, lib, N.Encoder(N.Vocab(raw, lib), pattern, device=0)


def pinned(lib, nbytes):
    p = C.c_void_p()
    lib.check(lib.L.tkz_host_alloc(nbytes, C.byref(p)))
    return p.value


def time_routes(args, vocab_name, pattern, pattern_name):
    import numpy as np
    N, lib, enc = load(args.lib, vocab_name, pattern)
    base = 1 << 18
    enc.set_special_tokens({s: base + i for i, s in enumerate(SPECIALS)})
    L, h = lib.L, enc._h
    allowed = (C.c_int32 * len(SPECIALS))(*range(len(SPECIALS)))
    rows = []
    for name, text, plain in make_inputs():
        n, cap = len(text), len(text)
        # (b) reads and writes page-locked memory; the single entries take ordinary pointers and stage the text themselves
        p_text, p_offs, p_ids, p_ooff = pinned(lib, n + 64), pinned(lib, 16), pinned(lib, 4 * cap), pinned(lib, 16)
        C.memmove(p_text, text, n)
        (C.c_int64 * 2).from_address(p_offs)[:] = [0, n]
        t_buf, c_buf = np.frombuffer(text, np.uint8), np.frombuffer(plain, np.uint8)
        ids_a, ids_c = np.empty(cap, np.int32), np.empty(cap, np.int32)
        na, nb, nc = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        pa, pc, pia, pic = t_buf.ctypes.data, c_buf.ctypes.data, ids_a.ctypes.data, ids_c.ctypes.data

        def a():
            return L.tkz_encode_special_utf8(h, pa, n, allowed, len(SPECIALS), pia, cap, C.byref(na))

        def b():
            return L.tkz_encode_batch_special_utf8(h, p_text, p_offs, 1, allowed, len(SPECIALS), p_ids, cap, p_ooff, C.byref(nb))

        def c():
            return L.tkz_encode_utf8(h, pc, len(plain), pic, cap, C.byref(nc))
        for _ in range(args.warmup):
            lib.check(a()); lib.check(b()); lib.check(c())
        got_b = list((C.c_int32 * nb.value).from_address(p_ids))
        assert ids_a[:na.value].tolist() == got_b, "the new entry and the batch entry disagree on %s" % name
        calls0 = enc.small_path_calls()
        ta, tb, tc = [], [], []
        clk = time.perf_counter_ns
        for _ in range(args.calls):
            t0 = clk(); a(); t1 = clk(); b(); t2 = clk(); c(); t3 = clk()
            ta.append(t1 - t0); tb.append(t2 - t1); tc.append(t3 - t2)
        calls1 = enc.small_path_calls()
        lib.check(a())
        st = enc.small_path_phases()
        ticks = [st[i + 1] - st[i] for i in range(len(PHASES))]
        row = {"vocab": vocab_name, "pattern": pattern_name, "input": name, "bytes": n, "tokens": na.value, "calls": args.calls, "warmup": args.warmup,
               "a_new_entry": spread(ta), "b_batch_entry_one_document": spread(tb), "c_plain_single_call": spread(tc),
               "a_over_b": round(statistics.median(ta) / statistics.median(tb), 3), "a_over_c": round(statistics.median(ta) / statistics.median(tc), 3),
               "single_launches": calls1[0] - calls0[0], "handed_back": calls1[1] - calls0[1],
               "phase_ticks": dict(zip(PHASES, ticks)), "kernel_ticks": st[len(PHASES)] - st[0]}
        assert row["single_launches"] == 2 * args.calls and row["handed_back"] == 0, row          # (a) and (c) took the launch, every time
        rows.append(row)
        print(json.dumps(row), flush=True)
        for p in (p_text, p_offs, p_ids, p_ooff):
            L.tkz_host_free(p)
    return rows


def plain_child(args):
    """one process, one library: the plain single call on 64 bytes (the single launch) and on 1 MB of literal-free text (the batch path).  The C ABI through
    ctypes directly: the parent's library does not export what tokenizer_amd._native binds."""
    import numpy as np
    L = C.CDLL(args.lib or os.path.join(ROOT, "tokenizer_amd", "lib", "libtkz.so"))
    vp, i64 = C.c_void_p, C.c_int64
    L.tkz_vocab_from_tiktoken.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.tkz_encoder_create.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.tkz_encode_utf8.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64)]
    L.tkz_last_error.restype = C.c_char_p

    def check(st):
        if st != 0:
            raise SystemExit("small_special_probe: status %d: %s" % (st, L.tkz_last_error().decode()))
    raw = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "gpt2.tiktoken.gz"), "rb").read())
    v, h = vp(), vp()
    check(L.tkz_vocab_from_tiktoken(raw, len(raw), C.byref(v)))
    check(L.tkz_encoder_create(v, 1, 0, C.byref(h)))
    out = {"lib": args.lib or "default"}
    for name, n, calls in (("64 B", 64, args.calls), ("1 MB", 1 << 20, max(50, args.calls // 10))):
        text = np.frombuffer(filler(n, 7).encode(), np.uint8)
        ids = np.empty(n, np.int32)
        k = i64(0)
        pt, pi = text.ctypes.data, ids.ctypes.data
        for _ in range(max(20, args.warmup // 4)):
            check(L.tkz_encode_utf8(h, pt, n, pi, n, C.byref(k)))
        ts = []
        clk = time.perf_counter_ns
        for _ in range(calls):
            t0 = clk(); L.tkz_encode_utf8(h, pt, n, pi, n, C.byref(k)); ts.append(clk() - t0)
        out[name] = median_us(ts)
        out[name + " tokens"] = k.value
    print(json.dumps(out), flush=True)


def plain_beside_parent(args):
    runs = {"parent": [], "new": []}
    new_lib = args.lib or os.path.join(ROOT, "tokenizer_amd", "lib", "libtkz.so")
    for r in range(args.runs):
        for which, path in (("parent", args.parent_lib), ("new", new_lib)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--lib", path, "--calls", str(args.calls), "--warmup", str(args.warmup)],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise SystemExit("small_special_probe: the child for %s ended with %d\n%s" % (path, out.returncode, out.stderr[-2000:]))
            runs[which].append(json.loads(out.stdout.strip().splitlines()[-1]))
    res = {"what": "tkz_encode_utf8, median us per call in alternating child processes", "runs": args.runs}
    for case in ("64 B", "1 MB"):
        p = [x[case] for x in runs["parent"]]
        n = [x[case] for x in runs["new"]]
        res[case] = {"parent_runs_us": p, "new_runs_us": n, "parent_median_us": statistics.median(p), "new_median_us": statistics.median(n),
                     "difference_us": round(statistics.median(n) - statistics.median(p), 2), "parent_spread_us": round(max(p) - min(p), 2)}
    print(json.dumps(res), flush=True)
    return res


def write_readme(out_dir, rows, plain):
    lines = ["# Encode(text, allowedSpecial) for one string: the single launch beside the routes it replaces", "",
             "Written by `tools/small_special_probe.py` on an MI355X; the raw lines are in `raw.jsonl`.  A host clock around calls that end in the entry's own",
             "synchronisation, the three routes alternating in one loop after %d warm-up calls of each, the median of %d calls (p10 .. p90 in brackets), microseconds." % (rows[0]["warmup"], rows[0]["calls"]), "",
             "- (a) `tkz_encode_special_utf8`: the new entry, one `k_small<true>` launch",
             "- (b) `tkz_encode_batch_special_utf8` with one document on page-locked buffers: the route the parent takes for the same text",
             "- (c) `tkz_encode_utf8` on the text with the literals removed: the plain single launch", "",
             "| vocabulary, pattern | input | tokens | (a) us | (b) us | (c) us | a/b | a/c |", "|---|---|---|---|---|---|---|---|"]
    f = lambda s: "%.1f [%.1f .. %.1f]" % (s["median_us"], s["p10_us"], s["p90_us"])
    for r in rows:
        lines.append("| %s, %s | %s | %d | %s | %s | %s | %.3f | %.3f |" % (r["vocab"], r["pattern"], r["input"], r["tokens"], f(r["a_new_entry"]), f(r["b_batch_entry_one_document"]),
                                                                        f(r["c_plain_single_call"]), r["a_over_b"], r["a_over_c"]))
    lines += ["", "## Phase stamps of the special launch", "",
              "Shader-clock ticks between the stamps of `tkz_encoder_small_path_phases` for one call of (a) after the timed loop; the share of the kernel in brackets.", "",
              "| vocabulary, input | kernel | " + " | ".join(PHASES) + " |", "|---|---|" + "---|" * len(PHASES)]
    for r in rows:
        k = max(1, r["kernel_ticks"])
        lines.append("| %s, %s | %d | " % (r["vocab"], r["input"], r["kernel_ticks"]) + " | ".join("%d (%d%%)" % (r["phase_ticks"][p], round(100.0 * r["phase_ticks"][p] / k)) for p in PHASES) + " |")
    lines += ["", "## The plain path beside the parent commit", ""]
    if plain:
        lines += ["`tkz_encode_utf8` through a `libtkz.so` built from the parent commit's sources and through this one, %d child processes of each, alternating;" % plain["runs"],
                  "per process the median of the calls, microseconds.  The difference is this tree's median of medians minus the parent's; the spread is the parent's",
                  "largest run minus its smallest.", "",
                  "| case | parent runs | this tree's runs | difference | parent's spread |", "|---|---|---|---|---|"]
        for case in ("64 B", "1 MB"):
            c = plain[case]
            lines.append("| %s | %s | %s | %+.2f | %.2f |" % (case, ", ".join("%.1f" % x for x in c["parent_runs_us"]), ", ".join("%.1f" % x for x in c["new_runs_us"]), c["difference_us"], c["parent_spread_us"]))
    else:
        lines.append("Not measured in this run (no --parent-lib).")
    lines.append("")
    with open(os.path.join(out_dir, "README.md"), "w") as fh:
        fh.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_special"))
    ap.add_argument("--plain-child", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("small_special_probe: no GPU (a timing taken elsewhere says nothing)")
    if args.plain_child:
        return plain_child(args)
    if args.calls < 2000:
        raise SystemExit("small_special_probe: the medians are of at least 2,000 calls")
    from tokenizer_amd import _native as N
    os.makedirs(args.out, exist_ok=True)
    rows = time_routes(args, "gpt2", N.P1, "pattern 1") + time_routes(args, "synth100k", N.CL100K, "cl100k")
    plain = plain_beside_parent(args) if args.parent_lib else None
    with open(os.path.join(args.out, "raw.jsonl"), "w") as fh:
        for r in rows + ([plain] if plain else []):
            fh.write(json.dumps(r) + "\n")
    write_readme(args.out, rows, plain)


if __name__ == "__main__":
    main()
