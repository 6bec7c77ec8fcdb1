#!/usr/bin/env python3
"""What EncodeTrimSuffix / EncodeTrimPrefix on ONE string costs through the single-launch kernel's trim form, beside the route it replaces.  Per vocabulary
(gpt2 with pattern 1, synth100k with cl100k), per input -- 64 bytes with one literal, a 2 KB chat prompt with six, 32 KB with forty, 96 KiB and 128 KiB of plain text (the trim launch's limit, and beyond it) --,
per side and per maximum (a quarter of the text's token count; above it: kept whole), three routes alternating in ONE loop after warm-up calls of all three, a
host clock around calls that end in the entry's own synchronisation, the median of --calls calls:
  (a) tkz_encode_trim_utf8                               the new entry
  (b) tkz_encode_batch_trim_utf8 with one document       the parent commit's route for the same text, in the PARENT's library (--parent-lib: a libtkz.so built
                                                         from the parent's sources, loaded beside this one); without --parent-lib: in this library, and the
                                                         README says so
  (c) tkz_encode_special_utf8 on the same text           the same launch without the cut phase
and the phase stamps of tkz_encoder_small_path_phases for the trim launch.  The results of (a) and (b) are compared.
Then what must not move (--parent-lib): tkz_encode_utf8 and tkz_encode_special_utf8 on the 64-byte text in child processes that alternate between the two
libraries, --runs of each; the README states the difference of the medians beside the spread of the parent's runs against one another.
Writes README.md and raw.jsonl into --out; --resources FILE: a text file (the compiler's resource report of k_small, parent and this tree) quoted in the README.
usage: python tools/small_trim_probe.py [--calls 2000] [--warmup 200] [--parent-lib PATH] [--runs 5] [--resources FILE] [--out profiles/small_trim]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import small_special_probe as SP  # noqa: E402  (the texts, the pinned buffers and the statistics of the special probe)

SPECIALS = SP.SPECIALS
PHASES = SP.PHASES + ["cut", "cut units"]
SUFFIX, PREFIX = 0, 1
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


def make_inputs(plain_sizes=None):
    """the four texts of the table; plain_sizes: plain text of those sizes instead (the crossover scan)"""
    if plain_sizes:
        return [("%d KiB, plain" % (n >> 10), SP.filler(n, 5).encode()) for n in plain_sizes]
    plain = SP.filler(131072, 5).encode()
    return [(name, text) for name, text, _ in SP.make_inputs()] + [("96 KiB, plain", plain[:98304]), ("128 KiB, plain", plain)]


def vocab_bytes(name):
    return gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".tiktoken.gz"), "rb").read())


class RawLib:
    """a libtkz.so through ctypes alone: the parent's library does not export what tokenizer_amd._native binds"""

    def __init__(self, path, vocab_name, pattern):
        L = self.L = C.CDLL(path)
        L.tkz_vocab_from_tiktoken.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.tkz_encoder_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
        L.tkz_encoder_set_special_tokens.argtypes = [vp, vp, vp, vp, i32]
        L.tkz_encode_utf8.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64)]
        L.tkz_encode_special_utf8.argtypes = [vp, vp, i64, vp, i32, vp, i64, C.POINTER(i64)]
        L.tkz_encode_batch_trim_utf8.argtypes = [vp, vp, vp, i64, vp, i32, i32, i64, vp, vp, i64, vp, vp, vp, C.POINTER(i64)]
        L.tkz_last_error.restype = C.c_char_p
        raw = vocab_bytes(vocab_name)
        v, h = vp(), vp()
        self.check(L.tkz_vocab_from_tiktoken(raw, len(raw), C.byref(v)))
        self.check(L.tkz_encoder_create(v, pattern, 0, C.byref(h)))
        blob = "".join(SPECIALS).encode()
        offs = (i64 * (len(SPECIALS) + 1))(*[sum(len(s) for s in SPECIALS[:k]) for k in range(len(SPECIALS) + 1)])
        ids = (i32 * len(SPECIALS))(*[(1 << 18) + i for i in range(len(SPECIALS))])
        self.check(L.tkz_encoder_set_special_tokens(h, ids, blob, offs, len(SPECIALS)))
        self.h = h

    def check(self, st):
        if st != 0:
            raise SystemExit("small_trim_probe: status %d: %s" % (st, self.L.tkz_last_error().decode()))


def time_routes(args, vocab_name, pattern, pattern_name):
    import numpy as np
    N, lib, enc = SP.load(args.lib, vocab_name, pattern)
    enc.set_special_tokens({s: (1 << 18) + i for i, s in enumerate(SPECIALS)})
    L, h = lib.L, enc._h
    old = RawLib(args.parent_lib, vocab_name, pattern) if args.parent_lib else None
    bL, bh = (old.L, old.h) if old else (L, h)
    allowed = (i32 * len(SPECIALS))(*range(len(SPECIALS)))
    na_ = len(SPECIALS)
    rows = []
    for name, text in make_inputs(args.plain_sizes):
        n = len(text)
        t_buf = np.frombuffer(text, np.uint8)
        ids_a, ids_b, ids_c = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        offs = (i64 * 2)(0, n)
        ooff = (i64 * 2)(0, 0)
        k = i64(0)
        lib.check(L.tkz_encode_special_utf8(h, t_buf.ctypes.data, n, allowed, na_, ids_c.ctypes.data, n, C.byref(k)))
        count = k.value
        for side, side_name in ((SUFFIX, "suffix"), (PREFIX, "prefix")):
            for mx, mx_name in ((max(1, count // 4), "a quarter"), (count + 1, "kept whole")):
                na, nb, nc, cb_a, cu_a, cb_b, cu_b = i64(0), i64(0), i64(0), i64(0), i64(0), i64(0), i64(0)
                pt, pia, pib, pic = t_buf.ctypes.data, ids_a.ctypes.data, ids_b.ctypes.data, ids_c.ctypes.data

                def a():
                    return L.tkz_encode_trim_utf8(h, pt, n, allowed, na_, side, mx, pia, n, C.byref(na), C.byref(cb_a), C.byref(cu_a))

                def b():
                    return bL.tkz_encode_batch_trim_utf8(bh, pt, offs, 1, allowed, na_, side, mx, None, pib, n, ooff, C.byref(cb_b), C.byref(cu_b), C.byref(nb))

                def c():
                    return L.tkz_encode_special_utf8(h, pt, n, allowed, na_, pic, n, C.byref(nc))
                warm = args.warmup if n <= 32768 else max(20, args.warmup // 4)
                for _ in range(warm):
                    lib.check(a())
                    st = b()
                    if st != 0:
                        raise SystemExit("small_trim_probe: (b) status %d" % st)
                    lib.check(c())
                assert ids_a[:na.value].tolist() == ids_b[:nb.value].tolist() and (cb_a.value, cu_a.value) == (cb_b.value, cu_b.value), "the new entry and the batch entry disagree on %s" % name
                calls0 = enc.small_path_calls()
                lib.check(a())
                a_launch = enc.small_path_calls()[0] - calls0[0]             # 1: the entry takes the launch for this text; 0: it routes it to the batch path
                calls0 = enc.small_path_calls()
                ta, tb, tc = [], [], []
                clk = time.perf_counter_ns
                for _ in range(args.calls):
                    t0 = clk(); a(); t1 = clk(); b(); t2 = clk(); c(); t3 = clk()
                    ta.append(t1 - t0); tb.append(t2 - t1); tc.append(t3 - t2)
                calls1 = enc.small_path_calls()
                lib.check(a())
                st = enc.small_path_phases()
                ticks = [st[i + 1] - st[i] for i in range(len(PHASES))] if a_launch else [0] * len(PHASES)
                row = {"vocab": vocab_name, "pattern": pattern_name, "input": name, "bytes": n, "tokens": count, "side": side_name, "max": mx, "max_name": mx_name,
                       "kept": na.value, "cut_bytes": cb_a.value, "a_route": "launch" if a_launch else "batch path", "calls": args.calls, "warmup": warm, "b_in_parent_library": bool(old),
                       "a_new_entry": SP.spread(ta), "b_batch_trim_one_document": SP.spread(tb), "c_special_single_call": SP.spread(tc),
                       "a_over_b": round(statistics.median(ta) / statistics.median(tb), 3), "a_minus_c_us": round((statistics.median(ta) - statistics.median(tc)) / 1000.0, 2),
                       "single_launches": calls1[0] - calls0[0], "handed_back": calls1[1] - calls0[1],
                       "phase_ticks": dict(zip(PHASES, ticks)), "kernel_ticks": st[len(PHASES)] - st[0] if a_launch else 0}
                assert row["handed_back"] == 0 and row["single_launches"] == (1 + a_launch) * args.calls, row      # (c), and (a) where the entry routes the text there, took the launch every time
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def still_child(args):
    """one process, one library: the plain and the special single call on the 64-byte text"""
    import numpy as np
    R = RawLib(args.lib or os.path.join(ROOT, "tokenizer_amd", "lib", "libtkz.so"), "gpt2", 1)
    L, h = R.L, R.h
    name, text = make_inputs()[0]
    plain = text
    for s in SPECIALS:
        plain = plain.replace(s.encode(), b"")
    allowed = (i32 * len(SPECIALS))(*range(len(SPECIALS)))
    out = {"lib": args.lib or "default"}
    for case, body, special in (("plain 64 B", plain, False), ("special 64 B", text, True)):
        buf = np.frombuffer(body, np.uint8)
        ids = np.empty(len(body), np.int32)
        k = i64(0)
        pt, pi, n = buf.ctypes.data, ids.ctypes.data, len(body)
        call = (lambda: L.tkz_encode_special_utf8(h, pt, n, allowed, len(SPECIALS), pi, n, C.byref(k))) if special else (lambda: L.tkz_encode_utf8(h, pt, n, pi, n, C.byref(k)))
        for _ in range(args.warmup):
            R.check(call())
        ts = []
        clk = time.perf_counter_ns
        for _ in range(args.calls):
            t0 = clk(); call(); ts.append(clk() - t0)
        out[case] = SP.median_us(ts)
    print(json.dumps(out), flush=True)


def still_beside_parent(args):
    runs = {"parent": [], "new": []}
    new_lib = args.lib or os.path.join(ROOT, "tokenizer_amd", "lib", "libtkz.so")
    for r in range(args.runs):
        for which, path in (("parent", args.parent_lib), ("new", new_lib)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--still-child", "--lib", path, "--calls", str(args.calls), "--warmup", str(args.warmup)],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise SystemExit("small_trim_probe: the child for %s ended with %d\n%s" % (path, out.returncode, out.stderr[-2000:]))
            runs[which].append(json.loads(out.stdout.strip().splitlines()[-1]))
    res = {"what": "tkz_encode_utf8 / tkz_encode_special_utf8 on 64 bytes, median us per call in alternating child processes", "runs": args.runs}
    for case in ("plain 64 B", "special 64 B"):
        p = [x[case] for x in runs["parent"]]
        n = [x[case] for x in runs["new"]]
        res[case] = {"parent_runs_us": p, "new_runs_us": n, "parent_median_us": statistics.median(p), "new_median_us": statistics.median(n),
                     "difference_us": round(statistics.median(n) - statistics.median(p), 2), "parent_spread_us": round(max(p) - min(p), 2)}
    print(json.dumps(res), flush=True)
    return res


def write_readme(out_dir, rows, still, resources, crossover=None, notes=()):
    in_parent = rows[0]["b_in_parent_library"]
    lines = ["# EncodeTrimSuffix / EncodeTrimPrefix for one string: the single launch beside the route it replaces", "",
             "Written by `tools/small_trim_probe.py` on an MI355X; the raw lines are in `raw.jsonl`.  A host clock around calls that end in the entry's own",
             "synchronisation, the three routes alternating in one loop after %d warm-up calls of each (%d for the 128 KiB text), the median of %d calls" % (rows[0]["warmup"], rows[-1]["warmup"], rows[0]["calls"]),
             "(p10 .. p90 in brackets), microseconds.  The maximum is a quarter of the text's token count, or one above the count (the text is kept whole).", "",
             "- (a) `tkz_encode_trim_utf8`: the new entry, one `k_small<SPECIAL, true>` launch",
             "- (b) `tkz_encode_batch_trim_utf8` with one document: the route the parent commit takes for the same text, " +
             ("in a `libtkz.so` built from the parent's sources and loaded beside this one" if in_parent else "IN THIS LIBRARY (no parent library was given: the parent's own was not measured)"),
             "- (c) `tkz_encode_special_utf8` on the same text: the same launch without the cut phase; a - c is what the cut adds", "",
             "| vocabulary, pattern | input | tokens | side | maximum | kept | (a) us | (b) us | (c) us | a/b | a - c us |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    f = lambda s: "%.1f [%.1f .. %.1f]" % (s["median_us"], s["p10_us"], s["p90_us"])
    for r in rows:
        lines.append("| %s, %s | %s | %d | %s | %s (%d) | %d | %s | %s | %s | %.3f | %+.1f |" % (
            r["vocab"], r["pattern"], r["input"] + ("" if r["a_route"] == "launch" else " (batch path)"), r["tokens"], r["side"], r["max_name"], r["max"], r["kept"], f(r["a_new_entry"]), f(r["b_batch_trim_one_document"]),
            f(r["c_special_single_call"]), r["a_over_b"], r["a_minus_c_us"]))
    worst = max(rows, key=lambda r: r["a_over_b"])
    lines += ["", "Verdict: the largest a/b over all rows is %.3f (%s, %s, %s, %s).  %s" % (
        worst["a_over_b"], worst["vocab"], worst["input"], worst["side"], worst["max_name"],
        "The new entry is faster than the route it replaces at every measured size." if worst["a_over_b"] < 1 else
        "Where the entry takes the launch it is faster than the route it replaces (largest a/b there: %.3f); a row marked (batch path) IS that route -- the entry hands texts of that size to the batch trim entry of this library -- and came out at a/b %.3f .. %.3f beside the parent's library." % (
            max([r["a_over_b"] for r in rows if r["a_route"] == "launch"] or [0]), min([r["a_over_b"] for r in rows if r["a_route"] != "launch"] or [0]), max([r["a_over_b"] for r in rows if r["a_route"] != "launch"] or [0])))]
    if crossover:
        cross = [json.loads(l) for l in open(crossover) if l.strip()]
        lines += ["", "## Where the launch stops paying: plain text of growing size", "",
                  "The same three routes on plain text (`--plain-sizes`), measured with a development build whose trim entry takes the launch up to 128 KiB",
                  "(`--lib`, built with `-DTKZ_SMALL_TRIM_MAX_BYTES=131072`); this is what the entry's size limit for the launch (`kSmallTrimMaxBytes`, tkz_kernels.h)",
                  "was chosen from.", "",
                  "| vocabulary, pattern | input | tokens | side | maximum | (a) us | (b) us | (c) us | a/b |", "|---|---|---|---|---|---|---|---|---|"]
        for r in cross:
            lines.append("| %s, %s | %s | %d | %s | %s (%d) | %s | %s | %s | %.3f |" % (r["vocab"], r["pattern"], r["input"], r["tokens"], r["side"], r["max_name"], r["max"],
                                                                                 f(r["a_new_entry"]), f(r["b_batch_trim_one_document"]), f(r["c_special_single_call"]), r["a_over_b"]))
    lines += ["", "## Phase stamps of the trim launch", "",
              "Shader-clock ticks between the stamps of `tkz_encoder_small_path_phases` for one call of (a) after the timed loop, suffix at a quarter of the count.", "",
              "| vocabulary, input | kernel | " + " | ".join(PHASES) + " |", "|---|---|" + "---|" * len(PHASES)]
    for r in rows:
        if r["side"] == "suffix" and r["max_name"] == "a quarter" and r["a_route"] == "launch":
            k = max(1, r["kernel_ticks"])
            lines.append("| %s, %s | %d | " % (r["vocab"], r["input"], r["kernel_ticks"]) + " | ".join("%d (%d%%)" % (r["phase_ticks"][p], round(100.0 * r["phase_ticks"][p] / k)) for p in PHASES) + " |")
    lines += ["", "## What must not move: the plain and the special single call beside the parent commit", ""]
    if still:
        lines += ["`tkz_encode_utf8` and `tkz_encode_special_utf8` on the 64-byte text through the parent's `libtkz.so` and through this one, %d child processes of each," % still["runs"],
                  "alternating; per process the median of the calls, microseconds.  The difference is this tree's median of medians minus the parent's; the spread is the",
                  "parent's largest run minus its smallest.  A difference inside the spread passes.", "",
                  "| case | parent runs | this tree's runs | difference | parent's spread | verdict |", "|---|---|---|---|---|---|"]
        for case in ("plain 64 B", "special 64 B"):
            c = still[case]
            lines.append("| %s | %s | %s | %+.2f | %.2f | %s |" % (case, ", ".join("%.1f" % x for x in c["parent_runs_us"]), ", ".join("%.1f" % x for x in c["new_runs_us"]), c["difference_us"],
                                                                c["parent_spread_us"], "inside" if abs(c["difference_us"]) <= c["parent_spread_us"] else "OUTSIDE"))
    else:
        lines.append("Not measured in this run (no --parent-lib).")
    lines += ["", "## The compiler's resource report for `k_small`, parent commit beside this tree", ""]
    lines += (["```"] + open(resources).read().rstrip("\n").splitlines() + ["```"]) if resources else ["Not recorded in this run (no --resources)."]
    lines += ["", "## What this run obtained", "",
              "- (a), (c) and the phase stamps: measured.",
              "- (b) in the parent commit's library: %s." % ("measured" if in_parent else "NOT obtained (measured in this tree's library instead)"),
              "- the plain and the special single call beside the parent's library: %s." % ("measured" if still else "NOT obtained"),
              "- the crossover scan: %s." % ("an earlier run's, tabulated above" if crossover else "NOT obtained"),
              "- the resource report: %s." % ("cross-compiled for gfx950 on a machine without a GPU, quoted above" if resources else "NOT obtained"),
              "- not measured by anyone: the o200k patterns (their launch ends at 1 KiB), the UTF-16 entry (the same launch behind a host transcode) and the mirrors."]
    lines += ["- " + n for n in notes]
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
    ap.add_argument("--resources", default=None)
    ap.add_argument("--plain-sizes", default=None, help="the crossover scan: plain text of these sizes (bytes, comma-separated) in place of the four texts; writes crossover.jsonl only")
    ap.add_argument("--note", action="append", default=[], help="a line for the README's closing section (may be given several times)")
    ap.add_argument("--crossover-file", default=None, help="a crossover.jsonl of an earlier run, tabulated in the README")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_trim"))
    ap.add_argument("--still-child", action="store_true")
    ap.add_argument("--from-raw", default=None, help="write the README again from a raw.jsonl of an earlier run (no GPU needed)")
    args = ap.parse_args()
    if args.from_raw:
        recs = [json.loads(l) for l in open(args.from_raw) if l.strip()]
        rows, still = [r for r in recs if "input" in r], ([r for r in recs if "input" not in r] or [None])[0]
        os.makedirs(args.out, exist_ok=True)
        return write_readme(args.out, rows, still, args.resources, args.crossover_file, args.note)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("small_trim_probe: no GPU (a timing taken elsewhere says nothing)")
    if args.still_child:
        return still_child(args)
    if args.calls < 2000:
        raise SystemExit("small_trim_probe: the medians are of at least 2,000 calls")
    from tokenizer_amd import _native as N
    os.makedirs(args.out, exist_ok=True)
    args.plain_sizes = [int(x) for x in args.plain_sizes.split(",")] if args.plain_sizes else None
    if args.plain_sizes:
        rows = time_routes(args, "gpt2", N.P1, "pattern 1") + time_routes(args, "synth100k", N.CL100K, "cl100k")
        with open(os.path.join(args.out, "crossover.jsonl"), "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
        return
    rows = time_routes(args, "gpt2", N.P1, "pattern 1") + time_routes(args, "synth100k", N.CL100K, "cl100k")
    still = still_beside_parent(args) if args.parent_lib else None
    with open(os.path.join(args.out, "raw.jsonl"), "w") as fh:
        for r in rows + ([still] if still else []):
            fh.write(json.dumps(r) + "\n")
    write_readme(args.out, rows, still, args.resources, args.crossover_file, args.note)


if __name__ == "__main__":
    main()
