#!/usr/bin/env python3
"""What Decode(int[]) of ONE id list costs through the single launch (tkz_decode_utf8 / tkz_decode_utf16: k_dec_small), beside the route it replaces.
gpt2 table; the ids of English-like text (the word filler of small_special_probe.py; --long-words: long words that are one token each, ~12 bytes an
id), the first 1, 16, 256, 4,096 and 32,768 of them (--sizes), in both output forms; per size the routes alternate in ONE loop after warm-up calls of all of
them, a host clock around calls that end in the entry's own synchronisation, median and p90 of --calls calls:
  (a) tkz_decode_utf8 / _utf16                                        the new entry (its route -- launch, hand-back, batch -- read from tkz_encoder_small_decode_calls)
  (b) tkz_decode_batch / _utf16 with one document, this library      the route the mirrors took: the parent commit's code, unchanged
  (p) the same in the PARENT's library (--parent-lib: a libtkz.so built from the parent commit's sources, loaded beside this one): the two batch figures should
      agree within run-to-run spread
and, for reference, tkz_encode_utf8 on a 64-byte prompt (the single-launch encode) in the same process.  (a) and (b) are compared item for item.  The phase
stamps of the last launch come from tkz_encoder_small_decode_phases.  Writes README.md and raw.jsonl into --out.
usage: python tools/small_decode_probe.py [--calls 400] [--warmup 100] [--sizes 1,16,256,4096,32768] [--long-words] [--parent-lib PATH] [--out profiles/small_decode]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import small_special_probe as SP  # noqa: E402  (the word filler, the library loader)
import small_trim_probe as TP  # noqa: E402  (RawLib: a parent library through ctypes alone)

PHASES8 = ["lengths", "scan", "bytes"]
PHASES16 = ["lengths", "scan", "bytes + bitmap", "unit counts", "unit scan", "units"]
LONG_WORDS = [" international", " government", " development", " information", " environment", " performance", " particularly", " organization"]
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


def spread(ns):
    q = statistics.quantiles(ns, n=10)
    return {"median_us": round(statistics.median(ns) / 1000.0, 2), "p90_us": round(q[-1] / 1000.0, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--sizes", default="1,16,256,4096,32768")
    ap.add_argument("--long-words", action="store_true", help="a text of long words that are single gpt2 tokens: ~12 bytes an id (a hand-back from 11,000 ids on)")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_decode"))
    args = ap.parse_args()
    import numpy as np
    N, lib, enc = SP.load(args.lib, "gpt2", 1)
    L, h = lib.L, enc._h
    old = TP.RawLib(args.parent_lib, "gpt2", 1) if args.parent_lib else None
    if old:
        old.L.tkz_decode_batch.argtypes = [vp, vp, vp, i64, vp, i64, vp, C.POINTER(i64)]
        old.L.tkz_decode_batch_utf16.argtypes = [vp, vp, vp, i64, vp, i64, vp, C.POINTER(i64)]
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.long_words:
        import random
        rng = random.Random(5)
        text = "".join(rng.choice(LONG_WORDS) for _ in range(max(sizes) + 8)).encode()
    else:
        text = SP.filler(6 * max(sizes) + 64, 5).encode()
    all_ids = np.asarray(enc.encode_utf8(text), np.int32)
    assert len(all_ids) >= max(sizes), "the text is too short for %d ids" % max(sizes)
    rows = []
    for n in sizes:
        ids = np.ascontiguousarray(all_ids[:n])
        offs = (i64 * 2)(0, n)
        ooff = (i64 * 2)(0, 0)
        for utf16 in (False, True):
            dt = np.uint16 if utf16 else np.uint8
            cap = 16 * n + 16
            out_a, out_b, out_p = np.zeros(cap, dt), np.zeros(cap, dt), np.zeros(cap, dt)
            na, nb, npar = i64(0), i64(0), i64(0)
            fa = L.tkz_decode_utf16 if utf16 else L.tkz_decode_utf8
            fb = L.tkz_decode_batch_utf16 if utf16 else L.tkz_decode_batch
            fp = (old.L.tkz_decode_batch_utf16 if utf16 else old.L.tkz_decode_batch) if old else None
            pi, pa, pb, pp = ids.ctypes.data, out_a.ctypes.data, out_b.ctypes.data, out_p.ctypes.data

            def a():
                return fa(h, pi, n, pa, cap, C.byref(na))

            def b():
                return fb(h, pi, offs, 1, pb, cap, ooff, C.byref(nb))

            def p():
                return fp(old.h, pi, offs, 1, pp, cap, ooff, C.byref(npar))
            routes = [a, b] + ([p] if old else [])
            warm = args.warmup if n <= 4096 else max(20, args.warmup // 4)
            for _ in range(warm):
                for f in routes:
                    st = f()
                    if st != 0:
                        raise SystemExit("small_decode_probe: status %d at %d ids" % (st, n))
            assert na.value == nb.value and np.array_equal(out_a[:na.value], out_b[:nb.value]), "the new entry and the batch entry disagree at %d ids" % n
            if old:
                assert npar.value == nb.value and np.array_equal(out_p[:npar.value], out_b[:nb.value])
            c0 = enc.small_decode_calls()
            lib.check(a())
            c1 = enc.small_decode_calls()
            route = {(1, 0): "launch", (1, 1): "hand-back", (0, 0): "batch"}[(c1[0] - c0[0], c1[1] - c0[1])]
            stamps = enc.small_decode_phases()
            times = [[] for _ in routes]
            for _ in range(args.calls):
                for k, f in enumerate(routes):
                    t0 = time.perf_counter_ns()
                    f()
                    times[k].append(time.perf_counter_ns() - t0)
            names = PHASES16 if utf16 else PHASES8
            ticks = [stamps[i + 1] - stamps[i] for i in range(len(names))] if route == "launch" else []
            row = {"ids": n, "form": "utf16" if utf16 else "utf8", "items": na.value, "route": route, "a": spread(times[0]), "b": spread(times[1]),
                   "p": spread(times[2]) if old else None, "phase_ticks": dict(zip(names, ticks)), "kernel_ticks": sum(ticks)}
            row["a_over_b"] = round(row["a"]["median_us"] / row["b"]["median_us"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    # the single-launch encode on a 64-byte prompt, same process
    prompt = np.frombuffer(SP.filler(64, 1).encode(), np.uint8)
    pids = np.zeros(64, np.int32)
    k = i64(0)
    te = []
    for r in range(args.warmup + args.calls):
        t0 = time.perf_counter_ns()
        lib.check(L.tkz_encode_utf8(h, prompt.ctypes.data, 64, pids.ctypes.data, 64, C.byref(k)))
        if r >= args.warmup:
            te.append(time.perf_counter_ns() - t0)
    enc_row = {"encode_64_bytes": spread(te)}
    print(json.dumps(enc_row), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "raw.jsonl"), "w") as f:
        for r in rows + [enc_row]:
            f.write(json.dumps(r) + "\n")
    lines = ["# Decode(int[]) of one id list: the single launch against the batch entry", "",
             "`tools/small_decode_probe.py --calls %d --warmup %d%s`, one MI355X, gpt2 table, the first n ids of English-like text%s; host clock, microseconds, median (p90)."
             % (args.calls, args.warmup, " --parent-lib PARENT/libtkz.so" if old else "", " (--long-words: long words of one token each)" if args.long_words else ""),
             "(a) `tkz_decode_utf8 / _utf16`; (b) `tkz_decode_batch / _utf16` with one document in this library; (p) the same in the parent commit's library.", "",
             "| ids | form | items | route of (a) | (a) | (b) | (p) | a / b |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        cell = lambda s: "%.1f (%.1f)" % (s["median_us"], s["p90_us"]) if s else "-"
        lines.append("| %d | %s | %d | %s | %s | %s | %s | %.2f |" % (r["ids"], r["form"], r["items"], r["route"], cell(r["a"]), cell(r["b"]), cell(r["p"]), r["a_over_b"]))
    lines += ["", "The single-launch encode (`tkz_encode_utf8`) on a 64-byte prompt in the same process: %.1f (%.1f)." % (enc_row["encode_64_bytes"]["median_us"], enc_row["encode_64_bytes"]["p90_us"]), "",
              "Phase clocks of the launch (shader-clock ticks, thread 0, `tkz_encoder_small_decode_phases`):", "",
              "| ids | form | kernel | phases |", "|---|---|---|---|"]
    for r in rows:
        if r["phase_ticks"]:
            lines.append("| %d | %s | %d | %s |" % (r["ids"], r["form"], r["kernel_ticks"], ", ".join("%s %d" % kv for kv in r["phase_ticks"].items())))
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
