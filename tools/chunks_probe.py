#!/usr/bin/env python3
"""What the chunk entry costs beside the trim entry.  One process, one RESERVED encoder per batch, the memo warmed by --warmup calls of every shape, then --steps
rounds of the device calls in turn, device events around each call:
  (a) tkz_encode_batch_device;
  (b) tkz_encode_batch_trim_device, suffix, with a maximum no document reaches -- the same piece-granular launch sequence, then cut + scan + gather of every id:
      THE YARDSTICK;
  (c) tkz_encode_batch_chunks_device at every budget of --budgets, with chunk_bytes and chunk_units;
  (d) the same at the first budget with both position arrays NULL (chunk_tokens only: no unit counts, no second look at the text).
Batches: `headline` (bench.py's headline batch: --docs synthetic kind-1 documents of 256..768 bytes, cl100k, synth100k), `mixed` (kind 2, --mixed-docs), `real`
(text files of the machine as bench.py's kind 6 reads them, --real-mb, pattern 1, gpt2), `one` (ONE document of --one-mb of the kind-1 text: the long-document
walk).  Then, in a pass of its own with profiling on, the K_DOCOFFS bracket of (b), (c) and (d) -- k_docoffs alone in (b), k_docoffs + the chunk stage in (c) and
(d): the difference is the stage by the library's own events.  `host`: tkz_encode_batch_trim_utf8 against tkz_encode_batch_chunks_utf8 on --host-mb of the kind-1
text in page-locked buffers, a host clock around calls that end synchronised.  The ids and offsets of every timed chunk call are compared with (a)'s.
Prints one JSON line per batch (and appends them to --out).
usage: python tools/chunks_probe.py [--shapes headline,mixed,real,one,host] [--budgets 64,512] [--steps 20] [--warmup 3] [--out FILE]"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HUGE = 1 << 40


def vocab_bytes(name):
    return gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".tiktoken.gz"), "rb").read())


def summary(series):
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in series.items()}


def verdict(row, base="b_trim"):
    m = {k: v[0] for k, v in row["ms"].items()}
    row["spread_of_the_trim_call_ms"] = round(row["ms"][base][2] - row["ms"][base][1], 4)
    for k in m:
        if k.startswith(("c_", "d_", "chunks")):
            row[k + "_minus_" + base] = round(m[k] - m[base], 4)
    return row


def device_shape(args, name, N, torch, vocab_name, pattern, d_bytes, d_offs, n_docs, total):
    dev = d_bytes.device
    stream = torch.cuda.current_stream().cuda_stream
    enc = N.Encoder(N.Vocab(vocab_bytes(vocab_name)), pattern, device=0)
    enc.reserve(total, n_docs)
    bp, op = d_bytes.data_ptr(), d_offs.data_ptr()
    d_ids = torch.empty(total, dtype=torch.int32, device=dev)
    o_a = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    tokens = enc.encode_batch_device(bp, op, n_docs, total, d_ids.data_ptr(), total, o_a.data_ptr(), stream)
    ids_a = d_ids[:tokens].clone()
    del d_ids
    cap = tokens
    ccap = max(N.Encoder.chunk_bound(n_docs, tokens, b) for b in args.budgets)      # (tokens, not bytes: the bound of tkz.h with the count known)
    ids = torch.empty(cap, dtype=torch.int32, device=dev)
    o_x = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    dco = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    ct, cb, cu = (torch.empty(ccap + 1, dtype=torch.int64, device=dev) for _ in range(3))
    chunks = {}

    def chunk_call(budget, positions):
        def call():
            n, c = enc.encode_batch_chunks_device(bp, op, n_docs, total, budget, [], ids.data_ptr(), cap, o_x.data_ptr(), dco.data_ptr(), ct.data_ptr(),
                                                  cb.data_ptr() if positions else 0, cu.data_ptr() if positions else 0, ccap, stream)
            chunks[budget] = c
            return n
        return call
    calls = [("a_encode", lambda: enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)),
             ("b_trim", lambda: enc.encode_batch_trim_device(bp, op, n_docs, total, [], N.TRIM_SUFFIX, HUGE, 0, ids.data_ptr(), cap, o_x.data_ptr(), 0, 0, stream))]
    calls += [("c_chunks_%d" % b, chunk_call(b, True)) for b in args.budgets]
    calls += [("d_chunks_%d_tokens_only" % args.budgets[0], chunk_call(args.budgets[0], False))]
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    series = {k: [] for k, _ in calls}
    same = True
    for _ in range(args.steps):
        for k, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            n = fn()
            e1.record()
            e1.synchronize()
            series[k].append(e0.elapsed_time(e1))
            same = same and n == tokens
            if k.startswith(("c_", "d_")):
                same = same and bool(torch.equal(ids[:tokens], ids_a)) and bool(torch.equal(o_x, o_a))
    # the brackets, in passes of their own (profiling serialises the launch sequence around its events)
    enc.set_profiling(True)
    brackets = {}
    for k, fn in calls:
        enc.kernel_ms(reset=True)
        for _ in range(args.profile_steps):
            fn()
        km = enc.kernel_ms(reset=True)
        brackets[k] = {q: round(km[q][0] / max(1, km[q][1]), 4) for q in ("k_place", "k_docoffs") if q in km}
    enc.set_profiling(False)
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "bytes": total, "tokens": tokens, "unit": "ms by device events",
           "steps": args.steps, "ms": summary(series), "ids_and_offsets_equal_to_the_encode_entry": same, "chunks": {str(b): c for b, c in chunks.items()},
           "brackets_ms_per_call": brackets, "chunk_calls": enc.chunks_calls(), "workspace_bytes": enc.workspace_bytes}
    if all("k_docoffs" in brackets[k] for k in brackets):
        row["chunk_stage_by_the_bracket_ms"] = {k: round(brackets[k]["k_docoffs"] - brackets["b_trim"]["k_docoffs"], 4) for k in brackets if k.startswith(("c_", "d_"))}
    return verdict(row)


def synthetic(N, torch, kind, n_docs, min_len=256, max_len=768):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    seed = 0x5EED0000 + {1: 2, 2: 3}[kind]
    d_offs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    total = N.corpus_generate_device(0, kind, seed, 0, n_docs, min_len, max_len, d_offs.data_ptr(), None, 0, stream)
    d_bytes = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    N.corpus_generate_device(0, kind, seed, 0, n_docs, min_len, max_len, d_offs.data_ptr(), d_bytes.data_ptr(), total, stream)
    torch.cuda.synchronize()
    return d_bytes, d_offs, total


def host_shape(args, N, torch, np):
    import ctypes as C
    n_docs = (args.host_mb << 20) // 512
    d_bytes, d_offs, total = synthetic(N, torch, 1, n_docs)
    text, offs = d_bytes[:total].cpu().numpy(), d_offs.cpu().numpy()
    del d_bytes, d_offs
    torch.cuda.empty_cache()
    pin = lambda n, dt: torch.empty(n, dtype=dt).pin_memory().numpy()
    h_text, h_offs = pin(total + 64, torch.uint8), pin(n_docs + 1, torch.int64)
    h_text[:total] = text; h_offs[:] = offs
    enc = N.Encoder(N.Vocab(vocab_bytes("synth100k")), N.CL100K, device=0)
    L, need, nch = enc.lib.L, C.c_int64(0), C.c_int64(0)
    st = L.tkz_encode_batch_trim_utf8(enc._h, h_text.ctypes.data, h_offs.ctypes.data, n_docs, None, 0, N.TRIM_SUFFIX, HUGE, None, None, 0,
                                      pin(n_docs + 1, torch.int64).ctypes.data, None, None, C.byref(need))      # (no room for ids: the count)
    assert st in (N.OK, N.E_CAPACITY), st
    cap = need.value
    ccap = max(N.Encoder.chunk_bound(n_docs, cap, b) for b in args.budgets)
    h_ids, o_b, o_c, h_dco = pin(cap, torch.int32), pin(n_docs + 1, torch.int64), pin(n_docs + 1, torch.int64), pin(n_docs + 1, torch.int64)
    h_ct, h_cb, h_cu = pin(ccap + 1, torch.int64), pin(ccap, torch.int64), pin(ccap, torch.int64)

    def trim():
        enc.lib.check(L.tkz_encode_batch_trim_utf8(enc._h, h_text.ctypes.data, h_offs.ctypes.data, n_docs, None, 0, N.TRIM_SUFFIX, HUGE, None, h_ids.ctypes.data, cap,
                                                   o_b.ctypes.data, None, None, C.byref(need)))
        return need.value

    def chunks(budget):
        def call():
            enc.lib.check(L.tkz_encode_batch_chunks_utf8(enc._h, h_text.ctypes.data, h_offs.ctypes.data, n_docs, None, 0, budget, h_ids.ctypes.data, cap, o_c.ctypes.data,
                                                         h_dco.ctypes.data, h_ct.ctypes.data, h_cb.ctypes.data, h_cu.ctypes.data, ccap, C.byref(need), C.byref(nch)))
            return need.value
        return call
    calls = [("b_trim", trim)] + [("chunks_%d" % b, chunks(b)) for b in args.budgets]
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    series = {k: [] for k, _ in calls}
    res = {}
    for _ in range(args.host_steps):
        for k, fn in calls:
            t0 = time.perf_counter()
            res[k] = fn()
            series[k].append((time.perf_counter() - t0) * 1e3)
    return verdict({"shape": "host_page_locked", "entry": "host", "vocab": "synth100k", "pattern": N.CL100K, "docs": n_docs, "bytes": total, "tokens": res["b_trim"],
                    "unit": "ms by a host clock", "steps": args.host_steps, "ms": summary(series),
                    "ids_and_offsets_equal_to_the_encode_entry": bool((o_b == o_c).all()) and all(v == res["b_trim"] for v in res.values()),
                    "workspace_bytes": enc.workspace_bytes})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,mixed,real,one,host")
    ap.add_argument("--budgets", default="64,512")
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mixed-docs", type=int, default=2_000_000)
    ap.add_argument("--real-mb", type=int, default=256)
    ap.add_argument("--one-mb", type=int, default=16)
    ap.add_argument("--host-mb", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=20)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.budgets = [int(b) for b in args.budgets.split(",")]
    import numpy as np
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("chunks_probe: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for shape in args.shapes.split(","):
        if shape in ("headline", "mixed"):
            kind, n_docs = (1, args.docs) if shape == "headline" else (2, args.mixed_docs)
            d_bytes, d_offs, total = synthetic(N, torch, kind, n_docs)
            emit(device_shape(args, shape, N, torch, "synth100k", N.CL100K, d_bytes, d_offs, n_docs, total))
        elif shape == "one":                                 # (the kind-1 text with its document boundaries taken out: ONE document)
            d_bytes, d_offs, total = synthetic(N, torch, 1, (args.one_mb << 20) // 512)
            one = torch.tensor([0, total], dtype=torch.int64, device=dev)
            emit(device_shape(args, "one_document", N, torch, "synth100k", N.CL100K, d_bytes, one, 1, total))
        elif shape == "real":
            import bench
            r_bytes, r_offs, meta = bench.real_text_corpus(args.real_mb << 20, 256, 768)
            total, n_docs = int(r_offs[-1]), len(r_offs) - 1
            padded = np.zeros(total + 64, np.uint8); padded[:total] = r_bytes[:total]
            row = device_shape(args, shape, N, torch, "gpt2", N.P1, torch.from_numpy(padded).to(dev), torch.from_numpy(np.ascontiguousarray(r_offs, np.int64)).to(dev), n_docs, total)
            row["text"] = {k: meta[k] for k in meta if k in ("files", "sha256", "roots")} if isinstance(meta, dict) else str(meta)[:200]
            emit(row)
        elif shape == "host":
            emit(host_shape(args, N, torch, np))
        else:
            raise SystemExit("chunks_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
