#!/usr/bin/env python3
"""What the overlap costs beside the chunk entry.  One process, one RESERVED encoder per batch, the memo warmed by --warmup calls of every shape, then --steps rounds
of the device calls in turn, device events around each call, medians with min and max:
  (a) tkz_encode_batch_chunks_device at every budget N of --budgets, with chunk_bytes and chunk_units: the existing entry.  With --existing-only nothing else runs
      and nothing of this commit is needed, so the same file measures the parent commit's library (python tools/chunks_overlap_probe.py --existing-only from the
      parent's tree): the entry must not have moved, the margin being the parent's own min-max spread;
  (b) tkz_encode_batch_chunks_overlap_device at overlap 0 with all four position arrays: the existing work plus the chunk_ends store and the end positions;
  (c) the same at overlap N / 8 and N / 2: about N / (N - overlap) times as many chunks -- the time per chunk stands beside (b)'s.
Batches: `headline`, `mixed`, `real` and `one` as tools/chunks_probe.py makes them (`one`: ONE document of --one-mb, the long-document walk; its budgets are
--one-budget and --one-overlap).  The ids and offsets of every timed overlap call are compared with the existing entry's, and at overlap 0 the starts as well.
Prints one JSON line per batch (and appends them to --out).
usage: python tools/chunks_overlap_probe.py [--shapes headline,mixed,real,one] [--budgets 64,512] [--steps 20] [--warmup 3] [--existing-only] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chunks_probe as CP      # noqa: E402  (the batches and the summary are that probe's)


def device_shape(args, name, N, torch, vocab_name, pattern, d_bytes, d_offs, n_docs, total, pairs):
    dev = d_bytes.device
    stream = torch.cuda.current_stream().cuda_stream
    enc = N.Encoder(N.Vocab(CP.vocab_bytes(vocab_name)), pattern, device=0)
    enc.reserve(total, n_docs)
    bp, op = d_bytes.data_ptr(), d_offs.data_ptr()
    d_ids = torch.empty(total, dtype=torch.int32, device=dev)
    o_a = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    tokens = enc.encode_batch_device(bp, op, n_docs, total, d_ids.data_ptr(), total, o_a.data_ptr(), stream)
    ids_a = d_ids[:tokens].clone()
    del d_ids
    cap = tokens
    bound = lambda b, o: n_docs + 2 * tokens // max(1, b - o)      # (tokens, not bytes: the bound of tkz.h with the count known)
    ccap = min(tokens, max(bound(b, o) for b, o in pairs)) + 1
    ids = torch.empty(cap, dtype=torch.int32, device=dev)
    o_x = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    dco = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    ct, ce, cb, cu, ceb, ceu = (torch.empty(ccap + 1, dtype=torch.int64, device=dev) for _ in range(6))
    ct0 = {b: torch.empty(ccap + 1, dtype=torch.int64, device=dev) for b in {b for b, _ in pairs}}      # the existing entry's starts, budget by budget
    chunks = {}

    def existing(budget):
        def call():
            n, c = enc.encode_batch_chunks_device(bp, op, n_docs, total, budget, [], ids.data_ptr(), cap, o_x.data_ptr(), dco.data_ptr(), ct0[budget].data_ptr(), cb.data_ptr(),
                                                  cu.data_ptr(), ccap, stream)
            chunks["a_chunks_%d" % budget] = c
            return n
        return call

    def overlap(budget, ov):
        def call():
            n, c = enc.encode_batch_chunks_overlap_device(bp, op, n_docs, total, budget, ov, [], ids.data_ptr(), cap, o_x.data_ptr(), dco.data_ptr(), ct.data_ptr(),
                                                          ce.data_ptr(), cb.data_ptr(), cu.data_ptr(), ceb.data_ptr(), ceu.data_ptr(), ccap, stream)
            chunks["overlap_%d_%d" % (budget, ov)] = c
            return n
        return call
    budgets = sorted({b for b, _ in pairs})
    calls = [("a_chunks_%d" % b, existing(b)) for b in budgets]
    if not args.existing_only:
        calls += [("overlap_%d_%d" % (b, o), overlap(b, o)) for b, o in pairs]
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
            same = same and n == tokens and bool(torch.equal(ids[:tokens], ids_a)) and bool(torch.equal(o_x, o_a))
            if k.startswith("overlap_") and k.endswith("_0"):        # overlap 0: the starts of the existing entry (left in ct0 by this round's (a) calls)
                c, old = chunks[k], ct0[int(k.split("_")[1])]
                same = same and c == chunks["a_chunks_" + k.split("_")[1]] and bool(torch.equal(ct[:c], old[:c])) and bool(torch.equal(ce[:c], old[1:c + 1]))
    ms = CP.summary(series)
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "bytes": total, "tokens": tokens, "unit": "ms by device events",
           "steps": args.steps, "ms": ms, "results_equal_to_the_existing_entries": same, "chunks": chunks,
           "ns_per_chunk": {k: round(1e6 * ms[k][0] / max(1, chunks[k]), 2) for k in ms}, "workspace_bytes": enc.workspace_bytes}
    for k in ms:
        if k.startswith("a_"):
            row[k + "_spread_ms"] = round(ms[k][2] - ms[k][1], 4)
        else:
            row[k + "_minus_existing_ms"] = round(ms[k][0] - ms["a_chunks_" + k.split("_")[1]][0], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,mixed,real,one")
    ap.add_argument("--budgets", default="64,512")
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mixed-docs", type=int, default=2_000_000)
    ap.add_argument("--real-mb", type=int, default=256)
    ap.add_argument("--one-mb", type=int, default=16)
    ap.add_argument("--one-budget", type=int, default=512)
    ap.add_argument("--one-overlap", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    budgets = [int(b) for b in args.budgets.split(",")]
    pairs = [(b, o) for b in budgets for o in sorted({0, b // 8, b // 2})]
    import numpy as np
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("chunks_overlap_probe: no GPU (a timing taken elsewhere says nothing)")
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
            d_bytes, d_offs, total = CP.synthetic(N, torch, kind, n_docs)
            emit(device_shape(args, shape, N, torch, "synth100k", N.CL100K, d_bytes, d_offs, n_docs, total, pairs))
        elif shape == "one":                                 # (the kind-1 text with its document boundaries taken out: ONE document)
            d_bytes, d_offs, total = CP.synthetic(N, torch, 1, (args.one_mb << 20) // 512)
            one = torch.tensor([0, total], dtype=torch.int64, device=dev)
            emit(device_shape(args, "one_document", N, torch, "synth100k", N.CL100K, d_bytes, one, 1, total, [(args.one_budget, 0), (args.one_budget, args.one_overlap)]))
        elif shape == "real":
            import bench
            r_bytes, r_offs, meta = bench.real_text_corpus(args.real_mb << 20, 256, 768)
            total, n_docs = int(r_offs[-1]), len(r_offs) - 1
            padded = np.zeros(total + 64, np.uint8); padded[:total] = r_bytes[:total]
            emit(device_shape(args, shape, N, torch, "gpt2", N.P1, torch.from_numpy(padded).to(dev), torch.from_numpy(np.ascontiguousarray(r_offs, np.int64)).to(dev), n_docs,
                              total, pairs))
        else:
            raise SystemExit("chunks_overlap_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
