#!/usr/bin/env python3
"""What the bucketed entry costs beside the encode entry and the padded entry, and how its sort compares with the one independent sort on the machine.  One
process, one RESERVED encoder per batch, the memo warmed by --warmup calls of every shape, then --steps rounds of the device calls in turn, device events around
each call:
  (a)        tkz_encode_batch_device;
  (c)        tkz_encode_batch_padded_device with an eos id, ids + mask, suffix cut, right padding, L = 512, M = 8 -- THE YARDSTICK for the writer: its stage,
             (c) - (a), per byte it moves: the parent's code doing the same job without the indirection;
  (d1024a)   tkz_encode_batch_bucketed_device with the same arguments, B = 1024, ascending, with rank;
  (d1024d)   the same, descending;
  (dn)       B = n_docs: ONE bucket, the padded call's rows in sorted order;
  (d64)      B = 64;
  (sort)     torch.sort(lens, stable=True) on the lens tensor the bucketed call left on the same device (rocPRIM's radix sort) -- THE YARDSTICK for the sort.
The bytes a stage moves come from the rule, not from a counter: 4 read per KEPT id, 5 written (ids + mask) per output position: n_docs * W for (c), P for (d).
What the bucketed stage moves besides (24 bytes a document and pass in the sort, 20 a row in the writer: order, lens, src) is listed beside that figure, not in it.
THE VERDICT of a batch: a bucketed stage meets the writer's yardstick when (d) - (a) <= its bytes / the padded stage's rate + the min-max spread of (c) in this
run -- the sort and the table are INSIDE (d) - (a), so this holds the whole stage against the writer's allowance; the kernel trace (`trace`) splits it.
Batches: `headline`, `mixed`, `real` as tools/padded_probe.py.  `host`: tkz_encode_batch_bucketed_utf8 (B = 1024) beside tkz_encode_batch_padded_utf8 and
tkz_encode_batch_utf8 at L = 128 on --host-mb of the headline text in pageable memory, host clock, with the download sizes.  `trace`: the headline batch's
(d1024a) alone, --trace-steps times, for a kernel trace taken around this process.
Prints one JSON line per batch (and appends them to --out).
usage: python tools/bucketed_probe.py [--shapes headline,mixed,real,host] [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import padded_probe as PP      # noqa: E402  (the batches and the summary are that probe's)

EOS, L, M = 2, 512, 8
BUCKETED = {"d1024a": (1024, 0), "d1024d": (1024, 1), "dn": (None, 0), "d64": (64, 0)}      # key: (bucket_rows -- None: n_docs --, order)


def verdict(row):
    m = {k: v[0] for k, v in row["ms"].items()}
    spread = round(row["ms"]["c_padded"][2] - row["ms"]["c_padded"][1], 4)
    stage_c = m["c_padded"] - m["a_encode"]
    rate_c = row["stage_bytes"]["c_padded"] / stage_c / 1e6 if stage_c > 0 else float("inf")      # GB/s: bytes per ms / 1e6
    row["spread_of_the_padded_call_ms"] = spread
    row["stage_ms"] = {k: round(m[k] - m["a_encode"], 4) for k in m if k not in ("a_encode", "torch_sort")}
    row["stage_GBps"] = {k: round(row["stage_bytes"][k] / v / 1e6, 1) if v > 0 else None for k, v in row["stage_ms"].items()}
    row["allowance_ms"] = {k: round(row["stage_bytes"][k] / rate_c / 1e6 + spread, 4) for k in BUCKETED}
    row["meets_the_writer_yardstick"] = {k: row["stage_ms"][k] <= row["allowance_ms"][k] for k in BUCKETED}
    row["torch_sort_Mkeys_per_s"] = round(row["docs"] / m["torch_sort"] / 1e3, 1)
    return row


def device_shape(args, name, N, torch, vocab_name, pattern, d_bytes, d_offs, n_docs, total, only=None):
    dev = d_bytes.device
    stream = torch.cuda.current_stream().cuda_stream
    enc = N.Encoder(N.Vocab(PP.vocab_bytes(vocab_name)), pattern, device=0)
    enc.reserve(total, n_docs)
    bp, op = d_bytes.data_ptr(), d_offs.data_ptr()
    cap = max(total, n_docs * L)
    ids = torch.empty(cap, dtype=torch.int32, device=dev)
    mask = torch.empty(cap, dtype=torch.uint8, device=dev)
    lens = torch.empty(max(1, n_docs), dtype=torch.int32, device=dev)
    order = torch.empty(max(1, n_docs), dtype=torch.int64, device=dev)
    rank = torch.empty(max(1, n_docs), dtype=torch.int64, device=dev)
    nbmax = N.Encoder.bucket_count(n_docs, 64)
    boffs = torch.empty(nbmax + 1, dtype=torch.int64, device=dev)
    widths = torch.empty(max(1, nbmax), dtype=torch.int32, device=dev)
    o_x = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    tokens = enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)
    figures, nbytes = {}, {}

    def padded():
        figures["c_padded"] = enc.encode_batch_padded_device(bp, op, n_docs, total, [], -1, EOS, L, 0, 0, 0, M, ids.data_ptr(), cap, mask.data_ptr(), 0, lens.data_ptr(), 0, stream)
        return figures["c_padded"][0]

    def bucketed(key):
        B, direction = BUCKETED[key]
        B = B or n_docs

        def call():
            figures[key] = enc.encode_batch_bucketed_device(bp, op, n_docs, total, [], -1, EOS, L, 0, 0, 0, M, B, direction, ids.data_ptr(), cap, mask.data_ptr(), 0, lens.data_ptr(), 0,
                                                            order.data_ptr(), rank.data_ptr(), boffs.data_ptr(), widths.data_ptr(), stream)
            return figures[key][0]
        return call
    calls = [("a_encode", lambda: enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)), ("c_padded", padded)]
    calls += [(k, bucketed(k)) for k in BUCKETED]
    if only:
        calls = [c for c in calls if c[0] == only]
        for _ in range(args.warmup + args.trace_steps):
            calls[0][1]()
        torch.cuda.synchronize()
        return {"shape": name, "entry": "device", "traced": only, "calls": args.warmup + args.trace_steps, "figures": list(figures[only])}
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
        torch.sort(lens[:n_docs], stable=True)
    series = {k: [] for k, _ in calls}
    series["torch_sort"] = []
    same, sorted_alike = True, True
    for _ in range(args.steps):
        for k, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            n = fn()
            e1.record()
            e1.synchronize()
            series[k].append(e0.elapsed_time(e1))
            same = same and n == tokens
            if k not in nbytes and k != "a_encode":            # (the kept ids from lens: every row holds one eos id)
                kept = int(lens[:n_docs].sum(dtype=torch.int64).item()) - n_docs
                positions = n_docs * figures[k][1] if k == "c_padded" else figures[k][1]
                nbytes[k] = 4 * kept + 5 * positions
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ref = torch.sort(lens[:n_docs], stable=True)
        e1.record()
        e1.synchronize()
        series["torch_sort"].append(e0.elapsed_time(e1))
        sorted_alike = sorted_alike and bool((ref.indices == order[:n_docs]).all().item())      # (the last bucketed call of the round is ascending)
    W = figures["c_padded"][1]
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "bytes": total, "tokens": tokens, "L": L, "M": M,
           "unit": "ms by device events: median, min, max", "steps": args.steps, "ms": PP.summary(series), "every_call_returned_its_total": same,
           "order_equals_torch_stable_sort": sorted_alike, "figures": {k: list(v) for k, v in figures.items()},
           "positions": dict({"c_padded n_docs * W": n_docs * W}, **{k: figures[k][1] for k in BUCKETED}), "stage_bytes": nbytes,
           "sort_bytes_a_pass": 24 * n_docs, "sort_passes": 2, "row_bytes_of_the_writer": 20 * n_docs, "bucketed_calls": enc.bucketed_calls(), "workspace_bytes": enc.workspace_bytes}
    return verdict(row)


def host_shape(args, name, N, torch, np, d_bytes, d_offs, n_docs, total):
    """tkz_encode_batch_bucketed_utf8 (B = 1024) beside tkz_encode_batch_padded_utf8 and tkz_encode_batch_utf8 at L = 128 on the same text, pageable buffers, host clock"""
    offs = d_offs.cpu().numpy()
    n = max(1, min(int(np.searchsorted(offs, args.host_mb << 20, side="right")) - 1, n_docs))
    nb = int(offs[n])
    data = d_bytes[:nb].cpu().numpy().copy()
    offs = offs[:n + 1].copy()
    enc = N.Encoder(N.Vocab(PP.vocab_bytes("synth100k")), N.CL100K, device=0)
    series = {"encode_utf8": [], "padded_utf8_L128": [], "bucketed_utf8_L128_M8_B1024": []}
    figures = {}
    for step in range(args.warmup + args.host_steps):
        t0 = time.perf_counter()
        ids, ooff = enc.encode_batch(data, offs)
        t1 = time.perf_counter()
        r = enc.encode_batch_padded(data, offs, 128, (), -1, EOS, 0, pad_multiple=0, want_pos=False, want_offs=False)
        t2 = time.perf_counter()
        q = enc.encode_batch_bucketed(data, offs, 128, 1024, 0, (), -1, EOS, 0, pad_multiple=8, want_pos=False, want_offs=False)
        t3 = time.perf_counter()
        if step >= args.warmup:
            for k, v in zip(series, (t1 - t0, t2 - t1, t3 - t2)):
                series[k].append(v * 1e3)
        nbk = len(q[8])
        figures = {"tokens": int(len(ids)), "W": int(r[0].shape[1]), "P": int(len(q[0])), "n_cut": int(r[6]),
                   "download_bytes": {"encode_utf8": 4 * int(len(ids)) + 8 * (n + 1), "padded_utf8_L128": 5 * n * int(r[0].shape[1]) + 4 * n,
                                      "bucketed_utf8_L128_M8_B1024": 5 * int(len(q[0])) + 20 * n + 12 * nbk + 8}}
    return {"shape": name, "entry": "utf8, pageable", "docs": n, "bytes": nb, "unit": "ms by the host clock: median, min, max", "steps": args.host_steps, "ms": PP.summary(series), **figures}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,mixed,real,host")
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mixed-docs", type=int, default=2_000_000)
    ap.add_argument("--real-mb", type=int, default=256)
    ap.add_argument("--host-mb", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--trace-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("bucketed_probe: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for shape in args.shapes.split(","):
        if shape in ("headline", "mixed", "trace"):
            kind, n_docs = (2, args.mixed_docs) if shape == "mixed" else (1, args.docs)
            d_bytes, d_offs, total = PP.synthetic(N, torch, kind, n_docs)
            emit(device_shape(args, shape, N, torch, "synth100k", N.CL100K, d_bytes, d_offs, n_docs, total, only="d1024a" if shape == "trace" else None))
        elif shape == "host":
            n_docs = max(1, (args.host_mb << 20) // (512 - 12))      # (a little more text than asked for, cut to --host-mb)
            d_bytes, d_offs, total = PP.synthetic(N, torch, 1, n_docs, 256, 768)
            emit(host_shape(args, shape, N, torch, np, d_bytes, d_offs, n_docs, total))
        elif shape == "real":
            import bench
            r_bytes, r_offs, meta = bench.real_text_corpus(args.real_mb << 20, 256, 768)
            total, n_docs = int(r_offs[-1]), len(r_offs) - 1
            padded = np.zeros(total + 64, np.uint8)
            padded[:total] = r_bytes[:total]
            row = device_shape(args, shape, N, torch, "gpt2", N.P1, torch.from_numpy(padded).to(dev), torch.from_numpy(np.ascontiguousarray(r_offs, np.int64)).to(dev), n_docs, total)
            row["text"] = {k: meta[k] for k in meta if k in ("files", "sha256", "roots")} if isinstance(meta, dict) else str(meta)[:200]
            emit(row)
        else:
            raise SystemExit("bucketed_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
