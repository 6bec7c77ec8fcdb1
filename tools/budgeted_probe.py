#!/usr/bin/env python3
"""What the budgeted entry costs beside the encode entry and the bucketed entry it extends.  One process, one RESERVED encoder per batch, the memo warmed by
--warmup calls of every shape, then --steps rounds of the device calls in turn, device events around each call:
  (a)        tkz_encode_batch_device;
  (d1024)    tkz_encode_batch_bucketed_device with an eos id, ids + mask, suffix cut, right padding, L = 512, M = 8, B = 1024, ascending, with rank -- THE
             YARDSTICK for the writer: k_tbk_write is k_bkt_write's loop, so its stage per byte of the rule must be no slower than this one's;
  (t512k)    tkz_encode_batch_budgeted_device with the same arguments, T = 1024 * 512, no row cap, ascending;
  (t512kd)   the same, descending;
  (tL)       T = L: a row or a few a bucket -- as many buckets as the batch can have;
  (t64L)     T = 64 L: a factor 64 fewer.  THE YARDSTICK for the chain: k_tbk_chain walks the runs, so its time must not differ between (tL) and (t64L); the call
             times differ by the table and the writer, the kernel trace (`trace`, `traceL`, `trace64L`) shows the chain alone.
The bytes a stage moves come from the rule, not from a counter: 4 read per KEPT id, 5 written (ids + mask) per output position P.
THE VERDICT of a batch: the budgeted stage meets the writer's yardstick when its rate, bytes / ((t512k) - (a)), is no lower than the bucketed stage's,
bytes / ((d1024) - (a)), less the min-max spread of (d1024) in this run -- the runs, the chain and the table are INSIDE (t512k) - (a).
Batches: `headline`, `mixed`, `real` as tools/padded_probe.py.  `trace` / `traceL` / `trace64L` / `traceB`: the headline batch's (t512k) / (tL) / (t64L) / (d1024)
alone, --trace-steps times, for a kernel trace taken around this process.
Prints one JSON line per batch (and appends them to --out).
usage: python tools/budgeted_probe.py [--shapes headline,mixed,real] [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import padded_probe as PP      # noqa: E402  (the batches and the summary are that probe's)

EOS, L, M = 2, 512, 8
NONE = (1 << 31) - 1
BUDGETED = {"t512k": (1024 * 512, 0), "t512kd": (1024 * 512, 1), "tL": (L, 0), "t64L": (64 * L, 0)}      # key: (token_budget, order)
TRACES = {"trace": "t512k", "traceL": "tL", "trace64L": "t64L", "traceB": "d1024"}


def verdict(row):
    m = {k: v[0] for k, v in row["ms"].items()}
    spread = round(row["ms"]["d1024"][2] - row["ms"]["d1024"][1], 4)
    row["spread_of_the_bucketed_call_ms"] = spread
    row["stage_ms"] = {k: round(m[k] - m["a_encode"], 4) for k in m if k != "a_encode"}
    row["stage_GBps"] = {k: round(row["stage_bytes"][k] / v / 1e6, 1) if v > 0 else None for k, v in row["stage_ms"].items()}
    rate_d = row["stage_bytes"]["d1024"] / row["stage_ms"]["d1024"] / 1e6 if row["stage_ms"]["d1024"] > 0 else float("inf")
    row["allowance_ms"] = {k: round(row["stage_bytes"][k] / rate_d / 1e6 + spread, 4) for k in BUDGETED}
    row["meets_the_writer_yardstick"] = {k: row["stage_ms"][k] <= row["allowance_ms"][k] for k in BUDGETED}
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
    boffs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)      # (n_docs buckets always suffice)
    brows = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    widths = torch.empty(max(1, n_docs), dtype=torch.int32, device=dev)
    o_x = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    tokens = enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)
    figures, nbytes = {}, {}

    def bucketed():
        figures["d1024"] = enc.encode_batch_bucketed_device(bp, op, n_docs, total, [], -1, EOS, L, 0, 0, 0, M, 1024, 0, ids.data_ptr(), cap, mask.data_ptr(), 0, lens.data_ptr(), 0,
                                                            order.data_ptr(), rank.data_ptr(), boffs.data_ptr(), widths.data_ptr(), stream)
        return figures["d1024"][0]

    def budgeted(key):
        T, direction = BUDGETED[key]

        def call():
            figures[key] = enc.encode_batch_budgeted_device(bp, op, n_docs, total, [], -1, EOS, L, 0, 0, 0, M, T, NONE, direction, ids.data_ptr(), cap, mask.data_ptr(), 0,
                                                            lens.data_ptr(), 0, order.data_ptr(), rank.data_ptr(), boffs.data_ptr(), brows.data_ptr(), widths.data_ptr(), n_docs, stream)
            return figures[key][0]
        return call
    calls = [("a_encode", lambda: enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)), ("d1024", bucketed)]
    calls += [(k, budgeted(k)) for k in BUDGETED]
    if only:
        calls = [c for c in calls if c[0] == only]
        for _ in range(args.warmup + args.trace_steps):
            calls[0][1]()
        torch.cuda.synchronize()
        return {"shape": name, "entry": "device", "traced": only, "calls": args.warmup + args.trace_steps, "figures": list(figures[only])}
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
            if k not in nbytes and k != "a_encode":            # (the kept ids from lens: every row holds one eos id)
                kept = int(lens[:n_docs].sum(dtype=torch.int64).item()) - n_docs
                nbytes[k] = 4 * kept + 5 * figures[k][1]
    # the budgeted call's buckets hold what they promise: rows * width <= T, and with T = 1024 * 512 they are the rows of the bucketed call's order
    nb = figures["t64L"][3]
    r, w = brows[:nb + 1], widths[:nb].to(torch.int64)
    fits = bool((((r[1:] - r[:-1]) * w) <= 64 * L).all().item()) and int(r[nb].item()) == n_docs
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "bytes": total, "tokens": tokens, "L": L, "M": M,
           "unit": "ms by device events: median, min, max", "steps": args.steps, "ms": PP.summary(series), "every_call_returned_its_total": same,
           "every_bucket_of_t64L_within_its_budget": fits, "figures (total, P, n_cut[, n_buckets])": {k: list(v) for k, v in figures.items()},
           "positions": {k: figures[k][1] for k in figures}, "buckets": dict({"d1024": N.Encoder.bucket_count(n_docs, 1024)}, **{k: figures[k][3] for k in BUDGETED}),
           "stage_bytes": nbytes, "budgeted_calls": enc.budgeted_calls(), "workspace_bytes": enc.workspace_bytes}
    return verdict(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,mixed,real")
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mixed-docs", type=int, default=2_000_000)
    ap.add_argument("--real-mb", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--trace-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("budgeted_probe: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for shape in args.shapes.split(","):
        if shape in ("headline", "mixed") or shape in TRACES:
            kind, n_docs = (2, args.mixed_docs) if shape == "mixed" else (1, args.docs)
            d_bytes, d_offs, total = PP.synthetic(N, torch, kind, n_docs)
            emit(device_shape(args, shape, N, torch, "synth100k", N.CL100K, d_bytes, d_offs, n_docs, total, only=TRACES.get(shape)))
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
            raise SystemExit("budgeted_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
