#!/usr/bin/env python3
"""What the pair entry costs beside the encode entry, and how its stage compares with the padded stage on the same documents.  One process, one RESERVED encoder
per batch, the memo warmed by --warmup calls of every shape, then --steps rounds of the device calls in turn, device events around each call.  The batch's
documents are read as pairs: documents 2p and 2p + 1 are the two texts of pair p.
  (a)     tkz_encode_batch_device;
  (c)     tkz_encode_batch_padded_device on the same documents, an eos id, ids + mask, suffix cut, right padding, L = 128, M = 8 -- THE YARDSTICK: its stage,
          (c) - (a), per byte it moves;
  (p_lf)  tkz_encode_batch_pairs_device, a bos id, one separator, an eos id, ids + mask + types, suffix cut, right padding, L = 256, M = 8, LONGEST_FIRST;
  (p_of)  the same under ONLY_FIRST;
  (p_os)  the same under ONLY_SECOND;
  (p_all) (p_lf) with pos, kept and the offsets as well.
The bytes a stage moves come from the rule, not from a counter: 4 per KEPT id read (the sum of lens less the framing), and per output position 4 + 1 written by
the padded stage (ids + mask), 4 + 1 + 1 by the pair stage (ids + mask + types), 4 more with pos.  The bytes per document and per pair (offsets read; lens written,
the row's record of 24 bytes written and read again) are listed beside that figure, not in it.
THE VERDICT of a batch: a pair stage meets the yardstick when its rate, bytes / ((p) - (a)), is no lower than the padded stage's rate with the padded call's
min-max spread over the rounds taken off the stage's time -- that is, (p) - (a) <= its bytes / the padded stage's rate + that spread.
Batches: `headline` (bench.py's headline batch: --docs synthetic kind-1 documents of 256..768 bytes, cl100k, synth100k), `mixed` (kind 2, --mixed-docs), `real`
(text files of the machine as bench.py's kind 6 reads them, --real-mb, pattern 1, gpt2).
Prints one JSON line per batch (and appends them to --out).
usage: python tools/pairs_probe.py [--shapes headline,mixed,real] [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import gzip
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOS, SEP, EOS = 1, 3, 2
PAD_L, PAIR_L, M = 128, 256, 8
PAIRS = {"p_lf": (0, False), "p_of": (1, False), "p_os": (2, False), "p_all": (0, True)}      # key: (strategy, with pos / kept / offsets)


def vocab_bytes(name):
    return gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".tiktoken.gz"), "rb").read())


def summary(series):
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in series.items()}


def verdict(row):
    m = {k: v[0] for k, v in row["ms"].items()}
    spread = round(row["ms"]["c_padded"][2] - row["ms"]["c_padded"][1], 4)
    stage_c = m["c_padded"] - m["a_encode"]
    rate_c = row["stage_bytes"]["c_padded"] / stage_c / 1e6 if stage_c > 0 else float("inf")      # GB/s: bytes per ms / 1e6
    row["spread_of_the_padded_call_ms"] = spread
    row["stage_ms"] = {k: round(m[k] - m["a_encode"], 4) for k in m if k != "a_encode"}
    row["stage_GBps"] = {k: round(row["stage_bytes"][k] / v / 1e6, 1) if v > 0 else None for k, v in row["stage_ms"].items()}
    row["allowance_ms"] = {k: round(row["stage_bytes"][k] / rate_c / 1e6 + spread, 4) for k in PAIRS}
    row["meets_the_yardstick"] = {k: row["stage_ms"][k] <= row["allowance_ms"][k] for k in PAIRS}
    return row


def device_shape(args, name, N, torch, vocab_name, pattern, d_bytes, d_offs, n_docs, total):
    dev = d_bytes.device
    stream = torch.cuda.current_stream().cuda_stream
    n_docs -= n_docs & 1                                       # (an even number of documents: the last one is left out; its bytes are not looked at)
    total = int(d_offs[n_docs].item())
    n_pairs = n_docs // 2
    enc = N.Encoder(N.Vocab(vocab_bytes(vocab_name)), pattern, device=0)
    enc.reserve(total, n_docs)
    bp, op = d_bytes.data_ptr(), d_offs.data_ptr()
    o_x = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    d_ids = torch.empty(total, dtype=torch.int32, device=dev)
    tokens = enc.encode_batch_device(bp, op, n_docs, total, d_ids.data_ptr(), total, o_x.data_ptr(), stream)
    del d_ids
    cap = max(tokens, n_docs * PAD_L, n_pairs * PAIR_L)
    ids = torch.empty(cap, dtype=torch.int32, device=dev)
    pos = torch.empty(cap, dtype=torch.int32, device=dev)
    mask = torch.empty(cap, dtype=torch.uint8, device=dev)
    types = torch.empty(cap, dtype=torch.uint8, device=dev)
    lens = torch.empty(max(1, n_docs), dtype=torch.int32, device=dev)
    kept = torch.empty(max(1, n_docs), dtype=torch.int32, device=dev)
    figures, nbytes = {}, {}

    def padded():
        figures["c_padded"] = enc.encode_batch_padded_device(bp, op, n_docs, total, [], -1, EOS, PAD_L, 0, 0, 0, M, ids.data_ptr(), cap, mask.data_ptr(), 0, lens.data_ptr(), 0, stream)
        return figures["c_padded"][0]

    def pairs(key):
        strategy, everything = PAIRS[key]

        def call():
            figures[key] = enc.encode_batch_pairs_device(bp, op, n_docs, total, [], BOS, SEP, 1, EOS, PAIR_L, strategy, 0, 0, 0, M, ids.data_ptr(), cap, mask.data_ptr(),
                                                         types.data_ptr(), pos.data_ptr() if everything else 0, lens.data_ptr(), kept.data_ptr() if everything else 0,
                                                         o_x.data_ptr() if everything else 0, stream)
            return figures[key][0]
        return call
    calls = [("a_encode", lambda: enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)), ("c_padded", padded)]
    calls += [(k, pairs(k)) for k in PAIRS]
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
            if k == "c_padded" and k not in nbytes:            # (the kept ids from lens: every row holds one eos id)
                nbytes[k] = 4 * (int(lens[:n_docs].sum(dtype=torch.int64).item()) - n_docs) + 5 * n_docs * figures[k][1]
            if k in PAIRS and k not in nbytes:                 # (... every pair row three framing ids)
                nbytes[k] = 4 * (int(lens[:n_pairs].sum(dtype=torch.int64).item()) - 3 * n_pairs) + (10 if PAIRS[k][1] else 6) * n_pairs * figures[k][1]
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "pairs": n_pairs, "bytes": total, "tokens": tokens,
           "padded": {"max_len": PAD_L, "pad_multiple": M}, "pair": {"max_len": PAIR_L, "pad_multiple": M, "sep_count": 1},
           "unit": "ms by device events: median, min, max", "steps": args.steps, "ms": summary(series), "every_call_returned_its_total": same,
           "figures": {k: list(v) for k, v in figures.items()}, "stage_bytes": nbytes, "per_document_bytes_of_the_padded_stage": 32 * n_docs,
           "per_pair_bytes_of_the_pair_stage": 76 * n_pairs, "pairs_calls": enc.pairs_calls(), "workspace_bytes": enc.workspace_bytes}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,mixed,real")
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mixed-docs", type=int, default=2_000_000)
    ap.add_argument("--real-mb", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("pairs_probe: no GPU (a timing taken elsewhere says nothing)")
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
            kind, n_docs = (2, args.mixed_docs) if shape == "mixed" else (1, args.docs)
            d_bytes, d_offs, total = synthetic(N, torch, kind, n_docs)
            emit(device_shape(args, shape, N, torch, "synth100k", N.CL100K, d_bytes, d_offs, n_docs, total))
        elif shape == "real":
            import bench
            r_bytes, r_offs, meta = bench.real_text_corpus(args.real_mb << 20, 256, 768)
            total, n_docs = int(r_offs[-1]), len(r_offs) - 1
            padded = np.zeros(total + 64, np.uint8); padded[:total] = r_bytes[:total]
            row = device_shape(args, shape, N, torch, "gpt2", N.P1, torch.from_numpy(padded).to(dev), torch.from_numpy(np.ascontiguousarray(r_offs, np.int64)).to(dev), n_docs, total)
            row["text"] = {k: meta[k] for k in meta if k in ("files", "sha256", "roots")} if isinstance(meta, dict) else str(meta)[:200]
            emit(row)
        else:
            raise SystemExit("pairs_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
