#!/usr/bin/env python3
"""What the padded entry costs beside the encode entry, and how its stage compares with the packed stage.  One process, one RESERVED encoder per batch, the memo
warmed by --warmup calls of every shape, then --steps rounds of the device calls in turn, device events around each call:
  (a)      tkz_encode_batch_device;
  (b)      tkz_encode_batch_packed_device with a bos and an eos id, rows of --row-len, with pos and seg_starts: the plain sequence, then one gather of every id --
           THE YARDSTICK: its stage, (b) - (a), per byte it moves;
  (c128)   tkz_encode_batch_padded_device with an eos id, ids + mask, suffix cut, right padding, L = 128, fixed width (M = 0);
  (c512)   the same at L = 512;
  (c512m8) L = 512, M = 8: the width follows the longest row;
  (c128p)  (c128) with pos;
  (c128l)  (c128) with the prefix cut and left padding.
The bytes a stage moves come from the rule, not from a counter: the packed stage reads 4 per token and 8 per document and writes 8 per stream position (ids and
pos), 8 per segment start and 8 per document; the padded stage reads 4 per KEPT id (at most 4 per uncut token) and writes 5 (ids + mask) or 9 (with pos) per output
position.  Its 32 bytes per document (offsets read, lens and the source start written and read again) are listed beside that figure, not in it.
THE VERDICT of a batch: a padded stage meets the yardstick when (c) - (a) <= its bytes / the packed stage's rate + the min-max spread of (b) in this run.
Batches: `headline` (bench.py's headline batch: --docs synthetic kind-1 documents of 256..768 bytes, cl100k, synth100k), `mixed` (kind 2, --mixed-docs), `real`
(text files of the machine as bench.py's kind 6 reads them, --real-mb, pattern 1, gpt2).  `host`: tkz_encode_batch_padded_utf8 at L = 128 beside
tkz_encode_batch_utf8 on --host-mb of the headline text in pageable memory, host clock, with the two download sizes; `hostlong`: the same on documents of
2,048..8,192 bytes, which L = 128 cuts to a fraction.  `trace`: the headline batch's (c128) alone,
--trace-steps times, for a kernel trace taken around this process.
Prints one JSON line per batch (and appends them to --out).
usage: python tools/padded_probe.py [--shapes headline,mixed,real,host,hostlong] [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOS, EOS = 1, 2
PADDED = {            # key: (max_len, pad_multiple, with pos, cut side, pad side)
    "c128": (128, 0, False, 0, 0), "c512": (512, 0, False, 0, 0), "c512m8": (512, 8, False, 0, 0), "c128p": (128, 0, True, 0, 0), "c128l": (128, 0, False, 1, 1),
}


def vocab_bytes(name):
    return gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".tiktoken.gz"), "rb").read())


def summary(series):
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in series.items()}


def verdict(row):
    m = {k: v[0] for k, v in row["ms"].items()}
    spread = round(row["ms"]["b_packed"][2] - row["ms"]["b_packed"][1], 4)
    stage_b = m["b_packed"] - m["a_encode"]
    rate_b = row["stage_bytes"]["b_packed"] / stage_b / 1e6 if stage_b > 0 else float("inf")      # GB/s: bytes per ms / 1e6
    row["spread_of_the_packed_call_ms"] = spread
    row["stage_ms"] = {k: round(m[k] - m["a_encode"], 4) for k in m if k != "a_encode"}
    row["stage_GBps"] = {k: round(row["stage_bytes"][k] / v / 1e6, 1) if v > 0 else None for k, v in row["stage_ms"].items()}
    row["allowance_ms"] = {k: round(row["stage_bytes"][k] / rate_b / 1e6 + spread, 4) for k in PADDED}
    row["meets_the_yardstick"] = {k: row["stage_ms"][k] <= row["allowance_ms"][k] for k in PADDED}
    return row


def device_shape(args, name, N, torch, vocab_name, pattern, d_bytes, d_offs, n_docs, total, only=None):
    dev = d_bytes.device
    stream = torch.cuda.current_stream().cuda_stream
    enc = N.Encoder(N.Vocab(vocab_bytes(vocab_name)), pattern, device=0)
    enc.reserve(total, n_docs)
    bp, op = d_bytes.data_ptr(), d_offs.data_ptr()
    RL = args.row_len
    d_ids = torch.empty(total, dtype=torch.int32, device=dev)
    o_a = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    tokens = enc.encode_batch_device(bp, op, n_docs, total, d_ids.data_ptr(), total, o_a.data_ptr(), stream)
    del d_ids
    pcap, scap = N.Encoder.packed_bounds(n_docs, tokens, RL, 2)      # (tokens, not bytes: the bounds of tkz.h with the count known)
    cap = max(pcap, tokens, n_docs * max(v[0] for v in PADDED.values()))
    ids = torch.empty(cap, dtype=torch.int32, device=dev)
    pos = torch.empty(cap, dtype=torch.int32, device=dev)
    mask = torch.empty(cap, dtype=torch.uint8, device=dev)
    lens = torch.empty(max(1, n_docs), dtype=torch.int32, device=dev)
    seg = torch.empty(scap + 1, dtype=torch.int64, device=dev)
    o_x = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    figures, nbytes = {}, {}

    def packed():
        figures["b_packed"] = T, rows, segs = enc.encode_batch_packed_device(bp, op, n_docs, total, [], BOS, EOS, RL, 0, ids.data_ptr(), cap, o_x.data_ptr(), pos.data_ptr(),
                                                                            seg.data_ptr(), scap, stream)
        nbytes["b_packed"] = 4 * tokens + 8 * n_docs + 8 * rows * RL + 8 * (segs + 1) + 8 * (n_docs + 1)
        return T

    def padded(key):
        L, M, with_pos, cut, side = PADDED[key]

        def call():
            figures[key] = enc.encode_batch_padded_device(bp, op, n_docs, total, [], -1, EOS, L, cut, side, 0, M, ids.data_ptr(), cap, mask.data_ptr(),
                                                          pos.data_ptr() if with_pos else 0, lens.data_ptr(), 0, stream)
            return figures[key][0]
        return call
    calls = [("a_encode", lambda: enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)), ("b_packed", packed)]
    calls += [(k, padded(k)) for k in PADDED]
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
            same = same and n == (tokens + 2 * n_docs if k == "b_packed" else tokens)
            if k in PADDED and k not in nbytes:                # (the kept ids from lens: every row holds one eos id)
                L, M, with_pos, cut, side = PADDED[k]
                kept = int(lens[:n_docs].sum(dtype=torch.int64).item()) - n_docs
                nbytes[k] = 4 * kept + (9 if with_pos else 5) * n_docs * figures[k][1]
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "bytes": total, "tokens": tokens, "row_len": RL,
           "unit": "ms by device events: median, min, max", "steps": args.steps, "ms": summary(series), "every_call_returned_its_total": same,
           "figures": {k: list(v) for k, v in figures.items()}, "stage_bytes": nbytes, "per_document_bytes_of_the_padded_stage": 32 * n_docs,
           "padded_calls": enc.padded_calls(), "workspace_bytes": enc.workspace_bytes}
    return verdict(row)


def host_shape(args, name, N, torch, np, d_bytes, d_offs, n_docs, total):
    """tkz_encode_batch_padded_utf8 at L = 128 beside tkz_encode_batch_utf8 on the same text, pageable buffers, host clock"""
    offs = d_offs.cpu().numpy()
    n = int(np.searchsorted(offs, args.host_mb << 20, side="right")) - 1
    n = max(1, min(n, n_docs))
    nb = int(offs[n])
    data = d_bytes[:nb].cpu().numpy().copy()
    offs = offs[:n + 1].copy()
    enc = N.Encoder(N.Vocab(vocab_bytes("synth100k")), N.CL100K, device=0)
    series = {"encode_utf8": [], "padded_utf8_L128": []}
    figures = {}
    for step in range(args.warmup + args.host_steps):
        t0 = time.perf_counter()
        ids, ooff = enc.encode_batch(data, offs)
        t1 = time.perf_counter()
        r = enc.encode_batch_padded(data, offs, 128, (), -1, EOS, 0, pad_multiple=0, want_pos=False, want_offs=False)
        t2 = time.perf_counter()
        if step >= args.warmup:
            series["encode_utf8"].append((t1 - t0) * 1e3)
            series["padded_utf8_L128"].append((t2 - t1) * 1e3)
        figures = {"tokens": int(len(ids)), "W": int(r[0].shape[1]), "n_cut": int(r[6]),
                   "download_bytes": {"encode_utf8": 4 * int(len(ids)) + 8 * (n + 1), "padded_utf8_L128": 5 * n * int(r[0].shape[1]) + 4 * n}}
    return {"shape": name, "entry": "utf8, pageable", "docs": n, "bytes": nb, "unit": "ms by the host clock: median, min, max", "steps": args.host_steps, "ms": summary(series), **figures}


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
    ap.add_argument("--shapes", default="headline,mixed,real,host,hostlong")
    ap.add_argument("--row-len", type=int, default=2048)
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
        raise SystemExit("padded_probe: no GPU (a timing taken elsewhere says nothing)")
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
            d_bytes, d_offs, total = synthetic(N, torch, kind, n_docs)
            emit(device_shape(args, shape, N, torch, "synth100k", N.CL100K, d_bytes, d_offs, n_docs, total, only="c128" if shape == "trace" else None))
        elif shape in ("host", "hostlong"):
            lo, hi = (256, 768) if shape == "host" else (2048, 8192)      # (a little more text than asked for, cut to --host-mb)
            n_docs = max(1, (args.host_mb << 20) // ((lo + hi) // 2 - 12))
            d_bytes, d_offs, total = synthetic(N, torch, 1, n_docs, lo, hi)
            emit(host_shape(args, shape, N, torch, np, d_bytes, d_offs, n_docs, total))
        elif shape == "real":
            import bench
            r_bytes, r_offs, meta = bench.real_text_corpus(args.real_mb << 20, 256, 768)
            total, n_docs = int(r_offs[-1]), len(r_offs) - 1
            padded = np.zeros(total + 64, np.uint8); padded[:total] = r_bytes[:total]
            row = device_shape(args, shape, N, torch, "gpt2", N.P1, torch.from_numpy(padded).to(dev), torch.from_numpy(np.ascontiguousarray(r_offs, np.int64)).to(dev), n_docs, total)
            row["text"] = {k: meta[k] for k in meta if k in ("files", "sha256", "roots")} if isinstance(meta, dict) else str(meta)[:200]
            emit(row)
        else:
            raise SystemExit("padded_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
