#!/usr/bin/env python3
"""What the packed entry costs beside the encode entry and the trim entry.  One process, one RESERVED encoder per batch, the memo warmed by --warmup calls of every
shape, then --steps rounds of the device calls in turn, device events around each call:
  (a)   tkz_encode_batch_device;
  (b)   tkz_encode_batch_trim_device, suffix, with a maximum no document reaches -- it also gathers every id once, behind the dearer piece-granular launch
        sequence: THE YARDSTICK the span and chunk stages were measured against;
  (p0)  tkz_encode_batch_packed_device without framing (f = 0), rows of --row-len, with pos and seg_starts: the ids stand where k_place wrote them;
  (p2)  the same with a bos and an eos id: the plain sequence, then one gather of every id;
  (p2n) (p2) with pos and seg_starts NULL.
In every timed round (p0)'s first T ids and its offsets are compared with (a)'s.
Batches: `headline` (bench.py's headline batch: --docs synthetic kind-1 documents of 256..768 bytes, cl100k, synth100k), `mixed` (kind 2, --mixed-docs), `real`
(text files of the machine as bench.py's kind 6 reads them, --real-mb, pattern 1, gpt2).  Then, in a pass of its own with profiling on, the K_DOCOFFS bracket of
(a) and the packed calls -- k_docoffs alone in (a), k_docoffs + the packing stage in the others: the difference is the stage by the library's own events.
Prints one JSON line per batch (and appends them to --out).
usage: python tools/packed_probe.py [--shapes headline,mixed,real] [--row-len 2048] [--steps 20] [--warmup 3] [--out FILE]"""
import argparse
import gzip
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HUGE = 1 << 40
BOS, EOS = 1, 2


def vocab_bytes(name):
    return gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".tiktoken.gz"), "rb").read())


def summary(series):
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in series.items()}


def verdict(row):
    m = {k: v[0] for k, v in row["ms"].items()}
    spread = round(row["ms"]["b_trim"][2] - row["ms"]["b_trim"][1], 4)
    row["spread_of_the_trim_call_ms"] = spread
    row["p2_minus_b_trim"] = round(m["p2_framed"] - m["b_trim"], 4)
    row["p2_within_the_trim_call_plus_its_spread"] = m["p2_framed"] <= m["b_trim"] + spread
    row["p0_minus_a_encode"] = round(m["p0_unframed"] - m["a_encode"], 4)
    return row


def device_shape(args, name, N, torch, vocab_name, pattern, d_bytes, d_offs, n_docs, total):
    dev = d_bytes.device
    stream = torch.cuda.current_stream().cuda_stream
    enc = N.Encoder(N.Vocab(vocab_bytes(vocab_name)), pattern, device=0)
    enc.reserve(total, n_docs)
    bp, op = d_bytes.data_ptr(), d_offs.data_ptr()
    L = args.row_len
    d_ids = torch.empty(total, dtype=torch.int32, device=dev)
    o_a = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    tokens = enc.encode_batch_device(bp, op, n_docs, total, d_ids.data_ptr(), total, o_a.data_ptr(), stream)
    ids_a = d_ids[:tokens].clone()
    del d_ids
    cap, scap = N.Encoder.packed_bounds(n_docs, tokens, L, 2)      # (tokens, not bytes: the bounds of tkz.h with the count known)
    ids = torch.empty(cap, dtype=torch.int32, device=dev)
    pos = torch.empty(cap, dtype=torch.int32, device=dev)
    seg = torch.empty(scap + 1, dtype=torch.int64, device=dev)
    o_x = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    figures = {}

    def packed(key, bos, eos, arrays):
        def call():
            figures[key] = enc.encode_batch_packed_device(bp, op, n_docs, total, [], bos, eos, L, 0, ids.data_ptr(), cap, o_x.data_ptr(), pos.data_ptr() if arrays else 0,
                                                          seg.data_ptr() if arrays else 0, scap, stream)
            return figures[key][0]
        return call
    calls = [("a_encode", lambda: enc.encode_batch_device(bp, op, n_docs, total, ids.data_ptr(), cap, o_x.data_ptr(), stream)),
             ("b_trim", lambda: enc.encode_batch_trim_device(bp, op, n_docs, total, [], N.TRIM_SUFFIX, HUGE, 0, ids.data_ptr(), cap, o_x.data_ptr(), 0, 0, stream)),
             ("p0_unframed", packed("p0_unframed", -1, -1, True)), ("p2_framed", packed("p2_framed", BOS, EOS, True)), ("p2n_framed_no_arrays", packed("p2n_framed_no_arrays", BOS, EOS, False))]
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
            if k == "p0_unframed":
                same = same and n == tokens and bool(torch.equal(ids[:tokens], ids_a)) and bool(torch.equal(o_x, o_a))
            else:
                same = same and n == (tokens if k[0] in "ab" else tokens + 2 * n_docs)
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
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "bytes": total, "tokens": tokens, "row_len": L,
           "unit": "ms by device events", "steps": args.steps, "ms": summary(series), "p0_ids_and_offsets_equal_to_the_encode_entry": same,
           "T_rows_segs": {k: list(v) for k, v in figures.items()}, "brackets_ms_per_call": brackets, "packed_calls": enc.packed_calls(), "workspace_bytes": enc.workspace_bytes}
    if all("k_docoffs" in brackets[k] for k in brackets):
        row["packing_stage_by_the_bracket_ms"] = {k: round(brackets[k]["k_docoffs"] - brackets["a_encode"]["k_docoffs"], 4) for k in brackets if k.startswith("p")}
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
    ap.add_argument("--row-len", type=int, default=2048)
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mixed-docs", type=int, default=2_000_000)
    ap.add_argument("--real-mb", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("packed_probe: no GPU (a timing taken elsewhere says nothing)")
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
        elif shape == "real":
            import bench
            r_bytes, r_offs, meta = bench.real_text_corpus(args.real_mb << 20, 256, 768)
            total, n_docs = int(r_offs[-1]), len(r_offs) - 1
            padded = np.zeros(total + 64, np.uint8); padded[:total] = r_bytes[:total]
            row = device_shape(args, shape, N, torch, "gpt2", N.P1, torch.from_numpy(padded).to(dev), torch.from_numpy(np.ascontiguousarray(r_offs, np.int64)).to(dev), n_docs, total)
            row["text"] = {k: meta[k] for k in meta if k in ("files", "sha256", "roots")} if isinstance(meta, dict) else str(meta)[:200]
            emit(row)
        else:
            raise SystemExit("packed_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
