#!/usr/bin/env python3
"""What Decode to UTF-16 on the device costs, beside what the parent does.  One batch of device-resident ids per corpus -- the encode (cl100k pattern,
synth100k) of bench.py's kind-1 (ASCII) and kind-2 (mixed UTF-8) corpora, --mb megabytes of text each -- and, timed with device events around calls that
alternate in one loop, after warm-up calls of both:
  (a) tkz_decode_batch_device         the parent's device work: ids -> bytes + byte offsets
  (b) tkz_decode_batch_utf16_device   ids -> code units + unit offsets (the byte decode into the workspace, then the transcode)
then (--host-steps > 0), with a host clock around calls that end synchronised, the host entries on the same ids in host memory:
  tkz_decode_batch + bytes.decode("utf-8", "replace") per document (TikTokenizer.DecodeBatch as the parent has it)
  tkz_decode_batch_utf16 + .decode("utf-16-le") per document      (TikTokenizer.DecodeBatchUtf16)
each also without the per-document conversion.  The strings of both host paths are compared.  Prints one JSON line (and writes it to --out).
usage: python tools/decode_u16_probe.py [--mb 256] [--steps 5] [--warmup 2] [--out FILE]"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--min-len", type=int, default=256)
    ap.add_argument("--max-len", type=int, default=768)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("decode_u16_probe: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    raw = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "synth100k.tiktoken.gz"), "rb").read())
    enc = N.Encoder(N.Vocab(raw), N.CL100K, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"what": "Decode of one batch of ids: device entries by device events (ms, median and min of --steps alternating calls), host entries by a host clock",
           "vocab": "synth100k", "pattern": "cl100k", "mb": args.mb, "steps": args.steps, "warmup": args.warmup, "corpora": {}}
    for kind in (1, 2):
        n_docs = (args.mb << 20) // ((args.min_len + args.max_len) // 2)
        seed = 0x5EED0000 + {1: 2, 2: 3}[kind]
        d_offs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        total = N.corpus_generate_device(0, kind, seed, 0, n_docs, args.min_len, args.max_len, d_offs.data_ptr(), None, 0, stream)
        d_bytes = torch.empty(total + 64, dtype=torch.uint8, device=dev)
        N.corpus_generate_device(0, kind, seed, 0, n_docs, args.min_len, args.max_len, d_offs.data_ptr(), d_bytes.data_ptr(), total, stream)
        d_ids = torch.empty(total, dtype=torch.int32, device=dev)
        d_ioffs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        n_ids = enc.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, d_ids.data_ptr(), total, d_ioffs.data_ptr(), stream=stream)
        d_out8 = torch.empty(total + 64, dtype=torch.uint8, device=dev)
        d_out16 = torch.empty(total + 64, dtype=torch.int16, device=dev)          # (a unit stands for at least one byte)
        d_ooffs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        calls = {"a_decode_batch_device": lambda: enc.decode_batch_device(d_ids.data_ptr(), d_ioffs.data_ptr(), n_docs, n_ids, d_out8.data_ptr(), total,
                                                                          d_ooffs.data_ptr(), stream=stream),
                 "b_decode_batch_utf16_device": lambda: enc.decode_batch_utf16_device(d_ids.data_ptr(), d_ioffs.data_ptr(), n_docs, n_ids, d_out16.data_ptr(),
                                                                                      total, d_ooffs.data_ptr(), stream=stream)}
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        ms = {k: [] for k in calls}
        res = {}
        for _ in range(args.steps):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res[k] = fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        assert res["a_decode_batch_device"] == total and bool((d_out8[:total] == d_bytes[:total]).all()), "decode(encode(x)) != x"
        row = {"docs": n_docs, "text_bytes": total, "ids": n_ids, "units": res["b_decode_batch_utf16_device"]}
        for k in calls:
            row[k + "_ms"] = [round(statistics.median(ms[k]), 3), round(min(ms[k]), 3)]
        row["b_over_a"] = round(statistics.median(ms["b_decode_batch_utf16_device"]) / statistics.median(ms["a_decode_batch_device"]), 2)
        if args.host_steps > 0:
            # the host entries
            ids = d_ids[:n_ids].cpu().numpy()
            ioffs = d_ioffs.cpu().numpy()
            del d_out8, d_out16, d_bytes, d_ids
            torch.cuda.empty_cache()

            def host_bytes(convert):
                data, boffs = enc.decode_batch(ids, ioffs, out_cap=total)
                if not convert:
                    return None
                rawb = data.tobytes()
                return [rawb[boffs[d]:boffs[d + 1]].decode("utf-8", "replace") for d in range(n_docs)]

            def host_units(convert):
                units, uoffs = enc.decode_batch_utf16(ids, ioffs, out_cap=total)
                if not convert:
                    return None
                rawu = units.tobytes()
                return [rawu[2 * uoffs[d]:2 * uoffs[d + 1]].decode("utf-16-le") for d in range(n_docs)]
            host = {"parent_decode_batch_then_utf8_decode_per_document": lambda: host_bytes(True), "decode_batch_utf16_then_string_per_document": lambda: host_units(True),
                    "parent_decode_batch_alone": lambda: host_bytes(False), "decode_batch_utf16_alone": lambda: host_units(False)}
            got = {k: fn() for k, fn in host.items()}                                # (warm-up, and the comparison of the strings)
            assert got["parent_decode_batch_then_utf8_decode_per_document"] == got["decode_batch_utf16_then_string_per_document"], "the two host paths give different strings"
            del got
            hs = {k: [] for k in host}
            for _ in range(args.host_steps):
                for k, fn in host.items():
                    t0 = time.perf_counter()
                    fn()
                    hs[k].append((time.perf_counter() - t0) * 1e3)
            row["host_ms"] = {k: [round(statistics.median(v), 1), round(min(v), 1)] for k, v in hs.items()}
        out["corpora"]["kind_%d" % kind] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
