#!/usr/bin/env python3
"""What a count call costs beside the encode call it replaces.  The reference for every time is the PARENT commit's library (--parent-lib: a libtkz.so built
from the parent commit's sources, loaded beside this one through ctypes alone) making the matching encode call; the count call is this library's.  Both run in
one process, alternating in one loop -- parent (series a), count, parent (series b) -- after warm-up calls of every shape; the two parent series are the same
call on the same encoder, so the difference of their medians is the parent's own spread.
  device shapes  tkz_encode_batch_device (parent) against tkz_count_batch_device, device events around each call:
                 `headline` bench.py's headline batch (--docs synthetic kind-1 documents of 256..768 bytes, cl100k, synth100k), `mixed` (kind 2, --mixed-docs),
                 `real` (text files of the machine as bench.py's kind 6 reads them, --real-mb, pattern 1, gpt2)
  host shapes    tkz_encode_batch_utf8 (parent) against tkz_count_batch_utf8 on --host-mb of the kind-1 text, page-locked and pageable buffers, and
                 tkz_encode_utf8 against tkz_count_utf8 on one text of 64 bytes and of 2 KB; a host clock around calls that end synchronised
Then, in passes of their own with profiling on, the K_PLACE bracket (k_place in the parent, k_tokcount in the count call) by the library's own events.  The share of
sub-tiles k_tokcount skips is computed from the document offsets (a 1 KiB sub-tile without a document start).  The count offsets are compared with the parent's
encode offsets on every document of every timed batch.  Prints one JSON line per shape (and appends them to --out).
usage: python tools/count_probe.py --parent-lib PARENT/libtkz.so [--shapes headline,mixed,real,host,single] [--steps 20] [--warmup 3] [--out FILE]"""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
K_PLACE = 4


def vocab_bytes(name):
    return gzip.decompress(open(os.path.join(ROOT, "tests", "golden", name + ".tiktoken.gz"), "rb").read())


class RawLib:
    """a libtkz.so through ctypes alone: the parent's library does not export what tokenizer_amd._native binds"""

    def __init__(self, path, vocab_name, pattern):
        L = self.L = C.CDLL(path)
        L.tkz_vocab_from_tiktoken.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.tkz_encoder_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
        L.tkz_encode_batch_device.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, C.POINTER(i64)]
        L.tkz_encode_batch_utf8.argtypes = [vp, vp, vp, i64, vp, i64, vp, C.POINTER(i64)]
        L.tkz_encode_utf8.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64)]
        L.tkz_encoder_set_profiling.argtypes = [vp, i32]
        L.tkz_encoder_kernel_ms.argtypes = [vp, vp, vp, i32]
        L.tkz_last_error.restype = C.c_char_p
        raw = vocab_bytes(vocab_name)
        v, h = vp(), vp()
        self.check(L.tkz_vocab_from_tiktoken(raw, len(raw), C.byref(v)))
        self.check(L.tkz_encoder_create(v, pattern, 0, C.byref(h)))
        self.h = h

    def check(self, st):
        if st != 0:
            raise SystemExit("count_probe: parent library: status %d: %s" % (st, self.L.tkz_last_error().decode()))

    def place_ms(self, reset):
        import numpy as np
        ms, n = np.zeros(8, np.float64), np.zeros(8, np.int64)
        self.check(self.L.tkz_encoder_kernel_ms(self.h, ms.ctypes.data, n.ctypes.data, 1 if reset else 0))
        return float(ms[K_PLACE]), int(n[K_PLACE])


def summary(series):
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in series.items()}


def verdict(row):
    a, b, c = (row["ms"][k][0] for k in ("parent_a", "parent_b", "count"))
    parent = (a + b) / 2
    row["parent_median"] = round(parent, 4)
    row["parent_spread"] = round(abs(a - b), 4)
    row["count_over_parent"] = round(c / parent, 3)
    row["count_below_parent_by_more_than_the_spread"] = bool(parent - c > abs(a - b))
    return row


def skipped_share(torch, d_offs, total):
    starts = d_offs[:-1]
    starts = starts[starts < total]
    ntiles = (total + 1023) // 1024
    return round(1.0 - torch.unique(starts // 1024).numel() / max(1, ntiles), 4)


def device_shape(args, name, N, torch, vocab_name, pattern, d_bytes, d_offs, n_docs, total):
    dev = d_bytes.device
    stream = torch.cuda.current_stream().cuda_stream
    new = N.Encoder(N.Vocab(vocab_bytes(vocab_name)), pattern, device=0)
    old = RawLib(args.parent_lib, vocab_name, pattern)
    d_ids = torch.empty(total, dtype=torch.int32, device=dev)
    o_old = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    o_new = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    tot = i64(0)

    def parent():
        old.check(old.L.tkz_encode_batch_device(old.h, d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, d_ids.data_ptr(), total, o_old.data_ptr(), stream, C.byref(tot)))
        return tot.value

    def count():
        return new.count_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, [], o_new.data_ptr(), stream=stream)
    calls = (("parent_a", parent), ("count", count), ("parent_b", parent))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    series = {k: [] for k, _ in calls}
    res = {}
    for _ in range(args.steps):
        for k, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res[k] = fn()
            e1.record()
            e1.synchronize()
            series[k].append(e0.elapsed_time(e1))
    same = bool(torch.equal(o_old, o_new)) and res["count"] == res["parent_a"]
    # the K_PLACE bracket, in passes of their own (profiling serialises the launch sequence around its events)
    old.check(old.L.tkz_encoder_set_profiling(old.h, 1)); new.set_profiling(True)
    old.place_ms(True); new.kernel_ms(reset=True)
    for _ in range(args.profile_steps):
        parent()
    p_ms, p_n = old.place_ms(True)
    for _ in range(args.profile_steps):
        count()
    c_ms, c_n = new.kernel_ms(reset=True)["k_place"]
    row = {"shape": name, "entry": "device", "vocab": vocab_name, "pattern": pattern, "docs": n_docs, "bytes": total, "tokens": res["count"], "unit": "ms by device events",
           "steps": args.steps, "ms": summary(series), "offsets_equal_on_every_document": same,
           "k_place_bracket_ms_per_launch": {"parent_k_place": round(p_ms / max(1, p_n), 4), "count_k_tokcount": round(c_ms / max(1, c_n), 4)},
           "sub_tiles_skipped_share": skipped_share(torch, d_offs, total), "id_buffer_bytes_not_needed": 4 * total}
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


def host_shapes(args, N, torch, np):
    n_docs = (args.host_mb << 20) // 512
    d_bytes, d_offs, total = synthetic(N, torch, 1, n_docs)
    text, offs = d_bytes[:total].cpu().numpy(), d_offs.cpu().numpy()
    del d_bytes, d_offs
    torch.cuda.empty_cache()
    rows = []
    for label in ("page_locked", "pageable"):
        pin = label == "page_locked"
        mk = (lambda n, dt: torch.empty(n, dtype=dt).pin_memory().numpy()) if pin else (lambda n, dt: np.empty(n, {torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64}[dt]))
        h_text, h_offs = mk(total + 64, torch.uint8), mk(n_docs + 1, torch.int64)
        h_text[:total] = text; h_offs[:] = offs
        h_ids, o_old, o_new = mk(total, torch.int32), mk(n_docs + 1, torch.int64), mk(n_docs + 1, torch.int64)
        new = N.Encoder(N.Vocab(vocab_bytes("synth100k")), N.CL100K, device=0)
        old = RawLib(args.parent_lib, "synth100k", N.CL100K)
        need, tot = i64(0), i64(0)

        def parent():
            old.check(old.L.tkz_encode_batch_utf8(old.h, h_text.ctypes.data, h_offs.ctypes.data, n_docs, h_ids.ctypes.data, total, o_old.ctypes.data, C.byref(need)))
            return need.value

        def count():
            new.lib.check(new.lib.L.tkz_count_batch_utf8(new._h, h_text.ctypes.data, h_offs.ctypes.data, n_docs, None, 0, o_new.ctypes.data, C.byref(tot)))
            return tot.value
        calls = (("parent_a", parent), ("count", count), ("parent_b", parent))
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
        rows.append(verdict({"shape": "host_" + label, "entry": "host", "vocab": "synth100k", "pattern": N.CL100K, "docs": n_docs, "bytes": total, "tokens": res["count"],
                             "unit": "ms by a host clock", "steps": args.host_steps, "ms": summary(series),
                             "offsets_equal_on_every_document": bool((o_old == o_new).all()) and res["count"] == res["parent_a"],
                             "workspace_bytes_count_encoder": new.workspace_bytes, "id_bytes_not_downloaded": 4 * res["count"]}))
        del new, old
    return rows


def single_shapes(args, N, np):
    rows = []
    words = "the quick brown fox jumps over the lazy dog, it's 12345 o'clock and all is well; "
    new = N.Encoder(N.Vocab(vocab_bytes("synth100k")), N.CL100K, device=0)
    old = RawLib(args.parent_lib, "synth100k", N.CL100K)
    for n in (64, 2048):
        text = np.frombuffer((words * (n // len(words) + 1))[:n].encode(), np.uint8)
        ids = np.empty(n, np.int32)
        k = i64(0)

        def parent():
            old.check(old.L.tkz_encode_utf8(old.h, text.ctypes.data, n, ids.ctypes.data, n, C.byref(k)))
            return k.value

        def count():
            new.lib.check(new.lib.L.tkz_count_utf8(new._h, text.ctypes.data, n, None, 0, C.byref(k)))
            return k.value
        calls = (("parent_a", parent), ("count", count), ("parent_b", parent))
        for _ in range(args.single_calls // 4):
            for _, fn in calls:
                fn()
        series = {q: [] for q, _ in calls}
        res = {}
        for _ in range(args.single_calls):
            for q, fn in calls:
                t0 = time.perf_counter()
                res[q] = fn()
                series[q].append((time.perf_counter() - t0) * 1e6)
        rows.append(verdict({"shape": "single_%d_bytes" % n, "entry": "single text", "vocab": "synth100k", "pattern": N.CL100K, "bytes": n, "tokens": res["count"],
                             "unit": "us by a host clock", "steps": args.single_calls, "ms": summary(series), "offsets_equal_on_every_document": res["count"] == res["parent_a"],
                             "count_calls": new.count_calls()}))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--shapes", default="headline,mixed,real,host,single")
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mixed-docs", type=int, default=2_000_000)
    ap.add_argument("--real-mb", type=int, default=256)
    ap.add_argument("--host-mb", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=20)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--single-calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from tokenizer_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("count_probe: no GPU (a timing taken elsewhere says nothing)")
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
        elif shape == "host":
            for row in host_shapes(args, N, torch, np):
                emit(row)
        elif shape == "single":
            for row in single_shapes(args, N, np):
                emit(row)
        else:
            raise SystemExit("count_probe: unknown shape " + shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
