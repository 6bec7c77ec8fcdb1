#!/usr/bin/env python3
"""TKZ_OPT_ADAPT on the pipelined host path AT REAL SIZES (no chunk knob, the production distances): about 2 GB of the box's source text through page-locked
tkz_encode_batch_utf8 in 64 MB calls -- 4 chunks of 16 MB a call, two launch sequences in flight -- on a fresh encoder, `repeats` times.  Per repeat: the
encoder's bookkeeping after the last call (tkz_encoder_adapt_stats) and the rate of the last ten calls; then the median of each over the repeats with its spread.
tools/adapt_probe.py is the same question on the device entry, where a call is one batch.
usage: adapt_host_probe.py [lib=the built one] [repeats=5] [vocab=gpt2] [pattern=1] [total_gb=2] [call_mb=64]   -> JSON lines"""
import ctypes as C
import gzip, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401 -- its HIP runtime initialises before libtkz is loaded
torch.cuda.init()
import bench
from tokenizer_amd import _native as N
arg = sys.argv[1:] + [""] * 6
lib = N.Library(arg[0]) if arg[0] else N.default_library()
repeats, vname, pattern = int(arg[1] or 5), arg[2] or "gpt2", int(arg[3] or 1)
total_bytes, call_bytes = int(float(arg[4] or 2) * (1 << 30)), int(arg[5] or 64) << 20
# the text: up to 512 MB of what the box holds, walked through again and again until total_bytes have been sent (a call is a run of whole documents)
r_bytes, r_offs, meta = bench.real_text_corpus(512 << 20, 256, 768)
n_docs_all, have = len(r_offs) - 1, int(r_offs[-1])
assert have > 0, "no text found"
calls, d0 = [], 0
while sum(int(r_offs[b] - r_offs[a]) for a, b in calls) < total_bytes:
    d1 = int(np.searchsorted(r_offs, r_offs[d0] + call_bytes, side="right")) - 1
    if d1 <= d0 or d1 > n_docs_all:
        d0 = 0
        continue
    calls.append((d0, d1))
    d0 = d1 if d1 < n_docs_all else 0
max_bytes = max(int(r_offs[b] - r_offs[a]) for a, b in calls)
max_docs = max(b - a for a, b in calls)
hp = [C.c_void_p() for _ in range(4)]
for h, n in zip(hp, [max_bytes + 64, 8 * (max_docs + 1), 4 * max_bytes + 64, 8 * (max_docs + 1)]):
    lib.check(lib.L.tkz_host_alloc(n, C.byref(h)))
raw = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", vname + ".tiktoken.gz"), "rb").read())
vocab = N.Vocab(raw, lib)
print(json.dumps({"lib": lib.path, "text_bytes": have, "files": meta["files"], "calls": len(calls), "call_bytes": max_bytes, "sent_bytes": sum(int(r_offs[b] - r_offs[a]) for a, b in calls)}), flush=True)
rows = []
for rep in range(repeats):
    enc = N.Encoder(vocab, pattern)
    rates = []
    for i, (a, b) in enumerate(calls):
        nb = int(r_offs[b] - r_offs[a])
        offs = np.ascontiguousarray(r_offs[a:b + 1] - r_offs[a], np.int64)
        C.memmove(hp[0], r_bytes[int(r_offs[a]):].ctypes.data, nb)
        C.memmove(hp[1], offs.ctypes.data, 8 * (b - a + 1))
        needed = C.c_int64(0)
        t0 = time.perf_counter()
        lib.check(lib.L.tkz_encode_batch_utf8(enc._h, hp[0], hp[1], b - a, hp[2], nb, hp[3], C.byref(needed)))
        rates.append(nb / (time.perf_counter() - t0) / 1e9)
    # (read once, at the end: tkz_encoder_adapt_stats waits for an install in flight on its thread, and between the calls that would order what production leaves to chance)
    s = enc.adapt_stats()
    row = {"repeat": rep, "relearns": s["relearns"], "promotions": s["promotions"], "promoted_pieces": s["promoted_pieces"], "settled_miss_share": s["settled_miss_share"], "GBps_last10": round(statistics.median(rates[-10:]), 2),
           "GBps_calls_2_to_11": round(statistics.median(rates[1:11]), 2), "engine_downloads": enc.engine_downloads}
    rows.append(row)
    print(json.dumps(row), flush=True)
    enc.close()


def spread(key):
    v = sorted(r[key] for r in rows)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1]}


print(json.dumps({"summary": {k: spread(k) for k in ("relearns", "promoted_pieces", "GBps_last10")}, "repeats": repeats}), flush=True)
for h in hp:
    lib.L.tkz_host_free(h)
