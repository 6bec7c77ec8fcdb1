#!/usr/bin/env python3
"""What special tokens on the device cost and what the mirrors gain.
  1. the kind-1 corpus generated on the device with <|endoftext|> written behind every document (one literal per ~512 bytes), timed with events on the
     launch stream: the plain device entry on those bytes (the literals encoded as text) against the special device entry; the K_DOCMARK and K_PRETOK
     brackets (which hold the literal scan / the segment bitmap and the literal fix-up on the special entry) for both and their difference;
  2. TikTokenizer.EncodeBatchFlat(texts, True) on 100,000 texts of ~2 KB with a literal each, wall clock, median of five.
usage: special_probe.py [n_docs=1000000] [out=profiles/special_tokens/special_probe.json]   (run it on the parent commit as well: leg 1's special entry is then absent)"""
import gzip, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from tokenizer_amd import _native as N
from tokenizer_amd.tokenizer import TikTokenizer, REGEX_CL100K, ENCODERS

n_docs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "special_tokens", "special_probe.json")
LIT = b"<|endoftext|>"
specials = ENCODERS["cl100k_base"][2]
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
raw = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "synth100k.tiktoken.gz"), "rb").read())

# ---- 1. the device entries ----
d_offs0 = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
total0 = N.corpus_generate_device(0, 1, 0x5EED0002, 0, n_docs, 256, 768, d_offs0.data_ptr(), None, 0, st)
d_bytes0 = torch.empty(total0 + 64, dtype=torch.uint8, device=dev)
N.corpus_generate_device(0, 1, 0x5EED0002, 0, n_docs, 256, 768, d_offs0.data_ptr(), d_bytes0.data_ptr(), total0, st)
torch.cuda.synchronize()
# every document followed by the literal: byte i of the corpus moves to i + 13 * (its document's index)
total = total0 + len(LIT) * n_docs
d_offs = d_offs0 + len(LIT) * torch.arange(n_docs + 1, dtype=torch.int64, device=dev)
d_bytes = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
lit = torch.frombuffer(bytearray(LIT), dtype=torch.uint8).to(dev)
CH = 1 << 16                                                    # (documents a step: the index arrays stay small)
for d0 in range(0, n_docs, CH):
    d1 = min(n_docs, d0 + CH)
    lo, hi = int(d_offs0[d0]), int(d_offs0[d1])
    lens = d_offs0[d0 + 1:d1 + 1] - d_offs0[d0:d1]
    doc = torch.repeat_interleave(torch.arange(d0, d1, device=dev), lens)
    d_bytes[torch.arange(lo, hi, device=dev) + len(LIT) * doc] = d_bytes0[lo:hi]
    ends = d_offs[d0 + 1:d1 + 1] - len(LIT)
    d_bytes[(ends[:, None] + torch.arange(len(LIT), device=dev)[None, :]).reshape(-1)] = lit.repeat(d1 - d0)
del d_bytes0, doc
d_ids = torch.empty(total, dtype=torch.int32, device=dev)
d_oo = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
has_special = hasattr(N.Encoder, "encode_batch_special_device")
result = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None,
          "n_docs": n_docs, "bytes": total, "literals": n_docs}


def timed(enc, special, steps=8, warmup=3):
    index = list(range(len(specials)))
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if special:
            n = enc.encode_batch_special_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, index, d_ids.data_ptr(), total, d_oo.data_ptr(), st)
        else:
            n = enc.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, d_ids.data_ptr(), total, d_oo.data_ptr(), st)
        b.record(); torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    enc.set_profiling(True)
    enc.kernel_ms(reset=True)
    for _ in range(3):
        (enc.encode_batch_special_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, index, d_ids.data_ptr(), total, d_oo.data_ptr(), st) if special
         else enc.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, d_ids.data_ptr(), total, d_oo.data_ptr(), st))
    k = enc.kernel_ms(reset=True)
    enc.set_profiling(False)
    med = statistics.median(ms)
    return {"ms": round(med, 3), "GBps": round(total / med / 1e6, 1), "tokens": int(n), "kernel_ms": k}


for name, special in (("plain_entry", False),) + ((("special_entry", True),) if has_special else ()):
    enc = N.Encoder(N.Vocab(raw), N.CL100K)
    enc.set_special_tokens(specials)
    result[name] = timed(enc, special)
    del enc
if has_special:
    result["ratio_special_over_plain"] = round(result["plain_entry"]["ms"] / result["special_entry"]["ms"], 3)

# ---- 2. the mirror ----
tok = TikTokenizer(raw, specials, REGEX_CL100K)
doc = N.corpus_doc_host(1, 0x5EED0002, 7, 2000, 2000).decode("utf-8", "replace")
texts = [doc[:1000] + "<|endoftext|>" + doc[1000:] + str(i) for i in range(100_000)]
tok.EncodeBatchFlat(texts[:1000], True)
wall = []
for _ in range(5):
    t0 = time.perf_counter()
    ids, offs = tok.EncodeBatchFlat(texts, True)
    wall.append(time.perf_counter() - t0)
result["mirror_EncodeBatchFlat_100k_texts"] = {"median_s": round(statistics.median(wall), 4), "all_s": [round(w, 4) for w in wall], "ids": int(len(ids)),
                                               "device_special_calls": tok._encoder.special_stats()[0] if has_special else 0}
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
print(json.dumps(result))
