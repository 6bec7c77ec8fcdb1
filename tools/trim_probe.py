#!/usr/bin/env python3
"""What EncodeTrimSuffix / EncodeTrimPrefix for a batch cost on the device.  One batch of the kind-1 (ASCII) corpus generated on the device, at three
maxima -- a quarter of, about, and four times the mean document token count --, timed with events on the launch stream (median of eight):
  1. tkz_encode_batch_trim_device on the device buffers, both sides;
  2. the plain tkz_encode_batch_device on the same batch (the difference is the price of piece granularity plus k_trim_cut, the scan, k_trim_gather);
  3. the parent's route to the same answer -- tkz_encode_batch_pieces_utf8 and the host walk over the pieces, text by text (TikTokenizer's fallback
     methods) -- on the first `n_host` documents, wall clock, against EncodeTrimSuffixBatch on the same texts;
  4. with --kernels: nothing but three trim calls, for `rocprofv3 --kernel-trace --stats -- python tools/trim_probe.py N OUT --kernels` (the times of
     k_trim_cut, k_scan_*64 / k_scan_top and k_trim_gather are read from its kernel statistics).
usage: trim_probe.py [n_docs=200000] [out=profiles/trim_device/trim_probe.json] [--kernels]"""
import gzip, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from tokenizer_amd import _native as N
from tokenizer_amd.tokenizer import TikTokenizer, REGEX_CL100K, ENCODERS

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_docs = int(args[0]) if len(args) > 0 else 200_000
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "trim_device", "trim_probe.json")
kernels_only = "--kernels" in sys.argv
n_host = 2000
specials = ENCODERS["cl100k_base"][2]
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
raw = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "synth100k.tiktoken.gz"), "rb").read())

d_offs = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
total = N.corpus_generate_device(0, 1, 0x5EED0002, 0, n_docs, 256, 768, d_offs.data_ptr(), None, 0, st)
d_bytes = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
N.corpus_generate_device(0, 1, 0x5EED0002, 0, n_docs, 256, 768, d_offs.data_ptr(), d_bytes.data_ptr(), total, st)
torch.cuda.synchronize()
d_ids = torch.empty(total, dtype=torch.int32, device=dev)
d_oo = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
d_cb = torch.empty(n_docs, dtype=torch.int64, device=dev)
d_cu = torch.empty(n_docs, dtype=torch.int64, device=dev)
enc = N.Encoder(N.Vocab(raw), N.CL100K)
enc.set_special_tokens(specials)
plain = lambda: enc.encode_batch_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, d_ids.data_ptr(), total, d_oo.data_ptr(), st)
trim = lambda side, mx: enc.encode_batch_trim_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, total, [], side, mx, 0, d_ids.data_ptr(), total, d_oo.data_ptr(),
                                                     d_cb.data_ptr(), d_cu.data_ptr(), st)
mean = max(4, plain() // n_docs)
if kernels_only:
    for mx in (mean // 4, mean, 4 * mean):
        trim(N.TRIM_SUFFIX, mx)
    torch.cuda.synchronize()
    sys.exit(0)


def timed(fn, steps=8, warmup=3):
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); n = fn(); b.record(); torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return {"ms": round(med, 3), "GBps": round(total / med / 1e6, 1), "tokens": int(n)}


result = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None,
          "n_docs": n_docs, "bytes": total, "mean_tokens_per_doc": int(mean), "plain_entry": timed(plain)}
for label, mx in (("below", mean // 4), ("near", mean), ("above", 4 * mean)):
    for side, sname in ((N.TRIM_SUFFIX, "suffix"), (N.TRIM_PREFIX, "prefix")):
        r = timed(lambda: trim(side, mx))
        r["max_tokens"] = int(mx)
        r["ratio_plain_over_trim"] = round(result["plain_entry"]["ms"] / r["ms"], 3)
        result["trim_%s_%s" % (sname, label)] = r
enc.set_profiling(True)
for name, fn in (("plain_entry", plain), ("trim_suffix_near", lambda: trim(N.TRIM_SUFFIX, mean))):
    enc.kernel_ms(reset=True)
    for _ in range(3):
        fn()
    result[name]["kernel_ms_of_3_calls"] = enc.kernel_ms(reset=True)       # (the same launch counts in every bracket: the trim kernels sit outside them)
enc.set_profiling(False)

# the parent's route: pieces to the host, the walk in the host language
tok = TikTokenizer(raw, specials, REGEX_CL100K)
texts = [N.corpus_doc_host(1, 0x5EED0002, d, 256, 768).decode("utf-8") for d in range(n_host)]
tok.EncodeTrimSuffixBatch(texts[:50], int(mean))
t0 = time.perf_counter(); a = tok.EncodeTrimSuffixBatch(texts, int(mean)); t1 = time.perf_counter()
b = [tok._trim_suffix_host(t, tok.SpecialTokens, int(mean)) for t in texts]; t2 = time.perf_counter()
assert a == b
result["mirror_%d_texts" % n_host] = {"EncodeTrimSuffixBatch_s": round(t1 - t0, 4), "pieces_entry_and_host_walk_s": round(t2 - t1, 4), "ratio": round((t2 - t1) / (t1 - t0), 1)}
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
print(json.dumps(result))
