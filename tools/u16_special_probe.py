#!/usr/bin/env python3
"""What the UTF-16 special and trim entries cost against what a UTF-16 caller had before them.
Workload: the real-text sample of bench.py (kind 6), cut into documents, `<|endoftext|>` behind every document, as UTF-16 code units.
GB/s of INPUT (code units x 2 bytes), wall clock around the call, median of five after two warm-up calls, pageable numpy buffers for every leg:
  special  (a) tkz_encode_batch_special_utf16
           (b) the route of a caller without it: the units transcoded to UTF-8 on the host, then tkz_encode_batch_special_utf8, timed together
               (the transcode here is ONE codec call over the whole batch -- faster than a GetByteCount + GetBytes per string --, and the byte offsets are not
               timed: the figure flatters (b))
           (c) the plain tkz_encode_batch_utf16
  trim     the same three with tkz_encode_batch_trim_utf16 / _utf8 at a maximum of 512 (suffix)
  brackets the K_DOCMARK (k_lit_scan, k_lit_resolve) and K_PRETOK (k_lit_fix) brackets of (a), with and without a literal that holds U+FFFD registered (the
           replaced-byte bitmap is written by k_u16_write -- outside the brackets, so its cost shows in (a)'s wall clock -- and read by the literal kernels)
(b) uses nothing this tool's commit adds: run the tool on the parent commit as well, where (a) and the trim (a) are reported as absent.
usage: u16_special_probe.py [megabytes=256] [out=profiles/u16_special/u16_special_probe.json]"""
import gzip, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from tokenizer_amd import _native as N
from tokenizer_amd.tokenizer import ENCODERS

mb = int(sys.argv[1]) if len(sys.argv) > 1 else 256
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "u16_special", "u16_special_probe.json")
EOT = b"<|endoftext|>"
specials = dict(ENCODERS["cl100k_base"][2])
raw = gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "synth100k.tiktoken.gz"), "rb").read())

data, offs, meta = bench.real_text_corpus(mb << 20, 256, 4096)
n = len(offs) - 1
parts = []
for d in range(n):
    parts.append(data[offs[d]:offs[d + 1]].tobytes())
    parts.append(EOT)
u8 = np.frombuffer(b"".join(parts), np.uint8)
del parts
b_offs = (offs + len(EOT) * np.arange(n + 1)).astype(np.int64)
units = np.frombuffer(u8.tobytes().decode("utf-8").encode("utf-16-le"), np.uint16)
per_byte = ((u8 & 0xC0) != 0x80).astype(np.int64) + (u8 >= 0xF0)
u_offs = np.concatenate([[0], np.cumsum(per_byte)])[b_offs].astype(np.int64)
assert u_offs[-1] == len(units)
in_bytes = units.nbytes
index = [list(specials).index(EOT.decode())]
has_new = hasattr(N.Encoder, "encode_batch_special_utf16")
result = {"commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None,
          "docs": n, "units": int(len(units)), "input_bytes": int(in_bytes), "utf8_bytes": int(len(u8)), "corpus": meta}


def gbps(fn, steps=5, warmup=2):
    t = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(in_bytes / statistics.median(t[warmup:]) / 1e9, 3)


def transcode():
    return np.frombuffer(units.tobytes().decode("utf-16-le").encode("utf-8"), np.uint8)


def legs(enc):
    ids = np.empty(len(u8), np.int32)
    ooff = np.empty(n + 1, np.int64)
    r = {}
    if has_new:
        r["special_a_utf16"] = gbps(lambda: enc.encode_batch_special_utf16(units, u_offs, index, out=(ids, ooff)))
    r["special_b_transcode_utf8"] = gbps(lambda: enc.encode_batch_special(transcode(), b_offs, index, out=(ids, ooff)))
    r["special_c_plain_utf16"] = gbps(lambda: enc.encode_batch_utf16(units, u_offs, out=(ids, ooff)))
    if has_new:
        r["trim_a_utf16"] = gbps(lambda: enc.encode_batch_trim_utf16(units, u_offs, index, N.TRIM_SUFFIX, 512))
    if hasattr(enc, "encode_batch_trim"):
        r["trim_b_transcode_utf8"] = gbps(lambda: enc.encode_batch_trim(transcode(), b_offs, index, N.TRIM_SUFFIX, 512))
    return r


def brackets(enc):
    enc.set_profiling(True)
    try:
        enc.encode_batch_special_utf16(units, u_offs, index)
        enc.kernel_ms(reset=True)
        for _ in range(3):
            enc.encode_batch_special_utf16(units, u_offs, index)
        return {k: [round(ms / 3, 3), cnt // 3] for k, (ms, cnt) in enc.kernel_ms(reset=True).items()}
    finally:
        enc.set_profiling(False)


vocab = N.Vocab(raw)
enc = N.Encoder(vocab, N.CL100K)
enc.set_special_tokens(specials)
result["gbps"] = legs(enc)
if has_new:
    result["brackets_ms_no_fffd_literal"] = brackets(enc)
    enc2 = N.Encoder(vocab, N.CL100K)
    enc2.set_special_tokens(dict(specials, **{"<�>": 300001}))
    result["brackets_ms_fffd_literal"] = brackets(enc2)
    result["gbps_fffd_literal"] = {"special_a_utf16": gbps(lambda: enc2.encode_batch_special_utf16(units, u_offs, index))}
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
for k, v in result["gbps"].items():
    print("%-28s %7.3f GB/s of input" % (k, v))
print("wrote", out_path)
